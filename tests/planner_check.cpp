// Host-only check of the loop kernel's planner (ladiff_amd/csrc/systolic_plan.hip): builds workspace layouts, block lists and stage
// tables on a fake workspace base and holds them to the properties the device code relies on, and holds the launch policy
// (sys_launch_policy) to its rule.  No HIP call, no GPU; test_planner.py compiles this file together with the planner under
// AddressSanitizer + UBSan and runs it as a child process (exit status 0 = all held).
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <set>
#include <tuple>
#include <utility>
#include <vector>

#include "systolic_plan.h"

using namespace ladiff;

static int g_failed = 0;
static char g_ctx[256] = "";
#define CHECK(cond)                                                                                     \
    do {                                                                                                \
        if (!(cond)) {                                                                                  \
            if (++g_failed <= 40) std::printf("FAILED %s:%d [%s] %s\n", __FILE__, __LINE__, g_ctx, #cond); \
        }                                                                                               \
    } while (0)

// never dereferenced: the planner only does arithmetic on them
static float* const WS_BASE = reinterpret_cast<float*>(uintptr_t(1) << 44);
static uintptr_t addr(const void* p) { return reinterpret_cast<uintptr_t>(p); }

static DenoiserW fake_weights(uintptr_t base) {
    std::vector<const float*> p(DEN_NPARAMS);
    for (int i = 0; i < DEN_NPARAMS; ++i) p[i] = reinterpret_cast<const float*>(base + 4096u * (uintptr_t)i);
    DenoiserW w;
    static_assert(sizeof(DenoiserW) == DEN_NPARAMS * sizeof(const float*), "a table of pointers");
    std::memcpy(&w, p.data(), sizeof(w));
    return w;
}

static size_t round64(size_t f) { return (f + 63) / 64 * 64; }

// ------------------------------------------------------------------ layout
static void check_layout(int MR, int NB) {
    std::snprintf(g_ctx, sizeof(g_ctx), "layout MR %d NB %d plan %d", MR, NB, g_loop.stage_plan.load());
    const SysLayout L = sys_layout(MR, NB);
    const size_t off[] = {L.off_stages, L.off_status, L.off_blocks, L.off_flags, L.off_xin0, L.off_xs, L.off_xo,
                          L.off_att, L.off_x1, L.off_x2, L.off_pc, L.off_pe};                                    // carve order
    const int n = sizeof(off) / sizeof(off[0]);
    for (int i = 0; i < n; ++i) CHECK(off[i] % 64 == 0);
    for (int i = 1; i < n; ++i) CHECK(off[i] > off[i - 1]);
    CHECK(L.total % 64 == 0);
    CHECK(L.off_status == sys_layout(2, 1).off_status);            // ladiff_reverse_status reads it without knowing the plan
    CHECK(L.off_status == sys_status_offset_floats(1, 1));
    CHECK(L.off_blocks == sys_blocks_offset_floats(MR, NB));
    CHECK(L.ring == (size_t)PRING * 16 * MR * LADIFF_LATENT_DIM);
    CHECK(L.blk == (size_t)NB * 16 * MR * LADIFF_LATENT_DIM);
    CHECK(L.total == L.off_pe + round64((size_t)NL * NSLICE * L.ring));
    // the regions whose size is a record count hold their records
    CHECK(L.off_status - L.off_stages >= 256 * sizeof(Stage) / sizeof(float));
    CHECK(L.off_flags - L.off_blocks >= (size_t)NB * sizeof(BlockDesc) / sizeof(float));
    CHECK(L.off_xin0 - L.off_flags >= (size_t)NL * GROUPS_PER_LAYER * NB * FLAG_SLOTS * FLAG_STRIDE);
    CHECK(L.nwg == plan_nwg(MR) && L.NB == NB && L.split == (MR == 1 ? 1 : 0));
}

// ------------------------------------------------------------------ stage table
static void check_stages(int MR, int NB) {
    std::snprintf(g_ctx, sizeof(g_ctx), "stages MR %d NB %d plan %d", MR, NB, g_loop.stage_plan.load());
    static_assert(sizeof(Stage) == 20 * sizeof(int) + 11 * sizeof(void*), "no padding: the tables are compared as bytes");
    const DenoiserW W = fake_weights(uintptr_t(2) << 44), WSP = fake_weights(uintptr_t(3) << 44);
    const SysLayout L = sys_layout(MR, NB);
    const uintptr_t lo = addr(WS_BASE + L.off_xin0), hi = addr(WS_BASE + L.total);
    std::vector<unsigned char> h_chain, h_placed;
    CHECK(sys_build_stages(W, WSP, WS_BASE, MR, NB, false, h_chain) == 0);
    CHECK(sys_build_stages(W, WSP, WS_BASE, MR, NB, true, h_placed) == 0);
    CHECK(h_chain.size() == (size_t)plan_nwg(MR) * sizeof(Stage) && h_placed.size() == h_chain.size());
    CHECK(plan_nwg(MR) <= 256);
    const int n = (int)(h_chain.size() / sizeof(Stage));
    std::vector<Stage> chain(n), placed(n);
    std::memcpy(chain.data(), h_chain.data(), h_chain.size());
    std::memcpy(placed.data(), h_placed.data(), h_placed.size());

    // no round robin: the table stays as built - nobody checks where it runs and everybody writes through (the launch relies on it)
    for (const Stage& s : chain) CHECK(s.xcd == -1 && s.out_local == 0);
    {
        std::vector<Stage> again = chain;
        sys_place_stages(again, false);
        CHECK(std::memcmp(again.data(), chain.data(), h_chain.size()) == 0);
    }
    // round robin: a permutation of the chain-order table (placement only fills in xcd and out_local), workgroup i on XCD i % 8
    {
        std::vector<Stage> again = chain;
        sys_place_stages(again, true);
        CHECK(again.size() == placed.size() && std::memcmp(again.data(), placed.data(), h_placed.size()) == 0);
        auto bytes_less = [](const Stage& a, const Stage& b) { return std::memcmp(&a, &b, sizeof(Stage)) < 0; };
        std::vector<Stage> a = chain, b = placed;
        for (Stage& s : b) { s.xcd = -1; s.out_local = 0; }
        std::sort(a.begin(), a.end(), bytes_less);
        std::sort(b.begin(), b.end(), bytes_less);
        CHECK(std::memcmp(a.data(), b.data(), h_chain.size()) == 0);
        for (int i = 0; i < n; ++i) CHECK(placed[i].xcd == i % 8);
    }
    for (const std::vector<Stage>* tab : {&chain, &placed}) {
        std::set<int> out_groups;
        for (const Stage& s : *tab) out_groups.insert(s.out_group);
        for (const Stage& s : *tab) {
            for (const void* p : {(const void*)s.in0, (const void*)s.in1, (const void*)s.in2, (const void*)s.out, (const void*)s.bp_buf})
                if (p != nullptr) CHECK(addr(p) >= lo && addr(p) < hi);
            CHECK(s.out != nullptr && s.in0 != nullptr);
            CHECK(s.role >= R_QKV && s.role <= R_TAIL);
            CHECK(s.out_group >= 0 && s.out_group < NL * GROUPS_PER_LAYER);          // SysLayout::off_flags holds that many groups
            CHECK(out_groups.count(s.wait_group) == 1);
            if (s.bp_n > 0) CHECK(out_groups.count(s.bp_group) == 1);
            CHECK(s.wait_n >= 1 && s.wait_slot0 >= 0 && s.wait_slot0 + s.wait_n <= FLAG_SLOTS);
            CHECK(s.out_rep >= 1 && s.out_slot >= 0 && s.out_slot + (s.out_rep - 1) * s.out_rep_stride < FLAG_SLOTS);
            if (s.bp_n > 0) CHECK(s.bp_slot0 >= 0 && s.bp_slot0 + s.bp_n <= FLAG_SLOTS);
            CHECK(s.bp_blocks <= MAX_BP_BLOCKS);
            CHECK(s.blkstride >= 1 && s.blk0 >= 0 && s.blk0 < s.blkstride);
            if ((s.role == R_LIN || s.role == R_FFN)) CHECK(s.bp_n > 0 && s.bp_blocks >= 1 && s.bp_buf != nullptr);
        }
    }
    // plain stores only where every reader of the rows and every poller of the flags shares the producer's XCD
    for (const Stage& p : placed) {
        CHECK(p.out_local == 0 || p.out_local == 1);
        if (p.out_local != 1) continue;
        for (const Stage& c : placed) {
            const bool reads = c.in0 == p.out || c.in1 == p.out || c.in2 == p.out;
            const bool polls = c.wait_group == p.out_group || (c.bp_n > 0 && c.bp_group == p.out_group);
            if (reads || polls) CHECK(c.xcd == p.xcd);
        }
    }
}

// ------------------------------------------------------------------ packing
struct Case { const char* name; int B, T; std::vector<int32_t> counts; bool masked, device_only; };

static int clamp_count(int c, int T) { return c > T ? T : (c < 1 ? 1 : c); }

// one sys_pack_blocks call: returns (mr, nb) through the arguments after checking the block list
static void check_pack(const Case& c, int want_mr, bool cfg, int* mr_out, int* nb_out) {
    std::snprintf(g_ctx, sizeof(g_ctx), "pack %s want_mr %d cfg %d plan %d", c.name, want_mr, (int)cfg, g_loop.stage_plan.load());
    const int B = c.B, T = c.T;
    const int32_t* h_counts = (c.masked && !c.device_only) ? c.counts.data() : nullptr;
    std::vector<unsigned char> raw;
    int mr = -1, nb = -1;
    sys_pack_blocks(B, T, want_mr, h_counts, c.masked, cfg, raw, &mr, &nb);
    *mr_out = mr; *nb_out = nb;
    CHECK(mr == 1 || mr == 2);
    CHECK(nb >= 1 && raw.size() == (size_t)nb * sizeof(BlockDesc));
    if (mr != 1 && mr != 2) return;
    if (!cfg) CHECK(mr == 1);
    if (cfg && want_mr == 2) CHECK(mr == 2);
    if (cfg && want_mr == 1) CHECK(mr == (c.device_only ? 2 : 1));          // counts on the device only: no length-aware packing
    // the workspace query covers whatever the packing returns
    CHECK(sys_layout(mr, nb).total <= sys_ws_floats(B, T));
    CHECK(nb <= (mr == 1 ? nb16_max(B, T) : nb32(B, T)));
    std::vector<BlockDesc> blk(nb);
    std::memcpy(blk.data(), raw.data(), raw.size());

    const int nbr = cfg ? 2 : 1, RT = 16 * mr;
    std::vector<int> seen((size_t)nbr * B, 0);
    for (int b = 0; b < nb; ++b) {
        const BlockDesc& d = blk[b];
        CHECK(d.nrows >= 1 && d.nrows <= RT);
        CHECK(d.nsb >= 1 && d.nsb <= (mr == 1 ? 8 : 14));                   // QKV parks <= 14 text K|V slots, 8 in the 16-row plan
        int rows_total = 0;
        for (int sx = 0; sx < 16; ++sx) {
            if (sx >= d.nsb) { CHECK(d.b2[sx] == -1); continue; }
            const int b2 = d.b2[sx];
            CHECK(b2 >= 0 && b2 < nbr * B);
            if (b2 < 0 || b2 >= nbr * B) continue;
            seen[b2] += 1;
            const int prompt = b2 % B;
            const int want_rows = mr == 1 ? (h_counts ? clamp_count(h_counts[prompt], T) : T) : T;
            int rows = 0;
            for (int r = 0; r < d.nrows; ++r)
                if (d.row_b2[r] == b2) {
                    CHECK(d.row_t[r] == rows && d.row_lat[r] == prompt * T + rows);        // its latents, in order
                    CHECK((d.row_pk[r] & 0xff) == sx);
                    rows += 1;
                }
            CHECK(rows == want_rows);
            rows_total += rows;
        }
        CHECK(rows_total == d.nrows);
        for (int r = d.nrows; r < 32; ++r) CHECK(d.row_b2[r] == -1 && d.row_lat[r] == -1);
        // guidance: the partner is the other branch of the same prompts
        if (cfg && mr == 1) {
            CHECK(nb % 2 == 0);
            if (nb % 2 != 0) continue;
            const BlockDesc& o = blk[b ^ 1];
            CHECK(o.nsb == d.nsb && o.nrows == d.nrows);
            for (int sx = 0; sx < d.nsb; ++sx) CHECK(o.b2[sx] == d.b2[sx] + ((b & 1) ? -B : B));
        }
        if (mr == 2) {
            CHECK(d.nsb % 2 == 0);
            for (int sx = 0; sx < d.nsb / 2; ++sx) CHECK(d.b2[sx] < B && d.b2[sx + d.nsb / 2] == d.b2[sx] + B);
        }
        // the reduce parts cover every row of the tile exactly once
        std::vector<int> covered(RT, 0);
        for (int part = 0; part < NRED; ++part)
            for (int k = 0; k < 12; ++k) {
                const int pk = d.part_pk[part][k];
                if (pk == -1) continue;
                const int r = (pk & PART_PAD) ? (pk & ~PART_PAD) : (pk & 0xff);
                CHECK(r >= 0 && r < RT);
                if (r >= 0 && r < RT) covered[r] += 1;
                CHECK(((pk & PART_PAD) != 0) == (r >= d.nrows));
            }
        for (int r = 0; r < RT; ++r) CHECK(covered[r] == 1);
    }
    for (int v : seen) CHECK(v == 1);                                      // every (prompt, branch) in exactly one block
}

static void check_case(const Case& c, std::set<std::pair<int, int>>& plans) {
    int mr = 0, nb = 0;
    for (int want_mr = 1; want_mr <= 2; ++want_mr) {
        check_pack(c, want_mr, true, &mr, &nb);
        plans.insert({mr, nb});
    }
    if (!c.device_only) {                                                  // no guidance with device-only counts runs launch per stage: no plan
        check_pack(c, 1, false, &mr, &nb);
        plans.insert({mr, nb});
    }
    // choose_plan: what ladiff_reverse_plan and ladiff_diffusion_reverse launch with
    const int32_t* h_counts = (c.masked && !c.device_only) ? c.counts.data() : nullptr;
    for (int loop_mode = 1; loop_mode <= 3; ++loop_mode)
        for (int f16x3 = 0; f16x3 <= 1; ++f16x3)
            for (int cfg = c.device_only ? 1 : 0; cfg <= 1; ++cfg) {
                std::snprintf(g_ctx, sizeof(g_ctx), "choose %s loop_mode %d f16x3 %d cfg %d", c.name, loop_mode, f16x3, cfg);
                std::vector<unsigned char> plan;
                mr = 0; nb = 0;
                choose_plan(c.B, c.T, h_counts, c.masked, loop_mode, f16x3 != 0, plan, &mr, &nb, cfg != 0);
                CHECK((mr == 1 || mr == 2) && nb >= 1 && plan.size() == (size_t)nb * sizeof(BlockDesc));
                CHECK(sys_layout(mr, nb).total <= sys_ws_floats(c.B, c.T));
                CHECK(nb <= (mr == 1 ? nb16_max(c.B, c.T) : nb32(c.B, c.T)));
                if (!cfg) CHECK(mr == 1);
                if (cfg && loop_mode == 3) CHECK(mr == 2);
                if (cfg && loop_mode == 2) CHECK(mr == (c.device_only ? 2 : 1));
                plans.insert({mr, nb});
            }
}

// ------------------------------------------------------------------ launch policy
// sys_launch_policy against its rule, restated here (constants as numbers): every field, over the shapes on both sides of the two
// block-count thresholds and every switch value that takes another branch.
static void check_policy() {
    {
        std::snprintf(g_ctx, sizeof(g_ctx), "switch snapshot");
        const LoopSwitches d = g_loop.snapshot();                          // the library's defaults
        CHECK(d.waves16 == 2 && d.handoff == 1 && d.stage_plan == 0 && d.poll_pause == 0 && d.stage_delay == -1 && d.pace == -1 &&
              d.look_ahead_from == -1 && d.small_upto == -1 && d.xcd_local == 1);
        g_loop.pace = 3 | 5 << 8; g_loop.xcd_local = 2;
        const LoopSwitches e = g_loop.snapshot();
        CHECK(e.pace == (3 | 5 << 8) && e.xcd_local == 2 && e.waves16 == 2 && e.stage_delay == -1);
        g_loop.pace = -1; g_loop.xcd_local = 1;
    }
    // (MR, fp32, multistep, edit, waves16, handoff, look_ahead) -> the key first seen for it
    std::map<std::tuple<int, bool, bool, bool, int, int, int>, LoopKey> keys;
    long n = 0;
    for (int MR : {1, 2}) for (bool fp32 : {false, true}) for (bool ms : {false, true}) for (bool edit : {false, true})
    for (int NB : {1, 59, 60, 61, 71, 72, 73, 255})
    for (int waves16 : {1, 2}) for (int handoff : {0, 1})
    for (int la_sw : {-1, 0, 66}) for (int small_sw : {-1, 0, 66})
    for (int pace : {-1, 0, 3 | 5 << 8}) for (int sd : {-1, 0, 9 | 4 << 8}) for (int pp : {0, 0xff | 64 << 8})
    for (int xcd_local : {0, 1, 2}) {
        std::snprintf(g_ctx, sizeof(g_ctx), "policy MR %d fp32 %d ms %d edit %d NB %d waves %d handoff %d la %d small %d pace %d sd %d pp %d xcd %d",
                      MR, (int)fp32, (int)ms, (int)edit, NB, waves16, handoff, la_sw, small_sw, pace, sd, pp, xcd_local);
        const LoopSwitches sw{waves16, handoff, 0, pp, sd, pace, la_sw, small_sw, xcd_local};
        const LoopLaunch p = sys_launch_policy(MR, NB, fp32, ms, edit, sw);
        ++n;
        const bool tagged = MR == 1 && waves16 == 2 && handoff == 1;
        const int la_from = la_sw >= 0 ? la_sw : 72, small = small_sw >= 0 ? small_sw : 60;
        const int look_ahead = NB >= la_from ? 1 : 0;
        CHECK(p.key.tagged == tagged);
        CHECK(p.key.waves == ((MR == 1 && waves16 == 2) ? 2 : 1));
        CHECK(p.key.mr == (MR == 1 ? 1 : 2));
        CHECK(p.look_ahead == look_ahead);
        CHECK(p.key.look_ahead == (tagged && look_ahead != 0));
        CHECK(p.key.fp32 == fp32 && p.key.multistep == ms && p.key.edit == edit);
        CHECK(p.pace == (pace >= 0 ? pace : (NB <= small ? 0 : (4 | 4 << 8))));
        if (sd < 0) CHECK(p.delay_mask == (NB <= small ? (1 | 8) : 0) && p.delay_len == 4);
        else CHECK(p.delay_mask == (sd & 0xff) && p.delay_len == ((sd >> 8) & 0x7f));
        CHECK(p.pause_mask == (pp & 0xff) && p.pause_len == ((pp >> 8) & 0xff));
        CHECK(p.force_mismatch == (xcd_local == 2 ? 1 : 0));
        // the key is a function of these seven and of nothing else
        const auto in = std::make_tuple(MR, fp32, ms, edit, waves16, handoff, look_ahead);
        const auto it = keys.find(in);
        if (it == keys.end()) keys.emplace(in, p.key);
        else {
            const LoopKey& k = it->second;                                 // field by field here, and by the library's operator==
            CHECK(k.mr == p.key.mr && k.waves == p.key.waves && k.tagged == p.key.tagged && k.look_ahead == p.key.look_ahead &&
                  k.fp32 == p.key.fp32 && k.multistep == p.key.multistep && k.edit == p.key.edit);
            CHECK(k == p.key);
        }
    }
    {
        std::snprintf(g_ctx, sizeof(g_ctx), "key equality");              // every field takes part
        const LoopKey k{1, 2, true, true, false, true, false};
        for (int f = 0; f < 7; ++f) {
            LoopKey o = k;
            if (f == 0) o.mr = 2; else if (f == 1) o.waves = 1; else if (f == 2) o.tagged = false; else if (f == 3) o.look_ahead = false;
            else if (f == 4) o.fp32 = true; else if (f == 5) o.multistep = false; else o.edit = true;
            CHECK(!(o == k) && o == o);
        }
    }
    std::snprintf(g_ctx, sizeof(g_ctx), "policy enumeration");
    CHECK(n == 2L * 2 * 2 * 2 * 8 * 2 * 2 * 3 * 3 * 3 * 3 * 2 * 3 && keys.size() == 2u * 2 * 2 * 2 * 2 * 2 * 2);
    CHECK(LOOK_AHEAD_BLOCKS == 72 && SMALL_LAUNCH_BLOCKS == 60);
}

int main() {
    check_policy();
    std::vector<Case> cases;
    cases.push_back({"1: B 1 T 1", 1, 1, {}, false, false});
    cases.push_back({"2: B 1 T 7", 1, 7, {}, false, false});
    cases.push_back({"3: B 3 T 7 counts 1 7 4", 3, 7, {1, 7, 4}, true, false});
    cases.push_back({"3b: B 3 T 7 counts outside [1, T]", 3, 7, {0, 12, 4}, true, false});
    cases.push_back({"4: B 9 T 8 full", 9, 8, std::vector<int32_t>(9, 8), true, false});
    cases.push_back({"5: B 17 T 2", 17, 2, {}, false, false});
    cases.push_back({"6: B 128 T 7 full", 128, 7, std::vector<int32_t>(128, 7), true, false});
    {
        std::vector<int32_t> cnt(128);
        uint32_t x = 12345u;
        for (int32_t& v : cnt) { x = x * 1664525u + 1013904223u; v = 1 + (int32_t)((x >> 16) % 7u); }
        cases.push_back({"7: B 128 T 7 mixed", 128, 7, cnt, true, false});
    }
    cases.push_back({"8: B 5 T 7 device-only counts", 5, 7, {}, true, true});
    cases.push_back({"9: B 6 T 3", 6, 3, {}, false, false});
    cases.push_back({"9b: B 6 T 3 counts", 6, 3, {3, 1, 2, 3, 1, 1}, true, false});

    for (int plan = 0; plan <= 1; ++plan) {                                // both ways of dealing a layer's spare workgroups (red_plan)
        g_loop.stage_plan = plan;
        std::set<std::pair<int, int>> plans;                               // every (MR, NB) the packing came up with
        for (const Case& c : cases) check_case(c, plans);
        for (int MR = 1; MR <= 2; ++MR)
            for (int NB : {1, 2, 3, 17, 64, 256}) plans.insert({MR, NB});
        for (const auto& p : plans) { check_layout(p.first, p.second); check_stages(p.first, p.second); }
        // case 5: eight prompts per 16-row block, the last block takes the remainder
        {
            std::snprintf(g_ctx, sizeof(g_ctx), "case 5 blocks");
            std::vector<unsigned char> raw;
            int mr = 0, nb = 0;
            sys_pack_blocks(17, 2, 1, nullptr, false, true, raw, &mr, &nb);
            CHECK(mr == 1 && nb == 6);
            std::vector<BlockDesc> blk(nb > 0 ? nb : 0);
            std::memcpy(blk.data(), raw.data(), std::min(raw.size(), blk.size() * sizeof(BlockDesc)));
            if (nb == 6) CHECK(blk[0].nsb == 8 && blk[2].nsb == 8 && blk[4].nsb == 1 && blk[5].nsb == 1);
        }
    }
    if (g_failed) { std::printf("planner_check: %d checks FAILED\n", g_failed); return 1; }
    std::printf("planner_check: ok\n");
    return 0;
}
