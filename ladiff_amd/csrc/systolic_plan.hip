// The host planner of the persistent denoiser loop (systolic.hip): the workspace carve, the block packing, the stage table and its
// XCD placement, and the choice between the 16- and the 32-row plan.  Integer and pointer arithmetic only - no HIP call, no device
// code, nothing a build variant's defines reach - so a C++ compiler builds it alone and tests/planner_check.cpp runs it without a GPU.
#include <algorithm>
#include <cstring>

#include "systolic_plan.h"

namespace ladiff {

LoopSwitchAtoms g_loop;

int plan_nwg(int MR) {
    const RedPlan rp = red_plan(MR);
    return NL * (4 + rp.out_groups + NSLICE + rp.red2_parts + NSLICE + rp.styl_parts * rp.styl_groups) + 2 * NSKIP + NTAIL;
}
// 32-row tiles: P prompts per block, both guidance branches, T rows each
int prompts_per_block32(int T) { int P = 32 / (2 * T); return P > 7 ? 7 : (P < 1 ? 1 : P); }   // QKV parks <= 14 text K|V slots
int nb32(int B, int T) { const int P = prompts_per_block32(T); return (B + P - 1) / P; }
// 16-row tiles, worst case of the packing (every prompt with all T rows): floor(16 / T) prompts (<= 8) per branch block
int nb16_max(int B, int T) { int P = 16 / T; P = P > 8 ? 8 : (P < 1 ? 1 : P); return 2 * ((B + P - 1) / P); }

SysLayout sys_layout(int MR, int NB) {
    SysLayout L;
    const int RT = 16 * MR;
    L.split = MR == 1 ? 1 : 0;
    L.NB = NB;
    L.nwg = plan_nwg(MR);
    L.blk = (size_t)NB * RT * D;
    size_t off = 0;
    auto take = [&](size_t floats) { const size_t o = off; off += (floats + 63) / 64 * 64; return o; };
    L.off_stages = take((size_t)256 * sizeof(Stage) / sizeof(float));
    L.off_status = take(64);      // before everything sized by the block geometry: ladiff_reverse_status reads it at a fixed offset
    L.off_blocks = take((size_t)NB * sizeof(BlockDesc) / sizeof(float));
    L.off_flags = take((size_t)NL * GROUPS_PER_LAYER * NB * FLAG_SLOTS * FLAG_STRIDE);
    L.off_xin0 = take(L.blk);
    L.off_xs = take(NSKIP * L.blk);
    L.off_xo = take(NL * L.blk);
    // one set per LAYER: a buffer is then written by the workgroups of one stage group only - on one XCD when the group stores
    // plainly (Stage::out_local), so that no line is ever dirty in two L2s
    L.off_att = take(NL * L.blk);
    L.off_x1 = take(NL * L.blk);
    L.off_x2 = take(NL * L.blk);
    L.ring = (size_t)PRING * RT * D;                                  // floats of one partial plane: a ring of PRING block slots
    L.off_pc = take((size_t)NL * NSLICE * L.ring);
    L.off_pe = take((size_t)NL * NSLICE * L.ring);
    L.total = off;
    return L;
}

size_t sys_ws_floats(int B, int T) {
    const size_t a = sys_layout(1, nb16_max(B, T)).total, b = sys_layout(2, nb32(B, T)).total;
    return a > b ? a : b;
}

// Block geometry for this call (host).  h_counts = the latent counts on the HOST (or NULL); masked = the call has device counts.
//   MR 2: blocks of P consecutive prompts, both branches, T rows per prompt; the count only masks keys (cnt = -1 when the host
//         does not know it: the kernel reads counts[] itself).
//   MR 1: LENGTH-AWARE packing - prompts sorted by latent count, a block = one guidance branch of as many prompts as fit in 16
//         rows with ONLY their count[b] valid rows (padded latent rows are never computed); needs the counts on the host.
// Returns the plan: `blocks`, and in `mr` the tile size actually planned (MR 1 falls back to 2 when the counts are device-only).
// cfg = false (no classifier-free guidance, ladiff.py:472-490: the network sees the B latents once): 16-row blocks of ONE branch, no
// partner block - the tail treats a block as a unit whose "conditional" row is the row itself (guidance then adds g * 0 exactly).
void sys_pack_blocks(int B, int T, int want_mr, const int32_t* h_counts, bool masked, bool cfg, std::vector<unsigned char>& out, int* mr, int* nb) {
    std::vector<BlockDesc> blocks;
    auto count_of = [&](int b) { int c = (masked && h_counts) ? h_counts[b] : T; return c > T ? T : (c < 1 ? 1 : c); };
    int MR = want_mr;
    if (!cfg) MR = 1;                                                  // the caller checked sys_plan_possible()
    if (MR == 1 && masked && h_counts == nullptr && cfg) MR = 2;
    auto fresh = [] { BlockDesc d; std::memset(&d, 0, sizeof(d)); for (int i = 0; i < 16; ++i) d.b2[i] = -1;
                      for (int r = 0; r < 32; ++r) { d.row_b2[r] = -1; d.row_lat[r] = -1; } return d; };
    // derived tables: the reduce parts' slots (the live rows split evenly over NRED parts) and the tail's (prompt, latent) pairs
    auto finish = [&](BlockDesc& d, const int* row_cnt, int npairs, int rc_off) {
        const int nparts = red_plan(MR).red2_parts;               // RED2 and STYL split a block's rows the same way
        const int RT = 16 * MR, per = (RT + nparts - 1) / nparts; // all rows of the tile, padding included (stored as zeros)
        for (int part = 0; part < NRED; ++part) {
            const int lo = part * per < RT ? part * per : RT, hi = lo + per < RT ? lo + per : RT;
            for (int k = 0; k < 12; ++k) {
                const int r = lo + k;
                d.part_pk[part][k] = -1; d.part_b2[part][k] = -1;
                if (part < nparts && r < hi) {
                    if (r < d.nrows) {
                        d.part_pk[part][k] = r | d.row_t[r] << 8 | (row_cnt[r] < 0 ? 0xff : row_cnt[r]) << 16;
                        d.part_b2[part][k] = d.row_b2[r];
                    } else {
                        d.part_pk[part][k] = PART_PAD | r;
                    }
                }
            }
        }
        // tail: pairs first; the slots behind them pad.  One-branch blocks (rc_off 0): slot q pads row q of both blocks of the unit;
        // two-branch blocks: the pad slots share the rows from nrows up, two each (both in the unit's one block)
        for (int q = 0; q < 16; ++q) {
            d.pair_lat[q] = -1; d.pair_t[q] = 0; d.pair_rc[q] = -1; d.pair_pad[q] = -1;
            if (q < npairs) { d.pair_lat[q] = d.row_lat[q]; d.pair_t[q] = d.row_t[q]; d.pair_rc[q] = q + rc_off; }
            else if (rc_off == 0) { if (q < RT) { d.pair_pad[q] = q; d.pair_rc[q] = q; } }
            else {
                const int r = d.nrows + 2 * (q - npairs);
                if (r < RT) d.pair_pad[q] = r;
                if (r + 1 < RT) d.pair_rc[q] = r + 1;
            }
        }
    };
    if (MR == 2) {
        const int P = prompts_per_block32(T);
        for (int p0 = 0; p0 < B; p0 += P) {
            const int Pb = B - p0 < P ? B - p0 : P;
            BlockDesc d = fresh();
            d.nsb = 2 * Pb; d.nrows = 2 * Pb * T;
            int row_cnt[32];
            for (int br = 0; br < 2; ++br)
                for (int pl = 0; pl < Pb; ++pl) {
                    const int sx = br * Pb + pl, prompt = p0 + pl;
                    const int cnt = masked ? (h_counts ? count_of(prompt) : -1) : T;
                    d.b2[sx] = br * B + prompt;
                    for (int t = 0; t < T; ++t) {
                        const int r = sx * T + t;
                        d.row_pk[r] = sx | (sx * T) << 8 | (cnt < 0 ? 0xff : cnt) << 16;
                        d.row_t[r] = t; d.row_b2[r] = br * B + prompt; row_cnt[r] = cnt; d.row_lat[r] = prompt * T + t;
                    }
                }
            finish(d, row_cnt, d.nrows / 2, d.nrows / 2);                // conditional row of a pair: nrows / 2 further
            blocks.push_back(d);
        }
    } else {
        std::vector<int> order(B);
        for (int b = 0; b < B; ++b) order[b] = b;
        std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return count_of(a) > count_of(b); });
        size_t i = 0;
        while (i < order.size()) {
            std::vector<int> group;
            int rows = 0;
            while (i < order.size() && group.size() < 8 && rows + count_of(order[i]) <= 16) { rows += count_of(order[i]); group.push_back(order[i]); ++i; }
            for (int br = 0; br < (cfg ? 2 : 1); ++br) {
                BlockDesc d = fresh();
                d.nsb = (int)group.size(); d.nrows = rows;
                int r0 = 0, row_cnt[32];
                for (int sx = 0; sx < (int)group.size(); ++sx) {
                    const int prompt = group[sx], cnt = count_of(prompt);
                    d.b2[sx] = br * B + prompt;
                    for (int t = 0; t < cnt; ++t) {
                        const int r = r0 + t;
                        d.row_pk[r] = sx | r0 << 8 | cnt << 16;
                        d.row_t[r] = t; d.row_b2[r] = br * B + prompt; row_cnt[r] = cnt; d.row_lat[r] = prompt * T + t;
                    }
                    r0 += cnt;
                }
                finish(d, row_cnt, rows, 0);                             // the conditional branch is the next block, same row
                blocks.push_back(d);
            }
        }
    }
    out.resize(blocks.size() * sizeof(BlockDesc));
    std::memcpy(out.data(), blocks.data(), out.size());
    *mr = MR; *nb = (int)blocks.size();
}

// ---- XCD placement.  The dispatcher hands workgroup i of a launch to XCD i % 8 (from wherever the previous launch
// stopped; checked once per device by a probe launch of the same shape, and by every pipeline workgroup when it starts: status 3).  `st` comes in CHAIN order (the order a block
// flows through the stages); the stages are dealt to the XCDs in that order, 32 (31) to each, so that a layer's hand-offs stay
// inside one XCD's L2 and the chain crosses an XCD boundary only 7 times (+ the skip connections and the tail).  A stage whose
// readers all sit on its own XCD stores plainly (Stage::out_local); everything else works as before (write-through).
// round_robin = what the probe found (and the ladiff_debug_set_xcd_local switch allows); false: no placement - the table stays in
// chain order, no workgroup checks where it runs (xcd -1) and every stage writes through.
void sys_place_stages(std::vector<Stage>& st, bool round_robin) {
    if (!round_robin) return;
    const int n = (int)st.size();
    std::vector<Stage> placed(n);
    int cnt[8] = {}, k = 0;
    for (int j = 0; j < n; ++j) {
        while (cnt[k] == (n - k + 7) / 8) ++k;                        // XCD k runs workgroups k, k + 8, ...
        st[j].xcd = k;
        placed[k + 8 * cnt[k]++] = st[j];
    }
    for (Stage& p : placed) {
        bool local = true;
        for (const Stage& c : placed) {
            const bool reads = c.in0 == p.out || c.in1 == p.out || c.in2 == p.out;                       // its rows
            const bool polls = c.wait_group == p.out_group || (c.bp_n > 0 && c.bp_group == p.out_group);  // its flags
            if ((reads || polls) && c.xcd != p.xcd) local = false;
        }
        p.out_local = local ? 1 : 0;
    }
    st.swap(placed);
}

// Builds the stage table (host) for this call's pointers.  `ws` = the systolic region of the reverse workspace.
int sys_build_stages(const DenoiserW& W, const DenoiserW& WS, float* ws, int MR, int NB, bool round_robin, std::vector<unsigned char>& host) {
    // WS = the S-format weight table in f16x3 mode; in fp32 mode the caller passes the fp32 table twice
    const SysLayout L = sys_layout(MR, NB);
    const RedPlan rp = red_plan(MR);
    std::vector<Stage> st;
    float* xin0 = ws + L.off_xin0;
    auto XO = [&](int l) { return ws + L.off_xo + (size_t)l * L.blk; };
    auto XS = [&](int l) { return ws + L.off_xs + (size_t)(l - NSKIP - 1) * L.blk; };
    auto G = [&](int l, int g) { return l * GROUPS_PER_LAYER + g; };
    const bool x2_rep = rp.red2_parts * NSLICE <= FLAG_SLOTS;
    for (int l = 0; l < NL; ++l) {
        const DenLayerW& w = W.layer[l];
        const DenLayerW& ws_ = WS.layer[l];
        float* att = ws + L.off_att + (size_t)l * L.blk; float* x1 = ws + L.off_x1 + (size_t)l * L.blk; float* x2 = ws + L.off_x2 + (size_t)l * L.blk;
        float* pc = ws + L.off_pc + (size_t)l * NSLICE * L.ring; float* pe = ws + L.off_pe + (size_t)l * NSLICE * L.ring;
        const float* xin; int xg, xn;
        if (l == 0) { xin = xin0; xg = G(0, G_XIN); xn = 1; }
        else if (l <= NSKIP) { xin = XO(l - 1); xg = G(l - 1, G_XO); xn = rp.styl_parts; }
        else { xin = XS(l); xg = G(l, G_XIN); xn = 2; }
        if (l > NSKIP) {
            const int i = l - NSKIP - 1;
            for (int c = 0; c < 2; ++c) {
                Stage s{};
                s.role = R_SKIP; s.layer = l; s.slice = c; s.wait_group = G(l - 1, G_XO); s.wait_n = rp.styl_parts;
                s.out_group = G(l, G_XIN); s.out_slot = c;
                s.w0 = WS.skip[i].w; s.b0 = W.skip[i].b; s.in0 = XO(l - 1); s.in1 = XO(NL - 1 - l); s.out = XS(l);
                st.push_back(s);
            }
        }
        for (int h = 0; h < H; ++h) {
            Stage s{};
            s.role = R_QKV; s.layer = l; s.slice = h; s.wait_group = xg; s.wait_n = xn; s.out_group = G(l, G_ATT); s.out_slot = h;
            s.w0 = ws_.sa_attn.in_w; s.b0 = w.sa_attn.in_b; s.in0 = xin; s.out = att;
            st.push_back(s);
        }
        for (int g = 0; g < rp.out_groups; ++g) {                         // groups: workgroups of their own on alternating blocks
            Stage s{};
            s.role = R_OUT; s.layer = l; s.wait_group = G(l, G_ATT); s.wait_n = H; s.out_group = G(l, G_X1); s.out_slot = 0;
            s.out_rep = NSLICE; s.out_rep_stride = 1;                     // one flag line per LIN workgroup
            s.blk0 = g; s.blkstride = rp.out_groups;
            s.w0 = ws_.sa_attn.out_w; s.b0 = w.sa_attn.out_b; s.g = w.sa_norm1.g; s.be = w.sa_norm1.b; s.in0 = att; s.in1 = xin; s.out = x1;
            st.push_back(s);
        }
        for (int j = 0; j < NSLICE; ++j) {
            Stage s{};
            s.role = R_LIN; s.layer = l; s.slice = j; s.wait_group = G(l, G_X1); s.wait_n = 1; s.out_group = G(l, G_PC); s.out_slot = j;
            s.wait_slot0 = j;
            s.bp_group = G(l, G_X2); s.bp_slot0 = x2_rep ? j * rp.red2_parts : 0; s.bp_n = rp.red2_parts; s.bp_blocks = 1; s.bp_buf = x2;
            s.w0 = ws_.sa_lin1.w; s.w1 = ws_.sa_lin2.w; s.b0 = w.sa_lin1.b; s.in0 = x1; s.out = pc;
            st.push_back(s);
        }
        for (int q = 0; q < rp.red2_parts; ++q) {
            Stage s{};
            s.role = R_RED2; s.layer = l; s.slice = q; s.wait_group = G(l, G_PC); s.wait_n = NSLICE; s.out_group = G(l, G_X2); s.out_slot = q;
            if (x2_rep) { s.out_rep = NSLICE; s.out_rep_stride = rp.red2_parts; }   // FFN workgroup j polls slots j parts + q
            s.b0 = w.sa_lin2.b; s.g = w.sa_norm2.g; s.be = w.sa_norm2.b; s.in0 = pc; s.in1 = x1; s.out = x2;
            st.push_back(s);
        }
        for (int j = 0; j < NSLICE; ++j) {
            Stage s{};
            s.role = R_FFN; s.layer = l; s.slice = j; s.wait_group = G(l, G_X2); s.wait_n = rp.red2_parts; s.out_group = G(l, G_PE); s.out_slot = j;
            if (x2_rep) s.wait_slot0 = j * rp.red2_parts;
            s.bp_group = G(l, G_XO); s.bp_slot0 = 0; s.bp_n = rp.styl_parts; s.bp_blocks = rp.styl_groups; s.bp_buf = XO(l);
            s.w0 = ws_.ffn1.w; s.w1 = ws_.ffn2.w; s.b0 = w.ffn1.b; s.in0 = x2; s.out = pe;
            st.push_back(s);
        }
        for (int g = 0; g < rp.styl_groups; ++g)
            for (int q = 0; q < rp.styl_parts; ++q) {
                Stage s{};
                s.role = R_STYL; s.layer = l; s.slice = q; s.wait_group = G(l, G_PE); s.wait_n = NSLICE; s.out_group = G(l, G_XO); s.out_slot = q;
                s.blk0 = g; s.blkstride = rp.styl_groups;
                s.w0 = ws_.ffn_proj.out.w; s.b0 = w.ffn_proj.out.b; s.b1 = w.ffn2.b; s.g = w.ffn_proj.norm.g; s.be = w.ffn_proj.norm.b;
                s.in0 = pe; s.in1 = x2; s.out = XO(l);
                st.push_back(s);
            }
    }
    for (int k = 0; k < NTAIL; ++k) {
        Stage s{};
        s.role = R_TAIL; s.layer = NL; s.slice = k; s.wait_group = G(NL - 1, G_XO); s.wait_n = rp.styl_parts; s.out_group = G(0, G_XIN); s.out_slot = 0;
        s.in0 = XO(NL - 1); s.out = xin0;
        st.push_back(s);
    }
    for (Stage& s : st) {
        if (s.blkstride == 0) s.blkstride = 1;                        // every other stage visits every block
        if (s.out_rep == 0) s.out_rep = 1;                            // one flag, one line
        s.xcd = -1;
    }
    if ((int)st.size() != L.nwg || st.size() > 256) return LADIFF_ERR_SHAPE;
    sys_place_stages(st, round_robin);
    host.resize(st.size() * sizeof(Stage));
    std::memcpy(host.data(), st.data(), host.size());
    return 0;
}

size_t sys_blocks_offset_floats(int MR, int NB) { return sys_layout(MR, NB).off_blocks; }
size_t sys_status_offset_floats(int B, int T) { (void)B; (void)T; return sys_layout(2, 1).off_status; }

// Block plan of the pipeline loop for one call (host only).  loop_mode: 1 = pick by the cost model, 2 / 3 = force 16- / 32-row blocks.
void choose_plan(int B, int T, const int32_t* h_counts, bool masked, int loop_mode, bool f16x3, std::vector<unsigned char>& plan,
                 int* plan_mr, int* plan_nb, bool cfg) {
    int mr16 = 1, nb16 = 0, mr32 = 2, nb32 = 0;
    std::vector<unsigned char> p16, p32;
    if (!cfg) {             // no guidance: one-branch 16-row blocks only (the caller made sure the counts are on the host, or absent)
        sys_pack_blocks(B, T, 1, h_counts, masked, false, plan, plan_mr, plan_nb);
        return;
    }
    sys_pack_blocks(B, T, 2, h_counts, masked, true, p32, &mr32, &nb32);
    int want = loop_mode == 2 ? 1 : (loop_mode == 3 ? 2 : 0);
    if (want != 2) sys_pack_blocks(B, T, 1, h_counts, masked, true, p16, &mr16, &nb16);
    if (want == 0) {
        // measured (scripts/try_pipeline.py uniform, 1 ... 128 prompts, final build of round 2): the busiest stage's time per block
        // and one block's unloaded trip through the 59 stages, in us, for 16- / 32-row blocks
        const double c16 = f16x3 ? 2.45 : 5.05, c32 = f16x3 ? 5.3 : 12.1, lat16 = f16x3 ? 172.0 : 310.0, lat32 = f16x3 ? 282.0 : 525.0;
        const double e16 = mr16 == 1 ? std::max(lat16, nb16 * c16) : 1e30, e32 = std::max(lat32, nb32 * c32);
        want = e16 < e32 ? 1 : 2;
    }
    if (want == 1 && mr16 == 1) { plan.swap(p16); *plan_mr = 1; *plan_nb = nb16; }
    else { plan.swap(p32); *plan_mr = 2; *plan_nb = nb32; }
}

LoopLaunch sys_launch_policy(int MR, int NB, bool fp32, bool multistep, bool edit, const LoopSwitches& sw, bool record) {
    const int la_from = sw.look_ahead_from >= 0 ? sw.look_ahead_from : LOOK_AHEAD_BLOCKS;      // ladiff_debug_set_loop_thresholds
    const int small_upto = sw.small_upto >= 0 ? sw.small_upto : SMALL_LAUNCH_BLOCKS;
    LoopLaunch p;
    p.look_ahead = NB >= la_from ? 1 : 0;               // whether tagged or not
    const bool tagged = MR == 1 && sw.waves16 == 2 && sw.handoff == 1;
    if (record && tagged) p.look_ahead = 0;             // the recording instantiations: none with look-ahead
    p.key = LoopKey{MR == 1 ? 1 : 2, MR == 1 && sw.waves16 == 2 ? 2 : 1, tagged, tagged && p.look_ahead, fp32, multistep, edit, record};
    p.pause_mask = sw.poll_pause & 0xff; p.pause_len = (sw.poll_pause >> 8) & 0xff; p.force_mismatch = sw.xcd_local == 2 ? 1 : 0;
    p.pace = sw.pace >= 0 ? sw.pace : (NB <= small_upto ? 0 : (4 | (4 << 8)));
    // Small launches (a block's trip through the stages bounds the step, the stages wait for rows most of the time): the LIN and FFN
    // workgroups idle ~0.25 us after every block before they start to poll for the next one's rows - those are being produced just then by
    // a stage on the critical path (OUT / RED2), and eight workgroups loading its lines do not make it faster.  Measured (profiles/r4/14_*):
    // loop -2.2 % at 32 ... 64 prompts and at 100 / 128 prompts of mixed lengths (<= 58 blocks), nothing from 65 blocks, a loss beyond.
    if (sw.stage_delay < 0) { p.delay_mask = NB <= small_upto ? 1 | 8 : 0; p.delay_len = 4; }
    else { p.delay_mask = sw.stage_delay & 0xff; p.delay_len = (sw.stage_delay >> 8) & 0x7f; }
    return p;
}

}  // namespace ladiff
