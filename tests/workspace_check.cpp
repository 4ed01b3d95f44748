// Host-only check of the workspace layouts (ladiff_amd/csrc/workspace.h): carves every layout on a fake 256-byte-aligned base and holds
// it to the properties the sequencing code and the kernels rely on.  No HIP call, no GPU; test_workspace.py compiles this file with the
// loop kernel's planner (the reverse loop embeds its workspace) under AddressSanitizer + UBSan and runs it as a child process.
// The region sizes are stated here a second time on purpose: this is the check, the header is the one statement the library uses.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "workspace.h"

using namespace ladiff;

static int g_failed = 0;
static char g_ctx[256] = "";
#define CHECK(cond)                                                                                     \
    do {                                                                                                \
        if (!(cond)) {                                                                                  \
            if (++g_failed <= 40) std::printf("FAILED %s:%d [%s] %s\n", __FILE__, __LINE__, g_ctx, #cond); \
        }                                                                                               \
    } while (0)

// never dereferenced: the layouts only do arithmetic on it
static float* const WS_BASE = reinterpret_cast<float*>(uintptr_t(1) << 44);
static uintptr_t addr(const void* p) { return reinterpret_cast<uintptr_t>(p); }
static size_t round64(size_t f) { return (f + 63) / 64 * 64; }
constexpr size_t D_ = LADIFF_LATENT_DIM, FF_ = LADIFF_FF_SIZE, TD_ = LADIFF_TEXT_DIM, NL_ = LADIFF_NUM_LAYERS, MAXF_ = LADIFF_MAX_FRAMES;

struct Reg { const void* p; size_t floats; bool vec16; };     // vec16: float rows that kernels read 16 bytes at a time
typedef std::vector<Reg> Regs;

// regions in declaration order, each starting where the one before ends (rounded to `align` floats), all inside [base, base + total);
// `slack` floats of unnamed tail; the same call on a null base: the same total, null pointers only
static void check_regions(const Regs& with_base, const Regs& with_null, size_t total, size_t null_total, size_t query, size_t align,
                          size_t slack) {
    CHECK(total == query && null_total == query);
    CHECK(with_base.size() == with_null.size());
    const uintptr_t lo = addr(WS_BASE), hi = lo + total * sizeof(float);
    uintptr_t cursor = lo;
    for (size_t i = 0; i < with_base.size(); ++i) {
        const Reg& r = with_base[i];
        CHECK(with_null[i].p == nullptr && with_null[i].floats == r.floats);
        CHECK(addr(r.p) >= cursor);                          // declaration order, no overlap
        CHECK(addr(r.p) == cursor);                          // and no gap: a layout does not move by a float
        CHECK(addr(r.p) % (align * sizeof(float)) == 0);
        if (r.vec16) CHECK(addr(r.p) % 16 == 0);
        cursor = addr(r.p) + (r.floats + align - 1) / align * align * sizeof(float);
        CHECK(cursor <= hi);
    }
    CHECK(cursor + slack * sizeof(float) == hi);
}
#define CHECK_LAYOUT(call_base, call_null, regs, query, slack)                                        \
    do {                                                                                              \
        const auto Lb = call_base; const auto Ln = call_null;                                         \
        check_regions(regs(Lb), regs(Ln), Lb.total, Ln.total, query, 1, slack);                       \
    } while (0)

static void xfmr_regs(const XfmrWs& x, size_t M, Regs& r) {
    for (float* p : x.P) r.push_back({p, M * D_, true});
    for (float* p : x.SK) r.push_back({p, M * D_, true});
    for (float* p : x.Ps) r.push_back({p, M * D_, true});
    for (float* p : x.SKs) r.push_back({p, M * D_, true});
    r.push_back({x.qkv, 3 * M * D_, true}); r.push_back({x.att, M * D_, true}); r.push_back({x.hid, M * FF_, true});
    CHECK(x.qkv_floats == 3 * M * D_ && x.hid_floats == M * FF_);
}

static const int STEPS[] = {1, 50, 64, 65, 67, 1000};

static void check_denoiser() {
    for (int B2 : {1, 2, 256, 600}) for (int T : {1, 5, 8}) {
        std::snprintf(g_ctx, sizeof(g_ctx), "den forward B2 %d T %d", B2, T);
        const size_t M = (size_t)B2 * T;
        auto regs = [&](const DenForwardWs& L) { Regs r; xfmr_regs(L, M, r); r.push_back({L.part, 4 * M * D_, true}); return r; };
        CHECK_LAYOUT(den_forward_layout(WS_BASE, M), den_forward_layout(nullptr, M), regs, den_forward_ws_floats(B2, T), 0);
        float *x = nullptr, *xs = nullptr;
        den_loop_io(WS_BASE, (int)M, &x, &xs);
        const DenForwardWs L = den_forward_layout(WS_BASE, M);
        CHECK(x == L.P[0] && xs == L.Ps[0] && x == WS_BASE && xs == WS_BASE + 8 * M * D_);
        den_loop_io(nullptr, (int)M, &x, &xs);
        CHECK(x == nullptr && xs == nullptr);
    }
    for (int n : STEPS) {
        std::snprintf(g_ctx, sizeof(g_ctx), "den time n %d", n);
        auto regs = [&](const DenTimeWs& L) { return Regs{{L.h1, n * D_, true}, {L.temb, n * D_, true}, {L.semb, n * D_, true}}; };
        CHECK_LAYOUT(den_time_layout(WS_BASE, n), den_time_layout(nullptr, n), regs, 3 * n * D_, 0);
        CHECK(den_tables_floats(n) == (size_t)n * NL_ * 6 * D_);
    }
    for (int B2 : {1, 2, 256, 600}) for (int n : {0, 1, 50, 64, 1000}) for (int N : {1, 2, 77}) {
        std::snprintf(g_ctx, sizeof(g_ctx), "den text B2 %d n %d N %d", B2, n, N);
        const size_t R = (size_t)B2 * N, ctab = NL_ * n * (B2 + 1) * D_;
        auto ws_regs = [&](const DenTextWs& L) {
            if (N > 1) { CHECK(L.u == nullptr && L.u_floats == 0); return Regs{{L.rl, R * TD_, true}, {L.tn, R * D_, true}, {L.key, R * D_, true}, {L.val, R * D_, true}}; }
            CHECK(L.key == nullptr && L.val == nullptr && L.u_floats == ctab);
            return Regs{{L.rl, R * TD_, true}, {L.tn, NL_ * B2 * D_, true}, {L.u, ctab, true}};
        };
        CHECK_LAYOUT(den_text_layout(WS_BASE, B2, n, N), den_text_layout(nullptr, B2, n, N), ws_regs, den_text_ws_floats(B2, n, N), 0);
        auto cache_regs = [&](const DenTextCache& L) {
            if (N > 1) { CHECK(L.nval == nullptr && L.ctab == nullptr); return Regs{{L.tproj, R * D_, true}, {L.tkv, NL_ * R * 2 * D_, true}, {L.catt, NL_ * B2 * 4 * 64 * 64, true}}; }
            CHECK(L.catt == nullptr);
            return Regs{{L.tproj, R * D_, true}, {L.tkv, NL_ * R * 2 * D_, true}, {L.nval, NL_ * B2 * D_, true}, {L.ctab, ctab, true}};
        };
        CHECK_LAYOUT(den_text_cache_layout(WS_BASE, B2, n, N), den_text_cache_layout(nullptr, B2, n, N), cache_regs, den_text_cache_floats(B2, n, N), 0);
        // the accessors of the forward pass and the loop kernel: the same places, whatever the step count
        const DenTextCache L = den_text_cache_layout(WS_BASE, B2, n, N);
        CHECK(den_cache_tkv(WS_BASE, B2, N) == L.tkv && L.tkv == WS_BASE + R * D_);
        CHECK(den_cache_ctab(WS_BASE, B2, N) == (N > 1 ? L.catt : L.ctab));
        CHECK(den_cache_ctab(WS_BASE, B2, N) == WS_BASE + R * D_ + NL_ * R * 2 * D_ + (N > 1 ? 0 : NL_ * B2 * D_));
        CHECK(den_cache_tkv(nullptr, B2, N) == nullptr && den_cache_ctab(nullptr, B2, N) == nullptr);
    }
    for (int B : {1, 7, 128}) for (int T : {1, 5, 8}) for (int N : {1, 2, 77}) {
        std::snprintf(g_ctx, sizeof(g_ctx), "lca B %d T %d N %d", B, T, N);
        const size_t R = (size_t)B * N, M = (size_t)B * T;
        auto regs = [&](const LcaWs& L) {
            return Regs{{L.tn, R * D_, true}, {L.key, R * D_, true}, {L.val, R * D_, true}, {L.catt, (size_t)B * 4 * 64 * 64, true},
                        {L.xn, M * D_, true}, {L.q, M * D_, true}, {L.semb, B * D_, true}, {L.mod, B * 2 * D_, true}};
        };
        CHECK_LAYOUT(lca_layout(WS_BASE, B, T, N), lca_layout(nullptr, B, T, N), regs, linear_cross_attention_ws_floats(B, T, N), 0);
    }
}

static void check_vae() {
    // rows around DEC_SMALL_ROWS = 4096 (64 * 64, 65 * 63, 241 * 17), odd ragged totals, the benchmark's 128 x 196
    const size_t rows[] = {1, 63, 64, 65, 480, 4095, 4096, 4097, 12345, 25088};
    for (int B : {1, 8, 128, 241}) for (size_t M : rows) for (int T : {1, 5, 8}) {
        std::snprintf(g_ctx, sizeof(g_ctx), "decoder B %d rows %zu T %d", B, M, T);
        const size_t kv = (size_t)T * B * 2 * D_, gu = (size_t)B * 4 * T * (2 * D_ + 1);
        auto regs = [&](const DecWs& L) {
            Regs r; xfmr_regs(L, M, r);
            CHECK(L.kv_layer == kv && L.gu_layer == gu && gu == dec_cross_ws_floats(B, T));
            r.push_back({L.kv, NL_ * kv, true}); r.push_back({L.guws, NL_ * gu, true}); r.push_back({L.row_out, round64(M), false});
            r.push_back({L.pex, MAXF_ * D_, true}); r.push_back({L.pexs, MAXF_ * D_, true}); r.push_back({L.qkv0, MAXF_ * 3 * D_, true});
            return r;
        };
        CHECK_LAYOUT(dec_layout(WS_BASE, B, M, T), dec_layout(nullptr, B, M, T), regs, dec_ws_floats(B, M, T), 0);
    }
    for (int B : {1, 3, 8, 128}) for (int F : {1, 60, 196, 208}) for (int T : {1, 5, 8}) for (int C : {1, 251, 263}) {
        if (2 * T + F > LADIFF_MAX_FRAMES) continue;
        std::snprintf(g_ctx, sizeof(g_ctx), "encoder B %d F %d T %d C %d", B, F, T, C);
        const size_t M = (size_t)B * (2 * T + F), Cp = (C + 31) / 32 * 32;
        CHECK((int)Cp == pad32(C));
        auto regs = [&](const EncWs& L) {
            Regs r; xfmr_regs(L, M, r);
            r.push_back({L.featp, (size_t)B * F * Cp, true}); r.push_back({L.wskel, D_ * Cp, true}); r.push_back({L.emb, (size_t)B * F * D_, true});
            r.push_back({L.keybits, (size_t)B * 8 + 64, false});
            return r;
        };
        CHECK_LAYOUT(enc_layout(WS_BASE, B, F, T, C), enc_layout(nullptr, B, F, T, C), regs, enc_ws_floats(B, F, T, C), 0);
    }
}

static void check_clip() {
    // rows around CLIP_SMALL_ROWS = 256 and CLIP_FC2_KPARTS_MAX_ROWS
    for (int B : {1, 4, 128}) for (int M : {1, 4, 128, 255, 256, 257, 2260, CLIP_FC2_KPARTS_MAX_ROWS - 1, CLIP_FC2_KPARTS_MAX_ROWS, CLIP_FC2_KPARTS_MAX_ROWS + 1, 9856}) {
        if (M < B) continue;
        std::snprintf(g_ctx, sizeof(g_ctx), "clip B %d rows %d", B, M);
        const size_t W = 768, MW = M * W;
        // the plane space, once more: [12][M][768] up to 256 rows, then the larger of that at 256 rows and [4][min(M, 8192)][768]
        const size_t planes = M <= 256 ? 12 * MW : (12 * 256 * W > 4 * W * (M < 8192 ? M : 8192) ? 12 * 256 * W : 4 * W * (M < 8192 ? M : 8192));
        CHECK(clip_plane_floats(M) == planes);
        auto regs = [&](const ClipWs& L) {
            return Regs{{L.x, MW, true}, {L.x2, MW, true}, {L.h, MW, true}, {L.qkv, 3 * MW, true}, {L.att, MW, true}, {L.mlp, 4 * MW, true},
                        {L.planes, planes, true}, {L.pooled, B * W, true}, {L.eos, (size_t)B + 64, false}};
        };
        CHECK_LAYOUT(clip_layout(WS_BASE, B, M), clip_layout(nullptr, B, M), regs, clip_ws_floats_rows(B, M), 0);
    }
    for (int B : {1, 16, 128}) for (int L : {1, 2, 16, 77}) CHECK(clip_ws_floats(B, L) == clip_ws_floats_rows(B, B * L));
}

static void check_gru(float* base, int B, int T, size_t Hs) {
    auto regs = [&](const GruHeadWs& L) {
        return Regs{{L.gi, 2 * B * T * 3 * Hs, true}, {L.gh, 2 * B * 3 * Hs, true}, {L.h, 2 * B * Hs, true}, {L.cat, B * 2 * Hs, true}, {L.hid, B * Hs, true}, {L.hidn, B * Hs, true}};
    };
    const GruHeadWs Lb = gru_head_layout(base, B, T, (int)Hs), Ln = gru_head_layout(nullptr, B, T, (int)Hs);
    Regs rb = regs(Lb);
    for (Reg& r : rb) r.p = WS_BASE + (static_cast<const float*>(r.p) - base);      // as if carved at the base: the sub-scratch starts inside a workspace
    check_regions(rb, regs(Ln), Lb.total, Ln.total, gru_head_floats(B, T, (int)Hs), 1, 64);
}

static void check_t2m() {
    for (int B : {1, 3, 32}) for (int F : {4, 5, 7, 196, 224}) for (int Cin : {1, 247, 259}) {
        std::snprintf(g_ctx, sizeof(g_ctx), "t2m movement B %d F %d Cin %d", B, F, Cin);
        const size_t T1 = F / 2, T2 = T1 / 2, K1 = (4 * Cin + 31) / 32 * 32, Hm = 512;
        auto regs = [&](const T2mMoveWs& L) {
            return Regs{{L.a1, B * T1 * K1, true}, {L.w1, Hm * K1, true}, {L.y1, B * T1 * Hm, true}, {L.a2, B * T2 * 4 * Hm, true}, {L.y2, B * T2 * Hm, true}};
        };
        const auto Lb = t2m_move_layout(WS_BASE, B, F, Cin); const auto Ln = t2m_move_layout(nullptr, B, F, Cin);
        check_regions(regs(Lb), regs(Ln), Lb.total, Ln.total, t2m_move_ws_floats(B, F, Cin), 1, 64);
    }
    for (int B : {1, 3, 32, 128}) for (int T : {1, 20, 49, 56, 77}) {
        std::snprintf(g_ctx, sizeof(g_ctx), "t2m motion B %d T %d", B, T);
        const size_t M = (size_t)B * T;
        auto mregs = [&](const T2mMotionWs& L) { return Regs{{L.emb, M * 1024, true}, {L.gru, gru_head_floats(B, T, 1024), true}}; };
        CHECK_LAYOUT(t2m_motion_layout(WS_BASE, B, T), t2m_motion_layout(nullptr, B, T), mregs, t2m_motion_ws_floats(B, T), 0);
        check_gru(t2m_motion_layout(WS_BASE, B, T).gru, B, T, 1024);
        std::snprintf(g_ctx, sizeof(g_ctx), "t2m text B %d L %d", B, T);
        const size_t Kp = 32, Kw = 320;
        auto tregs = [&](const T2mTextWs& L) {
            return Regs{{L.posp, M * Kp, true}, {L.wpos, 300 * Kp, true}, {L.wordp, M * Kw, true}, {L.winp, 512 * Kw, true}, {L.inp, M * Kw, true},
                        {L.emb, M * 512, true}, {L.gru, gru_head_floats(B, T, 512), true}};
        };
        CHECK_LAYOUT(t2m_text_layout(WS_BASE, B, T), t2m_text_layout(nullptr, B, T), tregs, t2m_text_ws_floats(B, T), 0);
        check_gru(t2m_text_layout(WS_BASE, B, T).gru, B, T, 512);
    }
}

static void check_reverse() {
    for (int B : {1, 3, 128, 300}) for (int T : {1, 5, 8}) for (int n : STEPS) for (int N : {1, 2, 77}) {
        std::snprintf(g_ctx, sizeof(g_ctx), "reverse B %d T %d n %d N %d", B, T, n, N);
        const int B2 = 2 * B, wcap = n < 64 ? n : 64;
        auto regs = [&](const ReverseWs& r) {
            return Regs{{r.d_step, 64, false}, {r.tables, den_tables_floats(n), true}, {r.cache, den_text_cache_floats(B2, wcap, N), true},
                        {r.latents, (size_t)B * T * D_, true}, {r.eps, (size_t)B2 * T * D_, true}, {r.fwd, r.fwd_floats, true},
                        {r.sys, sys_ws_floats(B, T), true}, {r.cws, r.cws_floats, true}};
        };
        const ReverseWs rb = carve_reverse(WS_BASE, B, T, n, N), rn = carve_reverse(nullptr, B, T, n, N);
        CHECK(rb.total_bytes % sizeof(float) == 0 && rb.fwd_floats == rn.fwd_floats && rb.cws_floats == rn.cws_floats);
        check_regions(regs(rb), regs(rn), rb.total_bytes / sizeof(float), rn.total_bytes / sizeof(float), rb.total_bytes / sizeof(float), 64, 0);
        CHECK(rb.sys == WS_BASE + rb.sys_off && rn.sys_off == rb.sys_off);
        // the shared region serves the time tables, the static text scratch and the forward pass; the c-table builder gets all layers' rows
        CHECK(rb.fwd_floats >= den_forward_ws_floats(B2, T) && rb.fwd_floats >= den_time_layout(nullptr, n).total);
        CHECK(rb.fwd_floats >= den_text_ws_floats(B2, 0, N) && rb.fwd_floats >= den_text_ws_floats(B2, 1, N));
        CHECK(rb.cws_floats == NL_ * wcap * (B2 + 1) * D_);
        CHECK(rb.window == rn.window && rb.window >= 1 && rb.window <= wcap && n % rb.window == 0);
    }
}

int main() {
    check_denoiser();
    check_vae();
    check_clip();
    check_t2m();
    check_reverse();
    if (g_failed) { std::printf("workspace_check: %d checks failed\n", g_failed); return 1; }
    std::printf("workspace_check: ok\n");
    return 0;
}
