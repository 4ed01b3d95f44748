// Workspace layouts: ONE carve per workspace-taking entry, read by both its *_workspace_bytes query (null base) and its sequencing
// function (the caller's base).  A layout function hands out consecutive regions with one Carver and returns a record of the region
// pointers plus `total` floats; the query is layout(nullptr, dims).total, so a buffer that is added, resized or moved changes both
// at once.  The loop kernel's own workspace has had this form from the start (sys_layout, systolic_plan.h).
// Plain C++17: no device code and no HIP header, so that tests/workspace_check.cpp holds every layout to its properties without a GPU.
#pragma once
#include <cstddef>
#include <cstdint>

#include "systolic_plan.h"      // sys_ws_floats (the reverse loop embeds the pipeline's workspace)
#include "weights.h"

namespace ladiff {

// Hands out consecutive regions of `base` and counts floats.  A null base yields null pointers and the same count (the queries): no
// arithmetic on a null pointer.  Every region's size is rounded up to `align` floats (1 = exact sizes).
struct Carver {
    float* base;
    size_t align, off = 0;
    explicit Carver(float* b, size_t a = 1) : base(b), align(a) {}
    float* take(size_t floats) {
        float* p = base ? base + off : nullptr;
        off += (floats + align - 1) / align * align;
        return p;
    }
};
inline int pad32(int c) { return (c + 31) / 32 * 32; }

// ------------------------------------------------------------------ shared transformer scratch (denoiser, LA-VAE decoder and encoder)
// M rows: x ping-pong / residual planes P, skip stack SK, their S-format twins (f16x3 mode; fp32 mode leaves them unused), q|k|v,
// attention output, hidden rows.  `qkv` and `hid` are re-used by later stages of a layer: their sizes are part of the record.
struct XfmrWs {
    float *P[4], *SK[NSKIP], *Ps[4], *SKs[NSKIP], *qkv, *att, *hid;
    size_t qkv_floats, hid_floats;
};
inline void carve_xfmr(Carver& c, size_t M, XfmrWs& x) {
    const size_t MD = M * D;
    for (float*& p : x.P) p = c.take(MD);
    for (float*& p : x.SK) p = c.take(MD);
    for (float*& p : x.Ps) p = c.take(MD);
    for (float*& p : x.SKs) p = c.take(MD);
    x.qkv_floats = 3 * MD; x.hid_floats = M * FF;
    x.qkv = c.take(x.qkv_floats);
    x.att = c.take(MD);
    x.hid = c.take(x.hid_floats);
}

// ------------------------------------------------------------------ denoiser
// time-table layout: tables[step][layer][1536] = { ca scale|shift (512), ffn scale|shift (512), time-token K|V (512) }
constexpr int DEN_OFF_CA_MOD = 0;
constexpr int DEN_OFF_FFN_MOD = 2 * D;
constexpr int DEN_OFF_TIME_KV = 4 * D;
constexpr int DEN_LAYER_STRIDE = 6 * D;
constexpr int DEN_STEP_STRIDE = NL * DEN_LAYER_STRIDE;
inline size_t den_tables_floats(int n_steps) { return (size_t)n_steps * DEN_STEP_STRIDE; }

struct DenForwardWs : XfmrWs { float* part; size_t total; };      // part: split-K partial planes [4][M][256]
inline DenForwardWs den_forward_layout(float* ws, size_t M) {
    DenForwardWs L;
    Carver c(ws);
    carve_xfmr(c, M, L);
    L.part = c.take(4 * M * D);
    L.total = c.off;
    return L;
}
inline size_t den_forward_ws_floats(int B2, int T) { return den_forward_layout(nullptr, (size_t)B2 * T).total; }

// time-table scratch of n steps: SiLU(linear_1(sinusoid)) | time_emb | SiLU(time_emb)
struct DenTimeWs { float *h1, *temb, *semb; size_t total; };
inline DenTimeWs den_time_layout(float* ws, int n) {
    DenTimeWs L;
    Carver c(ws);
    L.h1 = c.take((size_t)n * D); L.temb = c.take((size_t)n * D); L.semb = c.take((size_t)n * D);
    L.total = c.off;
    return L;
}

// text-cache scratch.  One text token: relu(text) | per-layer LN(text projection) [NL][B2][256] | c-table inputs of all layers for n
// steps (the per-layer launches are batched; n = 0: the step-invariant part alone).  ntxt > 1: relu(text) | LN | key | value of B2 ntxt rows.
struct DenTextWs { float *rl, *tn, *u, *key, *val; size_t u_floats, total; };
inline DenTextWs den_text_layout(float* ws, int B2, int n, int ntxt) {
    DenTextWs L{};
    Carver c(ws);
    const size_t R = (size_t)B2 * ntxt;
    L.rl = c.take(R * TEXT_DIM);
    if (ntxt > 1) {
        L.tn = c.take(R * D); L.key = c.take(R * D); L.val = c.take(R * D);
    } else {
        L.tn = c.take((size_t)NL * B2 * D);
        L.u_floats = (size_t)NL * n * (B2 + 1) * D;
        L.u = c.take(L.u_floats);
    }
    L.total = c.off;
    return L;
}
inline size_t den_text_ws_floats(int B2, int n_steps, int ntxt = 1) { return den_text_layout(nullptr, B2, n_steps, ntxt).total; }

// text cache, one text token:  [B2,256] emb_proj(text) | [9][B2,512] text K|V | [9][B2,256] LN(value) rows | [9][n][B2+1,256] c table
// ntxt > 1 (linear_ca.hip):    [B2 N,256] projected tokens | [9][B2 N,512] K|V | [9][B2][4][64][64] key^T value matrices (`catt`)
struct DenTextCache { float *tproj, *tkv, *nval, *ctab, *catt; size_t total; };
inline DenTextCache den_text_cache_layout(float* cache, int B2, int n, int ntxt) {
    DenTextCache L{};
    Carver c(cache);
    const size_t R = (size_t)B2 * ntxt;
    L.tproj = c.take(R * D);
    L.tkv = c.take((size_t)NL * R * 2 * D);
    if (ntxt > 1) {
        L.catt = c.take((size_t)NL * B2 * H * DH * DH);
    } else {
        L.nval = c.take((size_t)NL * B2 * D);
        L.ctab = c.take((size_t)NL * n * (B2 + 1) * D);
    }
    L.total = c.off;
    return L;
}
inline size_t den_text_cache_floats(int B2, int n_steps, int ntxt = 1) { return den_text_cache_layout(nullptr, B2, n_steps, ntxt).total; }
// the two parts of the cache that the forward pass and the loop kernel read (their places do not depend on the step count)
inline const float* den_cache_tkv(const float* cache, int B2, int ntxt) {
    return den_text_cache_layout(const_cast<float*>(cache), B2, 0, ntxt).tkv;
}
inline const float* den_cache_ctab(const float* cache, int B2, int ntxt) {      // ntxt > 1: the key^T value matrices
    const DenTextCache L = den_text_cache_layout(const_cast<float*>(cache), B2, 0, ntxt);
    return ntxt > 1 ? L.catt : L.ctab;
}
// the buffer of the forward workspace that holds both the network input and the last layer's output, and its S-format twin
inline void den_loop_io(float* ws, int rows, float** x, float** xs) {
    const DenForwardWs L = den_forward_layout(ws, (size_t)rows);
    *x = L.P[0]; *xs = L.Ps[0];
}

// one literal ca_block (linear_cross_attention): R = B N text rows, M = B T latent rows
struct LcaWs { float *tn, *key, *val, *catt, *xn, *q, *semb, *mod; size_t total; };
inline LcaWs lca_layout(float* ws, int B, int T, int N) {
    LcaWs L;
    Carver c(ws);
    const size_t R = (size_t)B * N, M = (size_t)B * T;
    L.tn = c.take(R * D); L.key = c.take(R * D); L.val = c.take(R * D);
    L.catt = c.take((size_t)B * H * DH * DH);
    L.xn = c.take(M * D); L.q = c.take(M * D);
    L.semb = c.take((size_t)B * D); L.mod = c.take((size_t)B * 2 * D);
    L.total = c.off;
    return L;
}
inline size_t linear_cross_attention_ws_floats(int B, int T, int N) { return lca_layout(nullptr, B, T, N).total; }

// ------------------------------------------------------------------ LA-VAE decoder and encoder
// G | U | c of one layer's folded cross-attention (dec_cross.hip)
inline size_t dec_cross_ws_floats(int B, int T) { return (size_t)B * H * T * (2 * D + 1); }

// M = B * F rows for the padded layout, or the sum of the lengths for the ragged one
struct DecWs : XfmrWs {
    float *kv, *guws;             // memory K | V and G | U | c of every layer: [NL] x kv_layer / gu_layer floats
    int32_t* row_out;             // ragged: place of each row in the padded output (rounded to 64: what follows is read 16 bytes at a time and by LDS-DMA)
    float *pex, *pexs, *qkv0;     // layer 0: pe[:F] (+ S-format twin) and its in_proj, shared by all samples
    size_t kv_layer, gu_layer, total;
};
inline DecWs dec_layout(float* ws, int B, size_t M, int T) {
    DecWs L;
    Carver c(ws);
    carve_xfmr(c, M, L);
    L.kv_layer = (size_t)T * B * 2 * D; L.gu_layer = dec_cross_ws_floats(B, T);
    L.kv = c.take(NL * L.kv_layer);
    L.guws = c.take(NL * L.gu_layer);
    L.row_out = reinterpret_cast<int32_t*>(c.take((M + 63) / 64 * 64));
    L.pex = c.take((size_t)LADIFF_MAX_FRAMES * D);
    L.pexs = c.take((size_t)LADIFF_MAX_FRAMES * D);
    L.qkv0 = c.take((size_t)LADIFF_MAX_FRAMES * 3 * D);
    L.total = c.off;
    return L;
}
inline size_t dec_ws_floats(int B, size_t rows, int T) { return dec_layout(nullptr, B, rows, T).total; }

// M = B (2 T + F) rows; features and skel_embedding padded to pad32(C) columns, the embedded frames, one key map per sample
struct EncWs : XfmrWs { float *featp, *wskel, *emb; uint32_t* keybits; size_t total; };
inline EncWs enc_layout(float* ws, int B, int F, int T, int C) {
    EncWs L;
    Carver c(ws);
    const size_t Cp = pad32(C);
    carve_xfmr(c, (size_t)B * (2 * T + F), L);
    L.featp = c.take((size_t)B * F * Cp);
    L.wskel = c.take((size_t)D * Cp);
    L.emb = c.take((size_t)B * F * D);
    L.keybits = reinterpret_cast<uint32_t*>(c.take((size_t)B * 8 + 64));
    L.total = c.off;
    return L;
}
inline size_t enc_ws_floats(int B, int F, int T, int C) { return enc_layout(nullptr, B, F, T, C).total; }

// ------------------------------------------------------------------ stage-"vae" losses (vae_losses.hip)
// [blocks][3] fp64 partial sums (recons_feature, recons_joints, kl_motion), one fixed slot per workgroup of the first launch.  The
// workgroup count depends on the shapes alone (one per 256 16-byte chunks of the longest array, VAE_LOSS_MAX_BLOCKS at most), so the sums'
// bits do not depend on the device.  The base must be 8-byte aligned.
constexpr int VAE_LOSS_MAX_BLOCKS = 512;
struct VaeLossWs { double* part; int blocks; size_t total; };
inline VaeLossWs vae_losses_layout(float* ws, int B, int F, int C, int J, int T) {
    VaeLossWs L;
    Carver c(ws);
    size_t n = (size_t)B * F * C;
    for (size_t m : {(size_t)B * F * J * 3, (size_t)T * B * D})
        if (m > n) n = m;
    const size_t blocks = ((n + 3) / 4 + 255) / 256;
    L.blocks = blocks < 1 ? 1 : (blocks > VAE_LOSS_MAX_BLOCKS ? VAE_LOSS_MAX_BLOCKS : (int)blocks);
    L.part = reinterpret_cast<double*>(c.take((size_t)L.blocks * 3 * 2));
    L.total = c.off;
    return L;
}
inline size_t vae_losses_ws_floats(int B, int F, int C, int J, int T) { return vae_losses_layout(nullptr, B, F, C, J, T).total; }

// ------------------------------------------------------------------ stage "diffusion": forward with one timestep per sample
// (diffusion_stage.hip).  Everything is per SAMPLE, where the sampling loop's tables are per STEP:
//   sinus   [B2][768]          sinusoid of sample b's timestep
//   tables  [B2][9][1536]      the time tables with row = sample (den_tables_floats(B2): the step axis of the loop's layout)
//   cache   the step-invariant text cache (den_text_cache_layout with n = 0: no c table inside)
//   dctab   [9][B2][2][256]    "diagonal" c table: c[layer][b][0] for sample b's valid rows and c[layer][b][1] for its padded rows,
//                              both under sample b's OWN timestep - 2 B2 rows per layer where the loop's [n][B2 + 1] would be B2 (B2 + 1)
//   u       [9][B2][2][256]    inputs of the out-projection that yields dctab (S-format in f16x3 mode)
//   tws     scratch of denoiser_time_tables for B2 rows | xws  scratch of denoiser_text_static | fwd  the layers' scratch
// O(B2 T) in all; the regions do not share space (a few hundred KiB per sample at most).
struct DenPerSampleWs { float *sinus, *tables, *cache, *dctab, *u, *tws, *xws, *fwd; size_t tws_floats, xws_floats, fwd_floats, total; };
inline DenPerSampleWs den_per_sample_layout(float* ws, int B2, int T) {
    DenPerSampleWs L;
    Carver c(ws, 64);
    L.sinus = c.take((size_t)B2 * TEXT_DIM);
    L.tables = c.take(den_tables_floats(B2));
    L.cache = c.take(den_text_cache_floats(B2, 0, 1));
    L.dctab = c.take((size_t)NL * B2 * 2 * D);
    L.u = c.take((size_t)NL * B2 * 2 * D);
    L.tws_floats = den_time_layout(nullptr, B2).total;
    L.tws = c.take(L.tws_floats);
    L.xws_floats = den_text_ws_floats(B2, 0, 1);
    L.xws = c.take(L.xws_floats);
    L.fwd_floats = den_forward_ws_floats(B2, T);
    L.fwd = c.take(L.fwd_floats);
    L.total = c.off;
    return L;
}
inline size_t den_per_sample_ws_floats(int B2, int T) { return den_per_sample_layout(nullptr, B2, T).total; }

// ------------------------------------------------------------------ stage-"diffusion" loss (diffusion_stage.hip)
// [blocks] fp64 partial sums of (noise_pred - noise)^2, one fixed slot per workgroup of the first launch; the workgroup count depends on
// n alone (one per 256 16-byte chunks, DIFF_LOSS_MAX_BLOCKS at most).  The base must be 8-byte aligned.
constexpr int DIFF_LOSS_MAX_BLOCKS = 512;
struct DiffLossWs { double* part; int blocks; size_t total; };
inline DiffLossWs diffusion_losses_layout(float* ws, size_t n) {
    DiffLossWs L;
    Carver c(ws);
    const size_t blocks = ((n + 3) / 4 + 255) / 256;
    L.blocks = blocks < 1 ? 1 : (blocks > DIFF_LOSS_MAX_BLOCKS ? DIFF_LOSS_MAX_BLOCKS : (int)blocks);
    L.part = reinterpret_cast<double*>(c.take((size_t)L.blocks * 2));
    L.total = c.off;
    return L;
}

// ------------------------------------------------------------------ CLIP text tower
constexpr int CLIP_W = LADIFF_TEXT_DIM;    // 768
constexpr int CLIP_FF = 4 * CLIP_W;        // 3072
// Few rows (a demo.py call: the empty prompt + one prompt = ~40 rows; round 6): the 128-row tiles of the large-M GEMM leave N / 128 =
// 6 .. 24 workgroups, each walking the whole K - 45 us per GEMM whatever its size, 1.9 of a single prompt's 10 ms (profiles/r6/11_*).
// Up to CLIP_SMALL_ROWS rows the split mode's GEMMs run on the denoiser's K-resident 64x64 tiles instead (gemm_kr.hip: one 256-wide
// K slice per workgroup, K / 256 = 3 or 12 partial planes, 36 .. 144 workgroups that each move 64 KB) and a row pass sums the
// planes and applies bias / quick_gelu / residual: the same S-format operands and split products, summed per K slice.
constexpr int CLIP_SMALL_ROWS = 256;
constexpr int CLIP_PLANE_COLS = 12 * CLIP_W;   // floats per row of the partial planes: max over the GEMMs of (K / 256) * N = 3 * 3072 = 12 * 768 = 9216
// Many rows: fc2 (K = 3072, N = 768) is 6 column tiles x a few dozen row tiles - about one workgroup per CU, each walking 96 K stages with
// ONE stage in flight (70 us at 2,260 rows, most of it load latency nobody hides).  Its K range is cut in CLIP_FC2_KPARTS parts over
// blockIdx.y (GemmArgs::ksplit: four times the workgroups, two per CU hiding each other's stages) and the row pass sums the planes.
constexpr int CLIP_FC2_KPARTS = 4;
constexpr int CLIP_FC2_KPARTS_MAX_ROWS = 8192;  // beyond, the tiles alone fill the chip
// Plane space for M rows: the largest need of any regime a call with AT MOST M rows can land in (small-row planes up to CLIP_SMALL_ROWS
// rows, fc2's K parts up to CLIP_FC2_KPARTS_MAX_ROWS, none beyond), so that the workspace query never shrinks when the row count grows: a
// caller that sizes its workspace once for its largest batch is served at every smaller one.
inline size_t clip_plane_floats(int M) {
    const size_t small_rows = (size_t)(M < CLIP_SMALL_ROWS ? M : CLIP_SMALL_ROWS) * CLIP_PLANE_COLS;
    const size_t kparts = M > CLIP_SMALL_ROWS ? (size_t)(M < CLIP_FC2_KPARTS_MAX_ROWS ? M : CLIP_FC2_KPARTS_MAX_ROWS) * CLIP_FC2_KPARTS * CLIP_W : 0;
    return small_rows > kparts ? small_rows : kparts;
}
// M rows (B * L padded, or the ragged total): residual stream x, ping-pong with x2 across the two sub-blocks | LN output h (S-format in
// split mode) | q|k|v | attention | MLP hidden | partial planes ([K / 256][M][ld] of the small-row path, [CLIP_FC2_KPARTS][M][768] of
// fc2 otherwise; 16-byte aligned: every size before it is a multiple of 768 floats) | pooled rows | EOS positions
struct ClipWs { float *x, *x2, *h, *qkv, *att, *mlp, *planes, *pooled; int32_t* eos; size_t total; };
inline ClipWs clip_layout(float* ws, int B, int M) {
    ClipWs L;
    Carver c(ws);
    const size_t MW = (size_t)M * CLIP_W;
    L.x = c.take(MW); L.x2 = c.take(MW); L.h = c.take(MW);
    L.qkv = c.take(3 * MW);
    L.att = c.take(MW);
    L.mlp = c.take((size_t)M * CLIP_FF);
    L.planes = c.take(clip_plane_floats(M));
    L.pooled = c.take((size_t)B * CLIP_W);
    L.eos = reinterpret_cast<int32_t*>(c.take((size_t)B + 64));
    L.total = c.off;
    return L;
}
inline size_t clip_ws_floats_rows(int B, int total_rows) { return clip_layout(nullptr, B, total_rows).total; }
inline size_t clip_ws_floats(int B, int L) { return clip_ws_floats_rows(B, B * L); }

// ------------------------------------------------------------------ T2M evaluator encoders
constexpr int T2M_MOVE_H = 512, T2M_MOTION_H = 1024, T2M_TEXT_H = 512, T2M_WORD = 300, T2M_POS = 15;

// bidirectional GRU + co-embedding head over T steps of width Hs: gi [2][B][T][3H] | gh [2][B][3H] | h [2][B][H] | cat [B][2H] |
// hid [B][H] (the head's Linear output) | hidn [B][H] (its LayerNorm output) | 64 floats of slack the query has always carried
struct GruHeadWs { float *gi, *gh, *h, *cat, *hid, *hidn; size_t total; };
inline GruHeadWs gru_head_layout(float* ws, int B, int T, int Hs) {
    GruHeadWs L;
    Carver c(ws);
    L.gi = c.take((size_t)2 * B * T * 3 * Hs);
    L.gh = c.take((size_t)2 * B * 3 * Hs);
    L.h = c.take((size_t)2 * B * Hs);
    L.cat = c.take((size_t)B * 2 * Hs);
    L.hid = c.take((size_t)B * Hs);
    L.hidn = c.take((size_t)B * Hs);
    c.take(64);
    L.total = c.off;
    return L;
}
inline size_t gru_head_floats(int B, int T, int Hs) { return gru_head_layout(nullptr, B, T, Hs).total; }

// movement encoder, F -> T1 = F / 2 -> T2 = F / 4 frames: im2col rows [B T1, K1] | conv0 weight padded to K1 columns | [B T1, 512] |
// im2col rows [B T2, 2048] | [B T2, 512] | the same 64 floats of slack
struct T2mMoveWs { float *a1, *w1, *y1, *a2, *y2; size_t total; };
inline T2mMoveWs t2m_move_layout(float* ws, int B, int F, int Cin) {
    T2mMoveWs L;
    Carver c(ws);
    const int T1 = F / 2, T2 = T1 / 2, K1 = pad32(4 * Cin);
    L.a1 = c.take((size_t)B * T1 * K1);
    L.w1 = c.take((size_t)T2M_MOVE_H * K1);
    L.y1 = c.take((size_t)B * T1 * T2M_MOVE_H);
    L.a2 = c.take((size_t)B * T2 * 4 * T2M_MOVE_H);
    L.y2 = c.take((size_t)B * T2 * T2M_MOVE_H);
    c.take(64);
    L.total = c.off;
    return L;
}
inline size_t t2m_move_ws_floats(int B, int F, int Cin) { return t2m_move_layout(nullptr, B, F, Cin).total; }

struct T2mMotionWs { float *emb, *gru; size_t total; };           // [B T, 1024] | gru_head's scratch
inline T2mMotionWs t2m_motion_layout(float* ws, int B, int T) {
    T2mMotionWs L;
    Carver c(ws);
    L.emb = c.take((size_t)B * T * T2M_MOTION_H);
    L.gru = c.take(gru_head_floats(B, T, T2M_MOTION_H));
    L.total = c.off;
    return L;
}
inline size_t t2m_motion_ws_floats(int B, int T) { return t2m_motion_layout(nullptr, B, T).total; }

// text encoder, M = B L rows: POS one-hots padded [M, Kp] | pos_emb.weight padded [300, Kp] | word_embs padded [M, Kw] (residual of the
// pos GEMM) | input_emb.weight padded [512, Kw] | word_embs + pos_emb(pos_onehot) [M, Kw] | [M, 512] | gru_head's scratch
struct T2mTextWs { float *posp, *wpos, *wordp, *winp, *inp, *emb, *gru; size_t total; };
inline T2mTextWs t2m_text_layout(float* ws, int B, int L_) {
    T2mTextWs L;
    Carver c(ws);
    const size_t M = (size_t)B * L_, Kp = pad32(T2M_POS), Kw = pad32(T2M_WORD);
    L.posp = c.take(M * Kp);
    L.wpos = c.take(T2M_WORD * Kp);
    L.wordp = c.take(M * Kw);
    L.winp = c.take(T2M_TEXT_H * Kw);
    L.inp = c.take(M * Kw);
    L.emb = c.take(M * T2M_TEXT_H);
    L.gru = c.take(gru_head_floats(B, L_, T2M_TEXT_H));
    L.total = c.off;
    return L;
}
inline size_t t2m_text_ws_floats(int B, int L) { return t2m_text_layout(nullptr, B, L).total; }

// ------------------------------------------------------------------ whole reverse loop (ladiff_diffusion_reverse)
// The hoisted cross-attention table is [9][steps][2B+1][256] floats: 118 MB for 50 steps at B = 128, but 2.4 GB for a
// 1000-step DDPM schedule.  Long schedules are run window by window (the largest divisor of n_steps that is <= 64 and a
// multiple of 10, so that the step graphs unroll ten-fold; failing that the largest divisor <= 64 of any kind), the table rebuilt
// before each window from the per-layer LN(value) rows kept in the cache.  A window never exceeds REVERSE_WINDOW_MAX steps, and the
// carve reserves the table for min(n_steps, REVERSE_WINDOW_MAX) steps whatever the window: the workspace query is then non-decreasing
// in n_steps (a 65-step schedule used to keep a 65-step table and ask for more than a 1000-step one).  A schedule longer than 64 steps
// with few divisors pays in table rebuilds (a prime length rebuilds per step), not in memory.
constexpr int REVERSE_WINDOW_MAX = 64;
inline int reverse_window(int n) {
    if (n <= REVERSE_WINDOW_MAX) return n;
    for (int w = REVERSE_WINDOW_MAX; w >= 10; --w)
        if (n % w == 0 && w % 10 == 0) return w;
    for (int w = REVERSE_WINDOW_MAX; w > 1; --w)
        if (n % w == 0) return w;
    return 1;
}
// every region rounded to 64 floats
struct ReverseWs {
    float *tables, *cache, *latents, *eps, *fwd, *sys, *cws;
    int32_t* d_step;
    size_t fwd_floats, cws_floats, total_bytes, sys_off;      // sys_off: floats from the workspace base to `sys`
    int window;                            // steps whose c-table rows are resident at a time
};
inline ReverseWs carve_reverse(void* ws, int B, int T, int n, int ntxt = 1) {
    ReverseWs r;
    const int B2 = 2 * B;
    Carver c(static_cast<float*>(ws), 64);
    r.d_step = reinterpret_cast<int32_t*>(c.take(64));
    r.tables = c.take(den_tables_floats(n));
    r.window = reverse_window(n);
    const int wcap = n < REVERSE_WINDOW_MAX ? n : REVERSE_WINDOW_MAX;  // >= r.window; sized by it so that the query never shrinks with n
    r.cache = c.take(den_text_cache_floats(B2, wcap, ntxt));           // the c table is the cache's last part: r.window steps of it are used
    r.latents = c.take((size_t)B * T * D);
    r.eps = c.take((size_t)B2 * T * D);
    // one region serves, in turn, the time-table scratch, the text-cache scratch (static part) and the forward pass
    r.fwd_floats = den_forward_ws_floats(B2, T);
    for (size_t pre : {den_time_layout(nullptr, n).total, den_text_ws_floats(B2, 1, ntxt)})
        if (pre > r.fwd_floats) r.fwd_floats = pre;
    r.fwd = c.take(r.fwd_floats);
    r.sys_off = c.off;
    r.sys = c.take(sys_ws_floats(B, T));                               // block buffers, flags and stage table of the pipeline loop
    r.cws_floats = den_text_layout(nullptr, B2, wcap, 1).u_floats;     // scratch of the c-table builder (all layers' input rows)
    r.cws = c.take(r.cws_floats);
    r.total_bytes = c.off * sizeof(float);
    return r;
}

}  // namespace ladiff
