// What the host sequencers (decoder.hip, encoder.hip, clip.hip, denoiser.hip) share: an activation with its S-format twin, a layer's weights
// as the current mode reads them, the argument builders of a projection, of the skip-connection concat and of GEMM + LayerNorm.  Host code
// only: plain structs and inline functions over the launchers' argument structs - no kernel, no allocation, no indirect call.
#pragma once
#include "gemm.h"
#include "gemm_kr.h"
#include "kernels.h"
#include "weights.h"

namespace ladiff {

// argument builders of the two small-GEMM launchers: one dense [N][K] weight, activations with their own row strides
inline GemmArgs lin(const float* A, int lda, const float* W, const float* bias, float* Y, int ldy, int M, int N, int K, int act = ACT_NONE) {
    GemmArgs g;
    g.A = A; g.lda = lda; g.W = W; g.ldw = K; g.bias = bias; g.Y = Y; g.ldy = ldy; g.M = M; g.N = N; g.K = K; g.act = act;
    return g;
}
inline GemmArgs lin(const float* A, int lda, const LinearW& l, float* Y, int ldy, int M, int N, int K, int act = ACT_NONE) {
    return lin(A, lda, l.w, l.b, Y, ldy, M, N, K, act);
}
inline KrArgs kr(const float* A, int lda, const float* W, const float* b, float* Y, int ldy, int M, int N, int K, int act = ACT_NONE) {
    KrArgs g;
    g.A = A; g.lda = lda; g.W = W; g.ldw = K; g.bias = b; g.Y = Y; g.ldy = ldy; g.M = M; g.N = N; g.K = K; g.act = act;
    return g;
}

struct Seq { bool sp; int M; hipStream_t s; };      // one call: sp = f16x3 mode (S-format operands and weight matrices), M rows, the caller's stream
// An activation and its S-format twin.  As a result: where a launch writes the fp32 rows and / or the twin (either may be null).
struct Twin {
    float* f = nullptr;      // fp32 rows: what residual and LayerNorm consumers read
    float* s = nullptr;      // S-format twin: what a matrix product reads in f16x3 mode; null in fp32 mode
    const float* op() const { return s != nullptr ? s : f; }      // the side a matrix product reads in the current mode
};
// a buffer that only matrix products read (attention output, hidden rows): S-format rows in f16x3 mode, fp32 rows otherwise
inline Twin operand_only(bool sp, float* p) { return sp ? Twin{nullptr, p} : Twin{p, nullptr}; }
// the tensors of a workspace layout (workspace.h keeps `P` / `Ps`, `SK` / `SKs` as fields) as pairs; fp32 mode has no twins
inline Twin pair(bool sp, float* f, float* s) { return Twin{f, sp ? s : nullptr}; }
template <int N> inline void pair_up(bool sp, float* const (&f)[N], float* const (&s)[N], Twin (&out)[N]) {
    for (int i = 0; i < N; ++i) out[i] = pair(sp, f[i], s[i]);
}

// A weight in its two tables: the matrix as the MFMA of the current mode reads it (from the S-format table in f16x3 mode), bias and
// LayerNorm from the fp32 table.  mfma_table picks the table the matrices come from; mixed() puts its matrices into a copy of the fp32
// entry, so a sequencer holds ONE `L` per layer.  (The decoder's cross-attention weights stay fp32: its prologue folds them in fp32.)
template <class W> inline const W& mfma_table(const W& w, const W* w_split) { return w_split != nullptr ? *w_split : w; }
inline LinearW mixed(LinearW l, const LinearW& m) { l.w = m.w; return l; }
inline MhaW mixed(MhaW a, const MhaW& m) { a.in_w = m.in_w; a.out_w = m.out_w; return a; }
template <class LayerW> inline LayerW mixed(LayerW L, const LayerW& m) {      // DecLayerW, EncLayerW (the other layers: the overloads below)
    L.self_attn = mixed(L.self_attn, m.self_attn); L.lin1 = mixed(L.lin1, m.lin1); L.lin2 = mixed(L.lin2, m.lin2);
    return L;
}
inline DenLayerW mixed(DenLayerW L, const DenLayerW& m) {
    L.sa_attn = mixed(L.sa_attn, m.sa_attn); L.sa_lin1 = mixed(L.sa_lin1, m.sa_lin1); L.sa_lin2 = mixed(L.sa_lin2, m.sa_lin2);
    L.ca_query = mixed(L.ca_query, m.ca_query); L.ca_proj.out = mixed(L.ca_proj.out, m.ca_proj.out);
    L.ffn1 = mixed(L.ffn1, m.ffn1); L.ffn2 = mixed(L.ffn2, m.ffn2); L.ffn_proj.out = mixed(L.ffn_proj.out, m.ffn_proj.out);
    return L;
}
inline ClipLayerW mixed(ClipLayerW L, const ClipLayerW& m) {
    L.q = mixed(L.q, m.q); L.k = mixed(L.k, m.k); L.v = mixed(L.v, m.v); L.o = mixed(L.o, m.o); L.fc1 = mixed(L.fc1, m.fc1); L.fc2 = mixed(L.fc2, m.fc2);
    return L;
}
inline LinearW in_proj(const MhaW& a) { return {a.in_w, a.in_b}; }
inline LinearW out_proj(const MhaW& a) { return {a.out_w, a.out_b}; }

// y = act(x . W^T + b) (+ res, row stride D) over c.M rows in the current mode: x's operand side, W as mixed() gives it, the fp32 result
// to y.f and / or its twin to y.s.  "f16x3 mode writes the hidden rows only as Ys" is y = operand_only(sp, hid).
template <class Args> inline Args in_mode(const Seq& c, Args g, Twin y, const float* res) {
    g.Ys = y.s; g.split = c.sp ? 1 : 0; g.res = res; g.ldres = res != nullptr ? D : 0;
    return g;
}
inline GemmArgs proj(const Seq& c, Twin x, int K, const LinearW& W, Twin y, int ldy, int N, int act = ACT_NONE, const float* res = nullptr) {
    return in_mode(c, lin(x.op(), K, W, y.f, ldy, c.M, N, K, act), y, res);
}
inline KrArgs proj_kr(const Seq& c, Twin x, int K, const LinearW& W, Twin y, int ldy, int N, int act = ACT_NONE, const float* res = nullptr) {
    return in_mode(c, kr(x.op(), K, W.w, W.b, y.f, ldy, c.M, N, K, act), y, res);
}

// The skip connection x = linear_blocks([x | skip]) (cross_attention.py:79-82, :140-142): K = 512 as two segments of 256 columns, one
// helper per launcher.  skip_kr leaves the two partial planes in `planes` (no bias: the caller's row pass sums them and adds it).
template <class Args> inline Args concat(Args g, const float* skip) { g.lda = D; g.A2 = skip; g.lda2 = D; g.K1 = D; return g; }
inline int skip_gemm(const Seq& c, Twin x, Twin skip, const LinearW& W, Twin y) {
    return launch_gemm(concat(proj(c, x, 2 * D, W, y, D, D), skip.op()), c.s);
}
inline int skip_kr(const Seq& c, Twin x, Twin skip, const LinearW& W, float* planes) {
    return launch_gemm_kr(concat(proj_kr(c, x, 2 * D, LinearW{W.w, nullptr}, Twin{planes, nullptr}, D, D), skip.op()), c.s);
}
inline int skip_rowln(const Seq& c, Twin x, Twin skip, const LinearW& W, Twin y) {      // f16x3 mode only (gemm_rowln.hip)
    RowLnArgs g;
    g.A = x.s; g.W = W.w; g.ldw = 2 * D; g.bias = W.b; g.Y = y.f; g.Ys = y.s; g.ldy = D; g.M = c.M; g.K = 2 * D;
    return launch_gemm_rowln(concat(g, skip.s), c.s);
}

// row pass: the sum of S planes of `src` (+ bias, + res), LayerNorm n (or none: RED_PLAIN) -> out; the caller adds what its mode reads
inline RedArgs red(const Seq& c, const float* src, int S, const float* bias, const float* res, const NormW* n, Twin out) {
    RedArgs r;
    r.P = src; r.S = S; r.M = c.M; r.bias = bias; r.res = res; r.out = out.f; r.outs = out.s;
    if (n != nullptr) { r.mode = RED_LN; r.g = n->g; r.b = n->b; }
    return r;
}

// dst = LN(res + x . W^T + b), then a second LayerNorm n2 if given.  fp32 mode: all of it in the GEMM's epilogue.  f16x3 mode: the GEMM
// (+ residual) in place, then the LayerNorm row pass that also writes the twin; n2 rides in that pass (ln2_same_pass, the decoder) or is a
// row pass of its own (the encoder) - one launch more, kept as each tower had it.
inline int gemm_ln(const Seq& c, Twin x, int K, const LinearW& W, const float* res, const NormW& n1, const NormW* n2, Twin dst, bool ln2_same_pass) {
    GemmArgs g = proj(c, x, K, W, Twin{dst.f, nullptr}, D, D, ACT_NONE, res);
    if (!c.sp) {
        g.ln_g = n1.g; g.ln_b = n1.b;
        if (n2 != nullptr) { g.ln2_g = n2->g; g.ln2_b = n2->b; }
        return launch_gemm(g, c.s);
    }
    LADIFF_TRY(launch_gemm(g, c.s));
    RedArgs r = red(c, dst.f, 1, nullptr, nullptr, &n1, Twin{dst.f, nullptr});
    if (n2 != nullptr && ln2_same_pass) { r.g2 = n2->g; r.b2 = n2->b; }
    else if (n2 != nullptr) { LADIFF_TRY(launch_reduce_rows(r, c.s)); r.g = n2->g; r.b = n2->b; }
    r.outs = dst.s;
    return launch_reduce_rows(r, c.s);
}

}  // namespace ladiff
