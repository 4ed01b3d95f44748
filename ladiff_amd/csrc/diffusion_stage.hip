// Stage "diffusion" outside the sampling loop (LADIFF.train_diffusion_forward, ladiff.py:874-1033, and _diffusion_process, :745-813):
//   q-sample            noisy = sqrt(acp[t_b]) z + sqrt(1 - acp[t_b]) noise          scheduler.add_noise + the LAD zeroing   :775-782
//   denoiser forward    with ONE TIMESTEP PER SAMPLE                                 self.denoiser(noisy, timesteps [B], ...) :785-794
//   inst_loss           mean (noise_pred - noise)^2 over every element               nn.MSELoss, losses/mld.py:69, :112
// The sampling loop's forward (denoiser.hip) reads one step counter per call in three places: the time token's K|V in self-attention,
// the hoisted cross-attention vector c added after norm2, and the (scale | shift) of the FFN's StylizationBlock.  The kernels here
// are the per-sample forms of those three row kernels - the table row is the GLOBAL sample index, the tables hold one row per sample
// (workspace.h, den_per_sample_layout) - plus the input kernel of the "diagonal" c table.  The GEMMs do not depend on the step and are
// the loop's own.  The kernels of the loop are not touched: they compile from the source they had.
#include "model.h"

namespace ladiff {

namespace {

constexpr int PS_ROWS_PER_BLOCK = 4;   // 256 threads = 4 waves = 4 rows of 256 floats, one f32x4 per lane (as rowops.hip)

// mean / rstd of a 256-wide row held as one f32x4 per lane: the arithmetic of rowops.hip's row_stats, restated here because that
// translation unit is the sampling loop's and stays as it is
__device__ __forceinline__ void ps_row_stats(const f32x4 v, float& mean, float& rstd) {
    const float s = wave_sum(v[0] + v[1] + v[2] + v[3]);
    mean = s * (1.f / 256.f);
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) { const float d = v[i] - mean; q += d * d; }
    q = wave_sum(q);
    rstd = rsqrtf(q * (1.f / 256.f) + LN_EPS);
}

// ------------------------------------------------------------------ diagonal c table: input rows
// u[layer][b][0] = SiLU(nval[layer][b] (1 + scale_b) + shift_b)     valid latent rows of sample b   (denoiser.hip, text cache)
// u[layer][b][1] = SiLU(beta[layer]    (1 + scale_b) + shift_b)     padded latent rows of sample b: LN(0) = beta, and the AdaLN of the
//                                                                   padded rows is sample b's too, because its timestep is
// rb (grid.y = layer): a = nval, g = beta, b = this layer's ca (scale | shift) of sample 0; samples are `row_stride` floats apart
__global__ __launch_bounds__(256) void ca_diag_input_kernel(const RowBatch rb, int row_stride, int M, int split_out) {
    const int row = blockIdx.x * PS_ROWS_PER_BLOCK + (threadIdx.x >> 6);       // row = 2 b + (padded ? 1 : 0)
    const int c = (threadIdx.x & 63) * 4;
    if (row >= M) return;
    const int k = blockIdx.y;
    const int b = row >> 1;
    const float* m = rb.b[k] + (size_t)b * row_stride;
    const f32x4 sc = ld4(m + c), sh = ld4(m + 256 + c);
    f32x4 v = (row & 1) ? ld4(rb.g[k] + c) : ld4(rb.a[k] + (size_t)b * D + c);
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = silu(v[i] * (1.f + sc[i]) + sh[i]);
    if (split_out) store_split4(rb.y[k] + (size_t)row * D, c, v);
    else st4(rb.y[k] + (size_t)row * D + c, v);
}

// ------------------------------------------------------------------ self-attention, time token per sample
// den_self_attn_kernel (attention.hip) with the time token's K|V taken from row `bg` of the tables, not from row *d_step
template <int T>
__global__ __launch_bounds__(256) void den_self_attn_ps_kernel(const float* __restrict__ qkv, const float* __restrict__ text_kv,
                                                               const float* __restrict__ tables, int kv_off, int row_stride,
                                                               const int32_t* __restrict__ counts, int b_off, float* __restrict__ out,
                                                               int split_out) {
    const int b2 = blockIdx.x;             // local sample: rows of qkv / out
    const int bg = b_off + b2;             // sample of the whole batch: text cache row, table row, counts
    const int col = threadIdx.x;           // = head * 64 + d
    float qv[T], kk[T + 2], vv[T + 2];
#pragma unroll
    for (int i = 0; i < T; ++i) {
        const float* r = qkv + ((size_t)b2 * T + i) * 768 + col;
        qv[i] = r[0] * 0.125f;
        kk[i] = r[256];
        vv[i] = r[512];
    }
    kk[T] = text_kv[(size_t)bg * 512 + col];
    vv[T] = text_kv[(size_t)bg * 512 + 256 + col];
    const float* tk = tables + (size_t)bg * row_stride + kv_off;
    kk[T + 1] = tk[col];
    vv[T + 1] = tk[256 + col];
    int nv = counts ? counts[bg] : T;
    nv = nv > T ? T : nv;
    __shared__ __attribute__((aligned(16))) float so[T * D];      // staged outputs for the S-format store
#pragma unroll
    for (int i = 0; i < T; ++i) {
        float s[T + 2];
        float m = -INFINITY;
#pragma unroll
        for (int j = 0; j < T + 2; ++j) {
            const float d = wave_sum(qv[i] * kk[j]);
            s[j] = (j < T && j >= nv) ? -INFINITY : d;
            m = fmaxf(m, s[j]);
        }
        float l = 0.f, o = 0.f;
#pragma unroll
        for (int j = 0; j < T + 2; ++j) {
            const float pv = expf(s[j] - m);
            l += pv;
            o += pv * vv[j];
        }
        if (split_out) so[i * D + col] = o / l;
        else out[((size_t)b2 * T + i) * D + col] = o / l;
    }
    if (split_out) {      // 16-byte units: 4 consecutive columns -> 8 B of hi + 8 B of lo
        __syncthreads();
        for (int u = threadIdx.x; u < T * (D / 4); u += 256) {
            const int r = u / (D / 4), c4 = (u % (D / 4)) * 4;
            store_split4(out + ((size_t)b2 * T + r) * D, c4, ld4(so + r * D + c4));
        }
    }
}

int launch_self_attention_ps(const float* qkv, const float* text_kv, const float* tables, int kv_off, int row_stride,
                             const int32_t* counts, int b_off, int b_n, int T, float* out, int split_out, hipStream_t s) {
    if (b_n == 0) return 0;
    const dim3 grid(b_n), block(256);
#define LADIFF_SA_CASE(TT)                                                                                                            \
    case TT:                                                                                                                          \
        hipLaunchKernelGGL(den_self_attn_ps_kernel<TT>, grid, block, 0, s, qkv, text_kv, tables, kv_off, row_stride, counts, b_off,  \
                           out, split_out);                                                                                           \
        break;
    switch (T) {
        LADIFF_SA_CASE(1) LADIFF_SA_CASE(2) LADIFF_SA_CASE(3) LADIFF_SA_CASE(4)
        LADIFF_SA_CASE(5) LADIFF_SA_CASE(6) LADIFF_SA_CASE(7) LADIFF_SA_CASE(8)
        default: return LADIFF_ERR_SHAPE;
    }
#undef LADIFF_SA_CASE
    LADIFF_LAUNCH_CHECK();
    return 0;
}

// ------------------------------------------------------------------ combine rows, table row per sample
// x = sum of the four split-K planes + bias (+ res), LayerNorm, then - with b = b_off + row / T -
//   ADD = true   y = LN(x) + dctab[b][row % T < counts[b] ? 0 : 1]        reduce_rows' RED_LN_ADD   (norm2 + the hoisted ca_block)
//   ADD = false  y = SiLU(LN(x) (1 + scale_b) + shift_b)                  reduce_rows' RED_LN_MOD   (the FFN's StylizationBlock)
// tab: ADD: this layer's [B2][2][256] rows; otherwise this layer's ffn (scale | shift) of sample 0, samples `row_stride` floats apart
struct PsRedArgs {
    const float* P; const float* bias; const float* res; const float* g; const float* b; const float* tab;
    const int32_t* counts; float* out; float* outs;
    size_t plane;
    int row_stride, T, b_off, M;
};

template <bool ADD>
__global__ __launch_bounds__(256) void reduce_rows_ps_kernel(const PsRedArgs p) {
    const int row = blockIdx.x * PS_ROWS_PER_BLOCK + (threadIdx.x >> 6);
    const int c = (threadIdx.x & 63) * 4;
    if (row >= p.M) return;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    const float* prow = p.P + (size_t)row * D + c;
    f32x4 pl[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) pl[s] = ld4(prow + s * p.plane);
    const f32x4 bi = ld4(p.bias + c);
    const f32x4 rs = p.res != nullptr ? ld4(p.res + (size_t)row * D + c) : zero;
    const f32x4 gg = ld4(p.g + c), bb = ld4(p.b + c);
    const int bg = p.b_off + row / p.T, tt = row % p.T;
    f32x4 t0, t1;
    if (ADD) {
        const int cnt = p.counts != nullptr ? p.counts[bg] : 0x7fffffff;
        t0 = ld4(p.tab + ((size_t)bg * 2 + (tt < cnt ? 0 : 1)) * D + c);
        t1 = zero;
    } else {
        const float* t = p.tab + (size_t)bg * p.row_stride;
        t0 = ld4(t + c); t1 = ld4(t + 256 + c);
    }
    f32x4 v;
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = ((pl[0][i] + pl[1][i]) + pl[2][i]) + pl[3][i] + bi[i] + rs[i];
    float mean, rstd;
    ps_row_stats(v, mean, rstd);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        v[i] = (v[i] - mean) * rstd * gg[i] + bb[i];
        v[i] = ADD ? v[i] + t0[i] : silu(v[i] * (1.f + t0[i]) + t1[i]);
    }
    st4(p.out + (size_t)row * D + c, v);
    if (p.outs != nullptr) store_split4(p.outs + (size_t)row * D, c, v);
}

template <bool ADD>
int launch_reduce_rows_ps(const PsRedArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(reduce_rows_ps_kernel<ADD>, dim3((a.M + PS_ROWS_PER_BLOCK - 1) / PS_ROWS_PER_BLOCK), dim3(256), 0, s, a);
    LADIFF_LAUNCH_CHECK();
    return 0;
}

GemmArgs lin(const float* A, int lda, const LinearW& l, float* Y, int ldy, int M, int N, int K) {
    GemmArgs g;
    g.A = A; g.lda = lda; g.W = l.w; g.ldw = K; g.bias = l.b; g.Y = Y; g.ldy = ldy; g.M = M; g.N = N; g.K = K;
    return g;
}
KrArgs kr(const float* A, int lda, const float* W, const float* b, float* Y, int ldy, int M, int N, int K, int act = ACT_NONE) {
    KrArgs g;
    g.A = A; g.lda = lda; g.W = W; g.ldw = K; g.bias = b; g.Y = Y; g.ldy = ldy; g.M = M; g.N = N; g.K = K; g.act = act;
    return g;
}

// dctab[layer][b][valid | pad] = ca_proj.out(u[layer][b][valid | pad]): one input launch and one batched GEMM for the nine layers
int denoiser_diag_ctab(const DenoiserW& w, const DenoiserW* wsp, const float* tables, const float* nval, int B2, float* u, float* dctab,
                       hipStream_t s) {
    RowBatch rb;
    GemmArgs g[NL];
    const size_t per_layer = (size_t)B2 * 2 * D;
    for (int l = 0; l < NL; ++l) {
        const DenLayerW& L = w.layer[l];
        float* ul = u + l * per_layer;
        rb.a[l] = nval + (size_t)l * B2 * D; rb.g[l] = L.ca_proj.norm.b;
        rb.b[l] = tables + (size_t)l * DEN_LAYER_STRIDE + DEN_OFF_CA_MOD; rb.y[l] = ul;
        g[l] = lin(ul, D, L.ca_proj.out, dctab + l * per_layer, D, 2 * B2, D, D);
        if (wsp != nullptr) { g[l].W = wsp->layer[l].ca_proj.out.w; g[l].split = 1; }
    }
    const int M = 2 * B2;
    hipLaunchKernelGGL(ca_diag_input_kernel, dim3((M + PS_ROWS_PER_BLOCK - 1) / PS_ROWS_PER_BLOCK, NL), dim3(256), 0, s, rb,
                       DEN_STEP_STRIDE, M, wsp != nullptr ? 1 : 0);
    LADIFF_LAUNCH_CHECK();
    return launch_gemm_batch(g, NL, s);
}

// The nine layers on M = B2 T rows (denoiser_forward's sequence for one text token, denoiser.hip, with the three per-sample kernels).
// f16x3 mode (wsp != NULL) is the UNFUSED sequence of the n_text > 1 path: split-operand gemm_kr and row kernels that also write the
// S-format twin; qkv_attn.hip and combine_gemm read *d_step and stay the loop's.
int denoiser_layers_ps(const DenoiserW& w, const DenoiserW* wsp, const float* tables, const float* tkv, const float* dctab,
                       const float* sample, int B2, int T, const int32_t* counts, float* eps, float* ws, hipStream_t s) {
    const int M = B2 * T;
    DenForwardWs a = den_forward_layout(ws, (size_t)M);
    const bool sp = wsp != nullptr;
    if (!sp) { for (float*& t : a.Ps) t = nullptr; for (float*& t : a.SKs) t = nullptr; }      // fp32 mode: no S-format twins
    float *const *P = a.P, *const *SK = a.SK, *const *Ps = a.Ps, *const *SKs = a.SKs;
    float *qkv = a.qkv, *att = a.att, *hid = a.hid, *part = a.part;
    auto gemm = [&](KrArgs g) { g.split = sp ? 1 : 0; return launch_gemm_kr(g, s); };
    auto red = [&](const float* bias, const float* res, const NormW& n, const float* tab, float* out, float* outs) {
        PsRedArgs r;
        r.P = part; r.bias = bias; r.res = res; r.g = n.g; r.b = n.b; r.tab = tab; r.counts = counts; r.out = out; r.outs = outs;
        r.plane = (size_t)M * D; r.row_stride = DEN_STEP_STRIDE; r.T = T; r.b_off = 0; r.M = M;
        return r;
    };

    LADIFF_TRY(launch_add_pe(sample, w.query_pe, B2, 0, B2, T, P[0], Ps[0], s));
    const float* cur = P[0]; const float* curs = Ps[0];
    for (int l = 0; l < NL; ++l) {
        const DenLayerW& L = w.layer[l];
        const DenLayerW& Ls = sp ? wsp->layer[l] : w.layer[l];      // matrices as the MFMA reads them
        const float* tl = tables + (size_t)l * DEN_LAYER_STRIDE;
        const bool is_in = l < NSKIP, is_out = l > NSKIP;
        if (is_out) {                                               // x = linear_blocks([x | xs.pop()])
            const LinearW& sk = w.skip[l - NSKIP - 1];
            if (sp) {
                RowLnArgs g;
                g.A = curs; g.lda = D; g.A2 = SKs[NL - 1 - l]; g.lda2 = D; g.K1 = D; g.W = wsp->skip[l - NSKIP - 1].w; g.ldw = 2 * D;
                g.bias = sk.b; g.Y = P[3]; g.Ys = Ps[3]; g.ldy = D; g.M = M; g.K = 2 * D;
                LADIFF_TRY(launch_gemm_rowln(g, s));
            } else {
                KrArgs g = kr(cur, D, sk.w, nullptr, part, D, M, D, 2 * D);
                g.A2 = SK[NL - 1 - l]; g.lda2 = D; g.K1 = D;
                LADIFF_TRY(gemm(g));
                LADIFF_TRY(launch_reduce_rows(part, 2, M, sk.b, nullptr, RED_PLAIN, nullptr, nullptr, nullptr, 0, nullptr, nullptr, 1, 1, 0, 0,
                                              P[3], nullptr, s));
            }
            cur = P[3]; curs = Ps[3];
        }
        // att = softmax over [latents | text | time_b] keys . V; f16x3: written as out_proj's S-format operand
        LADIFF_TRY(gemm(kr(sp ? curs : cur, D, Ls.sa_attn.in_w, L.sa_attn.in_b, qkv, 3 * D, M, 3 * D, D)));
        LADIFF_TRY(launch_self_attention_ps(qkv, tkv + (size_t)l * B2 * 2 * D, tl, DEN_OFF_TIME_KV, DEN_STEP_STRIDE, counts, 0, B2, T, att,
                                            sp ? 1 : 0, s));
        if (sp) {   // X1 = LN1(x + out_proj(att)) -> P[2] / Ps[2]
            RowLnArgs g;
            g.A = att; g.lda = D; g.W = Ls.sa_attn.out_w; g.ldw = D; g.bias = L.sa_attn.out_b; g.res = cur; g.ldres = D;
            g.ln_g = L.sa_norm1.g; g.ln_b = L.sa_norm1.b; g.Y = P[2]; g.Ys = Ps[2]; g.ldy = D; g.M = M; g.K = D;
            LADIFF_TRY(launch_gemm_rowln(g, s));
        } else {
            KrArgs g = kr(att, D, Ls.sa_attn.out_w, L.sa_attn.out_b, P[1], D, M, D, D);
            g.res = cur; g.ldres = D;
            LADIFF_TRY(gemm(g));
            LADIFF_TRY(launch_reduce_rows(P[1], 1, M, nullptr, nullptr, RED_LN, L.sa_norm1.g, L.sa_norm1.b, nullptr, 0, nullptr, nullptr, 1, 1,
                                          0, 0, P[2], nullptr, s));
        }
        {   // hid = relu(linear1(X1))
            KrArgs g = kr(sp ? Ps[2] : P[2], D, Ls.sa_lin1.w, L.sa_lin1.b, sp ? nullptr : hid, FF, M, FF, D, ACT_RELU);
            if (sp) g.Ys = hid;
            LADIFF_TRY(gemm(g));
        }
        // X3 = LN2(X1 + linear2(hid)) + c[layer][sample][valid | pad] -> P[1]
        LADIFF_TRY(gemm(kr(hid, FF, Ls.sa_lin2.w, nullptr, part, D, M, D, FF)));
        LADIFF_TRY(launch_reduce_rows_ps<true>(red(L.sa_lin2.b, P[2], L.sa_norm2, dctab + (size_t)l * B2 * 2 * D, P[1], Ps[1]), s));
        {   // hid = gelu(ffn.linear1(X3))
            KrArgs g = kr(sp ? Ps[1] : P[1], D, Ls.ffn1.w, L.ffn1.b, sp ? nullptr : hid, FF, M, FF, D, ACT_GELU);
            if (sp) g.Ys = hid;
            LADIFF_TRY(gemm(g));
        }
        // u = SiLU(LN(ffn.linear2(hid)) (1 + scale_b) + shift_b) -> P[2];  x' = X3 + out_layers(u)
        LADIFF_TRY(gemm(kr(hid, FF, Ls.ffn2.w, nullptr, part, D, M, D, FF)));
        LADIFF_TRY(launch_reduce_rows_ps<false>(red(L.ffn2.b, nullptr, L.ffn_proj.norm, tl + DEN_OFF_FFN_MOD, P[2], Ps[2]), s));
        float* dst = is_in ? SK[l] : P[0];
        float* dsts = is_in ? SKs[l] : Ps[0];
        KrArgs g = kr(sp ? Ps[2] : P[2], D, Ls.ffn_proj.out.w, L.ffn_proj.out.b, dst, D, M, D, D);
        g.res = P[1]; g.ldres = D; g.Ys = dsts;
        LADIFF_TRY(gemm(g));
        cur = dst; curs = dsts;
    }
    return launch_layernorm(cur, w.norm.g, w.norm.b, eps, M, s);      // encoder.norm
}

}  // namespace

// timesteps [B2] (device) -> sinusoid -> time tables with one row per sample -> step-invariant text cache -> diagonal c table -> layers.
// The number of launches does not depend on B2.
int denoiser_forward_timesteps(const DenoiserW& w, const DenoiserW* wsp, const float* text, const int64_t* timesteps, const float* sample,
                               int B2, int T, const int32_t* counts, float* eps, float* ws, size_t ws_floats, hipStream_t s) {
    if (B2 < 1 || T < 1 || T > LADIFF_MAX_LATENTS) return LADIFF_ERR_SHAPE;
    const DenPerSampleWs a = den_per_sample_layout(ws, B2, T);
    if (ws_floats < a.total) return LADIFF_ERR_WORKSPACE;
    LADIFF_TRY(launch_sinusoid(timesteps, B2, a.sinus, s));
    LADIFF_TRY(denoiser_time_tables(w, a.sinus, B2, a.tables, a.tws, a.tws_floats, s));
    LADIFF_TRY(denoiser_text_static(w, text, B2, a.cache, a.xws, a.xws_floats, s));
    const DenTextCache c = den_text_cache_layout(a.cache, B2, 0, 1);
    LADIFF_TRY(denoiser_diag_ctab(w, wsp, a.tables, c.nval, B2, a.u, a.dctab, s));
    return denoiser_layers_ps(w, wsp, a.tables, c.tkv, a.dctab, sample, B2, T, counts, eps, a.fwd, s);
}

// ------------------------------------------------------------------ q-sample
// noisy[b,t,:] = sqrt(acp[ts_b]) z[t,b,:] + sqrt(1 - acp[ts_b]) noise[b,t,:], rows t >= counts[b] of noisy zero (noise rows are kept: the
// reference's loss runs over all of them).  The two coefficients and the sum are fp64, rounded once.  gen.on: the noise is drawn here
// (noise_gen.h, schedule position 0) and written out.  The timestep is device data: clamped to the table before it indexes it.
__global__ __launch_bounds__(256) void q_sample_kernel(const float* __restrict__ z, const int64_t* __restrict__ ts, const float* __restrict__ acp,
                                                       int n_train, const int32_t* __restrict__ counts, const NoiseGen gen,
                                                       float* __restrict__ noise, float* __restrict__ noisy, int B, int T) {
    const int row = blockIdx.x * PS_ROWS_PER_BLOCK + (threadIdx.x >> 6);      // row = b * T + t
    const int c = (threadIdx.x & 63) * 4;
    if (row >= B * T) return;
    const int b = row / T, t = row % T;
    int64_t step = ts[b];
    step = step < 0 ? 0 : (step >= n_train ? n_train - 1 : step);
    const double a = (double)acp[step];
    const double ka = sqrt(a), kb = sqrt(1.0 - a);
    float* nrow = noise + (size_t)row * D + c;
    f32x4 e;
    if (gen.on) {
        float zz[4];
        noise_normal4(gen, 0, gen.prompt0 + (unsigned)b, t, c / 4, zz);
        e = f32x4{zz[0], zz[1], zz[2], zz[3]};
        st4(nrow, e);
    } else {
        e = ld4(nrow);
    }
    const f32x4 x = ld4(z + ((size_t)t * B + b) * D + c);
    const bool valid = counts == nullptr || t < counts[b];
    f32x4 v;
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = valid ? (float)(ka * (double)x[i] + kb * (double)e[i]) : 0.f;
    st4(noisy + (size_t)row * D + c, v);
}

int launch_q_sample(const float* z, const int64_t* ts, const float* acp, int n_train, const int32_t* counts, const NoiseGen& gen, float* noise,
                    float* noisy, int B, int T, hipStream_t s) {
    const int M = B * T;
    hipLaunchKernelGGL(q_sample_kernel, dim3((M + PS_ROWS_PER_BLOCK - 1) / PS_ROWS_PER_BLOCK), dim3(256), 0, s, z, ts, acp, n_train, counts, gen,
                       noise, noisy, B, T);
    LADIFF_LAUNCH_CHECK();
    return 0;
}

// ------------------------------------------------------------------ inst_loss
// As vae_losses.hip: per-workgroup fp64 partial sums in fixed slots, then one workgroup adds them in slot order, divides, writes
// batch = {inst_loss, total} and adds it to acc.  Which element a thread reads and the order of every addition are functions of n alone.
constexpr int DL_THREADS = 256;

__global__ __launch_bounds__(DL_THREADS) void diffusion_losses_partial_kernel(const float* __restrict__ pred, const float* __restrict__ noise,
                                                                              size_t n, int vec, double* __restrict__ part) {
    __shared__ double s_part[DL_THREADS / 64];
    const size_t gid = (size_t)blockIdx.x * DL_THREADS + threadIdx.x, stride = (size_t)gridDim.x * DL_THREADS;
    const size_t n4 = n / 4;
    double v = 0.0;
    for (size_t i = gid; i < n4; i += stride) {
        f32x4 x, y;
        if (vec) {
            x = ld4(pred + 4 * i); y = ld4(noise + 4 * i);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) { x[k] = pred[4 * i + k]; y[k] = noise[4 * i + k]; }
        }
        double d[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) d[k] = (double)x[k] - (double)y[k];
        v += ((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]) + d[3] * d[3];
    }
    const size_t tail = n4 * 4 + gid;              // n % 4 elements: threads 0 .. 2 of workgroup 0 at most
    if (tail < n) { const double d = (double)pred[tail] - (double)noise[tail]; v += d * d; }
    // lanes by butterfly, then the four waves in wave order
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = ((s_part[0] + s_part[1]) + s_part[2]) + s_part[3];
}

__global__ __launch_bounds__(64) void diffusion_losses_finalize_kernel(const double* __restrict__ part, int blocks, double n, double lambda_inst,
                                                                       double* __restrict__ batch, double* __restrict__ acc) {
    if (threadIdx.x != 0) return;
    double a = 0.0;
    for (int g = 0; g < blocks; ++g) a += part[g];
    const double inst = a / n, total = lambda_inst * inst;
    batch[0] = inst; batch[1] = total;
    acc[0] += inst; acc[1] += total;
}

int launch_diffusion_losses(const float* pred, const float* noise, size_t n, double lambda_inst, double* part, int blocks, double* batch,
                            double* acc, hipStream_t s) {
    const int vec = ((reinterpret_cast<uintptr_t>(pred) | reinterpret_cast<uintptr_t>(noise)) & 15) == 0;
    hipLaunchKernelGGL(diffusion_losses_partial_kernel, dim3(blocks), dim3(DL_THREADS), 0, s, pred, noise, n, vec, part);
    LADIFF_LAUNCH_CHECK();
    hipLaunchKernelGGL(diffusion_losses_finalize_kernel, dim3(1), dim3(64), 0, s, part, blocks, (double)n, lambda_inst, batch, acc);
    LADIFF_LAUNCH_CHECK();
    return 0;
}

}  // namespace ladiff
