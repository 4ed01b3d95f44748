// Stage "diffusion" outside the sampling loop (LADIFF.train_diffusion_forward, ladiff.py:874-1033, and _diffusion_process, :745-813):
//   q-sample            noisy = sqrt(acp[t_b]) z + sqrt(1 - acp[t_b]) noise          scheduler.add_noise + the LAD zeroing   :775-782
//   denoiser forward    with ONE TIMESTEP PER SAMPLE                                 self.denoiser(noisy, timesteps [B], ...) :785-794
//   inst_loss           mean (noise_pred - noise)^2 over every element               nn.MSELoss, losses/mld.py:69, :112
// The forward is the sampling loop's own (denoiser_forward, denoiser.hip) with a null step counter: the three row operations that read
// one table row per call there - the time token's K|V in self-attention, the hoisted cross-attention vector c added after norm2, the
// (scale | shift) of the FFN's StylizationBlock - read the row of the GLOBAL sample index here, from tables with one row per sample
// (workspace.h, den_per_sample_layout).  Which code runs:
//   denoiser_forward_timesteps   den_self_attn_kernel<T, true>  (attention.hip), reduce_rows_kernel<true>  (rowops.hip), unfused sequence
//   denoiser_forward, the loop   den_self_attn_kernel<T, false>,                 reduce_rows_kernel<false>, and in f16x3 mode the fused
//                                qkv_attn.hip / combine_gemm, which read *d_step
// This file adds what has no twin there: the "diagonal" c table, whose row mapping is its own, q-sample and the loss.
#include "model.h"

namespace ladiff {

namespace {

constexpr int PS_ROWS_PER_BLOCK = 4;   // 256 threads = 4 waves = 4 rows of 256 floats, one f32x4 per lane (as rowops.hip)

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
    return denoiser_forward(w, wsp, a.tables, nullptr, a.cache, 0, sample, B2, 1, T, counts, eps, a.fwd, a.fwd_floats, s, 0, B2, 0, 1, nullptr,
                            a.dctab);
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
