// The stage-"vae" validation losses of one batch on the device (MLDLosses.update, losses/mld.py:98-107, :141-147, :157-164):
//   recons_feature = mean SmoothL1(m_rst, m_ref)            torch.nn.SmoothL1Loss(reduction='mean'), beta 1        mld.py:81-84
//   recons_joints  = mean SmoothL1(joints_rst, joints_ref)
//   kl_motion      = mean kl_divergence(Normal(mu, std), Normal(0, 1)) = mean 0.5 (std^2 + mu^2 - 1 - log std^2)   mld.py:162-164
//   total          = lambda_rec recons_feature + lambda_joint recons_joints + lambda_kl kl_motion                  mld.py:95-96, :146
// The reference calls three torch reductions and adds the results to its state on the host side of a Metric; here one launch reads the
// six flat arrays once and leaves one fp64 partial sum per term and workgroup in a fixed slot of the workspace, and a second,
// one-workgroup launch adds the slots in slot order, divides by the element counts, writes the four values to `batch` and adds them to
// the caller's accumulator (the reference's `+=` per update) - no host synchronisation and no floating-point atomics: which element a
// thread reads and the order of every addition are functions of the shapes alone, so two calls on the same inputs leave the same bits.
// Inputs are widened to fp64 before the subtraction and every sum is fp64 (a few million elements: the rate does not matter).
// The arrays are read 16 bytes per lane where both of a pair are 16-byte aligned and as four scalars otherwise - the same elements in
// the same order either way - and the count's remainder below four by the first threads of workgroup 0.
#include "kernels.h"

namespace ladiff {

constexpr int VL_THREADS = 256;
constexpr int VL_WAVES = VL_THREADS / 64;

__device__ __forceinline__ double vl_smooth_l1(float a, float b) {
    const double d = (double)a - (double)b, ad = fabs(d);
    return ad < 1.0 ? 0.5 * d * d : ad - 0.5;
}

__device__ __forceinline__ double vl_kl(float mu, float sd) {
    const double m = (double)mu, v = (double)sd * (double)sd;
    return 0.5 * (v + m * m - 1.0 - log(v));
}

// this thread's share of sum_i term(a[i], b[i]): chunks of four elements dealt round-robin over the grid's threads
template <class Term>
__device__ __forceinline__ double vl_pair_sum(const float* __restrict__ a, const float* __restrict__ b, size_t n, bool vec, Term term) {
    const size_t gid = (size_t)blockIdx.x * VL_THREADS + threadIdx.x, stride = (size_t)gridDim.x * VL_THREADS;
    const size_t n4 = n / 4;
    double s = 0.0;
    for (size_t i = gid; i < n4; i += stride) {
        f32x4 x, y;
        if (vec) {
            x = ld4(a + 4 * i); y = ld4(b + 4 * i);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) { x[k] = a[4 * i + k]; y[k] = b[4 * i + k]; }
        }
        s += ((term(x[0], y[0]) + term(x[1], y[1])) + term(x[2], y[2])) + term(x[3], y[3]);
    }
    const size_t tail = n4 * 4 + gid;              // n % 4 elements: threads 0 .. 2 of workgroup 0 at most
    if (tail < n) s += term(a[tail], b[tail]);
    return s;
}

__global__ __launch_bounds__(VL_THREADS) void vae_losses_partial_kernel(const float* __restrict__ m_rst, const float* __restrict__ m_ref,
                                                                        size_t n_feat, int vec_feat, const float* __restrict__ j_rst,
                                                                        const float* __restrict__ j_ref, size_t n_joint, int vec_joint,
                                                                        const float* __restrict__ mu, const float* __restrict__ sd,
                                                                        size_t n_lat, int vec_lat, double* __restrict__ part) {
    __shared__ double s_part[VL_WAVES][3];
    double v[3];
    v[0] = vl_pair_sum(m_rst, m_ref, n_feat, vec_feat != 0, [](float a, float b) { return vl_smooth_l1(a, b); });
    v[1] = vl_pair_sum(j_rst, j_ref, n_joint, vec_joint != 0, [](float a, float b) { return vl_smooth_l1(a, b); });
    v[2] = vl_pair_sum(mu, sd, n_lat, vec_lat != 0, [](float a, float b) { return vl_kl(a, b); });
    // lanes by butterfly, then the four waves in wave order
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) v[k] += __shfl_xor(v[k], d);
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 3; ++k) s_part[wave][k] = v[k];
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        const int k = threadIdx.x;
        part[(size_t)blockIdx.x * 3 + k] = ((s_part[0][k] + s_part[1][k]) + s_part[2][k]) + s_part[3][k];
    }
}

// batch = {recons_feature, recons_joints, kl_motion, total}; acc += batch.  One workgroup: thread k < 3 adds term k's slots in slot order.
__global__ __launch_bounds__(64) void vae_losses_finalize_kernel(const double* __restrict__ part, int blocks, double n_feat, double n_joint,
                                                                 double n_lat, double l_rec, double l_joint, double l_kl,
                                                                 double* __restrict__ batch, double* __restrict__ acc) {
    __shared__ double s_mean[3];
    const int t = threadIdx.x;
    if (t < 3) {
        double a = 0.0;
        for (int g = 0; g < blocks; ++g) a += part[(size_t)g * 3 + t];
        s_mean[t] = a / (t == 0 ? n_feat : (t == 1 ? n_joint : n_lat));
    }
    __syncthreads();
    if (t < 4) {
        const double v = t < 3 ? s_mean[t] : (l_rec * s_mean[0] + l_joint * s_mean[1]) + l_kl * s_mean[2];
        batch[t] = v;
        acc[t] += v;
    }
}

static int vl_vec(const void* a, const void* b) { return ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) & 15) == 0; }

int launch_vae_losses(const float* m_rst, const float* m_ref, size_t n_feat, const float* j_rst, const float* j_ref, size_t n_joint,
                      const float* mu, const float* sd, size_t n_lat, double l_rec, double l_joint, double l_kl, double* part, int blocks,
                      double* batch, double* acc, hipStream_t s) {
    hipLaunchKernelGGL(vae_losses_partial_kernel, dim3(blocks), dim3(VL_THREADS), 0, s, m_rst, m_ref, n_feat, vl_vec(m_rst, m_ref), j_rst,
                       j_ref, n_joint, vl_vec(j_rst, j_ref), mu, sd, n_lat, vl_vec(mu, sd), part);
    LADIFF_LAUNCH_CHECK();
    hipLaunchKernelGGL(vae_losses_finalize_kernel, dim3(1), dim3(64), 0, s, part, blocks, (double)n_feat, (double)n_joint, (double)n_lat,
                       l_rec, l_joint, l_kl, batch, acc);
    LADIFF_LAUNCH_CHECK();
    return 0;
}

}  // namespace ladiff
