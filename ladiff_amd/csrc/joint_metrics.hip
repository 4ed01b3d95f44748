// Joint-space metrics on the device: APE / AVE (ComputeMetrics = "TemosMetric") and MPJPE / PA-MPJPE / ACCEL (MRMetrics).
//   reference: ComputeMetrics.update / transform   (ladiff/models/metrics/compute.py:102-196)
//              Rifke.forward, get_forward_direction, get_floor, softmin  (transforms/joints2jfeats/rifke.py:27-91, tools.py:14-55)
//              l2_norm, variance                   (models/metrics/utils.py:8-16)
//              MRMetrics.update                    (models/metrics/mr.py:73-96)
//              calc_mpjpe / calc_accel / calc_pampjpe / batch_compute_similarity_transform_torch  (utils.py:267-406)
// The reference copies [B,F,J,3] to the host and loops over the sequences in Python; here the joints that feats2joints left in HBM are
// reduced to one row of sums per sequence by one launch, and a second single-workgroup launch adds the rows to the caller's fp64
// accumulator in sequence order (no floating-point atomics: the accumulator's bits do not depend on how a set of sequences is cut
// into calls).
//
// One workgroup per sequence, one thread per frame (F <= 224 < 256 threads).  Inputs are fp32; the arithmetic is fp64 throughout (the
// work is a few thousand operations per frame on 13 MB of input, so the rate does not matter, and the only rounding a row sees is
// its final conversion to fp32); the frame axis is scanned with wave shuffles plus one LDS hop across the four waves, sums over frames
// are wave-shuffle reductions combined across the waves in wave order.  Joints are re-read from global memory (L2 hits) in each pass
// instead of being held: a frame is 2 x 66 floats, and the per-joint passes need only a dozen per-frame scalars beside them.
#include "kernels.h"

namespace ladiff {

constexpr int JM_THREADS = 256;
constexpr int JM_WAVES = JM_THREADS / 64;
constexpr int JM_RED = 14;                         // widest reduction: 12 means + 2 APE terms of one joint
static_assert(LADIFF_MAX_FRAMES <= JM_THREADS, "one thread per frame");

struct JmParts { int ls, rs, lh, rh, lm, rm, lf, rf; };

__device__ __forceinline__ double jm_wave_sum(double v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

// v[i] <- sum over the workgroup's threads of v[i], in every thread: lanes by butterfly, then the four waves in wave order
template <int N>
__device__ __forceinline__ void jm_block_sum(double (&v)[N], double (*s_part)[JM_RED]) {
    static_assert(N <= JM_RED, "s_part row");
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] = jm_wave_sum(v[i]);
    __syncthreads();                               // the previous round's readers are done with s_part
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < N; ++i) s_part[wave][i] = v[i];
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] = ((s_part[0][i] + s_part[1][i]) + s_part[2][i]) + s_part[3][i];
}

// (min, max) over the workgroup's threads
__device__ __forceinline__ void jm_block_minmax(double& mn, double& mx, double (*s_part)[JM_RED]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        mn = fmin(mn, __shfl_xor(mn, d));
        mx = fmax(mx, __shfl_xor(mx, d));
    }
    __syncthreads();
    if (lane == 0) { s_part[wave][0] = mn; s_part[wave][1] = mx; }
    __syncthreads();
    mn = fmin(fmin(s_part[0][0], s_part[1][0]), fmin(s_part[2][0], s_part[3][0]));
    mx = fmax(fmax(s_part[0][1], s_part[1][1]), fmax(s_part[2][1], s_part[3][1]));
}

// inclusive prefix sum over the thread index (torch.cumsum along frames)
__device__ __forceinline__ double jm_block_scan(double v, double* s_wave) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const double u = __shfl_up(v, d);
        if (lane >= d) v += u;
    }
    __syncthreads();
    if (lane == 63) s_wave[wave] = v;
    __syncthreads();
    double off = 0.0;
    for (int w = 0; w < wave; ++w) off += s_wave[w];
    return v + off;
}

// ------------------------------------------------------------------ APE / AVE
// Row layout (W = 4 + 2 (J - 1) + 2 J floats), the order of ComputeMetrics.metrics:
//   APE_root, APE_traj, APE_pose[J-1], APE_joints[J], AVE_root, AVE_traj, AVE_pose[J-1], AVE_joints[J]
__global__ __launch_bounds__(JM_THREADS) void joint_ape_ave_kernel(const float* __restrict__ rst, const float* __restrict__ ref,
                                                                   const int32_t* __restrict__ lengths, int F, int J, JmParts pi,
                                                                   double factor, float* __restrict__ seq_rows) {
    __shared__ double s_part[JM_WAVES][JM_RED];
    __shared__ double s_wave[JM_WAVES];
    __shared__ double s_nb[2][3][JM_THREADS];      // per tensor: trajectory x, z and forward angle of every frame (for the differences)
    const int b = blockIdx.x, t = threadIdx.x;
    const bool live = t < F;                       // a frame of the padded tensor
    int len = lengths[b];
    len = len < 1 ? 1 : (len > F ? F : len);       // the entry checked the host copy; never index by an unchecked device value
    const bool counted = t < len;                  // remove_padding                                          compute.py:188-196
    const float* src[2] = {rst + ((size_t)b * F + (live ? t : 0)) * J * 3, ref + ((size_t)b * F + (live ? t : 0)) * J * 3};
    const int W = 4 + 2 * (J - 1) + 2 * J;
    float* row = seq_rows + (size_t)b * W;
    const double T1 = (double)(len - 1);           // variance(x, T): divisor T - 1                            utils.py:12-16

    // per tensor, per frame
    double floor_[2], ty[2], rx[2], rz[2], fx[2], fy[2], cs[2], sn[2], gx[2], gz[2];
#pragma unroll
    for (int x = 0; x < 2; ++x) {
        const float* p = src[x];
        // floor = softmin(min over the four foot joints' heights, softness 0.5) over ALL F frames          tools.py:33-55
        double mn = INFINITY, mx = -INFINITY;
        if (live) {
            const double h = fmin(fmin((double)p[3 * pi.lm + 1], (double)p[3 * pi.lf + 1]),
                                  fmin((double)p[3 * pi.rm + 1], (double)p[3 * pi.rf + 1]));
            mn = h; mx = h;
        }
        jm_block_minmax(mn, mx, s_part);
        floor_[x] = mn - log(0.5 + exp(mn - mx));  // -(max(-h) + log(softness + exp(min(-h) - max(-h))))
        rx[x] = live ? (double)p[0] : 0.0;         // trajectory = root x, z                                   rifke.py:35-40
        rz[x] = live ? (double)p[2] : 0.0;
        ty[x] = live ? (double)p[1] - floor_[x] : 0.0;        // root_y
        // forward direction from hips and shoulders of the poses WITHOUT the root joint: the reference indexes the [.., J-1, 3] tensor
        // with the names' positions in the full list (rifke.py:43, :55, tools.py:22-27), i.e. joint (index + 1) of the input
        double ax = 0.0, az = 0.0;
        if (live) {
            const float *rh = p + 3 * (pi.rh + 1), *lh = p + 3 * (pi.lh + 1), *rs = p + 3 * (pi.rs + 1), *ls = p + 3 * (pi.ls + 1);
            ax = (((double)rh[0] - rx[x]) - ((double)lh[0] - rx[x]) + ((double)rs[0] - rx[x])) - ((double)ls[0] - rx[x]);
            az = (((double)rh[2] - rz[x]) - ((double)lh[2] - rz[x]) + ((double)rs[2] - rz[x])) - ((double)ls[2] - rz[x]);
        }
        const double nrm = fmax(sqrt(az * az + ax * ax), 1e-12);   // F.normalize: v / max(||v||, eps)
        fx[x] = -az / nrm;
        fy[x] = ax / nrm;
        s_nb[x][0][t] = rx[x];
        s_nb[x][1][t] = rz[x];
        s_nb[x][2][t] = atan2(fx[x], fy[x]);                                                                // rifke.py:62
    }
    __syncthreads();
#pragma unroll
    for (int x = 0; x < 2; ++x) {
        // first differences with a zero in front (rifke.py:49-52, :63-65), then ComputeMetrics.transform's re-integration
        const bool diff = live && t >= 1;
        const double vang = diff ? s_nb[x][2][t] - s_nb[x][2][t - 1] : 0.0;
        const double vx = diff ? rx[x] - s_nb[x][0][t - 1] : 0.0;
        const double vz = diff ? rz[x] - s_nb[x][1][t - 1] : 0.0;
        // angles = cumsum(vel_angles) - its first term, which is the zero put in front                       compute.py:140-144
        const double ang = jm_block_scan(vang, s_wave);
        cs[x] = cos(ang);
        sn[x] = sin(ang);
        // vel_trajectory_local = vel . R_inv(forward), then . R(angles)            rifke.py:68-69, :82-83; compute.py:145, :159-160
        const double lx = vx * fy[x] - vz * fx[x], lz = vx * fx[x] + vz * fy[x];
        const double wx = lx * cs[x] + lz * sn[x], wz = -lx * sn[x] + lz * cs[x];
        gx[x] = jm_block_scan(wx, s_wave);                                                                  // compute.py:163-165
        gz[x] = jm_block_scan(wz, s_wave);
    }

    // ---- root and trajectory: root = (traj.x, root_y, traj.z) / factor, trajectory = its x and z            compute.py:168-171
    double red[JM_RED];
    double rootv[2][3];
#pragma unroll
    for (int x = 0; x < 2; ++x) { rootv[x][0] = gx[x] / factor; rootv[x][1] = ty[x] / factor; rootv[x][2] = gz[x] / factor; }
    {
        const double dx = rootv[0][0] - rootv[1][0], dy = rootv[0][1] - rootv[1][1], dz = rootv[0][2] - rootv[1][2];
        red[0] = counted ? sqrt(dx * dx + dy * dy + dz * dz) : 0.0;        // APE_root                         compute.py:112
        red[1] = counted ? sqrt(dx * dx + dz * dz) : 0.0;                  // APE_traj                         :114
#pragma unroll
        for (int k = 0; k < 6; ++k) red[2 + k] = counted ? rootv[k / 3][k % 3] : 0.0;
        double r8[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) r8[k] = red[k];
        jm_block_sum(r8, s_part);
        double dev[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            const double d = rootv[k / 3][k % 3] - r8[2 + k] / (double)len;
            dev[k] = counted ? d * d : 0.0;
        }
        jm_block_sum(dev, s_part);
        if (t == 0) {
            const double sx = dev[0] / T1 - dev[3] / T1, sy = dev[1] / T1 - dev[4] / T1, sz = dev[2] / T1 - dev[5] / T1;
            const float ape_root = (float)r8[0], ave_root = (float)sqrt(sx * sx + sy * sy + sz * sz);
            row[0] = ape_root;
            row[1] = (float)r8[1];
            row[2 + (J - 1)] = ape_root;                                   // joint 0 of the global joints is the root
            row[2 + (J - 1) + J] = ave_root;                               // AVE_root                         :117-119
            row[2 + (J - 1) + J + 1] = (float)sqrt(sx * sx + sz * sz);     // AVE_traj                         :121-123
            row[2 + (J - 1) + J + 2 + (J - 1)] = ave_root;
        }
    }

    // ---- joints 1 .. J-1: local pose (the Rifke feature) and global joint
    for (int j = 1; j < J; ++j) {
        double v[2][6];                            // per tensor: local x, y, z, global x, y, z
#pragma unroll
        for (int x = 0; x < 2; ++x) {
            const float* p = src[x] + 3 * j;
            const double px = live ? (double)p[0] - rx[x] : 0.0, py = live ? (double)p[1] - floor_[x] : 0.0,
                         pz = live ? (double)p[2] - rz[x] : 0.0;
            const double lx = px * fy[x] - pz * fx[x], lz = px * fx[x] + pz * fy[x];                        // rifke.py:72-75
            v[x][0] = lx / factor; v[x][1] = py / factor; v[x][2] = lz / factor;                            // compute.py:189
            v[x][3] = (lx * cs[x] + lz * sn[x] + gx[x]) / factor;                                           // compute.py:153-156, :179
            v[x][4] = py / factor;
            v[x][5] = (-lx * sn[x] + lz * cs[x] + gz[x]) / factor;
        }
        {
            const double dx = v[0][0] - v[1][0], dy = v[0][1] - v[1][1], dz = v[0][2] - v[1][2];
            const double ex = v[0][3] - v[1][3], ey = v[0][4] - v[1][4], ez = v[0][5] - v[1][5];
            red[0] = counted ? sqrt(dx * dx + dy * dy + dz * dz) : 0.0;    // APE_pose[j-1]                    compute.py:113
            red[1] = counted ? sqrt(ex * ex + ey * ey + ez * ez) : 0.0;    // APE_joints[j]                    :115
        }
#pragma unroll
        for (int k = 0; k < 12; ++k) red[2 + k] = counted ? v[k / 6][k % 6] : 0.0;
        jm_block_sum(red, s_part);
        double dev[12];
#pragma unroll
        for (int k = 0; k < 12; ++k) {
            const double d = v[k / 6][k % 6] - red[2 + k] / (double)len;
            dev[k] = counted ? d * d : 0.0;
        }
        jm_block_sum(dev, s_part);
        if (t == 0) {
            double q[6];
#pragma unroll
            for (int k = 0; k < 6; ++k) q[k] = dev[k] / T1 - dev[6 + k] / T1;
            row[2 + (j - 1)] = (float)red[0];
            row[2 + (J - 1) + j] = (float)red[1];
            row[2 + (J - 1) + J + 2 + (j - 1)] = (float)sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2]);      // AVE_pose    :125-127
            row[2 + (J - 1) + J + 2 + (J - 1) + j] = (float)sqrt(q[3] * q[3] + q[4] * q[4] + q[5] * q[5]);  // AVE_joints  :129-131
        }
    }
}

// ------------------------------------------------------------------ MPJPE / PA-MPJPE / ACCEL
// One Jacobi rotation of the symmetric 3x3 `a` in the (P, Q) plane, accumulated into the eigenvector columns of `v`.
template <int P, int Q, int R>
__device__ __forceinline__ void jm_jacobi_rot(double (&a)[3][3], double (&v)[3][3]) {
    const double apq = a[P][Q];
    if (apq == 0.0) return;
    const double theta = (a[Q][Q] - a[P][P]) / (2.0 * apq);
    const double tt = copysign(1.0, theta) / (fabs(theta) + sqrt(theta * theta + 1.0));
    const double c = 1.0 / sqrt(tt * tt + 1.0), s = tt * c;
    a[P][P] -= tt * apq;
    a[Q][Q] += tt * apq;
    a[P][Q] = a[Q][P] = 0.0;
    const double arp = a[R][P], arq = a[R][Q];
    a[R][P] = a[P][R] = c * arp - s * arq;
    a[R][Q] = a[Q][R] = s * arp + c * arq;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const double vp = v[r][P], vq = v[r][Q];
        v[r][P] = c * vp - s * vq;
        v[r][Q] = s * vp + c * vq;
    }
}

template <int A, int B>
__device__ __forceinline__ void jm_sort_pair(double (&lam)[3], double (&v)[3][3]) {      // larger eigenvalue first
    if (lam[A] < lam[B]) {
        const double l = lam[A]; lam[A] = lam[B]; lam[B] = l;
#pragma unroll
        for (int r = 0; r < 3; ++r) { const double u = v[r][A]; v[r][A] = v[r][B]; v[r][B] = u; }
    }
}

// Eigen-decomposition of the symmetric 3x3 `a` by cyclic Jacobi (fp64, a fixed eight sweeps): eigenvalues on a's diagonal, eigenvectors
// in the columns of `v`.
__device__ __forceinline__ void jm_eig3(double (&a)[3][3], double (&v)[3][3]) {
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) v[r][c] = r == c ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 8; ++sweep) {
        jm_jacobi_rot<0, 1, 2>(a, v);
        jm_jacobi_rot<0, 2, 1>(a, v);
        jm_jacobi_rot<1, 2, 0>(a, v);
    }
}

// out = sum_i w[i] v_i v_i^T over the columns v_i of `v`
__device__ __forceinline__ void jm_spectral(const double (&v)[3][3], const double (&w)[3], double (&out)[3][3]) {
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) out[r][c] = w[0] * v[r][0] * v[c][0] + w[1] * v[r][1] * v[c][1] + w[2] * v[r][2] * v[c][2];
}

__device__ __forceinline__ void jm_mul3(const double (&x)[3][3], const double (&y)[3][3], double (&out)[3][3]) {
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) out[r][c] = x[r][0] * y[0][c] + x[r][1] * y[1][c] + x[r][2] * y[2][c];
}

// PA-MPJPE of one frame when the reference does NOT transpose (F = 2 or 3, utils.py:274-278): the frame is 3 points (its x, y and z
// columns) in J dimensions, the means run over x, y, z per joint, K = X1 X2^T is J x J of rank <= 2.  With G1 = X1^T X1, G2 = X2^T X2
// (3 x 3), H = G1^(1/2) and M = H G2 H, the singular values of K are the square roots of M's eigenvalues and the rotation's action on X1
// is (R X1)^T = X2 C with C = H M^(-1/2) H (pseudo-inverse on the range): S1_hat - S2 = X2 (scale C - I), scale = tr M^(1/2) / ||X1||^2.
// The det-sign fix touches a direction of singular value zero only.
__device__ double jm_pa_untransposed(const float* __restrict__ P, const float* __restrict__ G, int J) {
    double G1[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}}, G2[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}}, var1 = 0.0;
    for (int j = 0; j < J; ++j) {
        const double p0 = P[3 * j], p1 = P[3 * j + 1], p2 = P[3 * j + 2], g0 = G[3 * j], g1 = G[3 * j + 1], g2 = G[3 * j + 2];
        const double m1 = (p0 + p1 + p2) / 3.0, m2 = (g0 + g1 + g2) / 3.0;
        const double x1[3] = {p0 - m1, p1 - m1, p2 - m1}, x2[3] = {g0 - m2, g1 - m2, g2 - m2};
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            var1 += x1[a] * x1[a];
#pragma unroll
            for (int c = 0; c < 3; ++c) { G1[a][c] += x1[a] * x1[c]; G2[a][c] += x2[a] * x2[c]; }
        }
    }
    double V[3][3], w[3], H[3][3], T[3][3], M[3][3], Mi[3][3], C[3][3];
    jm_eig3(G1, V);
    double top = fmax(fmax(G1[0][0], G1[1][1]), G1[2][2]);
#pragma unroll
    for (int i = 0; i < 3; ++i) w[i] = G1[i][i] > 1e-12 * top ? sqrt(G1[i][i]) : 0.0;
    jm_spectral(V, w, H);
    jm_mul3(H, G2, T);
    jm_mul3(T, H, M);
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = r + 1; c < 3; ++c) M[r][c] = M[c][r] = 0.5 * (M[r][c] + M[c][r]);
    jm_eig3(M, V);
    top = fmax(fmax(M[0][0], M[1][1]), M[2][2]);
    double tr = 0.0;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const bool keep = M[i][i] > 1e-12 * top;
        const double sv = keep ? sqrt(M[i][i]) : 0.0;
        tr += sv;
        w[i] = keep ? 1.0 / sv : 0.0;
    }
    jm_spectral(V, w, Mi);
    jm_mul3(H, Mi, T);
    jm_mul3(T, H, C);
    const double scale = tr / var1;
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) C[r][c] = scale * C[r][c] - (r == c ? 1.0 : 0.0);
    double pa = 0.0;
    for (int j = 0; j < J; ++j) {
        const double g0 = G[3 * j], g1 = G[3 * j + 1], g2 = G[3 * j + 2], m2 = (g0 + g1 + g2) / 3.0;
        const double x2[3] = {g0 - m2, g1 - m2, g2 - m2};
        double d2 = 0.0;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double d = x2[0] * C[0][c] + x2[1] * C[1][c] + x2[2] * C[2][c];
            d2 += d * d;
        }
        pa += sqrt(d2);
    }
    return pa / (double)J;
}

// Row layout: MPJPE, PAMPJPE, ACCEL - each the sum over ALL F frames of the sequence (mr.py:92-96 passes rst[i] whole)
__global__ __launch_bounds__(JM_THREADS) void joint_mr_kernel(const float* __restrict__ rst, const float* __restrict__ ref, int F, int J,
                                                              float* __restrict__ seq_rows) {
    __shared__ double s_part[JM_WAVES][JM_RED];
    const int b = blockIdx.x, t = threadIdx.x;
    const bool live = t < F;
    const size_t stride = (size_t)J * 3;
    const float* P = rst + ((size_t)b * F + (live ? t : 0)) * stride;      // preds
    const float* G = ref + ((size_t)b * F + (live ? t : 0)) * stride;      // target
    double out[3] = {0.0, 0.0, 0.0};
    if (live) {
        // MPJPE: root-aligned (align_inds = [0]), joints with target.x == -2 masked out                     utils.py:347-369, :321-341
        double mu1[3] = {0, 0, 0}, mu2[3] = {0, 0, 0}, num = 0.0, den = 0.0;
        for (int j = 0; j < J; ++j) {
            double d2 = 0.0;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const double p = (double)P[3 * j + k], g = (double)G[3 * j + k];
                const double d = (p - (double)P[k]) - (g - (double)G[k]);
                d2 += d * d;
                mu1[k] += p;
                mu2[k] += g;
            }
            const double m = G[3 * j] != -2.0f ? 1.0 : 0.0;
            num += sqrt(d2) * m;
            den += m;
        }
        out[0] = num / den;
        // PA-MPJPE: similarity transform of preds onto target                                                utils.py:267-318, :389-406
#pragma unroll
        for (int k = 0; k < 3; ++k) { mu1[k] /= (double)J; mu2[k] /= (double)J; }
        double K[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}}, var1 = 0.0;
        for (int j = 0; j < J; ++j) {
            double x1[3], x2[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) { x1[k] = (double)P[3 * j + k] - mu1[k]; x2[k] = (double)G[3 * j + k] - mu2[k]; }
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                var1 += x1[a] * x1[a];
#pragma unroll
                for (int c = 0; c < 3; ++c) K[a][c] += x1[a] * x2[c];      // K = X1 X2^T
            }
        }
        // K = U S V^T from the eigenvectors V of K^T K (cyclic Jacobi, fp64); R = V Z U^T with Z = diag(1, 1, sign det(U V^T)).
        // With u3' = u1 x u2 (so det [u1 u2 u3'] = +1) the third term of R is det(V) v3 u3'^T: u3 itself, which K v3 / s3 gives
        // poorly when s3 is small, is never needed.
        double A[3][3], V[3][3];
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int c = 0; c < 3; ++c) A[a][c] = K[0][a] * K[0][c] + K[1][a] * K[1][c] + K[2][a] * K[2][c];
        jm_eig3(A, V);
        double lam[3] = {A[0][0], A[1][1], A[2][2]};
        jm_sort_pair<0, 1>(lam, V);
        jm_sort_pair<0, 2>(lam, V);
        jm_sort_pair<1, 2>(lam, V);
        double u1[3], u2[3], u3[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            u1[a] = K[a][0] * V[0][0] + K[a][1] * V[1][0] + K[a][2] * V[2][0];
            u2[a] = K[a][0] * V[0][1] + K[a][1] * V[1][1] + K[a][2] * V[2][1];
        }
        const double n1 = sqrt(u1[0] * u1[0] + u1[1] * u1[1] + u1[2] * u1[2]);
#pragma unroll
        for (int a = 0; a < 3; ++a) u1[a] /= n1;
        const double pr = u1[0] * u2[0] + u1[1] * u2[1] + u1[2] * u2[2];
#pragma unroll
        for (int a = 0; a < 3; ++a) u2[a] -= pr * u1[a];
        const double n2 = sqrt(u2[0] * u2[0] + u2[1] * u2[1] + u2[2] * u2[2]);
#pragma unroll
        for (int a = 0; a < 3; ++a) u2[a] /= n2;
        u3[0] = u1[1] * u2[2] - u1[2] * u2[1];
        u3[1] = u1[2] * u2[0] - u1[0] * u2[2];
        u3[2] = u1[0] * u2[1] - u1[1] * u2[0];
        const double detV = V[0][0] * (V[1][1] * V[2][2] - V[1][2] * V[2][1]) - V[0][1] * (V[1][0] * V[2][2] - V[1][2] * V[2][0]) +
                            V[0][2] * (V[1][0] * V[2][1] - V[1][1] * V[2][0]);
        const double z3 = detV < 0.0 ? -1.0 : 1.0;
        double Rm[3][3], tr = 0.0;
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int c = 0; c < 3; ++c) Rm[a][c] = V[a][0] * u1[c] + V[a][1] * u2[c] + z3 * V[a][2] * u3[c];
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int c = 0; c < 3; ++c) tr += Rm[a][c] * K[c][a];          // trace(R K)
        const double scale = tr / var1;
        double tv[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) tv[a] = mu2[a] - scale * (Rm[a][0] * mu1[0] + Rm[a][1] * mu1[1] + Rm[a][2] * mu1[2]);
        double pa = 0.0;
        for (int j = 0; j < J; ++j) {
            const double p0 = (double)P[3 * j], p1 = (double)P[3 * j + 1], p2 = (double)P[3 * j + 2];
            double d2 = 0.0;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const double d = scale * (Rm[a][0] * p0 + Rm[a][1] * p1 + Rm[a][2] * p2) + tv[a] - (double)G[3 * j + a];
                d2 += d * d;
            }
            pa += sqrt(d2);
        }
        // a 2- or 3-frame tensor is not transposed by the reference: each frame is aligned as 3 points in J dimensions instead
        out[1] = (F == 2 || F == 3) ? jm_pa_untransposed(P, G, J) : pa / (double)J;
        // ACCEL: second differences over frames t, t+1, t+2 (t <= F - 3), mean over the joints              utils.py:372-386
        if (t + 2 < F) {
            double acc = 0.0;
            for (int j = 0; j < J; ++j) {
                double d2 = 0.0;
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const size_t i = 3 * j + k;
                    const double ap = ((double)P[i] - 2.0 * (double)P[i + stride]) + (double)P[i + 2 * stride];
                    const double ag = ((double)G[i] - 2.0 * (double)G[i + stride]) + (double)G[i + 2 * stride];
                    d2 += (ap - ag) * (ap - ag);
                }
                acc += sqrt(d2);
            }
            out[2] = acc / (double)J;
        }
    }
    jm_block_sum(out, s_part);
    if (t < 3) seq_rows[(size_t)b * 3 + t] = (float)(t == 0 ? out[0] : (t == 1 ? out[1] : out[2]));
}

// acc[i] += rows[0][i] + rows[1][i] + ... in fp64, in sequence order: one workgroup, one thread per column
__global__ __launch_bounds__(128) void joint_rows_accumulate_kernel(const float* __restrict__ rows, int B, int W, double* __restrict__ acc) {
    const int i = threadIdx.x;
    if (i >= W) return;
    double a = acc[i];
    for (int b = 0; b < B; ++b) a += (double)rows[(size_t)b * W + i];
    acc[i] = a;
}

int launch_joint_ape_ave(const float* rst, const float* ref, const int32_t* lengths, int B, int F, int J, const int32_t* part_idx,
                         float factor, float* seq_rows, double* acc, hipStream_t s) {
    const int W = 4 + 2 * (J - 1) + 2 * J;
    if (W > 128) return LADIFF_ERR_SHAPE;
    const JmParts pi = {part_idx[0], part_idx[1], part_idx[2], part_idx[3], part_idx[4], part_idx[5], part_idx[6], part_idx[7]};
    hipLaunchKernelGGL(joint_ape_ave_kernel, dim3(B), dim3(JM_THREADS), 0, s, rst, ref, lengths, F, J, pi, (double)factor, seq_rows);
    LADIFF_LAUNCH_CHECK();
    hipLaunchKernelGGL(joint_rows_accumulate_kernel, dim3(1), dim3(128), 0, s, seq_rows, B, W, acc);
    LADIFF_LAUNCH_CHECK();
    return 0;
}

int launch_joint_mr(const float* rst, const float* ref, int B, int F, int J, float* seq_rows, double* acc, hipStream_t s) {
    hipLaunchKernelGGL(joint_mr_kernel, dim3(B), dim3(JM_THREADS), 0, s, rst, ref, F, J, seq_rows);
    LADIFF_LAUNCH_CHECK();
    hipLaunchKernelGGL(joint_rows_accumulate_kernel, dim3(1), dim3(128), 0, s, seq_rows, B, 3, acc);
    LADIFF_LAUNCH_CHECK();
    return 0;
}

}  // namespace ladiff
