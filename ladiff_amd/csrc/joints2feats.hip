// joints2feats on the device: joint positions [L,22,3] -> HumanML3D features [L-1,263], the inverse direction of feats2joints.hip.
//   reference: process_file / uniform_skeleton            (ladiff/data/humanml/scripts/motion_process.py:169-351, :13-36)
//              Skeleton.inverse_kinematics_np / forward_kinematics_np / get_offsets_joints (common/skeleton.py:43-147)
//              qbetween / qmul / qinv / qrot / quaternion_to_cont6d                      (common/quaternion.py)
//              scipy.ndimage.gaussian_filter1d(forward, 20, axis=0, mode='nearest')      (skeleton.py:68)
// The reference runs this on the CPU in numpy / torch, one motion per call; its quaternion helpers work in float32, so the kernel's
// fp32 is the reference's own format for everything but the floor, the initial facing and the forward vector's smoothing.
//
// One workgroup per motion, one thread per input frame (threads past the motion's last frame carry a copy of that frame, so every
// wave-wide exchange below runs with all lanes live; only stores are gated).  The 22 joints of a frame stay in registers: the t2m
// chains are a compile-time list (J2F_CHAINS), so every joint index is a constant.  Phases, with what crosses threads:
//   a  uniform skeleton (only with target offsets): per-frame IK with the unsmoothed forward vector, FK with the target offsets and
//      the root scaled by the leg-length ratio of FRAME 0 (read straight from global memory by every thread)
//   b  floor = min y over the motion (wave shuffles + 4 LDS words), frame 0's root to the XZ origin and its facing to +Z (thread 0
//      computes the quaternion, 6 LDS words)
//   c  forward vector per frame -> LDS (x and z only: y is exactly 0 before and after a filter of zeros), 161-tap gaussian with
//      replicated edges, root quaternion per frame -> LDS
//   d  walk the five chains: local quaternions -> cont6d, stored as they come
//   e  frame t + 1's joints come from the next lane (__shfl_down) and, across a wave boundary, from 4 x 66 LDS words that lane 0
//      of every wave left there; velocities, contacts, rotation-invariant positions, the optional (x - mean) / std in the store
// LDS: 2 x 256 (forward) + 4 x 256 (root quaternions) + 4 x 66 (wave edges) + 81 (filter taps) + 16 words = 7.5 KB.
//
// Reference quirks kept (tests/golden/joints2feats_humanml.npz pins them):
//   * inverse_kinematics_np reads face_joint_idx = [2, 1, 17, 16] as l_hip, r_hip, sdr_r, sdr_l where process_file reads it as
//     r_hip, l_hip, sdr_r, sdr_l: in the IK the hip and shoulder spans enter `across` with opposite signs, in the initial facing they add
//   * qbetween has no special case for anti-parallel vectors
//   * qbetween calls torch.cross WITHOUT a dim, which takes the first dimension of size 3: for the [L,3] arguments of a 3-FRAME
//     motion that is the frame axis.  A motion of exactly 3 frames therefore crosses each coordinate's 3 frame values (cross_frames)
#include "kernels.h"

namespace ladiff {

constexpr int J2F_MAXL = 256, J2F_J = 22, J2F_C = 263, J2F_RADIUS = 80, J2F_CHUNK = 1024;
struct J2FLengths { uint16_t n[J2F_CHUNK]; };        // the motions' frame counts ride in the kernel arguments: no copy, no allocation

// parent, child, the child's raw offset (utils/paramUtil.py t2m_raw_offsets), 1 = first bone of a chain (R restarts from the ROOT's rotation)
#define J2F_CHAINS(B)                                                                              \
    B(0, 2, -1, 0, 0, 1) B(2, 5, 0, -1, 0, 0) B(5, 8, 0, -1, 0, 0) B(8, 11, 0, 0, 1, 0)             \
    B(0, 1, 1, 0, 0, 1) B(1, 4, 0, -1, 0, 0) B(4, 7, 0, -1, 0, 0) B(7, 10, 0, 0, 1, 0)              \
    B(0, 3, 0, 1, 0, 1) B(3, 6, 0, 1, 0, 0) B(6, 9, 0, 1, 0, 0) B(9, 12, 0, 1, 0, 0) B(12, 15, 0, 0, 1, 0) \
    B(9, 14, -1, 0, 0, 1) B(14, 17, 0, -1, 0, 0) B(17, 19, 0, -1, 0, 0) B(19, 21, 0, -1, 0, 0)      \
    B(9, 13, 1, 0, 0, 1) B(13, 16, 0, -1, 0, 0) B(16, 18, 0, -1, 0, 0) B(18, 20, 0, -1, 0, 0)

namespace {

struct V3 { float x, y, z; };
struct Q4 { float w, x, y, z; };

__device__ __forceinline__ float dot3(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ V3 cross3(V3 a, V3 b) { return V3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
// torch.cross(v0, v1) of two [3,3] tensors (3 frames): component c of frame t is element t of (c of frames 0,1,2) x (c of frames 0,1,2)
__device__ __forceinline__ float cross_frames1(float a, float b, int t) {
    const float a0 = __shfl(a, 0), a1 = __shfl(a, 1), a2 = __shfl(a, 2), b0 = __shfl(b, 0), b1 = __shfl(b, 1), b2 = __shfl(b, 2);
    return t == 0 ? a1 * b2 - a2 * b1 : t == 1 ? a2 * b0 - a0 * b2 : a0 * b1 - a1 * b0;
}
__device__ __forceinline__ V3 cross_frames(V3 a, V3 b, int t) {
    return V3{cross_frames1(a.x, b.x, t), cross_frames1(a.y, b.y, t), cross_frames1(a.z, b.z, t)};
}
__device__ __forceinline__ Q4 qinv(Q4 q) { return Q4{q.w, -q.x, -q.y, -q.z}; }
__device__ __forceinline__ Q4 qmul(Q4 q, Q4 r) {                                    // quaternion.py:33-51
    return Q4{r.w * q.w - r.x * q.x - r.y * q.y - r.z * q.z, r.w * q.x + r.x * q.w - r.y * q.z + r.z * q.y,
              r.w * q.y + r.x * q.z + r.y * q.w - r.z * q.x, r.w * q.z - r.x * q.y + r.y * q.x + r.z * q.w};
}
__device__ __forceinline__ V3 qrot(Q4 q, V3 v) {                                    // quaternion.py:54-73
    const V3 qv{q.x, q.y, q.z};
    const V3 uv = cross3(qv, v), uuv = cross3(qv, uv);
    return V3{v.x + 2.f * (q.w * uv.x + uuv.x), v.y + 2.f * (q.w * uv.y + uuv.y), v.z + 2.f * (q.w * uv.z + uuv.z)};
}
// normalize([|v0||v1| + v0.v1, v0 x v1]), quaternion.py:387-397; frames3: the motion has exactly 3 frames (see the head of the file)
__device__ __forceinline__ Q4 qbetween(V3 v0, V3 v1, bool frames3, int t) {
    V3 v;
    if (frames3) v = cross_frames(v0, v1, t);
    else v = cross3(v0, v1);
    const float w = sqrtf(dot3(v0, v0) * dot3(v1, v1)) + dot3(v0, v1);
    const float nrm = sqrtf(w * w + v.x * v.x + v.y * v.y + v.z * v.z);
    return Q4{w / nrm, v.x / nrm, v.y / nrm, v.z / nrm};
}
// one bone of inverse_kinematics_np (skeleton.py:86-99): the local rotation of the child; R becomes the accumulated rotation
__device__ __forceinline__ Q4 ik_bone(Q4& R, V3 u, V3 d, bool frames3, int t) {
    const float len = sqrtf(dot3(d, d));
    const Q4 loc = qmul(qinv(R), qbetween(u, V3{d.x / len, d.y / len, d.z / len}, frames3, t));
    R = qmul(R, loc);
    return loc;
}
// forward vector of inverse_kinematics_np, un-normalised (skeleton.py:58-66): the hip term with the IK's own sign
__device__ __forceinline__ void ik_forward(const float (&px)[J2F_J], const float (&py)[J2F_J], const float (&pz)[J2F_J], float& fx, float& fz) {
    const float ax = (px[1] - px[2]) + (px[17] - px[16]), ay = (py[1] - py[2]) + (py[17] - py[16]), az = (pz[1] - pz[2]) + (pz[17] - pz[16]);
    const float len = sqrtf(ax * ax + ay * ay + az * az);
    fx = az / len; fz = -(ax / len);                                                // cross((0,1,0), across) = (across.z, 0, -across.x)
}
__device__ __forceinline__ Q4 root_from_forward(float fx, float fz, bool frames3, int t) {
    const float len = sqrtf(fx * fx + fz * fz);
    const Q4 q = qbetween(V3{fx / len, 0.f, fz / len}, V3{0.f, 0.f, 1.f}, frames3, t);
    return t == 0 ? Q4{1.f, 0.f, 0.f, 0.f} : q;                                      // skeleton.py:81
}

}  // namespace

__global__ __launch_bounds__(J2F_MAXL) void joints2feats_kernel(const float* __restrict__ joints, int L, const float* __restrict__ tgt,
                                                                float feet_thre, const float* __restrict__ mean,
                                                                const float* __restrict__ stdv, float* __restrict__ feats, int b0,
                                                                const J2FLengths lens) {
    __shared__ float s_fx[J2F_MAXL], s_fz[J2F_MAXL], s_q[J2F_MAXL][4], s_edge[4][3 * J2F_J], s_w[J2F_RADIUS + 1], s_misc[16];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int n = lens.n[blockIdx.x];
    const size_t b = (size_t)b0 + blockIdx.x;
    const bool frames3 = n == 3;
    const int tc = t < n ? t : n - 1;                                               // threads past the end carry the last frame
    const float* motion = joints + b * L * (3 * J2F_J);
    float px[J2F_J], py[J2F_J], pz[J2F_J];
    {
        const float* src = motion + (size_t)tc * (3 * J2F_J);
#pragma unroll
        for (int j = 0; j < J2F_J; ++j) { px[j] = src[3 * j]; py[j] = src[3 * j + 1]; pz[j] = src[3 * j + 2]; }
    }
    if (t <= J2F_RADIUS) s_w[t] = expf(-(float)(t * t) / 800.f);                    // exp(-x^2 / (2 sigma^2)), sigma = 20

    // ---- a. uniform skeleton                                                         motion_process.py:13-36
    if (tgt != nullptr) {
        auto bone_len = [&](int c, int p) {
            const float dx = motion[3 * c] - motion[3 * p], dy = motion[3 * c + 1] - motion[3 * p + 1], dz = motion[3 * c + 2] - motion[3 * p + 2];
            return sqrtf(dx * dx + dy * dy + dz * dz);
        };
        auto max_abs = [&](int c) { return fmaxf(fmaxf(fabsf(tgt[3 * c]), fabsf(tgt[3 * c + 1])), fabsf(tgt[3 * c + 2])); };
        // the raw offsets are unit axes, so |src_offset[i]|.max() is the bone length: lower legs 5 (parent 2) and 8 (parent 5) of frame 0
        const float scale = (max_abs(5) + max_abs(8)) / (bone_len(5, 2) + bone_len(8, 5));
        float fx, fz;
        ik_forward(px, py, pz, fx, fz);
        const Q4 root = root_from_forward(fx, fz, frames3, tc);
        float nx[J2F_J], ny[J2F_J], nz[J2F_J];
        nx[0] = px[0] * scale; ny[0] = py[0] * scale; nz[0] = pz[0] * scale;
        Q4 R = root;
#define J2F_BONE(P, C, UX, UY, UZ, START)                                                                          \
        {                                                                                                          \
            if (START) R = root;                                                                                   \
            ik_bone(R, V3{UX, UY, UZ}, V3{px[C] - px[P], py[C] - py[P], pz[C] - pz[P]}, frames3, tc);              \
            const V3 o = qrot(R, V3{tgt[3 * C], tgt[3 * C + 1], tgt[3 * C + 2]});                                   \
            nx[C] = o.x + nx[P]; ny[C] = o.y + ny[P]; nz[C] = o.z + nz[P];                                         \
        }
        J2F_CHAINS(J2F_BONE)
#undef J2F_BONE
#pragma unroll
        for (int j = 0; j < J2F_J; ++j) { px[j] = nx[j]; py[j] = ny[j]; pz[j] = nz[j]; }
    }

    // ---- b. floor, origin, initial facing                                            motion_process.py:177-213
    float lo = py[0];
#pragma unroll
    for (int j = 1; j < J2F_J; ++j) lo = fminf(lo, py[j]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) lo = fminf(lo, __shfl_xor(lo, o, 64));
    if (lane == 0) s_misc[wave] = lo;
    __syncthreads();
    const float floor_y = fminf(fminf(s_misc[0], s_misc[1]), fminf(s_misc[2], s_misc[3]));
#pragma unroll
    for (int j = 0; j < J2F_J; ++j) py[j] -= floor_y;
    if (t == 0) {
        // here the list IS r_hip, l_hip, sdr_r, sdr_l = 2, 1, 17, 16: both spans point the same way
        const float ax = (px[2] - px[1]) + (px[17] - px[16]), ay = (py[2] - py[1]) + (py[17] - py[16]), az = (pz[2] - pz[1]) + (pz[17] - pz[16]);
        const float alen = sqrtf(ax * ax + ay * ay + az * az);
        const float fx = az / alen, fz = -(ax / alen), flen = sqrtf(fx * fx + fz * fz);
        const Q4 q = qbetween(V3{fx / flen, 0.f, fz / flen}, V3{0.f, 0.f, 1.f}, false, 0);   // a [1,3] call: always the coordinate axis
        s_misc[4] = q.w; s_misc[5] = q.x; s_misc[6] = q.y; s_misc[7] = q.z; s_misc[8] = px[0]; s_misc[9] = pz[0];
    }
    __syncthreads();
    {
        const Q4 q{s_misc[4], s_misc[5], s_misc[6], s_misc[7]};
        const float x0 = s_misc[8], z0 = s_misc[9];
#pragma unroll
        for (int j = 0; j < J2F_J; ++j) {
            const V3 r = qrot(q, V3{px[j] - x0, py[j], pz[j] - z0});
            px[j] = r.x; py[j] = r.y; pz[j] = r.z;                                   // global_positions
        }
    }
    if (lane == 0) {
#pragma unroll
        for (int j = 0; j < J2F_J; ++j) { s_edge[wave][3 * j] = px[j]; s_edge[wave][3 * j + 1] = py[j]; s_edge[wave][3 * j + 2] = pz[j]; }
    }

    // ---- c. smoothed forward vector -> root rotation                                 skeleton.py:58-82
    {
        float fx, fz;
        ik_forward(px, py, pz, fx, fz);
        s_fx[t] = fx; s_fz[t] = fz;                                                  // entries past the motion hold its last frame: mode='nearest'
    }
    __syncthreads();
    Q4 r0;
    {
        float ax = s_fx[t] * s_w[0], az = s_fz[t] * s_w[0], wsum = s_w[0];
        for (int k = 1; k <= J2F_RADIUS; ++k) {
            const int i0 = t - k < 0 ? 0 : t - k, i1 = t + k > J2F_MAXL - 1 ? J2F_MAXL - 1 : t + k;
            const float w = s_w[k];
            ax += (s_fx[i0] + s_fx[i1]) * w; az += (s_fz[i0] + s_fz[i1]) * w; wsum += 2.f * w;
        }
        r0 = root_from_forward(ax / wsum, az / wsum, frames3, tc);
    }
    s_q[t][0] = r0.w; s_q[t][1] = r0.x; s_q[t][2] = r0.y; s_q[t][3] = r0.z;
    __syncthreads();

    const bool live = t < n - 1;                                                     // this thread owns output row t
    // a RUN-time switch on purpose: both modes run the same instructions up to the store, so the normalised output is (raw - mean) / std
    // of the raw mode's very bits (two instantiations contract differently; their values differed in the last place)
    const bool norm = mean != nullptr;
    float* out = feats + (b * (L - 1) + (live ? t : 0)) * J2F_C;
    auto put = [&](int c, float v) {
        if (live) out[c] = norm ? (v - mean[c]) / stdv[c] : v;
    };

    // ---- d. local rotations as cont6d                                                skeleton.py:84-99, quaternion.py:274-311
    {
        Q4 R = r0;
#define J2F_BONE(P, C, UX, UY, UZ, START)                                                                          \
        {                                                                                                          \
            if (START) R = r0;                                                                                     \
            const Q4 q = ik_bone(R, V3{UX, UY, UZ}, V3{px[C] - px[P], py[C] - py[P], pz[C] - pz[P]}, frames3, tc); \
            const float two_s = 2.f / (q.w * q.w + q.x * q.x + q.y * q.y + q.z * q.z);                             \
            const int c = 67 + 6 * (C - 1);                                                                        \
            put(c, 1.f - two_s * (q.y * q.y + q.z * q.z)); put(c + 1, two_s * (q.x * q.y + q.z * q.w));            \
            put(c + 2, two_s * (q.x * q.z - q.y * q.w)); put(c + 3, two_s * (q.x * q.y - q.z * q.w));              \
            put(c + 4, 1.f - two_s * (q.x * q.x + q.z * q.z)); put(c + 5, two_s * (q.y * q.z + q.x * q.w));        \
        }
        J2F_CHAINS(J2F_BONE)
#undef J2F_BONE
    }

    // ---- e. the row's other columns                                                  motion_process.py:229-247, :283-349
    const int t1 = t + 1 > J2F_MAXL - 1 ? J2F_MAXL - 1 : t + 1;
    const Q4 r1{s_q[t1][0], s_q[t1][1], s_q[t1][2], s_q[t1][3]};
    const Q4 rv = qmul(r1, qinv(r0));
    put(0, asinf(fminf(fmaxf(rv.y, -1.f), 1.f)));
    const float* edge = s_edge[(wave + 1) & 3];
    auto next = [&](float v, int slot) {                                             // the same value of frame t + 1
        const float s = __shfl_down(v, 1, 64);
        return lane == 63 ? edge[slot] : s;
    };
    {
        const V3 local = qrot(r0, V3{0.f, py[0], 0.f});
        put(3, local.y);
    }
#pragma unroll
    for (int j = 0; j < J2F_J; ++j) {
        const V3 d{next(px[j], 3 * j) - px[j], next(py[j], 3 * j + 1) - py[j], next(pz[j], 3 * j + 2) - pz[j]};
        if (j == 0) {
            const V3 vel = qrot(r1, d);
            put(1, vel.x); put(2, vel.z);
        } else {
            const V3 local = qrot(r0, V3{px[j] - px[0], py[j], pz[j] - pz[0]});
            put(4 + 3 * (j - 1), local.x); put(5 + 3 * (j - 1), local.y); put(6 + 3 * (j - 1), local.z);
        }
        const V3 lv = qrot(r0, d);
        put(193 + 3 * j, lv.x); put(194 + 3 * j, lv.y); put(195 + 3 * j, lv.z);
        // fid_l = [7, 10] -> columns 259, 260; fid_r = [8, 11] -> 261, 262; contacts are flags: never normalised away from 0 / 1 by mistake
        if (j == 7 || j == 10 || j == 8 || j == 11) {
            const float contact = (d.x * d.x + d.y * d.y) + d.z * d.z < feet_thre ? 1.f : 0.f;
            put(j == 7 ? 259 : j == 10 ? 260 : j == 8 ? 261 : 262, contact);
        }
    }
    // rows past the motion: zeros, as vae.decode leaves padding (in both modes)
    if (!live && t < L - 1) {
        float* pad = feats + (b * (L - 1) + t) * J2F_C;
        for (int c = 0; c < J2F_C; ++c) pad[c] = 0.f;
    }
}

int launch_joints2feats(const float* joints, const int32_t* h_lengths, int B, int L, const float* tgt, float feet_thre, const float* mean,
                        const float* stdv, float* feats, hipStream_t s) {
    if (L < 2 || L > J2F_MAXL) return LADIFF_ERR_SHAPE;
    for (int b = 0; b < B; ++b)
        if (h_lengths[b] < 2 || h_lengths[b] > L) return LADIFF_ERR_SHAPE;
    for (int b0 = 0; b0 < B; b0 += J2F_CHUNK) {
        const int nb = B - b0 < J2F_CHUNK ? B - b0 : J2F_CHUNK;
        J2FLengths lens{};
        for (int i = 0; i < nb; ++i) lens.n[i] = (uint16_t)h_lengths[b0 + i];
        hipLaunchKernelGGL(joints2feats_kernel, dim3(nb), dim3(J2F_MAXL), 0, s, joints, L, tgt, feet_thre, mean, stdv, feats, b0, lens);
        LADIFF_LAUNCH_CHECK();
    }
    return 0;
}

}  // namespace ladiff
