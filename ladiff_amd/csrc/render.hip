// The motion renderer: joint positions [B,L,J,3] -> stick-figure images, one per frame ("frames") or one per motion ("strip").
//   reference: plot_3d_motion (ladiff/data/humanml/utils/plot_script.py) - matplotlib, one frame at a time, tens of seconds per clip -
//              and the Blender "sequence" mode of render_batch; the chains are utils/paramUtil.py's t2m / kit_kinematic_chain.
// The image model is this library's own and is stated in include/ladiff_hip.h ("motion renderer"); tests/render_ref.py restates it.
//
// render_scene_kernel   one workgroup per motion, one thread per frame: min / max over the joints of the frames < len (wave shuffles +
//                       4 x 6 LDS words, no atomics), then the record of the motion: bounds, fitted strip distance, len, the strip's
//                       pose count and pose indices.  The record is all the workspace holds (REC_WORDS words per motion).
// render_raster_kernel  grid (64 x 16 pixel tiles, rendered frames, motions).  A thread owns 4 horizontally adjacent pixels (W % 4 == 0)
//                       and stores 12 bytes (uint8) or 48 bytes (fp32) once: the output is write-only.  Per pose the workgroup projects
//                       the J joints into LDS once, wave 0 tests every bone against the tile (one ballot: the surviving bones keep their
//                       order, which the compositing needs) and the threads walk the survivors; an empty tile costs the ground and the
//                       stores.  An image past its motion's length reads one word of the record and stores the background.
// Arithmetic is fp32 in every build flavour (no operand of this file is split); min / max are exact in any order and every other value
// of an image comes from its own motion's record and joints, so an image's bits do not depend on the batch it was launched in.
// Frames mode writes H x W x 3 bytes per image and reads 264 bytes of joints for it; measured it runs at 11.8 x a memset
// of its output: the per-pixel arithmetic and the per-pose barriers bound it, not yet the stores.
#include "kernels.h"

namespace ladiff {

constexpr int RND_MAXL = 256, RND_MAXJ = 22, RND_CHUNK = 1024, RND_TW = 64, RND_TH = 16, RND_THREADS = 256;
// the record of a motion, in 4-byte words: mins xyz, maxs xyz, the strip's camera distance | len, the strip's pose count | pose indices
constexpr int REC_MINS = 0, REC_MAXS = 3, REC_DIST = 6, REC_LEN = 7, REC_N = 8, REC_POSE = 16, REC_WORDS = REC_POSE + RND_MAXL;
struct RenderLengths { uint16_t n[RND_CHUNK]; };     // the frame counts ride in the scene kernel's arguments: no copy, no allocation

// what the raster kernel takes by value: the camera basis (computed on the host in double, rounded once) and the style
struct RenderCam {
    float dir[3], f[3], r[3], u[3];                  // eye = target + distance * dir; forward, right, up
    float target_y, dist, F, near, reach;            // reach = 0.5 + line_width / 2: where a bone's coverage reaches 0
    float margin, a_min, g_alpha;
    float bg[3], ground[3], chain[5][3];
};

namespace {

// (joint, joint, chain) of every bone, chains in table order, bones in chain order (utils/paramUtil.py)
constexpr int T2M_BONES = 21, KIT_BONES = 20;
__device__ const unsigned char RND_BONES[2][T2M_BONES][3] = {
    {{0, 2, 0}, {2, 5, 0}, {5, 8, 0}, {8, 11, 0}, {0, 1, 1}, {1, 4, 1}, {4, 7, 1}, {7, 10, 1}, {0, 3, 2}, {3, 6, 2}, {6, 9, 2}, {9, 12, 2},
     {12, 15, 2}, {9, 14, 3}, {14, 17, 3}, {17, 19, 3}, {19, 21, 3}, {9, 13, 4}, {13, 16, 4}, {16, 18, 4}, {18, 20, 4}},
    {{0, 11, 0}, {11, 12, 0}, {12, 13, 0}, {13, 14, 0}, {14, 15, 0}, {0, 16, 1}, {16, 17, 1}, {17, 18, 1}, {18, 19, 1}, {19, 20, 1}, {0, 1, 2},
     {1, 2, 2}, {2, 3, 2}, {3, 4, 2}, {3, 5, 3}, {5, 6, 3}, {6, 7, 3}, {3, 8, 4}, {8, 9, 4}, {9, 10, 4}, {0, 0, 0}}};

__device__ __forceinline__ float clamp01(float v) { return fminf(fmaxf(v, 0.f), 1.f); }      // NaN -> 0
__device__ __forceinline__ unsigned to_byte(float c) { return (unsigned)floorf(255.f * clamp01(c) + 0.5f); }

}  // namespace

__global__ __launch_bounds__(RND_THREADS) void render_scene_kernel(const float* __restrict__ joints, int L, int J, int n_poses, float dist,
                                                                   float strip_fit, float* __restrict__ ws, int b0,
                                                                   const RenderLengths lens) {
    __shared__ float s_red[RND_THREADS / 64][6];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int len = lens.n[blockIdx.x];
    const size_t b = (size_t)b0 + blockIdx.x;
    // threads past the motion's end read its frame 0 again: a minimum and a maximum do not change
    const float* src = joints + (b * L + (t < len ? t : 0)) * (size_t)(3 * J);
    float lo[3] = {src[0], src[1], src[2]}, hi[3] = {src[0], src[1], src[2]};
    for (int j = 1; j < J; ++j)
#pragma unroll
        for (int c = 0; c < 3; ++c) { lo[c] = fminf(lo[c], src[3 * j + c]); hi[c] = fmaxf(hi[c], src[3 * j + c]); }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { lo[c] = fminf(lo[c], __shfl_xor(lo[c], o, 64)); hi[c] = fmaxf(hi[c], __shfl_xor(hi[c], o, 64)); }
        if (lane == 0) { s_red[wave][c] = lo[c]; s_red[wave][3 + c] = hi[c]; }
    }
    __syncthreads();
    float* rec = ws + b * REC_WORDS;
    int* reci = reinterpret_cast<int*>(rec);
    const int n = n_poses < len ? n_poses : len;
    if (t == 0) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            lo[c] = fminf(fminf(s_red[0][c], s_red[1][c]), fminf(s_red[2][c], s_red[3][c]));
            hi[c] = fmaxf(fmaxf(s_red[0][3 + c], s_red[1][3 + c]), fmaxf(s_red[2][3 + c], s_red[3][3 + c]));
            rec[REC_MINS + c] = lo[c]; rec[REC_MAXS + c] = hi[c];
        }
        const float extent = fmaxf(hi[0] - lo[0], hi[2] - lo[2]);
        rec[REC_DIST] = dist * fmaxf(1.f, extent / strip_fit);
        reci[REC_LEN] = len; reci[REC_N] = n;
    }
    if (t < n) reci[REC_POSE + t] = n > 1 ? (t * (len - 1) + (n - 1) / 2) / (n - 1) : 0;
}

__global__ __launch_bounds__(RND_THREADS) void render_raster_kernel(const float* __restrict__ joints, const float* __restrict__ ws, int L, int J,
                                                                    int strip, int stride, int H, int W, int Lp, void* __restrict__ out,
                                                                    int out_is_float, int b0, const RenderCam cam) {
    __shared__ float s_sx[RND_MAXJ], s_sy[RND_MAXJ], s_zc[RND_MAXJ];
    __shared__ unsigned s_mask;
    const int tid = threadIdx.x;
    const int tiles_x = (W + RND_TW - 1) / RND_TW;
    const int tile_x = (blockIdx.x % tiles_x) * RND_TW, tile_y = (blockIdx.x / tiles_x) * RND_TH;
    const int col = tile_x + (tid & 15) * 4, row = tile_y + (tid >> 4);
    const size_t b = (size_t)b0 + blockIdx.z;
    const float* rec = ws + b * REC_WORDS;
    const int* reci = reinterpret_cast<const int*>(rec);
    const int len = reci[REC_LEN];
    const int t = strip ? 0 : blockIdx.y * stride;
    const size_t image = strip ? b : b * Lp + blockIdx.y;

    float c[4][3];
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
        for (int k = 0; k < 3; ++k) c[p][k] = cam.bg[k];

    if (t < len) {                                   // the same for the whole workgroup
        const float* motion = joints + b * L * (size_t)(3 * J);
        const float floor_y = rec[REC_MINS + 1];
        const float d = strip ? rec[REC_DIST] : cam.dist;
        const float ex = d * cam.dir[0], ey = cam.target_y + d * cam.dir[1], ez = d * cam.dir[2];      // the eye
        float offx, offz, x0, x1, z0, z1;            // what x and z are reduced by, and the ground rectangle after that
        if (strip) {
            offx = 0.5f * (rec[REC_MINS] + rec[REC_MAXS]); offz = 0.5f * (rec[REC_MINS + 2] + rec[REC_MAXS + 2]);
            x0 = rec[REC_MINS] - offx - cam.margin; x1 = rec[REC_MAXS] - offx + cam.margin;
            z0 = rec[REC_MINS + 2] - offz - cam.margin; z1 = rec[REC_MAXS + 2] - offz + cam.margin;
        } else {
            offx = motion[(size_t)t * (3 * J)]; offz = motion[(size_t)t * (3 * J) + 2];
            x0 = rec[REC_MINS] - offx; x1 = rec[REC_MAXS] - offx;
            z0 = rec[REC_MINS + 2] - offz; z1 = rec[REC_MAXS + 2] - offz;
        }
        const float py = (float)row + 0.5f, half_w = 0.5f * (float)W, half_h = 0.5f * (float)H;

        // ---- the ground, by ray
        {
            const float cy = -(py - half_h) / cam.F;
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                const float cx = ((float)(col + p) + 0.5f - half_w) / cam.F;
                const float dx = cam.f[0] + cx * cam.r[0] + cy * cam.u[0], dy = cam.f[1] + cx * cam.r[1] + cy * cam.u[1],
                            dz = cam.f[2] + cx * cam.r[2] + cy * cam.u[2];
                if (dy < 0.f) {
                    const float th = -ey / dy, hx = ex + th * dx, hz = ez + th * dz;
                    const float sd = fminf(fminf(hx - x0, x1 - hx), fminf(hz - z0, z1 - hz));
                    const float q = cam.g_alpha * clamp01(0.5f + sd * cam.F / th);
#pragma unroll
                    for (int k = 0; k < 3; ++k) c[p][k] = c[p][k] * (1.f - q) + cam.ground[k] * q;
                }
            }
        }

        // ---- the poses, in time order
        const int n = strip ? reci[REC_N] : 1;
        const int nbones = J == 22 ? T2M_BONES : KIT_BONES;
        const unsigned char(*bones)[3] = RND_BONES[J == 22 ? 0 : 1];
        for (int k = 0; k < n; ++k) {
            const int tk = strip ? reci[REC_POSE + k] : t;
            const float alpha = n > 1 ? cam.a_min + (1.f - cam.a_min) * ((float)k / (float)(n - 1)) : 1.f;
            __syncthreads();                         // the previous pose's readers are done
            if (tid < J) {
                const float* q = motion + ((size_t)tk * J + tid) * 3;
                const float vx = q[0] - offx - ex, vy = q[1] - floor_y - ey, vz = q[2] - offz - ez;
                const float zc = vx * cam.f[0] + vy * cam.f[1] + vz * cam.f[2];
                s_sx[tid] = half_w + cam.F * (vx * cam.r[0] + vy * cam.r[1] + vz * cam.r[2]) / zc;
                s_sy[tid] = half_h - cam.F * (vx * cam.u[0] + vy * cam.u[1] + vz * cam.u[2]) / zc;
                s_zc[tid] = zc;
            }
            __syncthreads();
            if (tid < 64) {                          // wave 0: one bone per lane against the tile, grown by the reach and a pixel of slack
                bool keep = false;
                if (tid < nbones) {
                    const int ja = bones[tid][0], jb = bones[tid][1];
                    const float ax = s_sx[ja], ay = s_sy[ja], bx = s_sx[jb], by = s_sy[jb], grow = cam.reach + 1.f;
                    keep = s_zc[ja] > cam.near && s_zc[jb] > cam.near && fmaxf(ax, bx) + grow >= (float)tile_x &&
                           fminf(ax, bx) - grow <= (float)(tile_x + RND_TW) && fmaxf(ay, by) + grow >= (float)tile_y &&
                           fminf(ay, by) - grow <= (float)(tile_y + RND_TH);
                }
                const unsigned long long m = __ballot(keep);
                if (tid == 0) s_mask = (unsigned)m;
            }
            __syncthreads();
            unsigned m = __builtin_amdgcn_readfirstlane(s_mask);
            while (m) {
                const int i = __ffs(m) - 1;
                m &= m - 1;
                const int ja = bones[i][0], jb = bones[i][1], chain = bones[i][2];
                const float ax = s_sx[ja], ay = s_sy[ja], bex = s_sx[jb] - ax, bey = s_sy[jb] - ay;
                const float den = fmaxf(bex * bex + bey * bey, 1e-12f);
                const float dy = py - ay;
#pragma unroll
                for (int p = 0; p < 4; ++p) {
                    const float px = (float)(col + p) + 0.5f, dx = px - ax;
                    const float s = clamp01((dx * bex + dy * bey) / den);
                    const float qx = px - (ax + s * bex), qy = py - (ay + s * bey);
                    const float q = alpha * clamp01(cam.reach - sqrtf(qx * qx + qy * qy));
#pragma unroll
                    for (int ch = 0; ch < 3; ++ch) c[p][ch] = c[p][ch] * (1.f - q) + cam.chain[chain][ch] * q;
                }
            }
        }
    }

    if (col < W && row < H) {
        const size_t pixel = (image * H + row) * W + col;
        if (out_is_float) {
            f32x4* dst = reinterpret_cast<f32x4*>(reinterpret_cast<float*>(out) + pixel * 3);
            dst[0] = f32x4{c[0][0], c[0][1], c[0][2], c[1][0]};
            dst[1] = f32x4{c[1][1], c[1][2], c[2][0], c[2][1]};
            dst[2] = f32x4{c[2][2], c[3][0], c[3][1], c[3][2]};
        } else {
            unsigned v[12];
#pragma unroll
            for (int p = 0; p < 4; ++p)
#pragma unroll
                for (int k = 0; k < 3; ++k) v[3 * p + k] = to_byte(c[p][k]);
            unsigned* dst = reinterpret_cast<unsigned*>(reinterpret_cast<unsigned char*>(out) + pixel * 3);
#pragma unroll
            for (int w = 0; w < 3; ++w) dst[w] = v[4 * w] | (v[4 * w + 1] << 8) | (v[4 * w + 2] << 16) | (v[4 * w + 3] << 24);
        }
    }
}

size_t render_ws_bytes(int B) { return B > 0 ? (size_t)B * REC_WORDS * sizeof(float) : 0; }

int launch_render_motion(const float* joints, const int32_t* h_lengths, int B, int L, int J, const ladiff_render_params& P, int mode,
                         int n_poses, int H, int W, void* out, int out_is_float, float* ws, size_t ws_bytes, hipStream_t s) {
    // ---- every refusal, on the host, before anything is enqueued
    const auto unit = [](float v) { return v >= 0.f && v <= 1.f; };
    bool ok = (mode == LADIFF_RENDER_FRAMES || mode == LADIFF_RENDER_STRIP) && n_poses >= 1 && P.frame_stride >= 1 && fabsf(P.elev_deg) < 90.f &&
              P.dist > 0.f && P.focal > 0.f && P.line_width > 0.f && P.near_plane > 0.f && P.strip_fit > 0.f && P.ground_margin >= 0.f &&
              unit(P.alpha_min) && unit(P.ground_alpha) && P.azim_deg == P.azim_deg && P.target_height == P.target_height;
    for (int k = 0; k < 3; ++k) ok = ok && unit(P.background_rgb[k]) && unit(P.ground_rgb[k]);
    for (int k = 0; k < 15; ++k) ok = ok && unit(P.chain_rgb[k / 3][k % 3]);
    LADIFF_CHECK_ARG(ok);
    const double rad = 3.14159265358979323846 / 180.0, el = P.elev_deg * rad, az = P.azim_deg * rad;
    const double dir[3] = {cos(el) * sin(az), sin(el), cos(el) * cos(az)};
    LADIFF_CHECK_ARG((double)P.target_height + (double)P.dist * dir[1] > 0.0);
    if (L < 1 || L > RND_MAXL || H < 16 || H > 1024 || W < 16 || W > 1024 || W % 4 != 0) return LADIFF_ERR_SHAPE;
    for (int b = 0; b < B; ++b)
        if (h_lengths[b] < 1 || h_lengths[b] > L) return LADIFF_ERR_SHAPE;
    if ((reinterpret_cast<uintptr_t>(joints) & 3) || (reinterpret_cast<uintptr_t>(ws) & 3) ||
        (reinterpret_cast<uintptr_t>(out) & (out_is_float ? 15 : 3)))
        return LADIFF_ERR_SHAPE;
    if (ws_bytes < render_ws_bytes(B)) return LADIFF_ERR_WORKSPACE;

    // ---- the camera: f = normalize(T - E) = -dir, r = normalize(f x (0,1,0)), u = r x f; none of them depends on the distance
    RenderCam cam{};
    const double f[3] = {-dir[0], -dir[1], -dir[2]};
    const double rn = sqrt(f[2] * f[2] + f[0] * f[0]);                   // > 0: |el| < 90
    const double r[3] = {-f[2] / rn, 0.0, f[0] / rn};
    const double u[3] = {r[1] * f[2] - r[2] * f[1], r[2] * f[0] - r[0] * f[2], r[0] * f[1] - r[1] * f[0]};
    for (int k = 0; k < 3; ++k) {
        cam.dir[k] = (float)dir[k]; cam.f[k] = (float)f[k]; cam.r[k] = (float)r[k]; cam.u[k] = (float)u[k];
        cam.bg[k] = P.background_rgb[k]; cam.ground[k] = P.ground_rgb[k];
        for (int ch = 0; ch < 5; ++ch) cam.chain[ch][k] = P.chain_rgb[ch][k];
    }
    cam.target_y = P.target_height; cam.dist = P.dist; cam.F = (float)((double)P.focal * H / 2.0); cam.near = P.near_plane;
    cam.reach = 0.5f + P.line_width / 2.f; cam.margin = P.ground_margin; cam.a_min = P.alpha_min; cam.g_alpha = P.ground_alpha;

    const int strip = mode == LADIFF_RENDER_STRIP, stride = strip ? 1 : P.frame_stride;
    const int Lp = strip ? 1 : (L + stride - 1) / stride;
    const int tiles = ((W + RND_TW - 1) / RND_TW) * ((H + RND_TH - 1) / RND_TH);
    for (int b0 = 0; b0 < B; b0 += RND_CHUNK) {
        const int nb = B - b0 < RND_CHUNK ? B - b0 : RND_CHUNK;
        RenderLengths lens{};
        for (int i = 0; i < nb; ++i) lens.n[i] = (uint16_t)h_lengths[b0 + i];
        hipLaunchKernelGGL(render_scene_kernel, dim3(nb), dim3(RND_THREADS), 0, s, joints, L, J, n_poses, P.dist, P.strip_fit, ws, b0, lens);
        LADIFF_LAUNCH_CHECK();
        hipLaunchKernelGGL(render_raster_kernel, dim3(tiles, Lp, nb), dim3(RND_THREADS), 0, s, joints, (const float*)ws, L, J, strip, stride, H, W,
                           Lp, out, out_is_float, b0, cam);
        LADIFF_LAUNCH_CHECK();
    }
    return 0;
}

}  // namespace ladiff
