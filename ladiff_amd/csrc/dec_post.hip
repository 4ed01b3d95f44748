// The decoder layer from the self-attention output to the layer output as ONE kernel (f16x3 mode):
//   x1n = LN1(x0 + att Wo^T + bo),   x2 = LN2(x1n + cross(x1n)),   y = LN3(x2 + W2 gelu(W1 x2 + b1) + b2)   [+ decoder.norm]
// TransformerDecoderLayer.forward_post, cross_attention.py:369-376, :407-412 (+ :150-151 on the last layer).
//
// Before: dec_out_cross_kernel (out_proj .. norm2; writes x2 as fp32 AND as S-format rows) + dec_mlp_kernel (reads both back).  Both are
// row-wise and all their workgroups load, compute and store in lockstep, so the memory phases at the seam add up.  Here the feed-forward
// kernel's skeleton (dec_mlp.hip, <8, 1>: eight waves x 16 rows, the rows as MFMA B fragments in registers, every product transposed,
// the weights through the eight-stage LDS-DMA ring in groups of four with exact vmcnt(0) waits) runs ONE MORE leading iteration:
//   * Wo (256 x 256, S-format) is 16 more stages of the ring's shape: two 128-row panels x eight 32-k steps, dealt by the same pi_row
//     permutation, multiplied with the wave's att rows (read from the S-format att buffer as dec_mlp reads xs) into `oacc`.
//   * mid-epilogue, per wave, in the accumulator layout (lane (frow, fk): row frow, four consecutive columns per accumulator):
//     LN1 of x0 + bo + att Wo^T (in-lane sum + two cross-lane steps); because of pi_row the result turns into the B fragments of the next
//     product by an in-lane split8.  Cross-attention with the folded keys / values of dec_cross.hip on the MFMA:
//       scores^T [32 x 16] = G x1n^T, G's rows dealt so that lane group fk holds head fk's 8 tokens across the two score tiles:
//       + c, mask by counts, softmax in base 2 - all in-lane - and the probabilities ARE the B fragment (k = 8 head + token) of
//       out^T = U^T P^T, which accumulates on top of x1n + bo_cross in `oacc`'s layout.  LN2 -> x2.
//     x2 is split in-lane into the feed-forward's B fragments, and x2 + b2 is what linear2's accumulators START from: the residual
//     needs no registers of its own and no trip through memory (as x0 + bo is what out_proj's accumulators start from).
//     x0 + out_proj(att), x1n and x2 never exist in memory.
//   * G is read as it lies (rows of 256 floats: two 16-byte loads per lane and k-step); U is needed TRANSPOSED (a lane's 8 values of
//     a U^T fragment are 8 different rows of U), so dec_post_gu_kernel re-lays each sample's U IN PLACE beforehand (its H T rows of
//     1 KiB, the odd ones of G | U) as U^T in fragment order: float (jj T + e) 64 + lane = U[head lane >> 4][token e][col(jj, lane & 15)]
//     - every U load of a wave is 256 contiguous bytes.  Same floats, same place: the workspace does not grow.
//   * no LDS-DMA is in flight inside the mid-epilogue (the wave waits vmcnt(0) in front of it), so its plain loads are waited for
//     with ordinary counted waits; it has no workgroup barrier - the waves meet again at the ring's next barrier.
// Row tiles are aligned to samples (ceil(len / 16) tiles per sample, padded and ragged alike): a tile has one sample's G | U | c | count.
#include <mutex>
#include "model.h"
#include "tile_mma.h"

namespace ladiff {

namespace {

constexpr int PST_NS = 8;                      // ring stages: two groups of PST_GRP
constexpr int PST_GRP = 4;                     // stages a wave requests as ONE batch and waits for with vmcnt(0)
constexpr int PST_STAGE = 16384;               // bytes: 128 weight rows x 128 B
constexpr int PST_NV = 11;                     // per-column vectors in LDS: b2, g3, be3, g4, be4 | bo, g1, be1, bo_cross, g2, be2
constexpr int PST_LDS = PST_NS * PST_STAGE + FF * 4 + PST_NV * D * 4;

typedef unsigned u32x4_p __attribute__((ext_vector_type(4)));

// weight row (within a 128-row panel) that sits in LDS row p of a stage (dec_mlp.hip)
__device__ __forceinline__ int pi_row(int p) { const int j = p >> 4, n = p & 15; return 32 * (j >> 1) + 8 * (n >> 2) + 4 * (j & 1) + (n & 3); }

template <int N> __device__ __forceinline__ void wait_vm() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }
template <int OFF>
__device__ __forceinline__ void fetch16(u32x4_p& v, unsigned addr) {
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "n"(OFF) : "memory");
}
template <int N>
__device__ __forceinline__ void wait_lgkm(u32x4_p& a, u32x4_p& b, u32x4_p& c, u32x4_p& d) {
    asm volatile("s_waitcnt lgkmcnt(%4)" : "+v"(a), "+v"(b), "+v"(c), "+v"(d) : "n"(N));
}
__device__ __forceinline__ s16x8 as_s16(const u32x4_p v) { return __builtin_bit_cast(s16x8, v); }

}  // namespace

// Each sample's U rows ([H][T][2][256]: G row, U row alternating, dec_cross_prep_kernel) re-laid in place for dec_post_kernel as U^T in
// fragment order: float o = (jj T + e) 64 + lane of the H T x 256 U floats = U[head lane >> 4][token e][column col(jj, lane & 15)],
// 1-KiB piece o >> 8 in the place of U row o >> 8.  G is not touched.  grid (B, layers); the sample's U is in LDS before anything is written.
__global__ __launch_bounds__(256) void dec_post_gu_kernel(float* guws, size_t gu_layer, int T) {
    __shared__ float us[32 * 257];
    const int tid = threadIdx.x, HT = H * T;
    float* g = guws + blockIdx.y * gu_layer + (size_t)blockIdx.x * HT * 2 * D;
    for (int hj = 0; hj < HT; ++hj) us[hj * 257 + tid] = g[(size_t)(2 * hj + 1) * D + tid];
    __syncthreads();                                                       // every load of the sample has returned (the barrier's fence)
    const int lane = tid & 63, n = lane & 15, fk = lane >> 4;
    for (int i = 0; i < HT; ++i) {
        const int q = 4 * i + (tid >> 6), jj = q / T, e = q - jj * T;
        const int col = 32 * (jj >> 1) + 8 * (n >> 2) + 4 * (jj & 1) + (n & 3);
        g[(size_t)(2 * i + 1) * D + tid] = us[(fk * T + e) * 257 + col];
    }
}

template <int TT>
__global__ __launch_bounds__(512, 2) void dec_post_kernel(const DecPostArgs p) {
    constexpr int NW = 8, NT = 64 * NW, PPW = 16 / NW;                     // waves, threads, DMA pieces per wave and stage
    extern __shared__ __attribute__((aligned(1024))) char lds[];
    float* const b1s = reinterpret_cast<float*>(lds + PST_NS * PST_STAGE);
    float* const prm = b1s + FF;                                          // [PST_NV][256]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int frow = lane & 15, fk = lane >> 4;
    constexpr int T = TT;
    const int M = p.M;

    // ---- this wave's row tile: tile t of the list "sample 0's ceil(len / 16) tiles, sample 1's, ..."
    const int t = blockIdx.x * NW + wave;
    int b = 0, f0 = 0, len = p.F, ntiles;
    if (p.row_off == nullptr) {
        const int tps = (p.F + 15) >> 4;
        ntiles = p.B * tps;
        b = t / tps; f0 = 16 * (t - b * tps);
    } else {
        int base = 0;
        for (int i0 = 0; i0 < p.B; i0 += 64) {                             // 64 samples at a time: inclusive scan of their tile counts
            const int i = i0 + lane;
            const int nt = i < p.B ? (p.row_off[i + 1] - p.row_off[i] + 15) >> 4 : 0;
            int incl = nt;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) { const int up = __shfl_up(incl, o, 64); if (lane >= o) incl += up; }
            incl += base;
            const unsigned long long hit = __ballot(t >= incl - nt && t < incl);
            if (hit != 0ull) {                                             // at most one sample owns tile t
                const int src = __ffsll((long long)hit) - 1;
                b = i0 + src; f0 = 16 * (t - __shfl(incl - nt, src, 64));
            }
            base = __shfl(incl, 63, 64);
        }
        ntiles = base;
    }
    if (blockIdx.x * NW >= ntiles) return;                                 // uniform over the workgroup (the ragged grid is an upper bound)
    const bool tile_ok = t < ntiles;
    b = __builtin_amdgcn_readfirstlane(tile_ok ? b : 0);
    f0 = __builtin_amdgcn_readfirstlane(tile_ok ? f0 : 0);
    int srow = b * p.F;
    if (p.row_off != nullptr) { srow = p.row_off[b]; len = p.row_off[b + 1] - srow; }
    int nrows = len - f0 < 16 ? len - f0 : 16;                             // rows of the tile that exist; a tile without rows computes on row M - 1 and stores nothing
    nrows = tile_ok ? nrows : 0;
    const int row0 = srow + f0;
    const int myrow = nrows > 0 ? row0 + (frow < nrows ? frow : nrows - 1) : M - 1;

    // ---- the wave's att rows as operand fragments: k-step s (32 columns) -> hi / lo 16 bytes of lane (row frow, k 8 fk .. + 7);
    // the same registers hold x1n's and then x2's fragments
    s16x8 xh[8], xl[8];
    {
        const char* xr = reinterpret_cast<const char*>(p.att) + (size_t)myrow * 1024 + fk * 16;
#pragma unroll
        for (int s = 0; s < 8; ++s) {
            xh[s] = *reinterpret_cast<const s16x8*>(xr + (s >> 1) * 256 + (s & 1) * 64);
            xl[s] = *reinterpret_cast<const s16x8*>(xr + (s >> 1) * 256 + (s & 1) * 64 + 128);
        }
    }
    // out_proj's accumulators start from the residual x0 (+ bo below): lane (frow, fk) holds row frow, columns col(jj) .. + 3 of accumulator jj
    f32x4 hacc[8], oacc[16];
#pragma unroll
    for (int jj = 0; jj < 16; ++jj) oacc[jj] = ld4(p.x0 + (size_t)myrow * D + 32 * (jj >> 1) + 8 * fk + 4 * (jj & 1));
    // the sample's score offsets of head fk and its count of valid tokens: needed in the middle of the kernel, asked for here
    float cv[8];
    {
        const float* cb = p.cc + (size_t)b * (H * T) + fk * T;
#pragma unroll
        for (int e = 0; e < 8; ++e) cv[e] = e < T ? cb[e < T ? e : 0] : 0.f;
    }
    int nv = p.counts != nullptr ? p.counts[b] : T;
    nv = nv > T ? T : nv;
    for (int i = tid; i < FF / 4; i += NT) st4(b1s + 4 * i, ld4(p.b1 + 4 * i));
    for (int i = tid; i < PST_NV * D / 4; i += NT) {
        const int which = i / (D / 4), c4 = i % (D / 4);
        const float* src = which == 0 ? p.b2 : which == 1 ? p.g3 : which == 2 ? p.be3 : which == 3 ? p.g4 : which == 4 ? p.be4
                         : which == 5 ? p.bo : which == 6 ? p.g1 : which == 7 ? p.be1 : which == 8 ? p.bo_c : which == 9 ? p.g2 : p.be2;
        if (src != nullptr) st4(prm + 4 * i, ld4(src + 4 * c4));
    }

    // ---- LDS-DMA of one stage: wave w brings the PPW pieces (a piece = 8 LDS rows x 128 B) q = w + NW i: LDS rows 8 q + (lane >> 3)
    const int cs = (lane & 7) ^ ((lane >> 4) & 3) ^ (4 * (wave & 1));    // source slot that lands in LDS slot (lane & 7) (dec_mlp.hip)
    const int koff = (cs < 4 ? cs * 4 : 32 + (cs - 4) * 4);              // floats inside the 64-float S-block: hi | lo halves
    int src[PPW];
#pragma unroll
    for (int i = 0; i < PPW; ++i) src[i] = pi_row(8 * (wave + NW * i) + (lane >> 3));
    char* const dma_dst = lds + (8 * wave) * 128;
    // piece i of a stage.  Wo iteration, stage u: k-step c = u >> 1 of the 256 model columns, Wo rows 128 (u & 1) ..
    // feed-forward slice hs, stage u: u < 8: W1 rows 128 hs .., k-step u;  u >= 8: v = u - 8, k-step v >> 1 of the slice, W2 rows 128 (v & 1) ..
    auto issue = [&](auto woc, int hs, auto uc, auto slotc, auto ic) __attribute__((always_inline)) {
        constexpr bool wo = decltype(woc)::value != 0;
        constexpr int u = decltype(uc)::value, slot = decltype(slotc)::value, i = decltype(ic)::value;
        const float* base; int ldw, n0, kb, half;
        if constexpr (wo) { constexpr int c = u >> 1; base = p.wo; ldw = D; n0 = 128 * (u & 1); kb = c >> 1; half = c & 1; }
        else if constexpr (u < 8) { base = p.w1; ldw = D; n0 = 128 * hs; kb = u >> 1; half = u & 1; }
        else { constexpr int v = u - 8, c = v >> 1; base = p.w2; ldw = FF; n0 = 128 * (v & 1); kb = 2 * hs + (c >> 1); half = c & 1; }
        const float* s0 = base + (size_t)(n0 + src[i]) * ldw + kb * 64 + half * 16 + koff;
        __builtin_amdgcn_global_load_lds(s0, (__attribute__((address_space(3))) void*)(dma_dst + slot * PST_STAGE + 8 * NW * i * 128), 16, 0, 0);
    };

    // fragment read addresses: tile j of a stage = LDS rows 16 j + frow; hi slot fk, lo slot 4 + fk, XORed with (frow >> 1) & 7
    const int sw = (frow >> 1) & 7;
    const unsigned rd_hi = lds_addr(lds) + frow * 128 + ((fk ^ sw) << 4);
    const unsigned rd_lo = lds_addr(lds) + frow * 128 + (((4 + fk) ^ sw) << 4);
    const unsigned rd_hi2 = rd_hi + 4 * PST_STAGE, rd_lo2 = rd_lo + 4 * PST_STAGE;

    s16x8 hh[4], hl[4];

    // one stage's products (dec_mlp.hip's stage_mma with one row tile per wave): acc[J0 + j] += W(tile j) . b^T over its 32 k, three
    // MFMAs per product (x_lo W_hi, x_hi W_lo, x_hi W_hi); the weight fragments run through a ring of four tile buffers that crosses
    // the stage boundaries, `next()` (the DMA wait / barrier) in front of tile 5, between(g) behind tile 2 g + 1
    u32x4_p wt[4][2];
    auto fetch_tile = [&](auto slotc, auto jc) __attribute__((always_inline)) {
        constexpr int slot = decltype(slotc)::value, j = decltype(jc)::value;
        const unsigned ah = slot < 4 ? rd_hi : rd_hi2, al = slot < 4 ? rd_lo : rd_lo2;
        constexpr int so = (slot & 3) * PST_STAGE;
        fetch16<so + j * 2048>(wt[j & 3][0], ah); fetch16<so + j * 2048>(wt[j & 3][1], al);
    };
    auto stage_mma = [&](auto slotc, auto& acc, auto j0c, const s16x8 bh, const s16x8 bl, auto&& between, auto&& next) __attribute__((always_inline)) {
        constexpr int slot = decltype(slotc)::value, J0 = decltype(j0c)::value;
        static_for<8>([&](auto jc) {
            constexpr int j = decltype(jc)::value, cur = j & 3;
            next(jc);
            asm volatile("s_waitcnt lgkmcnt(4)" : "+v"(wt[cur][0]), "+v"(wt[cur][1]));      // outstanding behind tile j's two reads: tiles j + 1, j + 2
            __builtin_amdgcn_sched_barrier(0);
            acc[J0 + j] = MFMA16_S16(as_s16(wt[cur][0]), bl, acc[J0 + j], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
            if constexpr (j + 3 < 8) fetch_tile(slotc, IntC<j + 3>{});
            else fetch_tile(IntC<(slot + 1) % PST_NS>{}, IntC<j + 3 - 8>{});
            __builtin_amdgcn_sched_barrier(0);
            acc[J0 + j] = MFMA16_S16(as_s16(wt[cur][1]), bh, acc[J0 + j], 0, 0, 0);
            acc[J0 + j] = MFMA16_S16(as_s16(wt[cur][0]), bh, acc[J0 + j], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
            if constexpr (j & 1) between(IntC<j / 2>{});
        });
    };

    // ---- the weight stream: dec_mlp.hip's batches (one per wave in flight, every wait vmcnt(0) with nothing younger outstanding,
    // barriers B1 / B2, the same issue schedule), over 16 Wo stages + 8 x 16 feed-forward stages
    auto landed = [&]() __attribute__((always_inline)) {
        wait_vm<0>();
        __builtin_amdgcn_s_barrier();
    };
    auto stage = [&](auto woc, int hs, auto uc) __attribute__((always_inline)) {
        constexpr bool wo = decltype(woc)::value != 0;
        constexpr int u = decltype(uc)::value, slot = u % PST_NS, r = u % PST_GRP;
        // piece `half` of the stage `ahead` further: behind the Wo iteration comes slice 0, behind the last slice a harmless re-fetch (slice 0)
        auto batch_piece = [&](auto aheadc, auto halfc) __attribute__((always_inline)) {
            constexpr int ua = u + decltype(aheadc)::value, ut = ua % 16, slot_t = ua % PST_NS;
            if constexpr (wo && ua < 16) issue(IntC<1>{}, 0, IntC<ut>{}, IntC<slot_t>{}, halfc);
            else if constexpr (wo) issue(IntC<0>{}, 0, IntC<ut>{}, IntC<slot_t>{}, halfc);
            else issue(IntC<0>{}, (hs + (ua >= 16 ? 1 : 0)) & 7, IntC<ut>{}, IntC<slot_t>{}, halfc);
        };
        auto between = [&](auto gc) __attribute__((always_inline)) {
            constexpr int g = decltype(gc)::value;
            if constexpr (r == 3 && g >= 2) batch_piece(IntC<5>{}, IntC<g - 2>{});          // stage 0 of the batch: behind B1
            else if constexpr (r == 0 && g < 2) batch_piece(IntC<5>{}, IntC<g>{});          // stage 1
            else if constexpr (r == 0 && g >= 2) batch_piece(IntC<6>{}, IntC<g - 2>{});     // stage 2
            else if constexpr (r == 1 && g < 2) batch_piece(IntC<6>{}, IntC<g>{});          // stage 3: its slot is free behind B2
        };
        auto next = [&](auto jc) __attribute__((always_inline)) {
            constexpr int j = decltype(jc)::value;
            if constexpr (r == 3 && j == 5) landed();                                                  // B1
            else if constexpr (r == 0 && j == 5) __builtin_amdgcn_s_barrier();                         // B2
        };
        if constexpr (wo) {
            constexpr int c = u >> 1, nh = u & 1;
            stage_mma(IntC<slot>{}, oacc, IntC<8 * nh>{}, xh[c], xl[c], between, next);
        } else if constexpr (u < 8) {
            if constexpr (u == 0) {
#pragma unroll
                for (int j = 0; j < 8; ++j) hacc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
            }
            stage_mma(IntC<slot>{}, hacc, IntC<0>{}, xh[u], xl[u], between, next);
        } else {
            constexpr int v = u - 8, c = v >> 1, nh = v & 1;
            if constexpr (nh == 0) {
                // hidden columns 32 c + 8 fk .. + 7 of the slice (tiles 2c, 2c+1): + bias, GELU, split -> operand fragment of k-step c
                const f32x4 ba = ld4(b1s + 128 * hs + 32 * c + 8 * fk), bb = ld4(b1s + 128 * hs + 32 * c + 8 * fk + 4);
                f32x4 va, vb;
#pragma unroll
                for (int e = 0; e < 4; ++e) { va[e] = gelu_erf(hacc[2 * c][e] + ba[e]); vb[e] = gelu_erf(hacc[2 * c + 1][e] + bb[e]); }
                split8(va, vb, hh[c], hl[c]);
            }
            stage_mma(IntC<slot>{}, oacc, IntC<8 * nh>{}, hh[c], hl[c], between, next);
        }
    };

    static_for<PST_GRP>([&](auto uc) {
        static_for<PPW>([&](auto ic) { issue(IntC<1>{}, 0, uc, uc, ic); });
    });
    __syncthreads();                                                     // the vectors are in LDS (plain stores: lgkmcnt, compiler-tracked)
#pragma unroll
    for (int jj = 0; jj < 16; ++jj) {
        const f32x4 bv = ld4(prm + 5 * D + 32 * (jj >> 1) + 8 * fk + 4 * (jj & 1));
#pragma unroll
        for (int e = 0; e < 4; ++e) oacc[jj][e] += bv[e];
    }
    landed();
    static_for<PPW>([&](auto ic) { issue(IntC<1>{}, 0, IntC<PST_GRP>{}, IntC<PST_GRP>{}, ic); });   // stage 0 of group 1
    static_for<3>([&](auto jc) { fetch_tile(IntC<0>{}, jc); });

    // ---- out_proj: oacc = x0 + bo + att Wo^T
    static_for<16>([&](auto uc) { stage(IntC<1>{}, 0, uc); });

    // ---- mid-epilogue.  Nothing of the ring is in flight inside it: the batch piece requested behind the last stage has landed
    // (vmcnt(0)), the three weight tiles fetched ahead for slice 0 are in their registers (lgkmcnt(0)).
    wait_vm<0>();
    wait_lgkm<0>(wt[0][0], wt[0][1], wt[1][0], wt[1][1]);
    wait_lgkm<0>(wt[2][0], wt[2][1], wt[3][0], wt[3][1]);
    {
        f32x4 (&v)[16] = oacc;
        // G rows of score tile ct as this lane reads them: row n = frow of the tile is (head n >> 2, token 4 ct + (n & 3)); a row that is
        // no token reads token 0's (an address other lanes read anyway) and counts as zeros.  Tile 0's k-steps are asked for in front of LN1.
        const float* gub = p.gu + (size_t)b * (H * T * 2 * D);
        auto g_row = [&](int ct) __attribute__((always_inline)) {
            const int tk = 4 * ct + (frow & 3);
            return gub + (size_t)(2 * ((frow >> 2) * T + (tk < T ? tk : 0))) * D + 8 * fk;
        };
        f32x4 g0[16];
        {
            const float* gp = g_row(0);
#pragma unroll
            for (int c = 0; c < 8; ++c) { g0[2 * c] = ld4(gp + 32 * c); g0[2 * c + 1] = ld4(gp + 32 * c + 4); }
        }
        // LayerNorm of the row in the accumulator layout: an in-lane sum + two cross-lane steps per statistic (two-pass)
        auto layer_norm = [&](const float* gp, const float* bp) __attribute__((always_inline)) {
            float s = 0.f;
#pragma unroll
            for (int jj = 0; jj < 16; ++jj) s += (v[jj][0] + v[jj][1]) + (v[jj][2] + v[jj][3]);
            s += __shfl_xor(s, 16, 64); s += __shfl_xor(s, 32, 64);      // the row's four lane groups
            const float mean = s * (1.f / 256.f);
            float q = 0.f;
#pragma unroll
            for (int jj = 0; jj < 16; ++jj)
#pragma unroll
                for (int e = 0; e < 4; ++e) { const float d = v[jj][e] - mean; q = fmaf(d, d, q); }
            q += __shfl_xor(q, 16, 64); q += __shfl_xor(q, 32, 64);
            const float rstd = rsqrtf(q * (1.f / 256.f) + LN_EPS);
#pragma unroll
            for (int jj = 0; jj < 16; ++jj) {
                const int col = 32 * (jj >> 1) + 8 * fk + 4 * (jj & 1);
                const f32x4 ga = ld4(gp + col), be = ld4(bp + col);
#pragma unroll
                for (int e = 0; e < 4; ++e) v[jj][e] = (v[jj][e] - mean) * rstd * ga[e] + be[e];
            }
        };
        layer_norm(prm + 6 * D, prm + 7 * D);                             // x1n
#pragma unroll
        for (int c = 0; c < 8; ++c) split8(v[2 * c], v[2 * c + 1], xh[c], xl[c]);

        // scores^T = G x1n^T: the accumulator of lane (frow, fk) holds head fk's tokens 4 ct .. 4 ct + 3 of row frow
        f32x4 sacc[2];
#pragma unroll
        for (int ct = 0; ct < 2; ++ct) {
            sacc[ct] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (4 * ct < T) {                                              // compile time
                const bool gv = 4 * ct + (frow & 3) < T;
                const float* gp = g_row(ct);
#pragma unroll
                for (int c = 0; c < 8; ++c) {
                    f32x4 ga = ct == 0 ? g0[2 * c] : ld4(gp + 32 * c), gb = ct == 0 ? g0[2 * c + 1] : ld4(gp + 32 * c + 4);
                    if (!gv) { ga = f32x4{0.f, 0.f, 0.f, 0.f}; gb = ga; }
                    s16x8 gh, gl;
                    split8(ga, gb, gh, gl);
                    sacc[ct] = MFMA16_S16(gh, xl[c], sacc[ct], 0, 0, 0);
                    sacc[ct] = MFMA16_S16(gl, xh[c], sacc[ct], 0, 0, 0);
                    sacc[ct] = MFMA16_S16(gh, xh[c], sacc[ct], 0, 0, 0);
                }
            }
        }
        // + c, tokens >= count masked (cross_attention.py:408-409), softmax over the head's tokens in base 2: all in this lane
        float sc[8], mx = -INFINITY;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            sc[e] = e < nv ? sacc[e >> 2][e & 3] + cv[e] : -INFINITY;
            mx = fmaxf(mx, sc[e]);
        }
        float l = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) { sc[e] = __builtin_amdgcn_exp2f((sc[e] - mx) * 1.4426950408889634f); l += sc[e]; }
        const float inv = 1.f / l;
        s16x8 ph, pl;                                                      // P^T as B fragment: k = 8 fk + e = (head fk, token e)
        split8(f32x4{sc[0] * inv, sc[1] * inv, sc[2] * inv, sc[3] * inv}, f32x4{sc[4] * inv, sc[5] * inv, sc[6] * inv, sc[7] * inv}, ph, pl);

        // out^T = U^T P^T on top of x1n + bo_cross; U^T fragment of column tile jj, token e: float o = (jj T + e) 64 + lane of
        // dec_post_gu_kernel's layout (1-KiB piece o >> 8 in the place of U row o >> 8); tokens >= T are zeros
        const float* ut = gub + D + lane;
#pragma unroll
        for (int jj = 0; jj < 16; ++jj) {
            const int col = 32 * (jj >> 1) + 8 * fk + 4 * (jj & 1);
            const f32x4 bc = ld4(prm + 8 * D + col);
            float u8[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) u8[e] = e < T ? ut[((jj * T + e) >> 2) * (2 * D) + ((jj * T + e) & 3) * 64] : 0.f;
            s16x8 uh, ul;
            split8(f32x4{u8[0], u8[1], u8[2], u8[3]}, f32x4{u8[4], u8[5], u8[6], u8[7]}, uh, ul);
#pragma unroll
            for (int e = 0; e < 4; ++e) v[jj][e] += bc[e];
            v[jj] = MFMA16_S16(uh, pl, v[jj], 0, 0, 0);
            v[jj] = MFMA16_S16(ul, ph, v[jj], 0, 0, 0);
            v[jj] = MFMA16_S16(uh, ph, v[jj], 0, 0, 0);
        }
        layer_norm(prm + 9 * D, prm + 10 * D);                             // x2
#pragma unroll
        for (int c = 0; c < 8; ++c) split8(v[2 * c], v[2 * c + 1], xh[c], xl[c]);
        // linear2's accumulators start from the residual and its bias
#pragma unroll
        for (int jj = 0; jj < 16; ++jj) {
            const f32x4 bv = ld4(prm + 32 * (jj >> 1) + 8 * fk + 4 * (jj & 1));
#pragma unroll
            for (int e = 0; e < 4; ++e) oacc[jj][e] += bv[e];
        }
    }

    // ---- feed-forward: dec_mlp.hip's slices
#pragma unroll 1
    for (int hs = 0; hs < 8; ++hs) static_for<16>([&](auto uc) { stage(IntC<0>{}, hs, uc); });
    wait_vm<0>();                                                        // no LDS-DMA may land after the workgroup has gone
    wait_lgkm<0>(wt[0][0], wt[0][1], wt[1][0], wt[1][1]);                // the fetches behind the last stage
    wait_lgkm<0>(wt[2][0], wt[2][1], wt[3][0], wt[3][1]);

    // ---- epilogue (dec_mlp.hip; x2 + b2 is in the accumulators already): LayerNorm(s) in the accumulator layout, then through the
    // (now free) ring so that every store writes one whole 1-KiB row
    __syncthreads();                                                      // every wave is done with the ring
    char* const stg = lds + wave * 16384;
    {
        f32x4 (&v)[16] = oacc;
        float s = 0.f;
#pragma unroll
        for (int jj = 0; jj < 16; ++jj) s += (v[jj][0] + v[jj][1]) + (v[jj][2] + v[jj][3]);
#pragma unroll
        for (int pass = 0; pass < 2; ++pass) {
            if (pass == 1 && p.g4 == nullptr) break;
            const float* gp = prm + (pass == 0 ? 1 : 3) * D;
            const float* bp = prm + (pass == 0 ? 2 : 4) * D;
            if (pass == 1) {
                s = 0.f;
#pragma unroll
                for (int jj = 0; jj < 16; ++jj) s += (v[jj][0] + v[jj][1]) + (v[jj][2] + v[jj][3]);
            }
            s += __shfl_xor(s, 16, 64); s += __shfl_xor(s, 32, 64);
            const float mean = s * (1.f / 256.f);
            float q = 0.f;
#pragma unroll
            for (int jj = 0; jj < 16; ++jj)
#pragma unroll
                for (int e = 0; e < 4; ++e) { const float d = v[jj][e] - mean; q = fmaf(d, d, q); }
            q += __shfl_xor(q, 16, 64); q += __shfl_xor(q, 32, 64);
            const float rstd = rsqrtf(q * (1.f / 256.f) + LN_EPS);
#pragma unroll
            for (int jj = 0; jj < 16; ++jj) {
                const int col = 32 * (jj >> 1) + 8 * fk + 4 * (jj & 1);
                const f32x4 ga = ld4(gp + col), be = ld4(bp + col);
#pragma unroll
                for (int e = 0; e < 4; ++e) v[jj][e] = (v[jj][e] - mean) * rstd * ga[e] + be[e];
            }
        }
#pragma unroll
        for (int jj = 0; jj < 16; ++jj) {
            const int ch = 8 * (jj >> 1) + 2 * fk + (jj & 1);
            *reinterpret_cast<f32x4*>(stg + frow * 1024 + ((ch ^ frow) << 4)) = v[jj];
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const f32x4 o = *reinterpret_cast<const f32x4*>(stg + r * 1024 + ((lane ^ r) << 4));
            if (r < nrows) {
                if (p.y != nullptr) st4(p.y + (size_t)(row0 + r) * D + 4 * lane, o);
                if (p.ys != nullptr) store_split4(p.ys + (size_t)(row0 + r) * D, 4 * lane, o);
            }
        }
    }
}

// hipFuncSetAttribute is per DEVICE and must not land inside a stream capture: once per device, under a mutex; the graphed decode
// calls it before it begins its capture
int dec_post_prepare() {
    static std::mutex mu;
    static bool attr_set[64] = {};
    int dev = 0;
    LADIFF_HIP(hipGetDevice(&dev));
    if (dev < 0 || dev >= 64) return LADIFF_ERR_ARG;
    std::lock_guard<std::mutex> lock(mu);
    if (!attr_set[dev]) {
        const void* k[8] = {reinterpret_cast<const void*>(dec_post_kernel<1>), reinterpret_cast<const void*>(dec_post_kernel<2>),
                            reinterpret_cast<const void*>(dec_post_kernel<3>), reinterpret_cast<const void*>(dec_post_kernel<4>),
                            reinterpret_cast<const void*>(dec_post_kernel<5>), reinterpret_cast<const void*>(dec_post_kernel<6>),
                            reinterpret_cast<const void*>(dec_post_kernel<7>), reinterpret_cast<const void*>(dec_post_kernel<8>)};
        for (int i = 0; i < 8; ++i) LADIFF_HIP(hipFuncSetAttribute(k[i], hipFuncAttributeMaxDynamicSharedMemorySize, PST_LDS));
        attr_set[dev] = true;
    }
    return 0;
}

// U of n layers re-laid in place for dec_post_kernel (guws: launch_decoder_cross_prep's output, gu_layer floats per layer)
int launch_dec_post_gu(float* guws, size_t gu_layer, int n, int B, int T, hipStream_t s) {
    if (B == 0 || n == 0) return 0;
    if (T < 1 || T > LADIFF_MAX_LATENTS) return LADIFF_ERR_SHAPE;
    hipLaunchKernelGGL(dec_post_gu_kernel, dim3(B, n), dim3(256), 0, s, guws, gu_layer, T);
    LADIFF_LAUNCH_CHECK();
    return 0;
}

// y / ys [M,256] = the layer's output rows from its self-attention output (a.att, S-format) and its input (a.x0); a.gu (U in
// launch_dec_post_gu's layout) / a.cc.  The tile list is sample-aligned: B ceil(F / 16) tiles (padded), at most (M + 15 B) / 16 (ragged).
int launch_dec_post(const DecPostArgs& a, hipStream_t s) {
    if (a.M <= 0 || a.B <= 0) return 0;
    if (a.T < 1 || a.T > LADIFF_MAX_LATENTS || a.F < 1) return LADIFF_ERR_SHAPE;
    LADIFF_TRY(dec_post_prepare());
    const long long tiles = a.row_off == nullptr ? (long long)a.B * ((a.F + 15) / 16) : ((long long)a.M + 15ll * a.B) / 16;
    const dim3 grid((unsigned)((tiles + 7) / 8));
#define LADIFF_DP_CASE(TT) \
    case TT: hipLaunchKernelGGL(dec_post_kernel<TT>, grid, dim3(512), PST_LDS, s, a); break;
    switch (a.T) {
        LADIFF_DP_CASE(1) LADIFF_DP_CASE(2) LADIFF_DP_CASE(3) LADIFF_DP_CASE(4)
        LADIFF_DP_CASE(5) LADIFF_DP_CASE(6) LADIFF_DP_CASE(7) LADIFF_DP_CASE(8)
        default: return LADIFF_ERR_SHAPE;
    }
#undef LADIFF_DP_CASE
    LADIFF_LAUNCH_CHECK();
    return 0;
}

}  // namespace ladiff
