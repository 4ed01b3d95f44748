/*
 * ladiff_hip.h - C ABI of libladiff_hip.so, the MI355X (gfx950) implementation of the LADiff
 * latent-diffusion sampling hot path.
 *
 * The reference (AlessioSam/LADiff) is pure Python/PyTorch and has no FFI of its own; the
 * "interface each entry point replaces" is therefore a Python call site of the reference, cited
 * per function as `src/...py:line`.  The binding a maintainer adds is a ctypes stub - see
 * INTEGRATION.md and ladiff_amd/_lib.py.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes only; no torch / C++ types.
 *   - every pointer is a DEVICE pointer (fp32 unless typed otherwise) except those named h_*.
 *   - return 0 = ok, < 0 = argument / shape / workspace error (LADIFF_ERR_*), > 0 = hipError_t.
 *   - work is enqueued on the given stream and scratch comes from the caller's workspace (size from the
 *     *_workspace_bytes query).  The unit kernels, the denoiser / decoder / encoder / CLIP / evaluator entries and
 *     ladiff_diffusion_reverse with sampler == NULL neither allocate, free nor synchronise and are hipGraph-capturable;
 *     calls are re-entrant across distinct (workspace, stream) pairs.  EXCEPTIONS, each stated again at the entry:
 *       ladiff_diffusion_reverse with a sampler  instantiates hipGraphs (captured on a stream the handle creates for itself, replayed
 *                                    on `stream`: a capture on the caller's stream would be invalidated by any other thread's
 *                                    hipEventQuery of an event of that stream - torch.distributed's watchdog does that) and creates
 *                                    two events on first use; when its capture
 *                                    key changes it calls hipStreamSynchronize(stream) before destroying the old graphs and after
 *                                    uploading a new stage table; it is NOT capturable itself (it captures); a pipeline launch
 *                                    takes a process-wide mutex and chains through one event per device, so that two pipeline
 *                                    kernels (which each need every CU) never share the GPU
 *       ladiff_sampler_destroy       hipDeviceSynchronize
 *       ladiff_sampler_loop_ms       hipEventSynchronize on the loop's end event
 *       ladiff_reverse_status        blocking hipMemcpy (use ladiff_reverse_status_offset_bytes + an async copy to poll)
 *       the first pipeline launch on a device  runs a probe kernel on a private stream (hipMalloc / hipFree / stream create)
 *   - workspaces: a workspace AT LEAST as large as the matching *_workspace_bytes query is sufficient (a larger one gives the
 *     same results), and every *_workspace_bytes query is non-decreasing in each of its size arguments (batch, rows, frames,
 *     latents, steps, text tokens): a caller may size one workspace for its largest call and use it for every smaller one.  (The
 *     *_floats queries size caller-held RESULTS, whose layout follows their arguments exactly: ladiff_denoiser_text_cache_floats
 *     has one layout for n_text == 1 and another for n_text > 1 and is not ordered across the two.)  An entry refuses
 *     (LADIFF_ERR_WORKSPACE, nothing enqueued, no output touched) a workspace below the query at its own arguments - for the three
 *     denoiser entries, which share ladiff_denoiser_workspace_bytes and take only some of its arguments, with the missing ones at 1.
 *     Except where an entry says otherwise (ladiff_diffusion_reverse) a workspace is pure scratch: no result depends on what it held
 *     before the call, and nothing in it needs to survive the call.
 *   - tensors are dense row-major fp32.  Arithmetic: w_split == NULL -> fp32-input MFMA, fp32 accumulate (exact fp32
 *     fma chains inside every product; the persistent pipeline kernel of ladiff_diffusion_reverse additionally clears the last
 *     mantissa bit of every activation word it hands from one stage to the next - the bit carries the hand-off's parity tag,
 *     csrc/systolic.hip tag4: a truncation of <= 1 ulp toward zero at each of the 59 hand-offs of a step, in both hand-off
 *     protocols; 1e-5 ... 3e-5 on the decoded frames against the fp64-checked oracle); w_split != NULL (and ladiff_gemm_split / ladiff_self_attention_split / split = 1) -> "f16x3": operands as
 *     fp16 hi + lo pairs (22 significant bits; each half saturates at +-65504 - round 6; rounds 1 - 5 and a -DLADIFF_SPLIT_BF16 build: bf16
 *     pairs, 16 bits, "bf16x3"; ladiff_split_format() tells), three 16-bit MFMAs per product, fp32 accumulate; softmax, LayerNorm statistics, guidance and the
 *     scheduler are fp32 in both.
 *   - weights are passed as an array of device pointers, one per state-dict tensor, in the order
 *     given by ladiff_{denoiser,decoder}_param_name(i) (names = the reference's state-dict keys,
 *     SURVEY.md Appendix A).
 */
#ifndef LADIFF_HIP_H
#define LADIFF_HIP_H

#include <stddef.h>
#include <stdint.h>

/* The library is built with -fvisibility=hidden: only the entries declared here (and, for measurement, in
 * ladiff_hip_debug.h) are exported. */
#ifndef LADIFF_API
#define LADIFF_API __attribute__((visibility("default")))
#endif

#ifdef __cplusplus
extern "C" {
#endif

typedef void* ladiff_stream_t; /* hipStream_t */

enum {
    LADIFF_OK = 0,
    LADIFF_ERR_ARG = -1,         /* null pointer / negative size */
    LADIFF_ERR_SHAPE = -2,       /* shape outside what the kernels are built for */
    LADIFF_ERR_WORKSPACE = -3,   /* workspace too small */
    LADIFF_ERR_UNSUPPORTED = -4  /* configuration branch of the reference that is not built */
};

/* activation codes for ladiff_gemm */
enum { LADIFF_ACT_NONE = 0, LADIFF_ACT_RELU = 1, LADIFF_ACT_GELU = 2, LADIFF_ACT_SILU = 3, LADIFF_ACT_QGELU = 4 /* x*sigmoid(1.702x) */,
       LADIFF_ACT_LRELU = 5 /* LeakyReLU(0.2) */ };

#define LADIFF_ABI_VERSION 6
#define LADIFF_LATENT_DIM 256     /* model.latent_dim[-1], config_ladiff_humanml3d.yaml:132 */
#define LADIFF_NUM_HEADS 4        /* configs/modules/denoiser.yaml:7 */
#define LADIFF_NUM_LAYERS 9       /* configs/modules/denoiser.yaml:6, motion_vae.yaml:5 */
#define LADIFF_FF_SIZE 1024       /* configs/modules/denoiser.yaml:5 */
#define LADIFF_TEXT_DIM 768       /* configs/modules/denoiser.yaml:4 */
#define LADIFF_MAX_LATENTS 8      /* MAX_IT <= 8 (shipped: 5, config_ladiff_humanml3d.yaml:58) */
#define LADIFF_MAX_FRAMES 224     /* frames per motion <= 224 (reference MAX_LEN 196, base.yaml:78) */
#define LADIFF_COEF_STRIDE 8      /* floats per scheduler-coefficient row */
#define LADIFF_CLIP_MAX_LAYERS 12  /* CLIP ViT-L/14 text tower: 12 layers, width 768 (= LADIFF_TEXT_DIM), 12 heads, MLP 3072 */
#define LADIFF_CLIP_MAX_POSITIONS 77

LADIFF_API int ladiff_version(void);
/* Element type of the two halves of an S-format pair in THIS build of the library: 1 = IEEE fp16 (the product: x ~ hi + lo carries 22
 * significant bits, saturating at +-65504 per half), 0 = bf16 (rounds 1 - 5 and `-DLADIFF_SPLIT_BF16`: 16 bits, fp32's exponent range).
 * Callers that only pass S-format buffers between entries of this library never need it; tests that decode the format do. */
LADIFF_API int ladiff_split_format(void);
LADIFF_API const char* ladiff_error_string(int code);

/* ------------------------------------------------------------------ weight tables */
LADIFF_API int ladiff_denoiser_num_params(void);
LADIFF_API const char* ladiff_denoiser_param_name(int i); /* state-dict key of LADiffDenoiser, ladiff_denoiser.py:62-123 */
LADIFF_API int ladiff_decoder_num_params(void);
LADIFF_API const char* ladiff_decoder_param_name(int i);  /* keys LADiffVae.decode reads, ladiff_vae.py:334-356 */

/* ------------------------------------------------------------------ unit kernels (parity tests)
 * Y[M,N] = LN?( act(A[M,K] . W[N,K]^T + bias) + res ), A optionally the concat [A | A2] along K.
 * Replaces nn.Linear (+ F.relu / F.gelu / residual / nn.LayerNorm) call sites such as
 * mdiff_transformer.py:62-66, cross_attention.py:79-82 and :408-412.  ln_gamma != NULL needs N == 256. */
LADIFF_API int ladiff_gemm(const float* A, int lda, const float* A2, int lda2, int K1, const float* W, int ldw,
                const float* bias, const float* res, int ldres, const float* ln_gamma,
                const float* ln_beta, float* Y, int ldy, int M, int N, int K, int act,
                ladiff_stream_t stream);

/* Small-M variant used by the denoiser loop (K-resident LDS-DMA tiles, K multiple of 256, N multiple of 4).
 *   K == 256:        Y = act( A . W^T + bias ) + res
 *   K == 512 / 1024: split-K - Y receives K/256 raw partial planes [K/256][M][ldy]; bias/act/res are NOT applied,
 *                    combine them with ladiff_combine_rows. */
LADIFF_API int ladiff_gemm_resident(const float* A, int lda, const float* A2, int lda2, int K1, const float* W, int ldw,
                         const float* bias, const float* res, int ldres, float* Y, int ldy, int M, int N, int K,
                         int act, int split, float* Ys, ladiff_stream_t stream);

/* Large-M f16x3 GEMM of the decoder / encoder / CLIP (128x128 tiles, persistent producer/consumer workgroups):
 *   Y and/or Ys = act( [A | A2] . W^T + bias ) (+ res);  A, A2, W are S-format rows (ladiff_split_rows), K and K1
 *   multiples of 64, N multiple of 128, ldy multiple of 64; Y fp32 and Ys its S-format twin, either may be NULL. */
LADIFF_API int ladiff_gemm_split(const float* A, int lda, const float* A2, int lda2, int K1, const float* W, int ldw,
                      const float* bias, const float* res, int ldres, float* Y, float* Ys, int ldy, int M, int N, int K,
                      int act, ladiff_stream_t stream);

/* f16x3 operand format ("S-format"): a row of K fp32 values (K multiple of 64) is stored in the same K*4 bytes as
 * K/64 blocks of [64 x 16-bit hi | 64 x 16-bit lo], x ~ hi + lo (fp16 halves, or bf16 in a -DLADIFF_SPLIT_BF16 build).  With split = 1 ladiff_gemm_resident reads A, A2 and W in
 * this format and evaluates every product as hi*hi + hi*lo + lo*hi on the 16-bit MFMA with fp32 accumulation.
 * fp16 halves (the default build, both rounded toward zero): |x| in [2^-3, 65504] keeps 22 significant bits (~2^-21 relative
 * error per operand); below 2^-3 lo reaches fp16's subnormal floor (absolute error up to ~2^-24); each half saturates at +-65504,
 * so up to 131008 the loss grows gradually and beyond that the value is clipped.  bf16 halves: 16 bits, fp32's exponent range.
 * Ys (may be NULL) receives the K == 256 result in S-format, Y (may then be NULL) in fp32.  ladiff_split_rows converts fp32 [R,K]
 * -> S-format [R,K]. */
LADIFF_API int ladiff_split_rows(const float* x, float* y, int R, int K, ladiff_stream_t stream);

/* dst[r][:] = src[index[r]][:] for r < n_rows: rows of row_floats floats (a multiple of 4; src and dst 16-byte aligned, rows contiguous),
 * index [n_rows] int32 on the DEVICE.  Pure data movement (bit-exact): expands per-prompt rows to per-sample rows - the R repeats of each
 * prompt in the multimodality pass (ladiff.py:1122-1132) and the "" rows of the guidance half of a [2B,1,768] text tensor - for callers
 * without torch.  The entry checks what the host can see (sizes, alignment); the index VALUES are device data: the caller must pass
 * 0 <= index[r] < rows of src.  src and dst must not overlap.  Asynchronous on `stream`; n_rows == 0 does nothing. */
LADIFF_API int ladiff_gather_rows(const float* src, const int32_t* index, int n_rows, int row_floats, float* dst, ladiff_stream_t stream);

/* What the S-format conversion of this build (ladiff_split_rows) does to n fp32 tensors, one launch: `tensors` [n] and `counts` [n]
 * are DEVICE arrays (pointer and element count of each tensor), max_count >= every count (sizes the grid; < 2^32).  stats [n][5]
 * (device, overwritten) receives per tensor:
 *   [0] max |x| over the values that are not NaN, as the bits of an fp32 in the low word (+inf when the tensor holds one)
 *   [1] max |x - (hi + lo)| over the finite values, fp32 bits in the low word
 *   [2] number of non-finite values (NaN, +-inf)
 *   [3] number of finite values beyond the format's exact range (|x| > 65504 for fp16 halves; always 0 for bf16 halves)
 *   [4] number of finite non-zero values whose round trip is worse than a single fp16: |x - (hi + lo)| > 2^-11 |x|
 * Asynchronous on `stream`, no allocation; n == 0 does nothing. */
LADIFF_API int ladiff_split_range_stats(const float* const* tensors, const int64_t* counts, int n, int64_t max_count,
                                        uint64_t* stats, ladiff_stream_t stream);

/* The decoder layer's feed-forward block as ONE kernel, f16x3 arithmetic (csrc/dec_mlp.hip):
 *   y / ys [M,256] = LN( x + W2 gelu(W1 x + b1) + b2 ), then a second LayerNorm when ln2_gamma != NULL
 * TransformerDecoderLayer.forward_post, cross_attention.py:410-412 (tgt = norm3(tgt + linear2(gelu(linear1(tgt))))) and, on the
 * last layer, decoder.norm (:150-151).  xs = S-format twin of x (the operand; x is the fp32 residual), w1s [1024,256] and
 * w2s [256,1024] S-format (ladiff_split_rows), b1 [1024], b2 [256]; y fp32 and / or ys S-format (either may be NULL). */
LADIFF_API int ladiff_mlp_ln_fused(const float* xs, const float* x, const float* w1s, const float* b1, const float* w2s, const float* b2,
                        const float* ln_gamma, const float* ln_beta, const float* ln2_gamma, const float* ln2_beta, float* y,
                        float* ys, int M, ladiff_stream_t stream);

/* Rows of 256: x = sum of n_planes partial planes [n_planes][M][256] + bias (+ res), then
 *   mode 0: x;   mode 1: LN(x);   mode 2: LN(x) + table[sample row | pad_row] (rows grouped T per sample, sample = row / T, padded when
 *   row % T >= counts[sample % Bs]);   mode 3: SiLU(LN(x) * (1 + table[0:256]) + table[256:512]).
 * Replaces the residual / LayerNorm / StylizationBlock element-wise tails at mdiff_transformer.py:65-66, :160-162. */
LADIFF_API int ladiff_combine_rows(const float* partials, int n_planes, int M, const float* bias, const float* res, int mode,
                        const float* ln_gamma, const float* ln_beta, const float* table, const int32_t* counts,
                        int Bs, int T, int pad_row, float* out, ladiff_stream_t stream);

/* y = LayerNorm(x) over rows of 256 (nn.LayerNorm, eps 1e-5), cross_attention.py:84-85, :150-151 */
LADIFF_API int ladiff_layernorm(const float* x, const float* gamma, const float* beta, float* y, int M,
                     ladiff_stream_t stream);

/* Self-attention core (softmax(QK^T/8 + key mask) V per sample and head) on packed qkv[B*F,768], F <= 224.
 * Key validity: keys < lengths[b], or - when keybits != NULL - bit k of the 256-bit map keybits[b][8] (uint32 words,
 * LSB first).  The nn.MultiheadAttention inside TransformerDecoderLayer.forward_post (cross_attention.py:367-369)
 * and TransformerEncoderLayer.forward_post (:298-300), without the in/out projections. */
LADIFF_API int ladiff_decoder_self_attention(const float* qkv, const int32_t* lengths, const uint32_t* keybits, float* out,
                                  int B, int F, ladiff_stream_t stream);

/* The same core in f16x3 arithmetic (q, k, v and the probabilities as hi + lo pairs, three 16-bit MFMAs per product,
 * fp32 softmax and accumulation) for any number of 64-wide heads: qkv[B*F, 3*64*nheads] packed [q | k | v],
 * out[B*F, 64*nheads] fp32.  lengths and keybits may both be NULL (all keys valid); causal != 0 adds key <= query. */
LADIFF_API int ladiff_self_attention_split(const float* qkv, const int32_t* lengths, const uint32_t* keybits, float* out, int B, int F,
                                 int nheads, int causal, ladiff_stream_t stream);

/* Decoder cross-attention core: q[B*F,256] against the T memory tokens kv[T*B,512] (row = t*B+b,
 * K | V), tokens >= counts[b] masked.  cross_attention.py:373-376. */
LADIFF_API int ladiff_decoder_cross_attention(const float* q, const float* kv, const int32_t* counts, float* out,
                                   int B, int F, int T, ladiff_stream_t stream);

/* ------------------------------------------------------------------ denoiser (LADiffDenoiser.forward)
 * Step-invariant and t-only work is hoisted:
 *   time tables  [n_steps][9 layers][1536] = AdaLN (scale|shift) of ca_block and ffn, K|V of the time token
 *                (tools/embeddings.py:245-305, mdiff_transformer.py:158-160, :308-311)
 *   text cache   emb_proj output, per-layer K|V of the text token, and the c table [9][n_steps][B2+1][256]: the
 *                whole cross-attention block (mdiff_transformer.py:219-247), which with ONE text token adds a
 *                vector that depends on (step, layer, sample) only (ladiff_denoiser.py:193-198).  It is built
 *                from the time tables, so call ladiff_denoiser_time_tables first.                             */
LADIFF_API size_t ladiff_denoiser_tables_floats(int n_steps);
/* n_text = text tokens per prompt.  1 (the CLIP pooled token, mld_clip.py:75-78) is the hoisted form above.  n_text > 1
 * (`clip_hidden` / `bert`, mld_clip.py:80-86) is the literal path in fp32 arithmetic (w_split must be NULL): the text
 * cache then holds emb_proj of every token, their per-layer K|V for the self-attention over [latents | text | time], and
 * per (layer, sample, head) the 64x64 matrix sum_n softmax_n(key) value^T of LinearTemporalCrossAttention
 * (mdiff_transformer.py:235-239), which depends on the text only. */
LADIFF_API size_t ladiff_denoiser_text_cache_floats(int B2, int n_steps, int n_text);
LADIFF_API size_t ladiff_denoiser_workspace_bytes(int B2, int T, int n_steps, int n_text);

/* sinusoid[n_steps,768] = Timesteps(768, flip_sin_to_cos, freq_shift 0)(t) for every step of the schedule
 * (tools/embeddings.py:245-285).  It is a t-only table like the scheduler coefficients; the host may fill it
 * itself (bit-identical to the reference's fp32 ops) or with ladiff_timestep_sinusoid. */
LADIFF_API int ladiff_timestep_sinusoid(const int64_t* timesteps, int n_steps, float* sinusoid, ladiff_stream_t stream);
LADIFF_API int ladiff_denoiser_time_tables(const float* const* w, const float* sinusoid, int n_steps,
                                float* tables, void* ws, size_t ws_bytes, ladiff_stream_t stream);
LADIFF_API int ladiff_denoiser_text_cache(const float* const* w, const float* text_emb /*[B2,n_text,768]*/, int B2, int n_text,
                               const float* tables, int n_steps, float* cache, void* ws, size_t ws_bytes,
                               ladiff_stream_t stream);

/* eps[Bs*dup,T,256] = denoiser(cat([sample]*dup), t = step *d_step of the time tables, text, counts).
 * ladiff_denoiser.py:153-295 (call site ladiff.py:472-485).  counts[Bs] (int32, valid latent rows per
 * prompt, ceil(len/48)) may be NULL = no masking (TEST_EFFICIENCY / max_iter_elements=None).
 * w_split = NULL: fp32-input MFMA everywhere (bit-for-bit fp32 fma chains).  w_split != NULL: the f16x3 matrix path;
 * it is a second pointer table in the same order as w whose >= 2-D entries are the S-format copies of the weight
 * matrices (ladiff_split_rows), the other entries are ignored. */
LADIFF_API int ladiff_denoiser_forward(const float* const* w, const float* const* w_split, const float* tables,
                            const int32_t* d_step, const float* text_cache, int n_text, int n_steps,
                            const float* sample /*[Bs,T,256]*/, int Bs, int dup, int T, const int32_t* counts, float* eps, void* ws,
                            size_t ws_bytes, ladiff_stream_t stream);

/* One LinearTemporalCrossAttention block, literal (mdiff_transformer.py:219-247), for any number of text tokens:
 *   out[B,T,256] = x + proj_out( softmax_d(query(LN x)) . sum_n softmax_n(key(LN_t xf)) value(LN_t xf)^T , emb )
 * x [B,T,256], xf [B,n_text,256] (text tokens already in the latent width), emb [B,256] time embedding per sample,
 * counts [B] valid latent rows (rows >= counts[b] have their query zeroed; NULL = none), `layer` = block index 0..8 in
 * the order input_blocks, middle_block, output_blocks.  Unit entry point of the n_text > 1 path. */
LADIFF_API size_t ladiff_linear_cross_attention_workspace_bytes(int B, int T, int n_text);
LADIFF_API int ladiff_linear_cross_attention(const float* const* w, int layer, const float* x, const float* xf, const float* emb,
                                  const int32_t* counts, int B, int T, int n_text, float* out, void* ws, size_t ws_bytes,
                                  ladiff_stream_t stream);

/* ------------------------------------------------------------------ guidance + scheduler step
 * latents <- step(eps_u + g (eps_c - eps_u)) with one row of coef per step:
 *   {sqrt(a_t), sqrt(1-a_t), k_x0, k_x, k_eps, k_noise, 0, 0}
 *   x0 = (x - sqrt(1-a_t) e) / sqrt(a_t);  x' = k_x0 x0 + k_x x + k_eps e + k_noise z
 * (DDIM: k_x0 = sqrt(a_prev), k_eps = sqrt(1-a_prev-sigma^2), k_noise = sigma; DDPM: posterior mean
 * coefficients and sqrt(variance)).  Replaces ladiff.py:487-492 + diffusers *Scheduler.step. */
LADIFF_API int ladiff_cfg_scheduler_step(const float* eps, float* latents /*[B,T,256] in/out*/, const float* coef,
                              const int32_t* d_step, const float* step_noise /*[n,B,T,256] or NULL*/,
                              float guidance_scale, int cfg, int B, int T, ladiff_stream_t stream);
/* The multistep form of the same step (DPM-Solver++(2M)): one more term from the PREVIOUS step's data prediction m1,
 *   {sqrt(a_s), sqrt(1-a_s), k_x0, k_x, k_eps, k_noise, k_m, 0}:  x' = k_x0 x0 + k_x x + k_eps e + k_noise z + k_m m1
 * x0_prev [B,T,256] (16-byte aligned) holds m1 on entry and this step's x0 on return.  It is read only at a step whose row has
 * k_m != 0: the first step of a schedule (k_m = 0) may find anything in it, NaN included.  Neither allocates nor synchronises. */
LADIFF_API int ladiff_cfg_scheduler_step_multistep(const float* eps, float* latents /*[B,T,256] in/out*/,
                              float* x0_prev /*[B,T,256] in/out*/, const float* coef, const int32_t* d_step,
                              const float* step_noise /*[n,B,T,256] or NULL*/, float guidance_scale, int cfg, int B, int T,
                              ladiff_stream_t stream);
/* The same step in a loop that starts from a source motion (ladiff_diffusion_reverse_from): prompt b enters the schedule at position
 * s_b = starts[b] ([B] int32 device; NULL: s_b = first_step).  At position s = *d_step a row of prompt b is
 *   s <  s_b  frozen: the latent row keeps its bits, x0_prev is neither read nor written, no noise is used;
 *   s == s_b  in the multistep form first order: k_x0 + k_m stands in for k_x0 and m1 is not read (A (1 + 1/(2 r0)) - A/(2 r0) = A);
 *   otherwise the rule above.
 * x0_prev may be NULL: the one-step rule. */
LADIFF_API int ladiff_cfg_scheduler_step_from(const float* eps, float* latents /*[B,T,256] in/out*/,
                              float* x0_prev /*[B,T,256] in/out, or NULL*/, const float* coef, const int32_t* d_step,
                              const float* step_noise /*[n,B,T,256] or NULL*/, float guidance_scale, int cfg, int B, int T,
                              const int32_t* starts /*[B] device or NULL*/, int first_step, ladiff_stream_t stream);
/* The same step with its record: the unit entry of the rule behind ladiff_diffusion_reverse_record.  traj_x / traj_x0 [n,B,T,256] fp32
 * device, 16-byte aligned (else LADIFF_ERR_SHAPE), the layout of step_noise; either or both may be NULL.  Only row s = *d_step is written:
 *   traj_x[s]   the latents after the step, the bits stored to `latents` (scheduler.step(...).prev_sample, ladiff.py:706-734);
 *   traj_x0[s]  the step's data prediction (x - sqrt(1-a_s) eps) / sqrt(a_s), eps the guided prediction (pred_original_sample);
 *   a frozen row (s < s_b): traj_x[s] = its latents as they stand, traj_x0[s] = 0.
 * Every other row of both buffers keeps its contents.  With both NULL this is ladiff_cfg_scheduler_step_from. */
LADIFF_API int ladiff_cfg_scheduler_step_record(const float* eps, float* latents /*[B,T,256] in/out*/,
                              float* x0_prev /*[B,T,256] in/out, or NULL*/, const float* coef, const int32_t* d_step,
                              const float* step_noise /*[n,B,T,256] or NULL*/, float guidance_scale, int cfg, int B, int T,
                              const int32_t* starts /*[B] device or NULL*/, int first_step, float* traj_x /*[n,B,T,256] or NULL*/,
                              float* traj_x0 /*[n,B,T,256] or NULL*/, ladiff_stream_t stream);
LADIFF_API int ladiff_advance_step(int32_t* d_step, ladiff_stream_t stream);

/* latents[B,T,256] = noise * valid * sigma  (ladiff.py:380-390, :407) */
LADIFF_API int ladiff_init_latents(const float* noise, const int32_t* counts, float init_noise_sigma, float* latents,
                        int B, int T, ladiff_stream_t stream);
/* Initial latents of a loop from a source motion, one kernel:
 *   latents[b,t,:] = valid(b,t) (coef[s_b][0] z0[t,b,:] + coef[s_b][1] noise[b,t,:]),  s_b = starts[b] or first_step
 * = scheduler.add_noise(z0, noise, timesteps[s_b]).  z0 is [T,B,256], the layout of the loop's z and of the encoder's output.  noise is a
 * [B,T,256] tensor, or NULL: the per-prompt generator (seeds, prompt_index) at position -1, as the loop's draw_init_noise draws it. */
LADIFF_API int ladiff_init_latents_from(const float* z0 /*[T,B,256]*/, const float* noise /*[B,T,256] or NULL*/,
                              const uint64_t* seeds /*[B] device or NULL*/, const uint32_t* prompt_index /*[B] device or NULL*/,
                              const int32_t* counts /*[B] or NULL*/, const float* coef /*[n,8]*/, const int32_t* starts /*[B] device or NULL*/,
                              int first_step, float* latents /*[B,T,256]*/, int B, int T, ladiff_stream_t stream);
/* z[T,B,256] = permute(latents) with rows >= counts[b] zeroed  (ladiff.py:500, :562-566).  (Inside
 * ladiff_diffusion_reverse the same kernel also reads the pipeline's abort word and writes NaN when the loop was abandoned.) */
LADIFF_API int ladiff_finalize_latents(const float* latents, const int32_t* counts, float* z, int B, int T,
                            ladiff_stream_t stream);

/* ------------------------------------------------------------------ whole reverse loop
 * LADIFF._diffusion_reverse (ladiff.py:333-571, live branch).  `sampler` (from ladiff_sampler_create, or
 * NULL) owns hipGraphs of the per-call prologue and of up to 10 steps (denoiser + guidance + scheduler + step
 * counter) that are captured on first use and replayed; they are re-captured when any argument changes.  The
 * weight tables are identified by a hash over all their pointers plus `weights_generation`, a number the caller
 * bumps whenever it rebuilds a table (a rebuilt table can reuse old addresses).
 *   cfg = 1: classifier-free guidance, text_emb is [2B,1,768] (unconditional half first, ladiff.py:258-264) and the
 *            network runs on cat([latents]*2) (:472-474); cfg = 0: text_emb is [B,1,768], no guidance (:472-490).
 *   counts       [B] latent rows per motion used as the denoiser's key mask and to zero the initial noise
 *                (ladiff.py:379-390; NULL = unmasked, the TEST_EFFICIENCY branch, ladiff_denoiser.py:254)
 *   final_counts [B] rows >= final_counts[b] of the result are zeroed (ladiff.py:559-566, applied in every branch;
 *                NULL = no zeroing)
 *   h_counts     [B] the same numbers as `counts` in HOST memory (or NULL): lets the pipeline loop pack prompts by their
 *                latent count so that padded latent rows are not computed at all (they never influence valid rows: masked as
 *                keys, every other op is per row, and the final zeroing removes them)
 * reuse_time_tables = 1 tells the call that `ws` still holds the time tables of a previous call with the same weights
 * and schedule.
 * What the workspace holds between calls:
 *   sampler == NULL, reuse_time_tables == 0: nothing - `ws` is pure scratch, its contents before the call do not matter and the caller
 *     may overwrite or reuse it as soon as the call's work on `stream` has completed.
 *   reuse_time_tables == 1: the time tables of the previous call (above); the caller must not have altered `ws` since.
 *   with a sampler: `ws` also holds STATE OF THE SAMPLER'S CAPTURE KEY - the pipeline kernel's stage table (device pointers into the
 *     weights and into `ws` itself), its block plan and the time tables - uploaded when the key changes (first call, or any pointer,
 *     shape, scalar or weight table differs) and only read by later calls with the same key.  `ws` is part of the key.  Between two
 *     calls with the same sampler the workspace MUST NOT be altered, copied elsewhere in place of the original, or lent to another
 *     entry: a later call would hand the kernel a table of stale pointers.  Before the FIRST call of a fresh sampler (and after
 *     ladiff_sampler_destroy) its contents do not matter.
 * Synchronisation / allocation: with sampler == NULL the call only enqueues.  With a sampler it instantiates graphs and creates
 * events on first use, calls hipStreamSynchronize(stream) whenever its capture key changes (before the old graphs are destroyed,
 * after a new stage table is uploaded, before a changed block plan replaces the previous host copy), and a pipeline launch takes
 * a process-wide mutex and waits (on the stream, not the host) for the previous pipeline launch of the device. */
LADIFF_API int ladiff_sampler_create(void** sampler);
LADIFF_API int ladiff_sampler_destroy(void* sampler);
/* How a sampler runs the N steps: 1 (default) = ONE persistent pipeline kernel for the whole loop when the call qualifies
 * (guidance on, one text token, a CU per pipeline stage; both arithmetic modes) - every CU keeps one stage's weights in
 * registers and blocks of prompts flow through the stages (csrc/systolic.hip).  The block geometry is planned per call: 32-row
 * blocks (both guidance branches of three prompts, padded to T latent rows) or LENGTH-AWARE 16-row blocks (one guidance branch of
 * as many prompts as fit with only their valid latent rows; needs h_counts) - whichever the stage-time model predicts faster;
 * 2 / 3 force the 16- / 32-row plan; 0 = one launch per stage, captured in a hipGraph of up to 10 steps. */
LADIFF_API int ladiff_sampler_set_loop(void* sampler, int mode);
/* The block plan ladiff_diffusion_reverse would use for a batch (host arithmetic only, no GPU call): rows per block (16 = the
 * length-aware packing, 32 = padded blocks) and the number of blocks.  h_counts = latent counts on the host or NULL, masked = the
 * call passes device counts, loop_mode 1 / 2 / 3 as ladiff_sampler_set_loop, f16x3 = the call passes w_split, cfg = the call's
 * guidance flag (without guidance: one-branch 16-row blocks; LADIFF_ERR_UNSUPPORTED when such a call has device-only counts - it runs
 * launch-per-stage and has no block plan). */
LADIFF_API int ladiff_reverse_plan(int B, int T, const int32_t* h_counts, int masked, int loop_mode, int f16x3, int cfg, int* rows_per_block,
                        int* n_blocks);
/* Device time of the N-step loop of the sampler's last call (HIP events recorded on the call's stream right around the
 * pipeline kernel, or around the graph replays); blocks until it has finished.  Measurement aid (bench.py). */
LADIFF_API int ladiff_sampler_loop_ms(void* sampler, float* ms);
/* Measurement aids (bench.py --config c3).  A schedule longer than 64 steps runs as several windows (the hoisted cross-attention
 * table is rebuilt per window, the latents carry over): with window timing on, every window's loop launches are bracketed by
 * their own event pair, and ladiff_sampler_window_ms returns their sum and count for the last call (blocks until they have
 * completed) - ladiff_sampler_loop_ms minus that sum is what the table rebuilds between the windows cost.
 * ladiff_sampler_last_loop: whether the last call ran the persistent pipeline kernel (1) or launch-per-stage graphs (0), and
 * the pipeline's block plan (rows per block, blocks; 0 otherwise). */
LADIFF_API int ladiff_sampler_set_window_timing(void* sampler, int on);
LADIFF_API int ladiff_sampler_window_ms(void* sampler, float* loop_ms_sum, int* n_windows);
LADIFF_API int ladiff_sampler_last_loop(void* sampler, int* pipeline, int* rows_per_block, int* n_blocks);
/* Blocking read (hipMemcpy: synchronises the device) of the pipeline kernel's status words of the last call in this workspace:
 * code 0 = completed, 2 = a stage timed out waiting for its producer (info = workgroup) - the loop was abandoned, every later
 * window of the call ended at once and z was filled with NaN; code 0 with info -1 = completed, but the workgroups were not on
 * the XCDs the plan assumed and every hand-off was written through (slower, same results).  The words are cleared once per
 * ladiff_diffusion_reverse call and are sticky over its windows; loop forms other than the pipeline leave them at 0. */
LADIFF_API int ladiff_reverse_status(void* ws, int B, int T, int n_steps, int n_text, int* code, int* info);
/* Where those two uint32 words {code, info} live: byte offset from the workspace base (0 = bad arguments).  A caller that must
 * not block copies the 8 bytes to pinned host memory with an async copy on the call's stream and reads them once an event
 * recorded behind the copy has completed (ladiff_amd/pipeline.py does, and raises / re-runs the call launch-per-stage). */
LADIFF_API size_t ladiff_reverse_status_offset_bytes(int B, int T, int n_steps, int n_text);
/* Fault injection for the abort-path tests, a property of ONE sampler handle: workgroup >= 0 makes that pipeline workgroup leave right
 * after the start-up handshake of every launch of this sampler, so that its consumers time out (-1: off); timeout_ms > 0 replaces the
 * 1.5 s bound of every wait (0: default).  Other samplers of the process are not affected. */
LADIFF_API int ladiff_sampler_set_fault(void* sampler, int workgroup, int timeout_ms);
/* Per-step noise of the stochastic schedulers (DDPM, DDIM with eta > 0) drawn ON THE DEVICE, where it is consumed, instead of read
 * from a [n_steps,B,T,256] tensor (655 MB for 1000 steps x 128 prompts).  Replaces diffusers' `randn_tensor` inside
 * `scheduler.step` (reference call site: ladiff.py:492; configs/modules_novae/scheduler.yaml:16-29).  A value is a pure function of
 * (seed, schedule position, global prompt index = first_prompt + b, latent, column): Philox4x32-10 bits, Box-Muller normals
 * (csrc/noise_gen.h; oracle/ladiff_oracle.py:device_noise is the numpy restatement) - so a batch sharded over ranks or cut into
 * chunks draws what the whole batch would, and a call is reproducible from its seed.
 *   ladiff_sampler_set_noise_generator: with enable != 0, calls of ladiff_diffusion_reverse on this sampler that pass
 *     step_noise = NULL draw from the generator (a non-NULL step_noise still wins); enable = 0: such calls add no noise (as before).
 *   ladiff_noise_fill: the same values as a tensor, out[i][b][t][:] for schedule positions first_step + i (tests, oracle checks,
 *     callers that want to keep the noise). */
LADIFF_API int ladiff_sampler_set_noise_generator(void* sampler, uint64_t seed, uint32_t first_prompt, int enable);
LADIFF_API int ladiff_noise_fill(uint64_t seed, uint32_t first_prompt, int first_step, int n_steps, int B, int T, float* out /*[n_steps,B,T,256]*/,
                      ladiff_stream_t stream);
LADIFF_API size_t ladiff_reverse_workspace_bytes(int B, int T, int n_steps, int n_text);
LADIFF_API int ladiff_diffusion_reverse(void* sampler, const float* const* w, const float* const* w_split /*or NULL*/,
                             uint64_t weights_generation, const float* text_emb /*[2B or B,n_text,768]*/,
                             const float* init_noise /*[B,T,256]*/, const int32_t* counts /*[B] or NULL*/,
                             const int32_t* final_counts /*[B] or NULL*/,
                             const int32_t* h_counts /*HOST copy of counts, or NULL*/,
                             const float* sinusoid /*[n,768]*/, const float* coef /*[n,8]*/,
                             const float* step_noise /*[n,B,T,256] or NULL*/, float guidance_scale,
                             float init_noise_sigma, int cfg, int B, int T, int n_text, int n_steps, float* z /*[T,B,256]*/,
                             void* ws, size_t ws_bytes, int reuse_time_tables, ladiff_stream_t stream);
/* The same loop with the prompts of one batch as separate requests: a guidance scale and a noise key per prompt.
 *   guidance_scales[b]: the scale of prompt b instead of `guidance_scale` (cfg != 0 only: LADIFF_ERR_ARG otherwise).  Every value is
 *     simply evaluated, eps_u + g (eps_c - eps_u), also g <= 1.
 *   seeds[b], prompt_index[b]: prompt b draws its per-step noise with Philox key seeds[b] and counter word 1 = prompt_index[b] (0 when
 *     prompt_index is NULL) instead of the sampler's (seed, first_prompt + b): the same request gives the same motion whatever batch it
 *     sits in and wherever in it.  Works without a sampler handle too.  prompt_index without seeds is LADIFF_ERR_ARG.
 *   draw_init_noise != 0: the initial noise is drawn on the device as well - the same function at schedule position -1 (counter word
 *     2 = 0xFFFFFFFF, which no schedule reaches) - so init_noise may be NULL; requires seeds (LADIFF_ERR_ARG otherwise).
 *   A non-NULL step_noise or init_noise tensor still wins over the generator.
 * The three arrays are DEVICE data: the call cannot check their values on the host, a non-finite scale gives non-finite latents for that
 * prompt only, and a sampler keys them by POINTER - new values in the same buffers replay the captured graphs, a new buffer captures
 * again.  All NULL and draw_init_noise = 0: exactly ladiff_diffusion_reverse (which forwards here). */
LADIFF_API int ladiff_diffusion_reverse_prompts(void* sampler, const float* const* w, const float* const* w_split /*or NULL*/,
                             uint64_t weights_generation, const float* text_emb /*[2B or B,n_text,768]*/,
                             const float* init_noise /*[B,T,256], or NULL with draw_init_noise*/, const int32_t* counts /*[B] or NULL*/,
                             const int32_t* final_counts /*[B] or NULL*/,
                             const int32_t* h_counts /*HOST copy of counts, or NULL*/,
                             const float* sinusoid /*[n,768]*/, const float* coef /*[n,8]*/,
                             const float* step_noise /*[n,B,T,256] or NULL*/, float guidance_scale,
                             float init_noise_sigma, int cfg, int B, int T, int n_text, int n_steps, float* z /*[T,B,256]*/,
                             void* ws, size_t ws_bytes, int reuse_time_tables, const float* guidance_scales /*[B] device or NULL*/,
                             const uint64_t* seeds /*[B] device or NULL*/, const uint32_t* prompt_index /*[B] device or NULL*/,
                             int draw_init_noise, ladiff_stream_t stream);
/* The same loop with a multistep scheduler (ladiff_cfg_scheduler_step_multistep is its step): x0_prev [B,T,256] device, 16-byte aligned,
 * carries the previous step's data prediction from step to step, in all three loop forms and across the windows of a long schedule.
 *   The coefficient table is DEVICE data: the host cannot see whether its column 6 (k_m) is used.  So the pointer selects the form:
 *   x0_prev set = the multistep form (column 6 is read, the buffer is written at every step); x0_prev NULL = column 6 is ignored, exactly
 *   ladiff_diffusion_reverse_prompts (which forwards here).
 *   The buffer is the CALLER's, not part of `ws`: ladiff_reverse_workspace_bytes does not change.  Its contents on entry do not matter
 *   (row 0 of a multistep table has k_m = 0, and the buffer is not read at such a step); a sampler keys it by pointer. */
LADIFF_API int ladiff_diffusion_reverse_multistep(void* sampler, const float* const* w, const float* const* w_split /*or NULL*/,
                             uint64_t weights_generation, const float* text_emb /*[2B or B,n_text,768]*/,
                             const float* init_noise /*[B,T,256], or NULL with draw_init_noise*/, const int32_t* counts /*[B] or NULL*/,
                             const int32_t* final_counts /*[B] or NULL*/,
                             const int32_t* h_counts /*HOST copy of counts, or NULL*/,
                             const float* sinusoid /*[n,768]*/, const float* coef /*[n,8]*/,
                             const float* step_noise /*[n,B,T,256] or NULL*/, float guidance_scale,
                             float init_noise_sigma, int cfg, int B, int T, int n_text, int n_steps, float* z /*[T,B,256]*/,
                             void* ws, size_t ws_bytes, int reuse_time_tables, const float* guidance_scales /*[B] device or NULL*/,
                             const uint64_t* seeds /*[B] device or NULL*/, const uint32_t* prompt_index /*[B] device or NULL*/,
                             int draw_init_noise, float* x0_prev /*[B,T,256] device, or NULL*/, ladiff_stream_t stream);
/* The same loop from a SOURCE MOTION (SDEdit): z0 [T,B,256] device, 16-byte aligned, is noised to each prompt's own schedule position
 * and denoised from there.  Positions first_step .. n_steps - 1 run exactly once each (0 <= first_step < n_steps, else LADIFF_ERR_ARG);
 * time-table rows, c-table windows, sinusoid rows and noise positions keep their full-schedule indices.  starts [B] int32 device or NULL:
 * prompt b starts at s_b = starts[b], NULL = first_step for all.  The values are device data: first_step <= starts[b] < n_steps is the
 * CALLER's contract.  starts without z0 is LADIFF_ERR_ARG.
 *   The prologue writes latents = valid (coef[s_b][0] z0 + coef[s_b][1] noise) (ladiff_init_latents_from) with noise = init_noise or, with
 *   draw_init_noise, the per-prompt generator at position -1; init_noise_sigma is not applied.  Every step ends as
 *   ladiff_cfg_scheduler_step_from describes.  Nothing mixes prompts: a prompt's result depends on its own (text, z0, s_b, seed, index, scale).
 *   z0 NULL = ladiff_diffusion_reverse_multistep exactly (which forwards here; first_step must then be 0).  z0 and starts are the caller's
 *   buffers, keyed by pointer; first_step is part of a sampler's key in the launch-per-stage form and in a call without starts, a launch
 *   argument otherwise.  n_text > 1 with z0 is LADIFF_ERR_UNSUPPORTED. */
LADIFF_API int ladiff_diffusion_reverse_from(void* sampler, const float* const* w, const float* const* w_split /*or NULL*/,
                             uint64_t weights_generation, const float* text_emb /*[2B or B,n_text,768]*/,
                             const float* init_noise /*[B,T,256], or NULL with draw_init_noise*/, const int32_t* counts /*[B] or NULL*/,
                             const int32_t* final_counts /*[B] or NULL*/,
                             const int32_t* h_counts /*HOST copy of counts, or NULL*/,
                             const float* sinusoid /*[n,768]*/, const float* coef /*[n,8]*/,
                             const float* step_noise /*[n,B,T,256] or NULL*/, float guidance_scale,
                             float init_noise_sigma, int cfg, int B, int T, int n_text, int n_steps, float* z /*[T,B,256]*/,
                             void* ws, size_t ws_bytes, int reuse_time_tables, const float* guidance_scales /*[B] device or NULL*/,
                             const uint64_t* seeds /*[B] device or NULL*/, const uint32_t* prompt_index /*[B] device or NULL*/,
                             int draw_init_noise, float* x0_prev /*[B,T,256] device, or NULL*/, const float* z0 /*[T,B,256] device, or NULL*/,
                             const int32_t* starts /*[B] device or NULL*/, int first_step, ladiff_stream_t stream);
/* The same loop with its DENOISING TRAJECTORY recorded (the reference's _diffusion_reverse_tsne, ladiff.py:706-734: latents appended after
 * every scheduler.step).  traj_x / traj_x0 [n_steps,B,T,256] fp32 device, the caller's, 16-byte aligned (else LADIFF_ERR_SHAPE), the layout
 * of step_noise; either or both may be NULL, with both NULL this is ladiff_diffusion_reverse_from exactly (which forwards here).  For every
 * position s the call runs (first_step <= s < n_steps; rows s < first_step are not touched):
 *   traj_x[s]   the latents after position s - scheduler.step(...).prev_sample, the bits the step stores to the latents;
 *   traj_x0[s]  the step's data prediction (x_s - sqrt(1-a_s) eps_s) / sqrt(a_s), eps the guided prediction;
 *   rows t >= final_counts[b] are exact zeros in both (final_counts NULL: no such rows);
 *   while prompt b is frozen (z0 set, s < starts[b]) traj_x[s] holds its latents as they stand (the noised source), traj_x0[s] zeros.
 * Row indices are positions of the full schedule, whatever windows the loop runs in.  Recording changes no arithmetic: z keeps the bits of
 * the same call without it, in every loop form.  The pointers are part of a sampler's key (on or off, which kinds, where); new values in
 * the same buffers replay what is there.  The persistent pipeline records loops from noise; a recording call with z0 runs as step graphs
 * (ladiff_sampler_last_loop says so).  n_text > 1 with either buffer is LADIFF_ERR_UNSUPPORTED.  No workspace size changes. */
LADIFF_API int ladiff_diffusion_reverse_record(void* sampler, const float* const* w, const float* const* w_split /*or NULL*/,
                             uint64_t weights_generation, const float* text_emb /*[2B or B,n_text,768]*/,
                             const float* init_noise /*[B,T,256], or NULL with draw_init_noise*/, const int32_t* counts /*[B] or NULL*/,
                             const int32_t* final_counts /*[B] or NULL*/,
                             const int32_t* h_counts /*HOST copy of counts, or NULL*/,
                             const float* sinusoid /*[n,768]*/, const float* coef /*[n,8]*/,
                             const float* step_noise /*[n,B,T,256] or NULL*/, float guidance_scale,
                             float init_noise_sigma, int cfg, int B, int T, int n_text, int n_steps, float* z /*[T,B,256]*/,
                             void* ws, size_t ws_bytes, int reuse_time_tables, const float* guidance_scales /*[B] device or NULL*/,
                             const uint64_t* seeds /*[B] device or NULL*/, const uint32_t* prompt_index /*[B] device or NULL*/,
                             int draw_init_noise, float* x0_prev /*[B,T,256] device, or NULL*/, const float* z0 /*[T,B,256] device, or NULL*/,
                             const int32_t* starts /*[B] device or NULL*/, int first_step, float* traj_x /*[n,B,T,256] device, or NULL*/,
                             float* traj_x0 /*[n,B,T,256] device, or NULL*/, ladiff_stream_t stream);
/* The per-prompt generator's values as a tensor: out[i][b][t][:] for schedule positions first_step + i of the prompt with key seeds[b]
 * and index prompt_index[b]; first_step = -1 starts at the initial noise.  first_step < -1 is LADIFF_ERR_ARG. */
LADIFF_API int ladiff_noise_fill_prompts(const uint64_t* seeds /*[B] device*/, const uint32_t* prompt_index /*[B] device or NULL*/,
                             int first_step /* >= -1 */, int n_steps, int B, int T, float* out /*[n_steps,B,T,256]*/,
                             ladiff_stream_t stream);

/* ------------------------------------------------------------------ LA-VAE decoder (LADiffVae.decode)
 * feats[B,F,C] from z[T,B,256]; frames >= lengths[b] come out zero.  ladiff_vae.py:288-362
 * (call site ladiff.py:283).  lengths/counts are int32 device arrays of B entries. */
/* w_split (f16x3 mode): the S-format copies of the weight matrices as for the denoiser.  final_layer.weight needs its C rows only
 * (ABI 4; ABI 3 asked for tables padded to ceil(C / 128) * 128 rows - such tables still work, the extra rows are not read): from 4,096
 * frame rows up the final projection runs on whole 128-column f16x3 tiles, and the library pads the rows it needs itself.  The bias is
 * taken from the fp32 table `w`. */
LADIFF_API size_t ladiff_decoder_workspace_bytes(int B, int F, int T, int C);
LADIFF_API int ladiff_vae_decode(const float* const* w, const float* const* w_split /*or NULL: fp32 MFMA*/, const float* z,
                      const int32_t* lengths, const int32_t* counts, int B, int F, int T, int C, float* feats,
                      void* ws, size_t ws_bytes, ladiff_stream_t stream);
/* The same decode computing ONLY the valid frames of a mixed-length batch (ragged rows): row_off[b] (device int32,
 * B + 1 entries, exclusive prefix sum of lengths, row_off[B] = total_rows) places sample b's frames in the packed row
 * space the decoder works in; the result is scattered to feats[B,F,C] (frames >= lengths[b] zero, as above).  A sample's
 * frames do not depend on the other samples or on padding - padded frames are masked keys (cross_attention.py:367-371)
 * and zeroed at the end (ladiff_vae.py:356-360) - so the output equals ladiff_vae_decode's.  The workspace of
 * ladiff_decoder_workspace_bytes(B, F, T, C) is enough. */
LADIFF_API int ladiff_vae_decode_ragged(const float* const* w, const float* const* w_split /*or NULL*/, const float* z,
                             const int32_t* lengths, const int32_t* counts, const int32_t* row_off, int total_rows, int B,
                             int F, int T, int C, float* feats, void* ws, size_t ws_bytes, ladiff_stream_t stream);

/* The same decode (padded rows when row_off == NULL - total_rows is then not read -, ragged otherwise) that ALSO returns the decoder's
 * cross-attention weights, frames against latents, of every layer: the `plot_att_map` analysis of the reference
 * (cross_attention.py:113-148, :373-406).  att_maps is dense float32 [9][B][F][T], layers in execution order (input_blocks.0..3,
 * middle_block, output_blocks.0..3):
 *   att_maps[l][b][f][j] = (1/4) sum_h softmax_j(q_h[b,f] . k_h[b,j] / 8),  the head-averaged weights nn.MultiheadAttention returns,
 * taken from the decode's own folded scores (fp32 in both modes), so they describe what this decode computed.  Tokens j >= counts[b]
 * are masked before the softmax and written as exactly 0.0f; counts == NULL masks no token.  Frames f >= lengths[b] are written as
 * zeros, as in feats (the reference computes weights for padded frames too).  Every word of att_maps and feats is written: nothing
 * depends on what they held.  The fused out_proj + cross-attention kernel of the f16x3 large-row route never forms the rows the
 * weights are taken from, so this call runs that step as its two launches (ladiff_debug_set_decoder_fusion(1 + 64) gives the same
 * feats); nine launches more than a decode, and never captured into a graph.  The workspace of
 * ladiff_decoder_workspace_bytes(B, F, T, C) is enough.  Argument, shape and workspace errors return before anything is queued. */
LADIFF_API int ladiff_vae_decode_att_maps(const float* const* w, const float* const* w_split /*or NULL*/, const float* z,
                             const int32_t* lengths, const int32_t* counts /*or NULL*/, const int32_t* row_off /*or NULL: padded rows*/,
                             int total_rows, int B, int F, int T, int C, float* feats, float* att_maps /*[9,B,F,T]*/, void* ws,
                             size_t ws_bytes, ladiff_stream_t stream);

/* The same decode (padded when row_off == NULL, ragged otherwise) captured into a hipGraph on first use and replayed: for batches
 * of few frame rows, where the ~110 launches of a decode are a few microseconds each and the host's launch rate, not the GPU, sets
 * the time (config c1: 8 motions x 60 frames).  `graph` comes from ladiff_decoder_graph_create; the graph is keyed on every pointer
 * argument (z, lengths, counts, row_off, feats, ws, stream), the shapes and the weight tables (hash of their pointers +
 * `weights_generation`, as ladiff_diffusion_reverse) and is re-captured - after a hipStreamSynchronize(stream) - when any of them
 * changes, so callers keep z / feats / ws in persistent buffers.  `stream` must not be the null stream (capture is illegal there).
 * ladiff_decoder_graph_destroy synchronises the device. */
LADIFF_API int ladiff_decoder_graph_create(void** graph);
LADIFF_API int ladiff_decoder_graph_destroy(void* graph);
LADIFF_API int ladiff_vae_decode_graphed(void* graph, const float* const* w, const float* const* w_split /*or NULL*/, uint64_t weights_generation,
                              const float* z, const int32_t* lengths, const int32_t* counts, const int32_t* row_off /*or NULL*/,
                              int total_rows, int B, int F, int T, int C, float* feats, void* ws, size_t ws_bytes,
                              ladiff_stream_t stream);

/* ------------------------------------------------------------------ LA-VAE encoder
 * LADiffVae.encode, ladiff_vae.py:162-286 (call sites ladiff.py:269, :324, :1096): features[B,F,C] ->
 * mu, std, latent, each [T,B,256] (sequence-first like the reference); latent = mu + std * eps with rows >= counts[b]
 * zeroed; eps[T,B,256] stands in for the draw inside Normal.rsample().  Limits: F >= 1, 1 <= T <= LADIFF_MAX_LATENTS, C >= 1 and
 * 3 <= F + 2T <= LADIFF_MAX_FRAMES (the sequence [T mu tokens | T logvar tokens | F frames] is one attention of at most 224 keys;
 * sequences of fewer than 8 rows are served like any other); LADIFF_ERR_SHAPE otherwise, before anything is queued.  B == 0 is a no-op.
 * lengths[b] in [1, F] and counts[b] in [1, T] are the caller's to keep: they only select keys.  Weight table as for the decoder:
 * ladiff_encoder_param_name(i) lists the state-dict keys. */
LADIFF_API int ladiff_encoder_num_params(void);
LADIFF_API const char* ladiff_encoder_param_name(int i);
LADIFF_API size_t ladiff_encoder_workspace_bytes(int B, int F, int T, int C);
LADIFF_API int ladiff_vae_encode(const float* const* w, const float* const* w_split /*or NULL*/, const float* features,
                      const int32_t* lengths, const int32_t* counts, const float* eps, int B, int F, int T, int C,
                      float* mu, float* std, float* latent, void* ws, size_t ws_bytes, ladiff_stream_t stream);
/* The same encode with the DVAE input corruption (ablation DVAE / PERCENTAGE_NOISED; LADiffVae.add_noise, ladiff_vae.py:136-150,
 * applied by every encode call, evaluation included: :175-176): the encoder reads
 *   features[b][f][c] + (slot[f*C + c] >= 0 ? values[b][slot[f*C + c]] : 0)
 * where slot is a device int32 [F*C] table (a column of values, or -1: the same positions for the whole batch, as the reference's one
 * np.random.choice per call) and values is [B, n] (one standard normal per sample and position).  The sum is formed in the pass that
 * brings the features into the workspace: no extra buffer, the same workspace query (ladiff_encoder_workspace_bytes), and every later
 * kernel is ladiff_vae_encode's.  A slot outside [0, n) adds nothing; with every slot -1 the results are ladiff_vae_encode's bits.
 * values may be NULL when n == 0. */
LADIFF_API int ladiff_vae_encode_dvae(const float* const* w, const float* const* w_split /*or NULL*/, const float* features,
                           const int32_t* lengths, const int32_t* counts, const float* eps, int B, int F, int T, int C,
                           float* mu, float* std, float* latent, void* ws, size_t ws_bytes, const int32_t* slot,
                           const float* values, int n, ladiff_stream_t stream);

/* ------------------------------------------------------------------ stage-"vae" losses (csrc/vae_losses.hip)
 * MLDLosses.update in stage "vae" (models/losses/mld.py:98-107, :141-147) on what LADIFF.train_vae_forward returns (ladiff.py:815-871):
 *   recons_feature = mean SmoothL1(m_rst, m_ref) over [B,F,C]            (torch.nn.SmoothL1Loss, beta 1: 0.5 d^2 if |d| < 1, else |d| - 0.5)
 *   recons_joints  = mean SmoothL1(joints_rst, joints_ref) over [B,F,J,3]
 *   kl_motion      = mean over ALL [T,B,256] elements of 0.5 (std^2 + mu^2 - 1 - log std^2)
 *                    (torch.distributions.kl_divergence(Normal(mu, std), Normal(0, 1)), mld.py:162-164; the rows at and beyond a
 *                    sample's latent count are part of the reference's dist_m and are included)
 *   total          = lambda_rec recons_feature + lambda_joint recons_joints + lambda_kl kl_motion            (mld.py:95-96, :146)
 * batch[4] (device fp64) receives {recons_feature, recons_joints, kl_motion, total}; acc[4] (device fp64, caller-owned state: zero it to
 * reset) gains them - the reference's `+=` per update - without a host synchronisation.  Inputs are widened to fp64 before the
 * subtraction, sums are fp64; two launches (per-workgroup partial sums in fixed workspace slots, then one workgroup adds them in slot
 * order), no floating-point atomics: two calls on the same inputs leave the same bits.  LADIFF_ERR_SHAPE for a size < 1 or a misaligned
 * pointer (inputs 4 bytes; batch, acc, ws 8).  The query is non-decreasing in every argument. */
LADIFF_API size_t ladiff_vae_losses_workspace_bytes(int B, int F, int C, int J, int T);
LADIFF_API int ladiff_vae_losses(const float* m_rst, const float* m_ref, const float* joints_rst, const float* joints_ref,
                      const float* mu, const float* std, int B, int F, int C, int J, int T, double lambda_rec,
                      double lambda_joint, double lambda_kl, double* batch, double* acc, void* ws, size_t ws_bytes,
                      ladiff_stream_t stream);

/* ------------------------------------------------------------------ stage "diffusion" outside the sampling loop (csrc/diffusion_stage.hip)
 * LADIFF._diffusion_process (ladiff.py:745-813) in the shipped branch (IDEA 'ard', ARDIFF False, LAD True, PREDICT_EPSILON True):
 * q-sample, the denoiser with ONE TIMESTEP PER SAMPLE, and MLDLosses' inst_loss (losses/mld.py:69, :112).
 *
 * ladiff_denoiser_forward_timesteps: eps[B2,T,256] = denoiser(sample[B2,T,256], timesteps[B2] (int64, device), text_emb[B2,768]) for one
 * text token (n_text != 1: LADIFF_ERR_UNSUPPORTED), counts[B2] latent counts or NULL, both arithmetic modes (w_split NULL = fp32).  Unlike
 * ladiff_denoiser_forward it takes no tables, step counter or text cache: those are per CALL there and per SAMPLE here, so the entry
 * builds them in its workspace - the sinusoid and the time tables with row b = sample b's timestep, the step-invariant text cache, and a
 * "diagonal" c table [9][B2][valid | pad][256] (the padded rows' vector depends on the sample's timestep too) - and then runs
 * ladiff_denoiser_forward's own layer sequence.  The three row kernels that read the step counter there are shared: their per-sample
 * instantiations (den_self_attn_kernel<T, true>, reduce_rows_kernel<true>) read table row b instead, the loop and ladiff_denoiser_forward
 * run the <.., false> ones.  The launch count does not depend on B2 and the workspace is O(B2 T).  f16x3 mode runs the unfused sequence
 * (split-operand GEMMs + row kernels that write the S-format twin; the two fused kernels read the step counter).  With equal timesteps the result
 * equals ladiff_denoiser_forward's within the fp32 gate (5e-6 measured in both modes; not bit for bit: the time-table GEMMs run on B2
 * rows here and on one row there, and the f16x3 kernels differ).  All pointers 16-byte aligned
 * (timesteps 8, counts 4): LADIFF_ERR_SHAPE otherwise and for T outside 1 .. LADIFF_MAX_LATENTS.  The query is non-decreasing.
 *
 * ladiff_q_sample, one launch: noisy[b,t,:] = sqrt(acp[ts[b]]) z[t,b,:] + sqrt(1 - acp[ts[b]]) noise[b,t,:] (scheduler.add_noise; z is
 * sequence-first [T,B,256] as vae.encode returns it: the read folds the permute of ladiff.py:939 in), rows t >= counts[b] of noisy zero
 * (ladiff.py:779-782; counts NULL: none); rows of noise are never zeroed (the loss runs over all of them).  alphas_cumprod[n_train]
 * fp32 on the device; 0 <= ts[b] < n_train is the caller's contract (a value outside is clamped so that the read stays inside the table,
 * never reported).  Coefficients and sum in fp64, rounded once.  draw == 0: noise is the caller's input.
 * draw != 0: noise is an OUTPUT, drawn in the kernel from the counter-based generator at schedule position 0 for global prompts
 * first_prompt + b - the values of ladiff_noise_fill(seed, first_prompt, 0, 1, B, T).
 *
 * ladiff_diffusion_losses: inst_loss = mean (noise_pred - noise)^2 over n elements (all B T 256, padded rows included), total =
 * lambda_inst inst_loss (the reference: 1).  batch[2] (device fp64) receives {inst_loss, total}; acc[2] gains them without a host
 * synchronisation.  fp64 throughout, two launches over fixed partial-sum slots, no floating-point atomics: same inputs, same bits.
 * LADIFF_ERR_SHAPE for n < 1 or a misaligned pointer (inputs 4 bytes; batch, acc, ws 8). */
LADIFF_API size_t ladiff_denoiser_forward_timesteps_workspace_bytes(int B2, int T);
LADIFF_API int ladiff_denoiser_forward_timesteps(const float* const* w, const float* const* w_split /*or NULL*/, const float* text_emb,
                      int n_text, const int64_t* timesteps /*[B2]*/, const float* sample, int B2, int T, const int32_t* counts /*or NULL*/,
                      float* eps, void* ws, size_t ws_bytes, ladiff_stream_t stream);
LADIFF_API int ladiff_q_sample(const float* z, const int64_t* timesteps, const float* alphas_cumprod, int n_train,
                      const int32_t* counts /*or NULL*/, int draw, uint64_t seed, uint32_t first_prompt, float* noise, float* noisy,
                      int B, int T, ladiff_stream_t stream);
LADIFF_API size_t ladiff_diffusion_losses_workspace_bytes(int64_t n);
LADIFF_API int ladiff_diffusion_losses(const float* noise_pred, const float* noise, int64_t n, double lambda_inst, double* batch,
                      double* acc, void* ws, size_t ws_bytes, ladiff_stream_t stream);

/* ------------------------------------------------------------------ CLIP text encoder (the caller side)
 * MldTextEncoder.forward, mld_clip.py:51-86, "clip" branch (call sites ladiff.py:265, :1048, :1144):
 * text_model.get_text_features(input_ids) of transformers' CLIPModel -> out[B,768] (the reference then unsqueezes to
 * [B,1,768]).  ids[B,S] int64 token ids as the CLIP tokenizer emits them (padding="max_length", S <= 77; tokenising is
 * host string work and stays with the caller).  Only the first L <= S positions are evaluated: under the causal mask
 * the pooled EOS row (argmax of the ids) does not depend on later positions, so any L > max_b argmax(ids[b]) gives the
 * same result as L = S.  The pointer table lists LADIFF_CLIP_MAX_LAYERS layers; a model with n_layers < 12 fills the
 * first 5 + 16 * n_layers entries (rest may be NULL).  vocab = rows of the token-embedding table. */
LADIFF_API int ladiff_clip_num_params(void);
LADIFF_API const char* ladiff_clip_param_name(int i);     /* keys of transformers.CLIPModel.state_dict() (text side) */
LADIFF_API size_t ladiff_clip_workspace_bytes(int B, int L);
LADIFF_API int ladiff_clip_text_encode(const float* const* w, const float* const* w_split /*or NULL*/, int n_layers, int vocab,
                            const int64_t* ids, int B, int S, int L, float* out, void* ws, size_t ws_bytes,
                            ladiff_stream_t stream);
/* The same with RAGGED rows: prompt b is evaluated at its OWN positions 0 .. eos_b only (same argument as L above, per prompt: nothing
 * behind a prompt's EOS reaches its pooled row), 2.3x fewer rows than the padded batch for prompts of 1 .. 30 words.  seq_len[B] =
 * eos_b + 1 (the caller computes it from the ids as the reference's argmax does, mld_clip.py:75-78 -> CLIPTextTransformer), row_off[B+1]
 * = exclusive prefix sums of seq_len (row_off[B] = total_rows), row_seq[total_rows] = the prompt of each row; all int32 on the device;
 * L = max seq_len.  Same result as ladiff_clip_text_encode within the arithmetic mode's rounding (the row tiling of the GEMMs differs).
 * The three arrays must be mutually consistent (only total_rows is range-checked on the host): inconsistent ones give wrong embeddings,
 * never an access outside ids / the position table (the kernels clamp prompt and position indices). */
LADIFF_API size_t ladiff_clip_workspace_bytes_ragged(int B, int total_rows);
LADIFF_API int ladiff_clip_text_encode_ragged(const float* const* w, const float* const* w_split /*or NULL*/, int n_layers, int vocab,
                            const int64_t* ids, int B, int S, int L, const int32_t* seq_len, const int32_t* row_off,
                            const int32_t* row_seq, int total_rows, float* out, void* ws, size_t ws_bytes, ladiff_stream_t stream);

/* ------------------------------------------------------------------ T2M evaluator encoders (evaluation)
 * The three frozen networks `t2m_eval` runs to get the embeddings of the TM2T metrics (ladiff.py:1264-1271), fp32:
 *   movement: MovementConvEncoder.forward, t2m_motionenc.py:21-25: the first Cin columns of feats[B,F,ld] (the caller
 *             drops the 4 foot-contact columns, ladiff.py:1264: Cin = nfeats - 4, ld = nfeats) -> out[B, (F/2)/2, 512].
 *   motion:   MotionEncoderBiGRUCo.forward, t2m_motionenc.py:51-64: movements[B,T,512], m_lens[B] (= lengths / 4,
 *             1 <= m_lens <= T; the reference's pack_padded_sequence wants them sorted descending, this entry does not
 *             care) -> out[B,512].
 *   text:     TextEncoderBiGRUCo.forward, t2m_textenc.py:32-48: word_embs[B,L,300], pos_onehot[B,L,15], cap_lens[B]
 *             -> out[B,512].
 * Pointer tables: ladiff_t2m_*_param_name(i) are the keys of the `movement_encoder` / `motion_encoder` / `text_encoder`
 * state dicts of the evaluator checkpoint (ladiff.py:205-212). */
LADIFF_API int ladiff_t2m_movement_num_params(void);
LADIFF_API const char* ladiff_t2m_movement_param_name(int i);
LADIFF_API int ladiff_t2m_motion_num_params(void);
LADIFF_API const char* ladiff_t2m_motion_param_name(int i);
LADIFF_API int ladiff_t2m_text_num_params(void);
LADIFF_API const char* ladiff_t2m_text_param_name(int i);
LADIFF_API size_t ladiff_t2m_movement_workspace_bytes(int B, int F, int Cin);
LADIFF_API size_t ladiff_t2m_motion_workspace_bytes(int B, int T);
LADIFF_API size_t ladiff_t2m_text_workspace_bytes(int B, int L);
LADIFF_API int ladiff_t2m_movement_encode(const float* const* w, const float* feats, int ld, int B, int F, int Cin, float* out,
                               void* ws, size_t ws_bytes, ladiff_stream_t stream);
LADIFF_API int ladiff_t2m_motion_encode(const float* const* w, const float* movements, const int32_t* m_lens, int B, int T, float* out,
                             void* ws, size_t ws_bytes, ladiff_stream_t stream);
LADIFF_API int ladiff_t2m_text_encode(const float* const* w, const float* word_embs, const float* pos_onehot, const int32_t* cap_lens,
                           int B, int L, float* out, void* ws, size_t ws_bytes, ladiff_stream_t stream);

/* ------------------------------------------------------------------ feats2joints (the step after the path)
 * joints[B,F,njoints,3] = recover_from_ric(feats * std + mean): HumanML3DDataModule.feats2joints
 * (data/HumanML3D.py:44-48, data/Kit.py:48-53; motion_process.py:362-381, :415-430).  feats [B,F,C] as produced by
 * ladiff_vae_decode, mean/std [C] (device), C = 263 with 22 joints or 251 with 21 joints, F <= 256. */
LADIFF_API int ladiff_feats2joints(const float* feats, const float* mean, const float* std, int B, int F, int C, int njoints,
                        float* joints, ladiff_stream_t stream);

/* ------------------------------------------------------------------ joints2feats (csrc/joints2feats.hip)
 * The inverse direction: feats[B,L-1,263] = process_file(joints[b, :h_lengths[b]], feet_thre)[0] per motion - what
 * HumanML3DDataModule.joints2feats is meant to call (data/HumanML3D.py:50-55; data/humanml/scripts/motion_process.py:169-351 with
 * uniform_skeleton :13-36, common/skeleton.py:43-147, common/quaternion.py, scipy's gaussian_filter1d(., 20, mode='nearest')).
 * joints [B,L,22,3] fp32, 2 <= h_lengths[b] <= L <= 256 (h_lengths: HOST int32 [B]; the counts travel in the kernel arguments, so
 * the entry neither copies, allocates nor synchronises; one launch per 1024 motions; no workspace).  Motion b fills rows
 * 0 .. h_lengths[b]-2 of feats[b]; every later row is written as zeros, as ladiff_vae_decode leaves padding.
 *   target_offsets  device [22,3] = Skeleton.get_offsets_joints of the target pose: the motion is first retargeted to that skeleton
 *                   (per-frame inverse kinematics, forward kinematics with these offsets, root scaled by the leg-length ratio of
 *                   frame 0).  NULL skips the step: the mode for motions already on the model's skeleton (ladiff_feats2joints output).
 *   feet_thre       a foot contact is set where the squared displacement of joints 7, 10 (left) and 8, 11 (right) to the next frame
 *                   is < feet_thre; the reference's data scripts use 0.002 for HumanML3D (motion_process.py:468).  NOT
 *                   HumanML3D.py:51, which passes njoints in this place.
 *   mean, std       device [263], both or neither: (x - mean) / std fused into the store (rows of padding stay zero).
 * Arithmetic is fp32 in every build flavour.  Kept from the reference: inverse_kinematics_np unpacks the face joints [2,1,17,16] as
 * l_hip, r_hip, ... where process_file unpacks r_hip, l_hip, ... (the per-frame forward vector comes from the DIFFERENCE of shoulder
 * and hip span, the initial facing from their sum); qbetween has no anti-parallel case; qbetween's torch.cross has no dim, so a motion
 * of exactly 3 frames takes its cross products along the frame axis; frame 0's root rotation is the identity.
 * Errors, all before any GPU work: njoints != 22 -> LADIFF_ERR_UNSUPPORTED (KIT is not built); LADIFF_ERR_ARG for B < 0, a NULL
 * joints / h_lengths / feats, feet_thre <= 0 or exactly one of mean / std NULL; LADIFF_ERR_SHAPE for L outside [2, 256], a length
 * outside [2, L] or a pointer not aligned to 4 bytes.  B == 0 does nothing. */
LADIFF_API int ladiff_joints2feats(const float* joints, const int32_t* h_lengths, int B, int L, int njoints, const float* target_offsets,
                        float feet_thre, const float* mean, const float* std, float* feats, ladiff_stream_t stream);

/* ------------------------------------------------------------------ joint-space metrics (csrc/joint_metrics.hip)
 * The reference's ComputeMetrics ("TemosMetric": APE / AVE, models/metrics/compute.py:102-196) and MRMetrics (MPJPE / PA-MPJPE /
 * ACCEL, models/metrics/mr.py:73-96) on joints_rst / joints_ref [B,F,J,3] as ladiff_feats2joints leaves them (call sites
 * ladiff.py:1443-1445, :1464-1466), J = 21 or 22, 1 <= F <= LADIFF_MAX_FRAMES.  Each entry enqueues two launches and neither
 * synchronises nor allocates: one workgroup per sequence writes that sequence's sums to seq_rows[b][:] (fp32; the arithmetic inside is
 * fp64), then one workgroup adds the rows to acc[:] in fp64 in the order b = 0 .. B-1 (acc is caller-owned state: zero it to reset).  No
 * floating-point atomics: acc's bits are reproducible, and one call on B sequences leaves the bits that calls on its consecutive parts
 * leave.  No workspace.  h_lengths is the HOST copy of the lengths; LADIFF_ERR_SHAPE (nothing enqueued) for J outside {21, 22}, F outside
 * [1, LADIFF_MAX_FRAMES], a length outside [1, F], a part index outside the skeleton or a misaligned pointer (4 bytes; acc 8).  B == 0
 * does nothing.
 *
 * ladiff_joint_ape_ave: ComputeMetrics.transform = Rifke.forward (transforms/joints2jfeats/rifke.py:27-91, tools.py:14-55) and the
 *   re-integration of compute.py:133-196 on both tensors - floor (soft minimum over ALL F frames of the padded tensor), root height,
 *   trajectory and its differences, forward direction, its angle, the angle differences' prefix sum, local poses rotated back, the
 *   local velocity rotated and prefix-summed, division by `factor` (compute.py:181-191: 1000 * 0.75 / 480 for humanml3d, 1000 for mmm,
 *   1 without force_in_meter) - then over the frames < lengths[b] (device int32 [B]) the L2 sums and the variance(x, T) terms
 *   (utils.py:8-16; a length of 1 divides by zero as the reference does).  seq_rows [B][W], acc [W], W = 4 + 2 (J - 1) + 2 J:
 *   APE_root, APE_traj, APE_pose[J-1], APE_joints[J], AVE_root, AVE_traj, AVE_pose[J-1], AVE_joints[J].
 *   h_part_idx[8] (host) = positions of LS, RS, LH, RH, LMrot, RMrot, LF, RF in the joint-name list (utils/joints.py:1-48).  As in the
 *   reference the four foot joints index the full skeleton, while hips and shoulders index the poses after the root joint has been
 *   removed (rifke.py:43, :55): joint (index + 1) of the input.
 * ladiff_joint_mr: per frame, over EVERY one of the F frames (mr.py:92-96 passes the padded sequence whole): MPJPE root-aligned with
 *   the target.x != -2 joint mask (utils.py:347-369), PA-MPJPE (utils.py:267-318, :389-406: means removed, K = X1 X2^T, its SVD with
 *   the det-sign fix, scale, translation, mean joint error), ACCEL (utils.py:372-386: second differences, frames 0 .. F-3; nothing
 *   when F < 3).  seq_rows [B][3], acc [3]: MPJPE, PAMPJPE, ACCEL.  F == 2 and F == 3: the reference takes a tensor whose
 *   first dimension is 2 or 3 as transposed already (utils.py:274-278) and aligns each frame as 3 points (its x, y, z columns) in J
 *   dimensions; PAMPJPE follows it there. */
LADIFF_API int ladiff_joint_ape_ave(const float* joints_rst, const float* joints_ref, const int32_t* lengths, const int32_t* h_lengths,
                         int B, int F, int J, const int32_t* h_part_idx, float factor, float* seq_rows, double* acc,
                         ladiff_stream_t stream);
LADIFF_API int ladiff_joint_mr(const float* joints_rst, const float* joints_ref, const int32_t* h_lengths, int B, int F, int J,
                    float* seq_rows, double* acc, ladiff_stream_t stream);

/* ------------------------------------------------------------------ motion renderer (csrc/render.hip)
 * Joint positions to pictures: a stick figure in the style of the reference's plot_3d_motion (data/humanml/utils/plot_script.py; the
 * end of demo.py) - five coloured kinematic chains over a grey ground rectangle on a plain background.  It does NOT reproduce
 * matplotlib's pixels: the image model below is this library's own, and it is what tests/render_ref.py restates and the tests hold the
 * kernels to.
 *
 * Inputs   joints [B,L,J,3] fp32.  J = 22: the chains of t2m_kinematic_chain, J = 21: kit_kinematic_chain (utils/paramUtil.py):
 *            t2m  {0,2,5,8,11} {0,1,4,7,10} {0,3,6,9,12,15} {9,14,17,19,21} {9,13,16,18,20}
 *            kit  {0,11,12,13,14,15} {0,16,17,18,19,20} {0,1,2,3,4} {3,5,6,7} {3,8,9,10}
 *          a bone joins two consecutive joints of a chain.  h_lengths: HOST int32 [B], 1 <= h_lengths[b] <= L <= 256.
 *          16 <= H, W <= 1024, W % 4 == 0.
 * Scene    per motion, over its own frames t < h_lengths[b] only: mins / maxs = the component-wise minimum / maximum over all joints of
 *          those frames.  Every y is shifted by -mins.y (the lowest point touches the ground y = 0).  "Root" is joint 0.
 * Camera   a pinhole look-at camera.  Target T = (0, target_height, 0); with el = elev_deg, az = azim_deg (degrees) and a distance d,
 *          eye E = T + d (cos el sin az, sin el, cos el cos az); f = normalize(T - E), r = normalize(f x (0,1,0)), u = r x f;
 *          F = focal H / 2 pixels.  A point P has dv = P - E, depth zc = dv.f, and the screen position sx = W/2 + F (dv.r) / zc,
 *          sy = H/2 - F (dv.u) / zc.  The centre of pixel (row i, column j) is (j + 0.5, i + 0.5).  |el| < 90 and E.y > 0 (at d = dist)
 *          are required.  f, r, u do not depend on d.
 * frames   (mode LADIFF_RENDER_FRAMES) one image per rendered frame: out [B, ceil(L / frame_stride), H, W, 3]; image (b, i) shows
 *          frame t = i frame_stride.  t >= h_lengths[b]: the whole image is the background colour.  Otherwise the pose is frame t with
 *          x and z reduced by the root's x and z at t; the ground rectangle at y = 0 is x in [mins.x - root_x(t), maxs.x - root_x(t)],
 *          z likewise; d = dist; one pose of opacity 1.
 * strip    (mode LADIFF_RENDER_STRIP) one image per motion: out [B, H, W, 3].  With len = h_lengths[b], n = min(n_poses, len), the
 *          poses are the frames t_k = (k (len - 1) + (n - 1) / 2) / (n - 1) in integer division, k = 0 .. n-1 (n = 1: t_0 = 0); x and z
 *          are reduced by the centre (mins + maxs) / 2 of the bounding box; the ground is the bounding rectangle grown by
 *          ground_margin on every side; pose k has opacity a_k = alpha_min + (1 - alpha_min) (k / (n - 1)) (n = 1: 1); the camera
 *          distance is d = dist max(1, extent / strip_fit), extent = max(maxs.x - mins.x, maxs.z - mins.z), computed on the device.
 * Pixel    c = background; then, in this fixed order, c <- c (1 - q) + colour q with q = opacity x cov: the ground (opacity
 *          ground_alpha, colour ground_rgb), then the poses in time order, the chains in table order, the bones in chain order (colour
 *          chain_rgb[chain]).  No depth sort: a fixed order is continuous in the input.
 * Bone     skipped unless both endpoints have zc > near.  With the screen endpoints A, B, e = B - A and the pixel centre p:
 *          s = clamp(((p - A).e) / max(e.e, 1e-12), 0, 1), dist2d = |p - (A + s e)|, cov = clamp(0.5 + line_width / 2 - dist2d, 0, 1):
 *          a one-pixel linear edge; line_width in pixels.  A zero-length bone is a dot; nothing is NaN.
 * Ground   by ray: D = f + cx r + cy u, cx = (px - W/2) / F, cy = -(py - H/2) / F.  D.y >= 0: cov = 0.  Otherwise th = -E.y / D.y, the
 *          hit point (hx, hz) = (E.x + th D.x, E.z + th D.z), sd = min(hx - x0, x1 - hx, hz - z0, z1 - hz) for the rectangle
 *          [x0,x1] x [z0,z1], cov = clamp(0.5 + sd F / th, 0, 1).  The rectangle is bounded, so cov -> 0 towards the horizon.
 * Output   fp32 c in [0,1] (out_is_float != 0) or uint8 floor(255 c + 0.5).
 * Defaults (ladiff_amd/render.py; nothing tests them): background white, ground (0.5, 0.5, 0.5) with ground_alpha 0.5, chain colours
 *          #DD5A37 #D69E00 #B75A39 #DD5A37 #D69E00 (the first five of the reference's list), line_width = H / 54 (the reference's 4 pt on
 *          a 3 in x 100 dpi figure), elev_deg 15, azim_deg 25, dist 3.6, focal 2, target_height 0.9, near 0.1, ground_margin 0.5,
 *          alpha_min 0.25, strip_fit 3: a standing HumanML3D figure (about 1.7 units tall) fills roughly the middle half of a square image.
 *
 * Two kernels, both fp32 in every build flavour.  The scene kernel (one workgroup per motion, no atomics) writes a per-motion record -
 * bounds, length, strip pose indices, fitted distance - to the workspace, which holds nothing else
 * (ladiff_render_workspace_bytes(B), non-decreasing in B).  The raster kernel (64 x 16 pixel tiles x images) projects its image's pose
 * into LDS, culls the bones against its tile and composites; a thread owns four horizontally adjacent pixels and stores 12 (uint8) or 48
 * (fp32) contiguous bytes; out is write-only and every element is written; an image past its motion's length does no scene work.  The
 * bits of an image depend on its own motion only (a motion of a ragged batch gives the bytes it gives alone).  The camera basis is
 * computed on the host in double and rounded once; the entry neither allocates, copies nor synchronises (the lengths travel in the
 * scene kernel's arguments, one launch pair per 1024 motions) and is capturable.
 * Errors, all before any GPU work: njoints outside {21, 22} -> LADIFF_ERR_UNSUPPORTED; LADIFF_ERR_ARG for a NULL joints / h_lengths /
 * params / out / ws, B < 0, a mode other than the two, n_poses < 1, frame_stride < 1, |elev_deg| >= 90, E.y <= 0, a non-positive dist,
 * focal, line_width, near_plane or strip_fit, a negative ground_margin, or an opacity or colour component outside [0, 1];
 * LADIFF_ERR_SHAPE for L outside [1, 256], H or W outside [16, 1024], W % 4 != 0, a length outside [1, L], joints or ws not aligned to
 * 4 bytes, out not aligned to 4 (uint8) or 16 (fp32) bytes; LADIFF_ERR_WORKSPACE for ws_bytes below the query.  B == 0 does nothing. */
enum { LADIFF_RENDER_FRAMES = 0, LADIFF_RENDER_STRIP = 1 };
typedef struct ladiff_render_params {
    float elev_deg, azim_deg, dist, focal, target_height, near_plane;
    float line_width;                 /* pixels */
    float ground_margin, alpha_min, strip_fit, ground_alpha;
    float background_rgb[3], ground_rgb[3], chain_rgb[5][3];
    int32_t frame_stride;             /* frames mode: every frame_stride-th frame is rendered (1 = all); ignored by the strip */
} ladiff_render_params;
LADIFF_API size_t ladiff_render_workspace_bytes(int B);
LADIFF_API int ladiff_render_motion(const float* joints, const int32_t* h_lengths, int B, int L, int njoints,
                         const ladiff_render_params* params, int mode, int n_poses, int H, int W, void* out, int out_is_float, void* ws,
                         size_t ws_bytes, ladiff_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* LADIFF_HIP_H */
