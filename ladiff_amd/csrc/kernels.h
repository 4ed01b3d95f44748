// Launchers of the non-GEMM kernels (rowops.hip, attention.hip).
#pragma once
#include "common.h"
#include "noise_gen.h"

namespace ladiff {

// rowops.hip
enum RedMode : int { RED_PLAIN = 0, RED_LN = 1, RED_LN_ADD = 2, RED_LN_MOD = 3 };
// reduce_rows_kernel's arguments (the kernel takes the struct as it is: the field order is its kernarg layout).  A caller sets what its
// mode reads; row `row` belongs to sample b2 = b_off + row / T of the duplicated batch, whose latent count is counts[b2 % Bs].
struct RedArgs {
    const float* P = nullptr;                 // S planes of [M][256], `plane` floats apart
    const float* bias = nullptr; const float* res = nullptr;
    const float* g = nullptr; const float* b = nullptr;               // LayerNorm (every mode but RED_PLAIN)
    const float* tab = nullptr;               // RED_LN_ADD: c table, rows [sample | pad_row]; RED_LN_MOD: (scale | shift); table row 0
    const int32_t* d_step = nullptr;          // table row = *d_step - *d_base, `tab_step_stride` floats apart (NULL = 0)
    const int32_t* counts = nullptr;          // RED_LN_ADD: latent rows >= counts[..] take the pad row (NULL = none does)
    float* out = nullptr; float* outs = nullptr;                      // fp32 result, S-format twin (each optional)
    const int32_t* d_base = nullptr;          // RED_LN_ADD: the table's first row belongs to step *d_base (windowed c table)
    const float* g2 = nullptr; const float* b2 = nullptr;             // RED_LN: a second LayerNorm on the result (the decoder's last layer: norm3, then decoder.norm)
    size_t plane = 0;                         // = M * 256, filled by the launcher
    int S = 1, mode = RED_PLAIN, tab_step_stride = 0, Bs = 1, T = 1, pad_row = 0, b_off = 0, M = 0;
};
// per_sample: the table row is the row's sample b2 instead of *d_step, and RED_LN_ADD's valid row is row 0 of it (pad_row = 1 and
// tab_step_stride = 512 address a [B2][valid | pad][256] table)
int launch_reduce_rows(const RedArgs& a, hipStream_t s, bool per_sample = false);
int launch_split_rows(const float* x, float* y, int R, int K, hipStream_t s);
int launch_gather_rows(const float* src, const int32_t* index, int n_rows, int row_floats, float* dst, hipStream_t s);
int launch_split_range_stats(const float* const* xs, const int64_t* counts, int n, int64_t max_count, unsigned long long* stats,
                             hipStream_t s);
int launch_layernorm(const float* x, const float* g, const float* b, float* y, int M, hipStream_t s);
constexpr int DEC_PREP_MAX = 9;
struct DecCrossPrepBatch { const float* kv[DEC_PREP_MAX]; const float* wq[DEC_PREP_MAX]; const float* bq[DEC_PREP_MAX];
                           const float* wo[DEC_PREP_MAX]; float* gu[DEC_PREP_MAX]; };
// the same op on up to ROW_BATCH_MAX independent (x, g, b, y) sets of one M, one launch (grid.y = set)
constexpr int ROW_BATCH_MAX = 9;
struct RowBatch { const float* a[ROW_BATCH_MAX]; const float* g[ROW_BATCH_MAX]; const float* b[ROW_BATCH_MAX]; float* y[ROW_BATCH_MAX]; };
int launch_layernorm_batch(const RowBatch& rb, int n, int M, hipStream_t s);
// ca_table_input for n_layers layers at once: a = nval, g = beta, b = mod (step 0) , y = u of each layer
int launch_ca_table_input_batch(const RowBatch& rb, int n_layers, int step_stride, int n, int B2, hipStream_t s, int split_out = 0);
int launch_ca_table_input(const float* nval, const float* beta, const float* mod, int step_stride, int n, int B2, float* u,
                          hipStream_t s);
int launch_add_pe(const float* sample, const float* pe, int Bs, int b_off, int b_n, int T, float* x, float* xs, hipStream_t s);
int launch_broadcast_pe(const float* pe, int B, int F, float* x, float* xs, hipStream_t s);
// ragged form: sample b owns rows [row_off[b], row_off[b + 1]); also writes each row's place in a [B, F_out, *] tensor to row_out
int launch_broadcast_pe_ragged(const float* pe, const int32_t* row_off, int B, int F, int F_out, float* x, float* xs, int32_t* row_out,
                               hipStream_t s);
int launch_relu(const float* x, float* y, size_t n, hipStream_t s);
int launch_pad_rows(const float* src, const float* srcb, float* dst, float* dstb, int C, int Np, hipStream_t s);
int launch_zero_fill(float* x, size_t n, hipStream_t s);          // kernel, not a memset node (graphs: graph_cache.h g_graph_epoch)
int launch_silu(const float* x, float* y, size_t n, hipStream_t s);
int launch_sinusoid(const int64_t* t, int n, float* out, hipStream_t s);
// What the end of a denoiser step takes besides its buffers and shape.  Whoever builds one sets every field: no defaults to hide a forgotten one.
struct StepEnd {
    const float *coef, *noise;    // the schedule's coefficient rows (step_coef, step_rule.h); step-noise tensor, or null: `gen`
    NoiseGen gen;                 // stands in for `noise` (off: NoiseGen{0u, 0u, 0u, 0}); schedules without noise look at neither
    float g; const float* gs;     // guidance scale of the call; [B] per-prompt scales (device) instead of it, or null
    int cfg;                      // classifier-free guidance: the network ran on both branches
    float* x0_prev;               // [B,T,256] previous data prediction (multistep form), or null (one-step rule)
    bool edit; const int32_t* starts; int first_step;   // a loop from a source motion: prompt b enters the schedule at starts[b] ([B], device; null: at first_step), step_gate in step_rule.h
    // the denoising trajectory ([n,B,T,256] each, or null): row `step` takes the latents after the step / the step's data prediction; rows
    // t >= traj_counts[b] are left alone (the loop's prologue zeroed them, launch_traj_zero_pad); traj_counts null: every row is written.  DESIGN 8k
    float *traj_x, *traj_x0; const int32_t* traj_counts;
    bool record() const { return traj_x != nullptr || traj_x0 != nullptr; }
};
// rows t >= counts[b] of positions [first, n) of a trajectory buffer = 0 (counts null: nothing to do).  A kernel, as launch_zero_fill is
int launch_traj_zero_pad(float* traj, const int32_t* counts, int first, int n, int B, int T, hipStream_t s);
int launch_cfg_step(const float* eps, float* lat, const int32_t* d_step, const StepEnd& e, int B, int T, hipStream_t s);
int launch_advance(int32_t* d_step, hipStream_t s);
int launch_step_tail(float* x, float* xs, const float* ng, const float* nb, float* lat, int32_t* d_step, const float* pe, const StepEnd& e,
                     int B, int T, hipStream_t s);
int launch_noise_fill(const NoiseGen& gen, int step0, int n, int B, int T, float* out, hipStream_t s);
int launch_init_latents(const float* noise, const int32_t* counts, float sigma, float* lat, int B, int T, hipStream_t s);
int launch_init_latents_gen(const NoiseGen& gen, const int32_t* counts, float sigma, float* lat, int B, int T, hipStream_t s);   // gen.seeds set
// latents = valid (alpha(s_b) z0 + sigma(s_b) noise): z0 [T,B,256]; noise null = gen at position -1; d_step (or null) is left at {first_step, 0, 0, 0}
int launch_init_latents_from(const float* z0, const float* noise, const NoiseGen& gen, const int32_t* counts, const float* coef,
                             const int32_t* starts, int first_step, float* lat, int B, int T, int32_t* d_step, hipStream_t s);
int launch_finalize_latents(const float* lat, const int32_t* counts, float* z, int B, int T, hipStream_t s, const unsigned* status = nullptr);

int launch_dec_qkv_attn(const float* xs, const float* w, const float* bias, const int32_t* lengths, const int32_t* row_off, float* out,
                        int B, int F, int split_out, hipStream_t s);
int launch_scatter_feats(const float* tmp, int ldt, int C, int M, int F, const int32_t* row_len, const int32_t* row_map, float* feats,
                         hipStream_t s);
int launch_pad_cols(const float* x, float* y, int R, int C, int Cp, hipStream_t s);
// pad_cols of features [B,F,C] with the DVAE corruption added on the way: slot [F*C] (a column of values [B,n], or -1)
int launch_dvae_pad_cols(const float* x, const int32_t* slot, const float* values, int n, float* y, int B, int F, int C, int Cp,
                         hipStream_t s);
int launch_encoder_assemble(const float* token, const float* emb, const float* pe, const int32_t* lengths,
                            const int32_t* counts, int B, int F, int T, float* x, float* xs, uint32_t* keybits, hipStream_t s);
int launch_encoder_finalize(const float* out, const float* eps, const int32_t* counts, int B, int T, int S, float* mu, float* sd,
                            float* latent, hipStream_t s);

// linear_ca.hip: text conditioning with more than one text token per prompt
int launch_lca_kv(const float* key, const float* value, int B, int N, float* att, hipStream_t s);
int launch_lca_apply(const float* q, const float* att, const int32_t* counts, int Bs, int b_off, int b_n, int T, const float* mod,
                     int step_stride, int sample_stride, const int32_t* d_step, const float* g, const float* be, float* u,
                     hipStream_t s);
int launch_denoiser_self_attention_general(const float* qkv, const float* text_kv, int N, const float* tables, int kv_off,
                                           int step_stride, const int32_t* d_step, const int32_t* counts, int Bs, int b_off,
                                           int b_n, int T, float* out, hipStream_t s);

// dec_cross.hip: the decoder's cross-attention block (q projection, attention over <= 8 memory tokens, out projection,
// residual, norm2) as a per-sample low-rank map
int launch_decoder_cross_prep(const DecCrossPrepBatch& pb, int n, int B, int T, hipStream_t s);
// g1 / b1 (optional): x holds pre-norm1 rows and the kernel applies LayerNorm(g1, b1) to each row as it loads it
int launch_decoder_out_cross(const float* att_s, const float* x0, const float* wo_s, const float* bo, const float* g1, const float* b1,
                             const float* bo_c, const float* g2, const float* b2, const int32_t* counts, int B, int F, int T,
                             const float* gu_ws, float* y, float* ys, hipStream_t s, const int32_t* row_off);
int launch_decoder_cross_apply(const float* x, const float* bo, const float* g2, const float* b2, const int32_t* counts, int B, int F,
                               int T, const float* gu_ws, float* y, float* ys, hipStream_t s, const int32_t* row_off = nullptr,
                               const float* g1 = nullptr, const float* b1 = nullptr);
// the head-averaged cross-attention weights of the rows cross_apply reads (same x, g1 / b1, gu_ws): maps [B][F][T], frames >= lengths[b]
// and tokens >= counts[b] zero
int launch_decoder_cross_maps(const float* x, const int32_t* counts, const int32_t* lengths, int B, int F, int T, const float* gu_ws,
                              float* maps, hipStream_t s, const int32_t* row_off, const float* g1, const float* b1);

// feats2joints.hip
int launch_feats2joints(const float* feats, const float* mean, const float* stdv, int B, int F, int C, int J, float* joints,
                        hipStream_t s);

// joints2feats.hip: h_lengths is the HOST array of frame counts (they travel in the kernel arguments)
int launch_joints2feats(const float* joints, const int32_t* h_lengths, int B, int L, const float* tgt, float feet_thre, const float* mean,
                        const float* stdv, float* feats, hipStream_t s);

// render.hip: joints -> stick-figure images (the image model: include/ladiff_hip.h).  Every refusal but the NULL / B / njoints ones is
// made here, on the host, before the first launch; ws holds render_ws_bytes(B) of per-motion scene records and nothing else
size_t render_ws_bytes(int B);
int launch_render_motion(const float* joints, const int32_t* h_lengths, int B, int L, int J, const ladiff_render_params& P, int mode,
                         int n_poses, int H, int W, void* out, int out_is_float, float* ws, size_t ws_bytes, hipStream_t s);

// joint_metrics.hip: one row of sums per sequence, then the rows added to acc in fp64 in sequence order
int launch_joint_ape_ave(const float* rst, const float* ref, const int32_t* lengths, int B, int F, int J, const int32_t* part_idx,
                         float factor, float* seq_rows, double* acc, hipStream_t s);
int launch_joint_mr(const float* rst, const float* ref, int B, int F, int J, float* seq_rows, double* acc, hipStream_t s);

// vae_losses.hip: the stage-"vae" losses of one batch (per-workgroup fp64 partial sums in fixed slots, then one workgroup adds them)
int launch_vae_losses(const float* m_rst, const float* m_ref, size_t n_feat, const float* j_rst, const float* j_ref, size_t n_joint,
                      const float* mu, const float* sd, size_t n_lat, double l_rec, double l_joint, double l_kl, double* part, int blocks,
                      double* batch, double* acc, hipStream_t s);

// attention.hip
// d_step == NULL: the time token's K|V of sample b come from table row b (one timestep per sample), not from row *d_step
int launch_denoiser_self_attention(const float* qkv, const float* text_kv, const float* tables, int kv_off,
                                   int step_stride, const int32_t* d_step, const int32_t* counts, int Bs, int b_off,
                                   int b_n, int T, float* out, int split_out, hipStream_t s);
// row_off (optional, B + 1 entries): ragged rows - sample b owns rows [row_off[b], row_off[b + 1]) and F only bounds the lengths
int launch_decoder_self_attention(const float* qkv, const int32_t* lengths, const uint32_t* keybits, float* out, int B, int F,
                                  int split_out, hipStream_t s, const int32_t* row_off = nullptr, int shared_qkv = 0);
int launch_self_attention(const float* qkv, const int32_t* lengths, const uint32_t* keybits, float* out, int B, int F, int nheads,
                          int causal, int split_out, hipStream_t s, const int32_t* row_off = nullptr);
int launch_self_attention_split(const float* qkv, const int32_t* lengths, const uint32_t* keybits, float* out, int B, int F,
                                 int nheads, int causal, int split_out, hipStream_t s, const int32_t* row_off = nullptr, int shared_qkv = 0);
int launch_decoder_cross_attention(const float* q, const float* kv, const int32_t* counts, float* out, int B, int F,
                                   int T, int split_out, hipStream_t s);

}  // namespace ladiff
