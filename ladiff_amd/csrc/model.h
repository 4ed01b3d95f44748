// Host-side sequencing entry points shared by denoiser.hip / decoder.hip / reverse.hip / api.hip.  Where each entry's workspace regions lie, and the
// size queries (*_ws_floats, *_floats, den_cache_*, den_loop_io, carve_reverse), is workspace.h's: one layout per workspace.
#pragma once
#include <atomic>
#include "graph_key.h"
#include "seq.h"             // gemm.h, gemm_kr.h, kernels.h, weights.h; lin / kr, the pair type and the builders the sequencers share
#include "systolic_plan.h"
#include "workspace.h"

namespace ladiff {

int denoiser_time_tables(const DenoiserW& w, const float* sinus, int n, float* tables, float* ws, size_t ws_floats, hipStream_t s);
int denoiser_text_cache(const DenoiserW& w, const float* text, int B2, const float* tables, int n_steps, float* cache,
                        float* ws, size_t ws_floats, hipStream_t s, int ntxt = 1);
int denoiser_forward(const DenoiserW& w, const DenoiserW* w_split, const float* tables, const int32_t* d_step,
                     const float* cache, int n_steps, const float* sample, int Bs, int dup, int T, const int32_t* counts, float* eps, float* ws,
                     size_t ws_floats, hipStream_t s, int b_lo = 0, int b_n = -1, int loop_mode = 0, int ntxt = 1,
                     const int32_t* d_base = nullptr, const float* dctab = nullptr);
// n_steps = steps the c table inside `cache` covers; d_base (or NULL = 0) holds the step its first row belongs to
// d_step == NULL: one timestep per SAMPLE - `tables` holds one row per sample of the batch and the c table is the diagonal
// dctab [9][B2][valid | pad][256] (diffusion_stage.hip), not the one inside `cache`; one text token, no loop_mode
int denoiser_text_static(const DenoiserW& w, const float* text, int B2, float* cache, float* ws, size_t ws_floats, hipStream_t s);
int denoiser_ctab(const DenoiserW& w, const float* tables_lo, int n, float* cache, int B2, float* u, size_t u_floats, hipStream_t s,
                  const DenoiserW* w_split = nullptr);
int linear_cross_attention(const DenoiserW& w, int layer, const float* x, const float* xf, const float* emb, const int32_t* counts,
                           int B, int T, int N, float* out, float* ws, size_t ws_floats, hipStream_t s);

// diffusion_stage.hip: the forward with one timestep per sample (stage "diffusion" outside the sampling loop; one text token) in `ws`
// (den_per_sample_layout), q-sample, and the noise-prediction loss
int denoiser_forward_timesteps(const DenoiserW& w, const DenoiserW* w_split, const float* text, const int64_t* timesteps, const float* sample,
                               int B2, int T, const int32_t* counts, float* eps, float* ws, size_t ws_floats, hipStream_t s);
int launch_q_sample(const float* z, const int64_t* ts, const float* acp, int n_train, const int32_t* counts, const NoiseGen& gen, float* noise,
                    float* noisy, int B, int T, hipStream_t s);
int launch_diffusion_losses(const float* pred, const float* noise, size_t n, double lambda_inst, double* part, int blocks, double* batch,
                            double* acc, hipStream_t s);

// reverse.hip: the whole reverse loop of ladiff_diffusion_reverse (arguments checked by the caller); sp may be null (plain launches)
struct Sampler;      // sampler.h
int diffusion_reverse(Sampler* sp, const DenoiserW& w, const DenoiserW* w_split, const ReverseArgs& a);

// decoder.hip.  Its measurement switches (ladiff_debug_set_decoder_fusion / _mlp_variant), an object like the loop's (systolic_plan.h, g_loop): a decode
// reads them ONCE - the snapshot (DecSwitches, graph_key.h) routes the whole call and is in its graph's key
struct DecSwitchAtoms {
    std::atomic<int> fused_mlp{1}, small_rows_path{1}, final_split{1}, out_cross{1}, fused_attn{1}, mlp_variant{0}, post_off{0};
    DecSwitches snapshot() const { return {fused_mlp, small_rows_path, final_split, out_cross, fused_attn, mlp_variant, post_off}; }
};
extern DecSwitchAtoms g_dec;
int dec_mlp_prepare();           // per-device kernel attributes (dynamic LDS): outside any stream capture, under a mutex
int dec_qkv_attn_prepare();
int dec_cross_prepare();
int dec_mlp_min_rows();
// att_maps (optional, [NL][B][F][T]): the head-averaged cross-attention weights of every layer as well (an analysis call, nine launches more)
int vae_decode(const DecoderW& w, const DecoderW* w_split, const float* z, const int32_t* lengths, const int32_t* counts,
               const int32_t* row_off, int R, int B, int F, int T, int C, float* feats, float* ws, size_t ws_floats, hipStream_t s, const DecSwitches& sw,
               float* att_maps = nullptr);

// dec_mlp.hip: the decoder layer's feed-forward block (linear1, GELU, linear2, residual, LayerNorm[s]) as one kernel, f16x3 mode
int launch_dec_mlp(const float* xs, const float* x, const float* w1, const float* b1, const float* w2, const float* b2, const float* g3,
                   const float* be3, const float* g4, const float* be4, float* y, float* ys, int M, hipStream_t s, int variant);      // DecSwitches::mlp_variant

// dec_post.hip: out_proj + norm1 + cross-attention + norm2 + the feed-forward block above as one kernel, f16x3 mode (DecRoute::post)
struct DecPostArgs {
    const float* att;          // [M,256] S-format: the self-attention output (heads concatenated)
    const float* x0;           // [M,256] fp32: the layer input (residual)
    const float* wo;           // self_attn.out_proj.weight [256,256] S-format
    const float *bo, *g1, *be1;                    // out_proj bias, norm1
    const float *gu, *cc;                          // the layer's G | U^T (launch_dec_post_gu's layout) and score offsets
    const float *bo_c, *g2, *be2;                  // cross-attention out_proj bias, norm2
    const int32_t *counts, *row_off;
    const float *w1, *b1, *w2, *b2, *g3, *be3, *g4, *be4;      // as launch_dec_mlp
    float *y, *ys;             // fp32 / S-format results (either may be NULL)
    int B, F, T, M;
};
int dec_post_prepare();          // per-device kernel attribute, as dec_mlp_prepare
int launch_dec_post_gu(float* guws, size_t gu_layer, int n, int B, int T, hipStream_t s);
int launch_dec_post(const DecPostArgs& a, hipStream_t s);

int vae_encode(const EncoderW& w, const EncoderW* w_split, const float* features, const int32_t* lengths,
               const int32_t* counts, const float* eps, int B, int F, int T, int C, float* mu, float* sd, float* latent, float* ws,
               size_t ws_floats, hipStream_t s, const int32_t* slot = nullptr, const float* values = nullptr, int n_values = 0);

// systolic.hip: the guided denoiser loop as one persistent weight-stationary pipeline (both arithmetic modes); its host planner
// (workspace carve, block packing, stage table, choose_plan) is systolic_plan.hip, declared in systolic_plan.h
#ifdef LADIFF_STAMPS
extern unsigned long long* g_sys_stamps;
extern int g_sys_probe;
#endif
bool sys_supported(int B, int T, int cfg, bool split);
int sys_reset_status(float* ws, hipStream_t s);
int sys_build_stages(const DenoiserW& W, const DenoiserW& WS, float* ws, int MR, int NB, std::vector<unsigned char>& host);   // probes the device, then the planner's
int launch_systolic_loop(const DenoiserW& W, float* ws, const float* tables, const float* tkv, const float* ctab, int n_ctab, float* lat,
                         const int32_t* counts, const StepEnd& e, int B, int T, int step_lo, int n, int fp32, int MR, int NB, hipStream_t s,
                         int fault_wg, unsigned long long timeout_ticks);

// qkv_attn.hip: in_proj GEMM + self-attention of the denoiser's sa_block in one launch (f16x3 mode, S-format in / out)
int launch_qkv_attention(const float* x, const float* w, const float* bias, const float* text_kv, const float* tables,
                         int kv_off, int step_stride, const int32_t* d_step, const int32_t* counts, int Bs, int b_off,
                         int b_n, int T, float* out, hipStream_t s);

int clip_text_encode(const ClipW& w, const ClipW* w_split, int n_layers, int vocab, const int64_t* ids, int B, int S, int L,
                     float* out, float* ws, size_t ws_floats, hipStream_t s, const int32_t* seq_len = nullptr,
                     const int32_t* row_off = nullptr, const int32_t* row_seq = nullptr, int total_rows = 0);

// evaluator.hip: T2M evaluator encoders; tables are pointer arrays in *_param_names() order
const std::vector<std::string>& t2m_move_param_names();
const std::vector<std::string>& t2m_motion_param_names();
const std::vector<std::string>& t2m_text_param_names();
int t2m_movement_encode(const float* const* w, const float* feats, int ld, int B, int F, int Cin, float* out, float* ws,
                        size_t ws_floats, hipStream_t s);
int t2m_motion_encode(const float* const* w, const float* mov, const int32_t* m_lens, int B, int T, float* out, float* ws,
                      size_t ws_floats, hipStream_t s);
int t2m_text_encode(const float* const* w, const float* word_embs, const float* pos_onehot, const int32_t* cap_lens, int B, int L,
                    float* out, float* ws, size_t ws_floats, hipStream_t s);

}  // namespace ladiff
