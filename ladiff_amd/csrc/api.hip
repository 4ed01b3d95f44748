// extern "C" surface of libladiff_hip.so (declared in include/ladiff_hip.h).
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "model.h"
#include "sampler.h"
#include "../../include/ladiff_hip_debug.h"

using namespace ladiff;

namespace {

inline hipStream_t S(ladiff_stream_t s) { return reinterpret_cast<hipStream_t>(s); }

bool all_set(const float* const* w, size_t n) {
    if (w == nullptr) return false;
    for (size_t i = 0; i < n; ++i)
        if (w[i] == nullptr) return false;
    return true;
}
template <class W>
bool load_weights(W& dst, const float* const* ptrs) {
    if (!all_set(ptrs, sizeof(W) / sizeof(const float*))) return false;
    std::memcpy(&dst, ptrs, sizeof(W));
    return true;
}
const char* name_at(const std::vector<std::string>& n, int i) { return (i >= 0 && i < (int)n.size()) ? n[i].c_str() : nullptr; }

}  // namespace

#ifdef LADIFF_STAMPS
static unsigned long long* g_stamps = nullptr;
#endif

extern "C" {

int ladiff_version(void) { return LADIFF_ABI_VERSION; }
int ladiff_split_format(void) {
#ifndef LADIFF_SPLIT_BF16
    return 1;
#else
    return 0;
#endif
}

const char* ladiff_error_string(int code) {
    switch (code) {
        case LADIFF_OK: return "ok";
        case LADIFF_ERR_ARG: return "invalid argument (null pointer or negative size)";
        case LADIFF_ERR_SHAPE: return "shape not supported by the gfx950 kernels";
        case LADIFF_ERR_WORKSPACE: return "workspace too small";
        case LADIFF_ERR_UNSUPPORTED: return "configuration branch not built";
        default: return code > 0 ? hipGetErrorString((hipError_t)code) : "unknown ladiff error";
    }
}

int ladiff_denoiser_num_params(void) { return DEN_NPARAMS; }
const char* ladiff_denoiser_param_name(int i) { return name_at(denoiser_param_names(), i); }
int ladiff_decoder_num_params(void) { return DEC_NPARAMS; }
const char* ladiff_decoder_param_name(int i) { return name_at(decoder_param_names(), i); }

// ------------------------------------------------------------------ unit kernels
int ladiff_gemm(const float* A, int lda, const float* A2, int lda2, int K1, const float* W, int ldw, const float* bias,
                const float* res, int ldres, const float* ln_gamma, const float* ln_beta, float* Y, int ldy, int M,
                int N, int K, int act, ladiff_stream_t stream) {
    LADIFF_CHECK_ARG(A && W && Y && M >= 0 && N > 0 && K > 0);
    GemmArgs g;
    g.A = A; g.lda = lda; g.A2 = A2; g.lda2 = lda2; g.K1 = A2 ? K1 : K; g.W = W; g.ldw = ldw; g.bias = bias;
    g.res = res; g.ldres = ldres; g.ln_g = ln_gamma; g.ln_b = ln_beta; g.Y = Y; g.ldy = ldy; g.M = M; g.N = N; g.K = K;
    g.act = act;
    return launch_gemm(g, S(stream));
}

int ladiff_gemm_resident(const float* A, int lda, const float* A2, int lda2, int K1, const float* W, int ldw,
                         const float* bias, const float* res, int ldres, float* Y, int ldy, int M, int N, int K, int act,
                         int split, float* Ys, ladiff_stream_t stream) {
    LADIFF_CHECK_ARG(A && W && (Y || Ys) && M >= 0 && N > 0 && K > 0);
    if (M == 0) return 0;
    KrArgs g;
    g.A = A; g.lda = lda; g.A2 = A2; g.lda2 = lda2; g.K1 = A2 ? K1 : K; g.W = W; g.ldw = ldw; g.bias = bias;
    g.res = res; g.ldres = ldres; g.Y = Y; g.ldy = ldy; g.M = M; g.N = N; g.K = K; g.act = act;
    g.split = split; g.Ys = Ys;
#ifdef LADIFF_STAMPS
    g.stamps = g_stamps;
#endif
    return launch_gemm_kr(g, S(stream));
}

int ladiff_gemm_split(const float* A, int lda, const float* A2, int lda2, int K1, const float* W, int ldw, const float* bias,
                      const float* res, int ldres, float* Y, float* Ys, int ldy, int M, int N, int K, int act,
                      ladiff_stream_t stream) {
    LADIFF_CHECK_ARG(A && W && (Y || Ys) && M >= 0 && N > 0 && K > 0);
    if (M == 0) return 0;
    GemmArgs g;
    g.A = A; g.lda = lda; g.A2 = A2; g.lda2 = lda2; g.K1 = A2 ? K1 : K; g.W = W; g.ldw = ldw; g.bias = bias;
    g.res = res; g.ldres = ldres; g.Y = Y; g.Ys = Ys; g.ldy = ldy; g.M = M; g.N = N; g.K = K; g.act = act; g.split = 1;
    return launch_gemm(g, S(stream));
}

#ifdef LADIFF_STAMPS
void ladiff_debug_set_stamps(unsigned long long* p) { g_stamps = p; }   // diagnostic builds only
void ladiff_debug_set_sys_stamps(unsigned long long* p) { ladiff::g_sys_stamps = p; }
void ladiff_debug_set_probe(int v) { ladiff::g_sys_probe = v; }        // timing probes of the pipeline kernel: garbage results
#endif

int ladiff_combine_rows(const float* partials, int n_planes, int M, const float* bias, const float* res, int mode,
                        const float* ln_gamma, const float* ln_beta, const float* table, const int32_t* counts, int Bs,
                        int T, int pad_row, float* out, ladiff_stream_t stream) {
    LADIFF_CHECK_ARG(partials && out && n_planes > 0 && M >= 0 && Bs > 0 && T > 0);
    if (mode != RED_PLAIN && mode != RED_LN && mode != RED_LN_ADD && mode != RED_LN_MOD) return LADIFF_ERR_ARG;
    if (mode != RED_PLAIN && !(ln_gamma && ln_beta)) return LADIFF_ERR_ARG;
    if ((mode == RED_LN_ADD || mode == RED_LN_MOD) && !table) return LADIFF_ERR_ARG;
    if (M == 0) return 0;
    RedArgs r;
    r.P = partials; r.S = n_planes; r.M = M; r.bias = bias; r.res = res; r.mode = mode; r.g = ln_gamma; r.b = ln_beta; r.tab = table;
    r.counts = counts; r.Bs = Bs; r.T = T; r.pad_row = pad_row; r.out = out;
    return launch_reduce_rows(r, S(stream));
}

int ladiff_layernorm(const float* x, const float* gamma, const float* beta, float* y, int M, ladiff_stream_t stream) {
    LADIFF_CHECK_ARG(x && gamma && beta && y && M >= 0);
    return launch_layernorm(x, gamma, beta, y, M, S(stream));
}

int ladiff_timestep_sinusoid(const int64_t* timesteps, int n, float* out, ladiff_stream_t stream) {
    LADIFF_CHECK_ARG(timesteps && out && n >= 0);
    if (n == 0) return 0;
    return launch_sinusoid(timesteps, n, out, S(stream));
}

int ladiff_decoder_self_attention(const float* qkv, const int32_t* lengths, const uint32_t* keybits, float* out, int B,
                                  int F, ladiff_stream_t stream) {
    LADIFF_CHECK_ARG(qkv && (lengths || keybits) && out && B >= 0);
    return launch_decoder_self_attention(qkv, lengths, keybits, out, B, F, 0, S(stream));
}

int ladiff_self_attention_split(const float* qkv, const int32_t* lengths, const uint32_t* keybits, float* out, int B, int F,
                                 int nheads, int causal, ladiff_stream_t stream) {
    LADIFF_CHECK_ARG(qkv && out && B >= 0);
    return launch_self_attention_split(qkv, lengths, keybits, out, B, F, nheads, causal, 0, S(stream));
}

int ladiff_decoder_cross_attention(const float* q, const float* kv, const int32_t* counts, float* out, int B, int F,
                                   int T, ladiff_stream_t stream) {
    LADIFF_CHECK_ARG(q && kv && out && B >= 0 && F >= 0);
    return launch_decoder_cross_attention(q, kv, counts, out, B, F, T, 0, S(stream));
}

// ------------------------------------------------------------------ denoiser
size_t ladiff_denoiser_tables_floats(int n_steps) { return den_tables_floats(n_steps); }
size_t ladiff_denoiser_text_cache_floats(int B2, int n_steps, int n_text) { return den_text_cache_floats(B2, n_steps, n_text); }
size_t ladiff_denoiser_workspace_bytes(int B2, int T, int n_steps, int n_text) {
    // the largest of the three entries' layouts.  n_text > 1 switches the text cache to another algorithm with less scratch: never less
    // than the one-token form asks for, so that the query is non-decreasing in every argument
    return sizeof(float) * std::max({den_forward_ws_floats(B2, T), den_time_layout(nullptr, n_steps).total,
                                     den_text_ws_floats(B2, n_steps, n_text), den_text_ws_floats(B2, n_steps, 1)});
}
// The three denoiser entries share one query, but none of them takes all of its arguments: each refuses a workspace below the query at
// its OWN arguments (the ones it does not take at 1).  The query is non-decreasing, so this is never more than the caller's query.

int ladiff_denoiser_time_tables(const float* const* w, const float* sinusoid, int n_steps, float* tables, void* ws,
                                size_t ws_bytes, ladiff_stream_t stream) {
    DenoiserW W;
    LADIFF_CHECK_ARG(load_weights(W, w) && sinusoid && tables && ws && n_steps > 0);
    if (ws_bytes < ladiff_denoiser_workspace_bytes(1, 1, n_steps, 1)) return LADIFF_ERR_WORKSPACE;
    return denoiser_time_tables(W, sinusoid, n_steps, tables, (float*)ws, ws_bytes / sizeof(float), S(stream));
}

int ladiff_denoiser_text_cache(const float* const* w, const float* text_emb, int B2, int n_text, const float* tables, int n_steps,
                               float* cache, void* ws, size_t ws_bytes, ladiff_stream_t stream) {
    DenoiserW W;
    LADIFF_CHECK_ARG(load_weights(W, w) && text_emb && tables && cache && ws && B2 > 0 && n_steps > 0 && n_text >= 1);
    if (ws_bytes < ladiff_denoiser_workspace_bytes(B2, 1, n_steps, n_text)) return LADIFF_ERR_WORKSPACE;
    return denoiser_text_cache(W, text_emb, B2, tables, n_steps, cache, (float*)ws, ws_bytes / sizeof(float), S(stream), n_text);
}

int ladiff_denoiser_forward(const float* const* w, const float* const* w_split, const float* tables, const int32_t* d_step,
                            const float* text_cache, int n_text, int n_steps, const float* sample, int Bs, int dup, int T,
                            const int32_t* counts, float* eps, void* ws, size_t ws_bytes, ladiff_stream_t stream) {
    DenoiserW W, WS;
    LADIFF_CHECK_ARG(load_weights(W, w) && tables && d_step && text_cache && sample && eps && ws && Bs > 0 && dup > 0 && n_steps > 0 &&
                     n_text >= 1);
    if (w_split != nullptr) LADIFF_CHECK_ARG(load_weights(WS, w_split));
    if (T < 1 || T > LADIFF_MAX_LATENTS) return LADIFF_ERR_SHAPE;
    if (ws_bytes < ladiff_denoiser_workspace_bytes(Bs * dup, T, n_steps, n_text)) return LADIFF_ERR_WORKSPACE;
    return denoiser_forward(W, w_split ? &WS : nullptr, tables, d_step, text_cache, n_steps, sample, Bs, dup, T, counts, eps, (float*)ws,
                            ws_bytes / sizeof(float), S(stream), 0, -1, 0, n_text);
}

size_t ladiff_linear_cross_attention_workspace_bytes(int B, int T, int n_text) {
    return linear_cross_attention_ws_floats(B, T, n_text) * sizeof(float);
}
int ladiff_linear_cross_attention(const float* const* w, int layer, const float* x, const float* xf, const float* emb,
                                  const int32_t* counts, int B, int T, int n_text, float* out, void* ws, size_t ws_bytes,
                                  ladiff_stream_t stream) {
    DenoiserW W;
    LADIFF_CHECK_ARG(load_weights(W, w) && x && xf && emb && out && ws && B > 0);
    return linear_cross_attention(W, layer, x, xf, emb, counts, B, T, n_text, out, (float*)ws, ws_bytes / sizeof(float), S(stream));
}

// ------------------------------------------------------------------ guidance + scheduler
// the step end of the three entries below: no generator and no per-prompt scales
static StepEnd step_end(const float* coef, const float* step_noise, float guidance_scale, int cfg, float* x0_prev, bool edit, const int32_t* starts, int first_step,
                        float* traj_x = nullptr, float* traj_x0 = nullptr) {
    return StepEnd{coef, step_noise, NoiseGen{0u, 0u, 0u, 0}, guidance_scale, nullptr, cfg, x0_prev, edit, starts, first_step, traj_x, traj_x0, nullptr};
}
int ladiff_cfg_scheduler_step(const float* eps, float* latents, const float* coef, const int32_t* d_step,
                              const float* step_noise, float guidance_scale, int cfg, int B, int T,
                              ladiff_stream_t stream) {
    LADIFF_CHECK_ARG(eps && latents && coef && d_step && B > 0 && T > 0);
    return launch_cfg_step(eps, latents, d_step, step_end(coef, step_noise, guidance_scale, cfg, nullptr, false, nullptr, 0), B, T, S(stream));
}
int ladiff_cfg_scheduler_step_multistep(const float* eps, float* latents, float* x0_prev, const float* coef, const int32_t* d_step,
                                        const float* step_noise, float guidance_scale, int cfg, int B, int T, ladiff_stream_t stream) {
    LADIFF_CHECK_ARG(eps && latents && x0_prev && coef && d_step && B > 0 && T > 0);
    if (reinterpret_cast<uintptr_t>(x0_prev) & 15) return LADIFF_ERR_SHAPE;
    return launch_cfg_step(eps, latents, d_step, step_end(coef, step_noise, guidance_scale, cfg, x0_prev, false, nullptr, 0), B, T, S(stream));
}
int ladiff_cfg_scheduler_step_from(const float* eps, float* latents, float* x0_prev, const float* coef, const int32_t* d_step,
                                   const float* step_noise, float guidance_scale, int cfg, int B, int T, const int32_t* starts, int first_step,
                                   ladiff_stream_t stream) {
    LADIFF_CHECK_ARG(eps && latents && coef && d_step && B > 0 && T > 0 && first_step >= 0);
    if ((reinterpret_cast<uintptr_t>(x0_prev) & 15) || (reinterpret_cast<uintptr_t>(starts) & 3)) return LADIFF_ERR_SHAPE;
    return launch_cfg_step(eps, latents, d_step, step_end(coef, step_noise, guidance_scale, cfg, x0_prev, true, starts, first_step), B, T, S(stream));
}
int ladiff_cfg_scheduler_step_record(const float* eps, float* latents, float* x0_prev, const float* coef, const int32_t* d_step,
                                     const float* step_noise, float guidance_scale, int cfg, int B, int T, const int32_t* starts, int first_step,
                                     float* traj_x, float* traj_x0, ladiff_stream_t stream) {
    LADIFF_CHECK_ARG(eps && latents && coef && d_step && B > 0 && T > 0 && first_step >= 0);
    if ((reinterpret_cast<uintptr_t>(x0_prev) & 15) || (reinterpret_cast<uintptr_t>(starts) & 3) || (reinterpret_cast<uintptr_t>(traj_x) & 15) ||
        (reinterpret_cast<uintptr_t>(traj_x0) & 15))
        return LADIFF_ERR_SHAPE;
    return launch_cfg_step(eps, latents, d_step, step_end(coef, step_noise, guidance_scale, cfg, x0_prev, true, starts, first_step, traj_x, traj_x0),
                           B, T, S(stream));
}
int ladiff_advance_step(int32_t* d_step, ladiff_stream_t stream) {
    LADIFF_CHECK_ARG(d_step);
    return launch_advance(d_step, S(stream));
}
int ladiff_init_latents(const float* noise, const int32_t* counts, float sigma, float* latents, int B, int T,
                        ladiff_stream_t stream) {
    LADIFF_CHECK_ARG(noise && latents && B > 0 && T > 0);
    return launch_init_latents(noise, counts, sigma, latents, B, T, S(stream));
}
int ladiff_init_latents_from(const float* z0, const float* noise, const uint64_t* seeds, const uint32_t* prompt_index, const int32_t* counts,
                             const float* coef, const int32_t* starts, int first_step, float* latents, int B, int T, ladiff_stream_t stream) {
    LADIFF_CHECK_ARG(z0 && coef && latents && B > 0 && T > 0 && first_step >= 0);
    LADIFF_CHECK_ARG(noise != nullptr || seeds != nullptr);
    LADIFF_CHECK_ARG(prompt_index == nullptr || seeds != nullptr);
    if ((reinterpret_cast<uintptr_t>(z0) & 15) || (reinterpret_cast<uintptr_t>(noise) & 15) || (reinterpret_cast<uintptr_t>(latents) & 15) ||
        (reinterpret_cast<uintptr_t>(seeds) & 7) || (reinterpret_cast<uintptr_t>(prompt_index) & 3) || (reinterpret_cast<uintptr_t>(starts) & 3))
        return LADIFF_ERR_SHAPE;
    const NoiseGen gen = noise == nullptr ? NoiseGen{0u, 0u, 0u, 1, reinterpret_cast<const unsigned long long*>(seeds), prompt_index}
                                          : NoiseGen{0u, 0u, 0u, 0};
    return launch_init_latents_from(z0, noise, gen, counts, coef, starts, first_step, latents, B, T, nullptr, S(stream));
}
int ladiff_finalize_latents(const float* latents, const int32_t* counts, float* z, int B, int T, ladiff_stream_t stream) {
    LADIFF_CHECK_ARG(latents && z && B > 0 && T > 0);
    return launch_finalize_latents(latents, counts, z, B, T, S(stream));
}

// ------------------------------------------------------------------ whole reverse loop
int ladiff_sampler_create(void** sampler) {
    LADIFF_CHECK_ARG(sampler);
    *sampler = new Sampler();
    return 0;
}
int ladiff_sampler_destroy(void* sampler) {
    Sampler* sp = reinterpret_cast<Sampler*>(sampler);
    if (sp == nullptr) return 0;
    (void)hipDeviceSynchronize();         // a replay of these graphs may still be queued
    sp->drain_retired();
    if (sp->exec) (void)hipGraphExecDestroy(sp->exec);
    if (sp->setup) (void)hipGraphExecDestroy(sp->setup);
    if (sp->ev0) (void)hipEventDestroy(sp->ev0);
    if (sp->ev1) (void)hipEventDestroy(sp->ev1);
    for (hipEvent_t e : sp->wev) (void)hipEventDestroy(e);
    sp->cap.destroy();
    delete sp;
    return 0;
}

int ladiff_reverse_plan(int B, int T, const int32_t* h_counts, int masked, int loop_mode, int f16x3, int cfg, int* rows_per_block, int* n_blocks) {
    LADIFF_CHECK_ARG(B >= 1 && T >= 1 && T <= LADIFF_MAX_LATENTS && loop_mode >= 1 && loop_mode <= 3 && rows_per_block && n_blocks);
    if (!cfg && masked && h_counts == nullptr) return LADIFF_ERR_UNSUPPORTED;      // such a call runs launch-per-stage (no block plan)
    std::vector<unsigned char> plan;
    int mr = 2, nb = 0;
    choose_plan(B, T, h_counts, masked != 0, loop_mode, f16x3 != 0, plan, &mr, &nb, cfg != 0);
    *rows_per_block = 16 * mr; *n_blocks = nb;
    return 0;
}

int ladiff_debug_set_stage_waves(int waves_per_simd) {
    LADIFF_CHECK_ARG(waves_per_simd == 1 || waves_per_simd == 2);
    g_loop.waves16 = waves_per_simd;
    return 0;
}

int ladiff_debug_set_handoff(int tagged) {
    LADIFF_CHECK_ARG(tagged == 0 || tagged == 1);
    g_loop.handoff = tagged;
    return 0;
}

int ladiff_debug_set_mlp_variant(int v) {
#ifdef LADIFF_STAMPS
    LADIFF_CHECK_ARG((v >= 0 && v <= 3) || (v >= 11 && v <= 17) || (v >= 21 && v <= 26));    // the diagnostic twin also carries the timing builds
#else
    LADIFF_CHECK_ARG(v >= 0 && v <= 3);          // workgroup forms of the fused feed-forward kernel; every one gives the same result
#endif
    g_dec.mlp_variant = v;
    return 0;
}

int ladiff_debug_set_decoder_fusion(int on) {
    LADIFF_CHECK_ARG(on >= 0 && on <= 254 && (on & 3) != 3 && (on & 48) != 48);
    g_dec.post_off = (on & 128) ? 1 : 0;
    g_dec.out_cross = (on & 64) ? 0 : 1;
    g_dec.fused_mlp = on & 3;
    g_dec.small_rows_path = (on & 4) ? 0 : 1;
    g_dec.final_split = (on & 8) ? 0 : 1;
    g_dec.fused_attn = (on & 16) ? 0 : (on & 32) ? 2 : 1;
    return 0;
}

int ladiff_debug_set_stage_plan(int v) {
    LADIFF_CHECK_ARG(v >= 0 && v <= 1);
    g_loop.stage_plan = v;
    return 0;
}

int ladiff_debug_set_poll_pause(int mask, int len) {
    LADIFF_CHECK_ARG(mask >= 0 && mask <= 255 && len >= 0 && len <= 64);
    g_loop.poll_pause = mask | (len << 8);
    return 0;
}

int ladiff_debug_set_pacing(int eighths, int mask) {
    if (eighths == -1) { g_loop.pace = -1; return 0; }       // back to the built-in choice by launch size
    LADIFF_CHECK_ARG(eighths >= 0 && eighths <= 8 && mask >= 0 && mask <= 255);
    g_loop.pace = eighths | (mask << 8);
    return 0;
}

int ladiff_debug_set_stage_delay(int mask, int len) {
    LADIFF_CHECK_ARG(mask >= -1 && mask <= 255 && len >= 0 && len <= 64);
    g_loop.stage_delay = mask < 0 ? -1 : (mask | (len << 8));
    return 0;
}

int ladiff_debug_set_loop_thresholds(int look_ahead_from, int small_upto) {
    LADIFF_CHECK_ARG(look_ahead_from >= -1 && small_upto >= -1);
    g_loop.look_ahead_from = look_ahead_from;
    g_loop.small_upto = small_upto;
    return 0;
}

int ladiff_debug_set_graph_epoch_rule(int on) {
    LADIFF_CHECK_ARG(on == 0 || on == 1);
    g_graph_epoch_rule = on;
    return 0;
}

int ladiff_debug_graph_instantiations(void) { return g_graph_instantiations.load(); }

int ladiff_debug_set_xcd_local(int on) {
    LADIFF_CHECK_ARG(on >= 0 && on <= 2);
    g_loop.xcd_local = on;
    return 0;
}

int ladiff_sampler_set_loop(void* sampler, int mode) {
    Sampler* sp = reinterpret_cast<Sampler*>(sampler);
    LADIFF_CHECK_ARG(sp != nullptr && mode >= 0 && mode <= 3);
    sp->loop = mode != 0;
    sp->loop_mode = mode;
    return 0;
}

int ladiff_sampler_loop_ms(void* sampler, float* ms) {
    Sampler* sp = reinterpret_cast<Sampler*>(sampler);
    LADIFF_CHECK_ARG(sp != nullptr && ms != nullptr && sp->ev1 != nullptr);
    LADIFF_HIP(hipEventSynchronize(sp->ev1));
    LADIFF_HIP(hipEventElapsedTime(ms, sp->ev0, sp->ev1));
    return 0;
}

int ladiff_sampler_set_window_timing(void* sampler, int on) {
    Sampler* sp = reinterpret_cast<Sampler*>(sampler);
    LADIFF_CHECK_ARG(sp != nullptr);
    sp->time_windows = on != 0;
    return 0;
}

int ladiff_sampler_window_ms(void* sampler, float* loop_ms_sum, int* n_windows) {
    Sampler* sp = reinterpret_cast<Sampler*>(sampler);
    LADIFF_CHECK_ARG(sp != nullptr && loop_ms_sum != nullptr && n_windows != nullptr);
    float sum = 0.f;
    for (int i = 0; i < sp->n_windows; ++i) {
        float ms = 0.f;
        LADIFF_HIP(hipEventSynchronize(sp->wev[2 * i + 1]));
        LADIFF_HIP(hipEventElapsedTime(&ms, sp->wev[2 * i], sp->wev[2 * i + 1]));
        sum += ms;
    }
    *loop_ms_sum = sum; *n_windows = sp->n_windows;
    return 0;
}

int ladiff_sampler_last_loop(void* sampler, int* pipeline, int* rows_per_block, int* n_blocks) {
    Sampler* sp = reinterpret_cast<Sampler*>(sampler);
    LADIFF_CHECK_ARG(sp != nullptr && pipeline != nullptr);
    *pipeline = sp->last_pipeline;
    if (rows_per_block) *rows_per_block = sp->last_pipeline ? 16 * sp->plan_mr : 0;
    if (n_blocks) *n_blocks = sp->last_pipeline ? sp->plan_nb : 0;
    return 0;
}

int ladiff_sampler_set_noise_generator(void* sampler, uint64_t seed, uint32_t first_prompt, int enable) {
    Sampler* sp = reinterpret_cast<Sampler*>(sampler);
    LADIFF_CHECK_ARG(sp != nullptr);
    sp->gen = NoiseGen{(unsigned)(seed & 0xffffffffull), (unsigned)(seed >> 32), first_prompt, enable ? 1 : 0};
    return 0;
}

int ladiff_noise_fill(uint64_t seed, uint32_t first_prompt, int first_step, int n_steps, int B, int T, float* out, ladiff_stream_t stream) {
    LADIFF_CHECK_ARG(out != nullptr && first_step >= 0 && n_steps >= 0 && B >= 0);
    if (T < 1 || T > LADIFF_MAX_LATENTS) return LADIFF_ERR_SHAPE;
    return launch_noise_fill(NoiseGen{(unsigned)(seed & 0xffffffffull), (unsigned)(seed >> 32), first_prompt, 1}, first_step, n_steps, B, T, out,
                             S(stream));
}

int ladiff_noise_fill_prompts(const uint64_t* seeds, const uint32_t* prompt_index, int first_step, int n_steps, int B, int T, float* out,
                              ladiff_stream_t stream) {
    LADIFF_CHECK_ARG(out != nullptr && first_step >= -1 && n_steps >= 0 && B >= 0 && (seeds != nullptr || B == 0));
    if (T < 1 || T > LADIFF_MAX_LATENTS) return LADIFF_ERR_SHAPE;
    if ((reinterpret_cast<uintptr_t>(seeds) & 7) || (reinterpret_cast<uintptr_t>(prompt_index) & 3)) return LADIFF_ERR_SHAPE;
    return launch_noise_fill(NoiseGen{0u, 0u, 0u, 1, reinterpret_cast<const unsigned long long*>(seeds), prompt_index}, first_step, n_steps, B, T,
                             out, S(stream));
}

int ladiff_sampler_set_fault(void* sampler, int workgroup, int timeout_ms) {
    Sampler* sp = reinterpret_cast<Sampler*>(sampler);
    LADIFF_CHECK_ARG(sp != nullptr && workgroup >= -1 && workgroup < 256 && timeout_ms >= 0);
    sp->fault_wg = workgroup;
    sp->timeout_ticks = (unsigned long long)timeout_ms * 100000ull;    // s_memrealtime: 100 MHz
    return 0;
}

size_t ladiff_reverse_status_offset_bytes(int B, int T, int n_steps, int n_text) {
    if (B < 1 || T < 1 || T > LADIFF_MAX_LATENTS || n_steps < 1 || n_text < 1) return 0;
    const ReverseWs r = carve_reverse(nullptr, B, T, n_steps, n_text);
    return (r.sys_off + sys_status_offset_floats(B, T)) * sizeof(float);
}

int ladiff_reverse_status(void* ws, int B, int T, int n_steps, int n_text, int* code, int* info) {
    LADIFF_CHECK_ARG(ws && code && B > 0 && n_steps > 0);
    if (T < 1 || T > LADIFF_MAX_LATENTS) return LADIFF_ERR_SHAPE;
    const ReverseWs r = carve_reverse(ws, B, T, n_steps, n_text);
    unsigned st[2] = {0u, 0u};
    LADIFF_HIP(hipMemcpy(st, r.sys + sys_status_offset_floats(B, T), sizeof(st), hipMemcpyDeviceToHost));   // synchronises
    *code = (int)st[0];
    if (info) *info = (int)st[1];
    return 0;
}

size_t ladiff_reverse_workspace_bytes(int B, int T, int n_steps, int n_text) { return carve_reverse(nullptr, B, T, n_steps, n_text).total_bytes; }

int ladiff_mlp_ln_fused(const float* xs, const float* x, const float* w1s, const float* b1, const float* w2s, const float* b2,
                        const float* ln_gamma, const float* ln_beta, const float* ln2_gamma, const float* ln2_beta, float* y, float* ys,
                        int M, ladiff_stream_t stream) {
    LADIFF_CHECK_ARG(xs && x && w1s && b1 && w2s && b2 && ln_gamma && ln_beta && (y || ys) && M >= 0);
    if ((ln2_gamma == nullptr) != (ln2_beta == nullptr)) return LADIFF_ERR_ARG;
    return launch_dec_mlp(xs, x, w1s, b1, w2s, b2, ln_gamma, ln_beta, ln2_gamma, ln2_beta, y, ys, M, S(stream), g_dec.mlp_variant.load());
}

int ladiff_split_rows(const float* x, float* y, int R, int K, ladiff_stream_t stream) {
    LADIFF_CHECK_ARG(x && y && R >= 0 && K > 0);
    if (K % 64) return LADIFF_ERR_SHAPE;
    if (R == 0) return 0;
    return launch_split_rows(x, y, R, K, S(stream));
}

int ladiff_gather_rows(const float* src, const int32_t* index, int n_rows, int row_floats, float* dst, ladiff_stream_t stream) {
    LADIFF_CHECK_ARG(n_rows >= 0 && row_floats > 0);
    if (n_rows == 0) return 0;
    LADIFF_CHECK_ARG(src && index && dst);
    // what the host can see: 16-byte rows at 16-byte addresses, and a grid that fits (the index VALUES are device data)
    if (row_floats % 4 || (reinterpret_cast<uintptr_t>(src) & 15) || (reinterpret_cast<uintptr_t>(dst) & 15)) return LADIFF_ERR_SHAPE;
    if ((reinterpret_cast<uintptr_t>(index) & 3) || n_rows > (1 << 30)) return LADIFF_ERR_SHAPE;
    return launch_gather_rows(src, index, n_rows, row_floats, dst, S(stream));
}

int ladiff_split_range_stats(const float* const* tensors, const int64_t* counts, int n, int64_t max_count, uint64_t* stats,
                             ladiff_stream_t stream) {
    LADIFF_CHECK_ARG(n >= 0 && max_count >= 0);
    if (n == 0) return 0;
    LADIFF_CHECK_ARG(tensors && counts && stats);
    if (n > 65535 || max_count >= (int64_t(1) << 32)) return LADIFF_ERR_SHAPE;
    return launch_split_range_stats(tensors, counts, n, max_count, reinterpret_cast<unsigned long long*>(stats), S(stream));
}

int ladiff_diffusion_reverse(void* sampler, const float* const* w, const float* const* w_split, uint64_t weights_generation,
                             const float* text_emb, const float* init_noise, const int32_t* counts, const int32_t* final_counts,
                             const int32_t* h_counts, const float* sinusoid, const float* coef, const float* step_noise, float guidance_scale,
                             float init_noise_sigma, int cfg, int B, int T, int n_text, int n_steps, float* z, void* ws, size_t ws_bytes,
                             int reuse_time_tables, ladiff_stream_t stream) {
    return ladiff_diffusion_reverse_prompts(sampler, w, w_split, weights_generation, text_emb, init_noise, counts, final_counts, h_counts, sinusoid,
                                            coef, step_noise, guidance_scale, init_noise_sigma, cfg, B, T, n_text, n_steps, z, ws, ws_bytes,
                                            reuse_time_tables, nullptr, nullptr, nullptr, 0, stream);
}

int ladiff_diffusion_reverse_prompts(void* sampler, const float* const* w, const float* const* w_split, uint64_t weights_generation,
                                     const float* text_emb, const float* init_noise, const int32_t* counts, const int32_t* final_counts,
                                     const int32_t* h_counts, const float* sinusoid, const float* coef, const float* step_noise,
                                     float guidance_scale, float init_noise_sigma, int cfg, int B, int T, int n_text, int n_steps, float* z,
                                     void* ws, size_t ws_bytes, int reuse_time_tables, const float* guidance_scales, const uint64_t* seeds,
                                     const uint32_t* prompt_index, int draw_init_noise, ladiff_stream_t stream) {
    return ladiff_diffusion_reverse_multistep(sampler, w, w_split, weights_generation, text_emb, init_noise, counts, final_counts, h_counts,
                                              sinusoid, coef, step_noise, guidance_scale, init_noise_sigma, cfg, B, T, n_text, n_steps, z, ws,
                                              ws_bytes, reuse_time_tables, guidance_scales, seeds, prompt_index, draw_init_noise, nullptr, stream);
}

int ladiff_diffusion_reverse_multistep(void* sampler, const float* const* w, const float* const* w_split, uint64_t weights_generation,
                                       const float* text_emb, const float* init_noise, const int32_t* counts, const int32_t* final_counts,
                                       const int32_t* h_counts, const float* sinusoid, const float* coef, const float* step_noise,
                                       float guidance_scale, float init_noise_sigma, int cfg, int B, int T, int n_text, int n_steps, float* z,
                                       void* ws, size_t ws_bytes, int reuse_time_tables, const float* guidance_scales, const uint64_t* seeds,
                                       const uint32_t* prompt_index, int draw_init_noise, float* x0_prev, ladiff_stream_t stream) {
    return ladiff_diffusion_reverse_from(sampler, w, w_split, weights_generation, text_emb, init_noise, counts, final_counts, h_counts, sinusoid,
                                         coef, step_noise, guidance_scale, init_noise_sigma, cfg, B, T, n_text, n_steps, z, ws, ws_bytes,
                                         reuse_time_tables, guidance_scales, seeds, prompt_index, draw_init_noise, x0_prev, nullptr, nullptr, 0,
                                         stream);
}

int ladiff_diffusion_reverse_from(void* sampler, const float* const* w, const float* const* w_split, uint64_t weights_generation,
                                  const float* text_emb, const float* init_noise, const int32_t* counts, const int32_t* final_counts,
                                  const int32_t* h_counts, const float* sinusoid, const float* coef, const float* step_noise,
                                  float guidance_scale, float init_noise_sigma, int cfg, int B, int T, int n_text, int n_steps, float* z,
                                  void* ws, size_t ws_bytes, int reuse_time_tables, const float* guidance_scales, const uint64_t* seeds,
                                  const uint32_t* prompt_index, int draw_init_noise, float* x0_prev, const float* z0, const int32_t* starts,
                                  int first_step, ladiff_stream_t stream) {
    return ladiff_diffusion_reverse_record(sampler, w, w_split, weights_generation, text_emb, init_noise, counts, final_counts, h_counts, sinusoid,
                                           coef, step_noise, guidance_scale, init_noise_sigma, cfg, B, T, n_text, n_steps, z, ws, ws_bytes,
                                           reuse_time_tables, guidance_scales, seeds, prompt_index, draw_init_noise, x0_prev, z0, starts, first_step,
                                           nullptr, nullptr, stream);
}

int ladiff_diffusion_reverse_record(void* sampler, const float* const* w, const float* const* w_split, uint64_t weights_generation,
                                    const float* text_emb, const float* init_noise, const int32_t* counts, const int32_t* final_counts,
                                    const int32_t* h_counts, const float* sinusoid, const float* coef, const float* step_noise,
                                    float guidance_scale, float init_noise_sigma, int cfg, int B, int T, int n_text, int n_steps, float* z,
                                    void* ws, size_t ws_bytes, int reuse_time_tables, const float* guidance_scales, const uint64_t* seeds,
                                    const uint32_t* prompt_index, int draw_init_noise, float* x0_prev, const float* z0, const int32_t* starts,
                                    int first_step, float* traj_x, float* traj_x0, ladiff_stream_t stream) {
    DenoiserW W, WS;
    // a loop from a source motion: `starts` means nothing without z0, and the first position is one of the schedule's
    LADIFF_CHECK_ARG(starts == nullptr || z0 != nullptr);
    LADIFF_CHECK_ARG(first_step >= 0 && (first_step < n_steps || n_steps <= 0) && (z0 != nullptr || first_step == 0));
    // what the host can see of the per-prompt arguments, before anything touches the GPU (their VALUES are device data)
    LADIFF_CHECK_ARG(guidance_scales == nullptr || cfg != 0);
    LADIFF_CHECK_ARG(prompt_index == nullptr || seeds != nullptr);
    LADIFF_CHECK_ARG(!draw_init_noise || seeds != nullptr);
    LADIFF_CHECK_ARG(init_noise != nullptr || draw_init_noise);
    LADIFF_CHECK_ARG(load_weights(W, w) && text_emb && sinusoid && coef && z && ws && B > 0 && n_steps > 0);
    if (w_split != nullptr) LADIFF_CHECK_ARG(load_weights(WS, w_split));
    if (T < 1 || T > LADIFF_MAX_LATENTS || n_text < 1) return LADIFF_ERR_SHAPE;
    if ((reinterpret_cast<uintptr_t>(guidance_scales) & 3) || (reinterpret_cast<uintptr_t>(seeds) & 7) ||
        (reinterpret_cast<uintptr_t>(prompt_index) & 3) || (reinterpret_cast<uintptr_t>(x0_prev) & 15) ||
        (reinterpret_cast<uintptr_t>(z0) & 15) || (reinterpret_cast<uintptr_t>(starts) & 3) || (reinterpret_cast<uintptr_t>(traj_x) & 15) ||
        (reinterpret_cast<uintptr_t>(traj_x0) & 15))
        return LADIFF_ERR_SHAPE;
    if (z0 != nullptr && n_text != 1) return LADIFF_ERR_UNSUPPORTED;      // the text-sequence form has no loop from a source motion
    if ((traj_x != nullptr || traj_x0 != nullptr) && n_text != 1) return LADIFF_ERR_UNSUPPORTED;      // nor a recorded trajectory
    return diffusion_reverse(reinterpret_cast<Sampler*>(sampler), W, w_split ? &WS : nullptr,
                             ReverseArgs{w, w_split, weights_generation, text_emb, init_noise, counts, final_counts, h_counts, sinusoid, coef,
                                         step_noise, guidance_scale, init_noise_sigma, cfg, B, T, n_text, n_steps, z, ws, ws_bytes,
                                         reuse_time_tables, stream, guidance_scales, seeds, prompt_index, draw_init_noise ? 1 : 0, x0_prev, z0,
                                         z0 != nullptr ? starts : nullptr, z0 != nullptr ? first_step : 0, traj_x, traj_x0});
}

// ------------------------------------------------------------------ LA-VAE encoder
int ladiff_encoder_num_params(void) { return ENC_NPARAMS; }
const char* ladiff_encoder_param_name(int i) { return name_at(encoder_param_names(), i); }
size_t ladiff_encoder_workspace_bytes(int B, int F, int T, int C) { return enc_ws_floats(B, F, T, C) * sizeof(float); }

int ladiff_vae_encode(const float* const* w, const float* const* w_split, const float* features, const int32_t* lengths,
                      const int32_t* counts, const float* eps, int B, int F, int T, int C, float* mu, float* std,
                      float* latent, void* ws, size_t ws_bytes, ladiff_stream_t stream) {
    EncoderW W, WS;
    LADIFF_CHECK_ARG(load_weights(W, w) && features && lengths && counts && eps && mu && std && latent && ws && B >= 0);
    if (w_split != nullptr) LADIFF_CHECK_ARG(load_weights(WS, w_split));
    return vae_encode(W, w_split ? &WS : nullptr, features, lengths, counts, eps, B, F, T, C, mu, std, latent, (float*)ws,
                      ws_bytes / sizeof(float), S(stream));
}

int ladiff_vae_encode_dvae(const float* const* w, const float* const* w_split, const float* features, const int32_t* lengths,
                           const int32_t* counts, const float* eps, int B, int F, int T, int C, float* mu, float* std, float* latent,
                           void* ws, size_t ws_bytes, const int32_t* slot, const float* values, int n, ladiff_stream_t stream) {
    EncoderW W, WS;
    LADIFF_CHECK_ARG(load_weights(W, w) && features && lengths && counts && eps && mu && std && latent && ws && B >= 0);
    LADIFF_CHECK_ARG(slot && n >= 0 && (values || n == 0));
    if (w_split != nullptr) LADIFF_CHECK_ARG(load_weights(WS, w_split));
    if ((reinterpret_cast<uintptr_t>(slot) & 3) || (reinterpret_cast<uintptr_t>(values) & 3)) return LADIFF_ERR_SHAPE;
    return vae_encode(W, w_split ? &WS : nullptr, features, lengths, counts, eps, B, F, T, C, mu, std, latent, (float*)ws,
                      ws_bytes / sizeof(float), S(stream), slot, values, n);
}

// ------------------------------------------------------------------ stage-"vae" losses (csrc/vae_losses.hip)
size_t ladiff_vae_losses_workspace_bytes(int B, int F, int C, int J, int T) { return vae_losses_ws_floats(B, F, C, J, T) * sizeof(float); }

int ladiff_vae_losses(const float* m_rst, const float* m_ref, const float* joints_rst, const float* joints_ref, const float* mu,
                      const float* std, int B, int F, int C, int J, int T, double lambda_rec, double lambda_joint, double lambda_kl,
                      double* batch, double* acc, void* ws, size_t ws_bytes, ladiff_stream_t stream) {
    LADIFF_CHECK_ARG(m_rst && m_ref && joints_rst && joints_ref && mu && std && batch && acc && ws);
    if (B < 1 || F < 1 || C < 1 || J < 1 || T < 1) return LADIFF_ERR_SHAPE;
    for (const void* p : {(const void*)m_rst, (const void*)m_ref, (const void*)joints_rst, (const void*)joints_ref, (const void*)mu,
                          (const void*)std})
        if (reinterpret_cast<uintptr_t>(p) & 3) return LADIFF_ERR_SHAPE;
    for (const void* p : {(const void*)batch, (const void*)acc, (const void*)ws})
        if (reinterpret_cast<uintptr_t>(p) & 7) return LADIFF_ERR_SHAPE;
    const VaeLossWs a = vae_losses_layout((float*)ws, B, F, C, J, T);
    if (ws_bytes / sizeof(float) < a.total) return LADIFF_ERR_WORKSPACE;
    return launch_vae_losses(m_rst, m_ref, (size_t)B * F * C, joints_rst, joints_ref, (size_t)B * F * J * 3, mu, std, (size_t)T * B * D,
                             lambda_rec, lambda_joint, lambda_kl, a.part, a.blocks, batch, acc, S(stream));
}

// ------------------------------------------------------------------ stage "diffusion" (csrc/diffusion_stage.hip)
size_t ladiff_denoiser_forward_timesteps_workspace_bytes(int B2, int T) { return den_per_sample_ws_floats(B2, T) * sizeof(float); }

int ladiff_denoiser_forward_timesteps(const float* const* w, const float* const* w_split, const float* text_emb, int n_text,
                                      const int64_t* timesteps, const float* sample, int B2, int T, const int32_t* counts, float* eps,
                                      void* ws, size_t ws_bytes, ladiff_stream_t stream) {
    DenoiserW W, WS;
    LADIFF_CHECK_ARG(load_weights(W, w) && text_emb && timesteps && sample && eps && ws);
    if (w_split != nullptr) LADIFF_CHECK_ARG(load_weights(WS, w_split));
    if (n_text != 1) return LADIFF_ERR_UNSUPPORTED;
    if (B2 < 1 || T < 1 || T > LADIFF_MAX_LATENTS) return LADIFF_ERR_SHAPE;
    for (const void* p : {(const void*)text_emb, (const void*)sample, (const void*)eps, (const void*)ws})
        if (reinterpret_cast<uintptr_t>(p) & 15) return LADIFF_ERR_SHAPE;
    if ((reinterpret_cast<uintptr_t>(timesteps) & 7) || (reinterpret_cast<uintptr_t>(counts) & 3)) return LADIFF_ERR_SHAPE;
    if (ws_bytes < ladiff_denoiser_forward_timesteps_workspace_bytes(B2, T)) return LADIFF_ERR_WORKSPACE;
    return denoiser_forward_timesteps(W, w_split ? &WS : nullptr, text_emb, timesteps, sample, B2, T, counts, eps, (float*)ws,
                                      ws_bytes / sizeof(float), S(stream));
}

int ladiff_q_sample(const float* z, const int64_t* timesteps, const float* alphas_cumprod, int n_train, const int32_t* counts, int draw,
                    uint64_t seed, uint32_t first_prompt, float* noise, float* noisy, int B, int T, ladiff_stream_t stream) {
    LADIFF_CHECK_ARG(z && timesteps && alphas_cumprod && noise && noisy && n_train > 0);
    if (B < 1 || T < 1 || T > LADIFF_MAX_LATENTS) return LADIFF_ERR_SHAPE;
    for (const void* p : {(const void*)z, (const void*)noise, (const void*)noisy})
        if (reinterpret_cast<uintptr_t>(p) & 15) return LADIFF_ERR_SHAPE;
    if ((reinterpret_cast<uintptr_t>(timesteps) & 7) || (reinterpret_cast<uintptr_t>(alphas_cumprod) & 3) ||
        (reinterpret_cast<uintptr_t>(counts) & 3))
        return LADIFF_ERR_SHAPE;
    return launch_q_sample(z, timesteps, alphas_cumprod, n_train, counts,
                           NoiseGen{(unsigned)(seed & 0xffffffffull), (unsigned)(seed >> 32), first_prompt, draw ? 1 : 0}, noise, noisy, B, T,
                           S(stream));
}

size_t ladiff_diffusion_losses_workspace_bytes(int64_t n) { return n < 1 ? 0 : diffusion_losses_layout(nullptr, (size_t)n).total * sizeof(float); }

int ladiff_diffusion_losses(const float* noise_pred, const float* noise, int64_t n, double lambda_inst, double* batch, double* acc, void* ws,
                            size_t ws_bytes, ladiff_stream_t stream) {
    LADIFF_CHECK_ARG(noise_pred && noise && batch && acc && ws);
    if (n < 1) return LADIFF_ERR_SHAPE;
    if ((reinterpret_cast<uintptr_t>(noise_pred) & 3) || (reinterpret_cast<uintptr_t>(noise) & 3)) return LADIFF_ERR_SHAPE;
    for (const void* p : {(const void*)batch, (const void*)acc, (const void*)ws})
        if (reinterpret_cast<uintptr_t>(p) & 7) return LADIFF_ERR_SHAPE;
    const DiffLossWs a = diffusion_losses_layout((float*)ws, (size_t)n);
    if (ws_bytes / sizeof(float) < a.total) return LADIFF_ERR_WORKSPACE;
    return launch_diffusion_losses(noise_pred, noise, (size_t)n, lambda_inst, a.part, a.blocks, batch, acc, S(stream));
}

// ------------------------------------------------------------------ CLIP text encoder
int ladiff_clip_num_params(void) { return CLIP_NPARAMS; }
const char* ladiff_clip_param_name(int i) { return name_at(clip_param_names(), i); }
size_t ladiff_clip_workspace_bytes(int B, int L) { return clip_ws_floats(B, L) * sizeof(float); }

static bool load_clip(ClipW& dst, const float* const* ptrs, int n_layers) {     // only the first n_layers must be present
    if (ptrs == nullptr || n_layers < 1 || n_layers > CLIP_MAX_LAYERS) return false;
    const int n = CLIP_HEAD_NPARAMS + CLIP_LAYER_NPARAMS * n_layers;
    for (int i = 0; i < n; ++i)
        if (ptrs[i] == nullptr) return false;
    std::memset(&dst, 0, sizeof(dst));
    std::memcpy(&dst, ptrs, n * sizeof(const float*));
    return true;
}

int ladiff_clip_text_encode(const float* const* w, const float* const* w_split, int n_layers, int vocab, const int64_t* ids,
                            int B, int seq, int L, float* out, void* ws, size_t ws_bytes, ladiff_stream_t stream) {
    ClipW W, WS;
    LADIFF_CHECK_ARG(load_clip(W, w, n_layers) && ids && out && ws && B >= 0);
    if (w_split != nullptr) LADIFF_CHECK_ARG(load_clip(WS, w_split, n_layers));
    return clip_text_encode(W, w_split ? &WS : nullptr, n_layers, vocab, ids, B, seq, L, out, (float*)ws,
                            ws_bytes / sizeof(float), S(stream));
}

size_t ladiff_clip_workspace_bytes_ragged(int B, int total_rows) { return clip_ws_floats_rows(B, total_rows) * sizeof(float); }

int ladiff_clip_text_encode_ragged(const float* const* w, const float* const* w_split, int n_layers, int vocab, const int64_t* ids,
                                   int B, int seq, int L, const int32_t* seq_len, const int32_t* row_off, const int32_t* row_seq,
                                   int total_rows, float* out, void* ws, size_t ws_bytes, ladiff_stream_t stream) {
    ClipW W, WS;
    LADIFF_CHECK_ARG(load_clip(W, w, n_layers) && ids && out && ws && B >= 0 && seq_len && row_off && row_seq && total_rows >= 0);
    if (w_split != nullptr) LADIFF_CHECK_ARG(load_clip(WS, w_split, n_layers));
    return clip_text_encode(W, w_split ? &WS : nullptr, n_layers, vocab, ids, B, seq, L, out, (float*)ws,
                            ws_bytes / sizeof(float), S(stream), seq_len, row_off, row_seq, total_rows);
}

// ------------------------------------------------------------------ T2M evaluator encoders
int ladiff_t2m_movement_num_params(void) { return (int)t2m_move_param_names().size(); }
const char* ladiff_t2m_movement_param_name(int i) { return name_at(t2m_move_param_names(), i); }
int ladiff_t2m_motion_num_params(void) { return (int)t2m_motion_param_names().size(); }
const char* ladiff_t2m_motion_param_name(int i) { return name_at(t2m_motion_param_names(), i); }
int ladiff_t2m_text_num_params(void) { return (int)t2m_text_param_names().size(); }
const char* ladiff_t2m_text_param_name(int i) { return name_at(t2m_text_param_names(), i); }
size_t ladiff_t2m_movement_workspace_bytes(int B, int F, int Cin) { return t2m_move_ws_floats(B, F, Cin) * sizeof(float); }
size_t ladiff_t2m_motion_workspace_bytes(int B, int T) { return t2m_motion_ws_floats(B, T) * sizeof(float); }
size_t ladiff_t2m_text_workspace_bytes(int B, int L) { return t2m_text_ws_floats(B, L) * sizeof(float); }

int ladiff_t2m_movement_encode(const float* const* w, const float* feats, int ld, int B, int F, int Cin, float* out, void* ws,
                               size_t ws_bytes, ladiff_stream_t stream) {
    LADIFF_CHECK_ARG(all_set(w, t2m_move_param_names().size()) && feats && out && ws && B >= 0);
    return t2m_movement_encode(w, feats, ld, B, F, Cin, out, (float*)ws, ws_bytes / sizeof(float), S(stream));
}
int ladiff_t2m_motion_encode(const float* const* w, const float* movements, const int32_t* m_lens, int B, int T, float* out,
                             void* ws, size_t ws_bytes, ladiff_stream_t stream) {
    LADIFF_CHECK_ARG(all_set(w, t2m_motion_param_names().size()) && movements && m_lens && out && ws && B >= 0);
    return t2m_motion_encode(w, movements, m_lens, B, T, out, (float*)ws, ws_bytes / sizeof(float), S(stream));
}
int ladiff_t2m_text_encode(const float* const* w, const float* word_embs, const float* pos_onehot, const int32_t* cap_lens,
                           int B, int L, float* out, void* ws, size_t ws_bytes, ladiff_stream_t stream) {
    LADIFF_CHECK_ARG(all_set(w, t2m_text_param_names().size()) && word_embs && pos_onehot && cap_lens && out && ws && B >= 0);
    return t2m_text_encode(w, word_embs, pos_onehot, cap_lens, B, L, out, (float*)ws, ws_bytes / sizeof(float), S(stream));
}

// ------------------------------------------------------------------ feats2joints (the step after the path)
int ladiff_feats2joints(const float* feats, const float* mean, const float* std, int B, int F, int C, int njoints,
                        float* joints, ladiff_stream_t stream) {
    LADIFF_CHECK_ARG(feats && mean && std && joints && B >= 0);
    return launch_feats2joints(feats, mean, std, B, F, C, njoints, joints, S(stream));
}

// ------------------------------------------------------------------ joints2feats (csrc/joints2feats.hip)
int ladiff_joints2feats(const float* joints, const int32_t* h_lengths, int B, int L, int njoints, const float* target_offsets, float feet_thre,
                        const float* mean, const float* std, float* feats, ladiff_stream_t stream) {
    LADIFF_CHECK_ARG(B >= 0);
    if (njoints != 22) return LADIFF_ERR_UNSUPPORTED;            // the reference has joints2feats for HumanML3D only
    if (B == 0) return 0;
    LADIFF_CHECK_ARG(joints && h_lengths && feats && feet_thre > 0.f && (mean == nullptr) == (std == nullptr));
    for (const void* p : {(const void*)joints, (const void*)target_offsets, (const void*)mean, (const void*)std, (const void*)feats})
        if (reinterpret_cast<uintptr_t>(p) & 3) return LADIFF_ERR_SHAPE;
    return launch_joints2feats(joints, h_lengths, B, L, target_offsets, feet_thre, mean, std, feats, S(stream));
}

// ------------------------------------------------------------------ joint-space metrics (csrc/joint_metrics.hip)
namespace {
// what both entries check on the host before anything is launched
int joint_metrics_check(const void* rst, const void* ref, const int32_t* h_lengths, int B, int F, int J, const void* seq_rows, const void* acc) {
    if (J != 21 && J != 22) return LADIFF_ERR_SHAPE;
    if (F < 1 || F > LADIFF_MAX_FRAMES) return LADIFF_ERR_SHAPE;
    for (int b = 0; b < B; ++b)
        if (h_lengths[b] < 1 || h_lengths[b] > F) return LADIFF_ERR_SHAPE;
    if ((reinterpret_cast<uintptr_t>(rst) & 3) || (reinterpret_cast<uintptr_t>(ref) & 3) || (reinterpret_cast<uintptr_t>(seq_rows) & 3) ||
        (reinterpret_cast<uintptr_t>(acc) & 7))
        return LADIFF_ERR_SHAPE;
    return 0;
}
}  // namespace

int ladiff_joint_ape_ave(const float* joints_rst, const float* joints_ref, const int32_t* lengths, const int32_t* h_lengths, int B, int F,
                         int J, const int32_t* h_part_idx, float factor, float* seq_rows, double* acc, ladiff_stream_t stream) {
    LADIFF_CHECK_ARG(B >= 0);
    if (B == 0) return 0;
    LADIFF_CHECK_ARG(joints_rst && joints_ref && lengths && h_lengths && h_part_idx && seq_rows && acc && factor > 0.f);
    LADIFF_TRY(joint_metrics_check(joints_rst, joints_ref, h_lengths, B, F, J, seq_rows, acc));
    if (reinterpret_cast<uintptr_t>(lengths) & 3) return LADIFF_ERR_SHAPE;
    // LS, RS, LH, RH index the poses WITHOUT the root joint (J - 1 of them), the four foot joints the full skeleton
    for (int i = 0; i < 8; ++i)
        if (h_part_idx[i] < 0 || h_part_idx[i] >= (i < 4 ? J - 1 : J)) return LADIFF_ERR_SHAPE;
    return launch_joint_ape_ave(joints_rst, joints_ref, lengths, B, F, J, h_part_idx, factor, seq_rows, acc, S(stream));
}

int ladiff_joint_mr(const float* joints_rst, const float* joints_ref, const int32_t* h_lengths, int B, int F, int J, float* seq_rows,
                    double* acc, ladiff_stream_t stream) {
    LADIFF_CHECK_ARG(B >= 0);
    if (B == 0) return 0;
    LADIFF_CHECK_ARG(joints_rst && joints_ref && h_lengths && seq_rows && acc);
    LADIFF_TRY(joint_metrics_check(joints_rst, joints_ref, h_lengths, B, F, J, seq_rows, acc));
    return launch_joint_mr(joints_rst, joints_ref, B, F, J, seq_rows, acc, S(stream));
}

// ------------------------------------------------------------------ motion renderer (csrc/render.hip)
size_t ladiff_render_workspace_bytes(int B) { return render_ws_bytes(B); }

int ladiff_render_motion(const float* joints, const int32_t* h_lengths, int B, int L, int njoints, const ladiff_render_params* params, int mode,
                         int n_poses, int H, int W, void* out, int out_is_float, void* ws, size_t ws_bytes, ladiff_stream_t stream) {
    if (njoints != 21 && njoints != 22) return LADIFF_ERR_UNSUPPORTED;      // the two skeletons whose chains the renderer restates
    LADIFF_CHECK_ARG(B >= 0);
    if (B == 0) return 0;
    LADIFF_CHECK_ARG(joints && h_lengths && params && out && ws);
    return launch_render_motion(joints, h_lengths, B, L, njoints, *params, mode, n_poses, H, W, out, out_is_float, (float*)ws, ws_bytes,
                                S(stream));
}

// ------------------------------------------------------------------ LA-VAE decoder
size_t ladiff_decoder_workspace_bytes(int B, int F, int T, int C) {
    (void)C;
    return dec_ws_floats(B, (size_t)B * F, T) * sizeof(float);
}

int ladiff_vae_decode(const float* const* w, const float* const* w_split, const float* z, const int32_t* lengths,
                      const int32_t* counts, int B, int F, int T, int C, float* feats, void* ws, size_t ws_bytes,
                      ladiff_stream_t stream) {
    DecoderW W, WS;
    LADIFF_CHECK_ARG(load_weights(W, w) && z && lengths && feats && ws && B >= 0);
    if (w_split != nullptr) LADIFF_CHECK_ARG(load_weights(WS, w_split));
    return vae_decode(W, w_split ? &WS : nullptr, z, lengths, counts, nullptr, 0, B, F, T, C, feats, (float*)ws, ws_bytes / sizeof(float),
                      S(stream), g_dec.snapshot());
}

// ---- the decode as a replayed hipGraph (launch-bound sizes: config c1's 8 x 60 frames is ~110 launches of a few microseconds)
namespace {
struct DecodeGraph {
    hipGraphExec_t exec = nullptr;
    GraphSlot slot;                       // capture key (decode_key, graph_key.h) and epoch of `exec`
    CaptureStream cap;
};
}  // namespace

int ladiff_decoder_graph_create(void** graph) {
    LADIFF_CHECK_ARG(graph);
    *graph = new DecodeGraph();
    return 0;
}
int ladiff_decoder_graph_destroy(void* graph) {
    DecodeGraph* g = reinterpret_cast<DecodeGraph*>(graph);
    if (g == nullptr) return 0;
    (void)hipDeviceSynchronize();         // a replay may still be queued
    if (g->exec) (void)hipGraphExecDestroy(g->exec);
    g->cap.destroy();
    delete g;
    return 0;
}

int ladiff_vae_decode_graphed(void* graph, const float* const* w, const float* const* w_split, uint64_t weights_generation, const float* z,
                              const int32_t* lengths, const int32_t* counts, const int32_t* row_off, int total_rows, int B, int F, int T,
                              int C, float* feats, void* ws, size_t ws_bytes, ladiff_stream_t stream) {
    DecodeGraph* dg = reinterpret_cast<DecodeGraph*>(graph);
    DecoderW W, WS;
    LADIFF_CHECK_ARG(dg && load_weights(W, w) && z && lengths && feats && ws && B >= 0 && stream != nullptr);
    if (w_split != nullptr) LADIFF_CHECK_ARG(load_weights(WS, w_split));
    if (F < 1 || F > LADIFF_MAX_FRAMES || T < 1 || T > LADIFF_MAX_LATENTS || C < 1) return LADIFF_ERR_SHAPE;      // as the ragged entry
    if (ws_bytes < ladiff_decoder_workspace_bytes(B, F, T, C)) return LADIFF_ERR_WORKSPACE;
    hipStream_t s = S(stream);
    const DecSwitches sw = g_dec.snapshot();      // one reading: what the key holds is what the capture runs
    const GraphKey key = decode_key(w, w_split, DEC_NPARAMS, weights_generation, z, lengths, counts, row_off, total_rows, B, F, T, C, feats, ws,
                                    stream, sw);
    if (!(dg->exec && dg->slot.key == key && dg->slot.newest())) {
        if (dg->exec) { LADIFF_HIP(hipStreamSynchronize(s)); (void)hipGraphExecDestroy(dg->exec); dg->exec = nullptr; }
        LADIFF_TRY(dec_mlp_prepare());            // kernel attributes are set outside the capture
        LADIFF_TRY(dec_qkv_attn_prepare());
        LADIFF_TRY(dec_cross_prepare());
        LADIFF_TRY(dec_post_prepare());
        LADIFF_TRY(dg->cap.ensure());
        LADIFF_TRY(capture_graph(dg->cap.s, [&](hipStream_t cs) {
            // inside the capture: a zero-fill KERNEL, never a memset node (g_graph_epoch)
            if (row_off != nullptr) LADIFF_TRY(launch_zero_fill(feats, (size_t)B * F * C, cs));
            return vae_decode(W, w_split ? &WS : nullptr, z, lengths, counts, row_off, total_rows, B, F, T, C, feats, (float*)ws,
                              ws_bytes / sizeof(float), cs, sw);
        }, &dg->exec));
        dg->slot.stamp(key);
    }
    LADIFF_HIP(hipGraphLaunch(dg->exec, s));
    return 0;
}

int ladiff_vae_decode_ragged(const float* const* w, const float* const* w_split, const float* z, const int32_t* lengths,
                             const int32_t* counts, const int32_t* row_off, int total_rows, int B, int F, int T, int C, float* feats,
                             void* ws, size_t ws_bytes, ladiff_stream_t stream) {
    DecoderW W, WS;
    LADIFF_CHECK_ARG(load_weights(W, w) && z && lengths && row_off && feats && ws && B >= 0 && total_rows >= 0);
    if (w_split != nullptr) LADIFF_CHECK_ARG(load_weights(WS, w_split));
    // the documented size is the padded batch's (the ragged rows need less): refused below it, and before feats is touched
    if (F < 1 || F > LADIFF_MAX_FRAMES || T < 1 || T > LADIFF_MAX_LATENTS || C < 1) return LADIFF_ERR_SHAPE;
    if (ws_bytes < ladiff_decoder_workspace_bytes(B, F, T, C)) return LADIFF_ERR_WORKSPACE;
    // frames past each length: zero, whatever the buffer held (ladiff_vae.py:356-360)
    LADIFF_HIP(hipMemsetAsync(feats, 0, (size_t)B * F * C * sizeof(float), S(stream)));
    return vae_decode(W, w_split ? &WS : nullptr, z, lengths, counts, row_off, total_rows, B, F, T, C, feats, (float*)ws,
                      ws_bytes / sizeof(float), S(stream), g_dec.snapshot());
}

// the decode (padded when row_off == NULL, ragged otherwise) that also returns every layer's cross-attention weights; never captured
int ladiff_vae_decode_att_maps(const float* const* w, const float* const* w_split, const float* z, const int32_t* lengths,
                               const int32_t* counts, const int32_t* row_off, int total_rows, int B, int F, int T, int C, float* feats,
                               float* att_maps, void* ws, size_t ws_bytes, ladiff_stream_t stream) {
    DecoderW W, WS;
    LADIFF_CHECK_ARG(load_weights(W, w) && z && lengths && feats && att_maps && ws && B >= 0 && total_rows >= 0);
    if (w_split != nullptr) LADIFF_CHECK_ARG(load_weights(WS, w_split));
    if (F < 1 || F > LADIFF_MAX_FRAMES || T < 1 || T > LADIFF_MAX_LATENTS || C < 1) return LADIFF_ERR_SHAPE;
    if (row_off != nullptr && (size_t)total_rows > (size_t)B * F) return LADIFF_ERR_SHAPE;
    if (ws_bytes < ladiff_decoder_workspace_bytes(B, F, T, C)) return LADIFF_ERR_WORKSPACE;
    if (B == 0) return 0;
    if (row_off != nullptr) {
        LADIFF_HIP(hipMemsetAsync(feats, 0, (size_t)B * F * C * sizeof(float), S(stream)));      // as ladiff_vae_decode_ragged
        if (total_rows == 0) LADIFF_HIP(hipMemsetAsync(att_maps, 0, (size_t)NL * B * F * T * sizeof(float), S(stream)));      // no row, no launch
    }
    return vae_decode(W, w_split ? &WS : nullptr, z, lengths, counts, row_off, row_off ? total_rows : 0, B, F, T, C, feats, (float*)ws,
                      ws_bytes / sizeof(float), S(stream), g_dec.snapshot(), att_maps);
}

}  // extern "C"
