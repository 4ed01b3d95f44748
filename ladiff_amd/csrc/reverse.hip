// The whole reverse loop behind ladiff_diffusion_reverse: per-call prologue, N denoiser steps (the persistent pipeline kernel, replayed
// step graphs, or plain launches without a sampler), final masking.  Host sequencing only: no kernel lives here.
#include <vector>

#include "model.h"
#include "sampler.h"

namespace ladiff {
namespace {

// (a) What one call works with: its arguments, its carve of the workspace and what follows from both.
struct Call {
    const DenoiserW& W;
    const DenoiserW* WSp;
    const ReverseArgs& a;
    ReverseWs r;
    hipStream_t s;                        // the caller's stream
    int dup, B2;                          // guidance: the network sees cat([latents]*2) with text [uncond | cond]  ladiff.py:472-474
    StepEnd end;                          // what every step's tail takes, whichever loop form runs it
    float *xio, *xios;                    // network input / last-layer output buffer of the forward workspace
    bool pipeline;                        // this call runs the persistent pipeline kernel
    std::vector<unsigned char> plan;      // its block descriptors
    int plan_mr, plan_nb;
    bool edit() const { return end.edit; }                       // a loop from a source motion (ladiff_diffusion_reverse_from): z0 set
    int first() const { return end.edit ? a.first_step : 0; }    // the first schedule position this call runs
};

// the generator of a call with per-prompt seeds: no seed of its own, the arrays by pointer
NoiseGen prompt_gen(const ReverseArgs& a) {
    return NoiseGen{0u, 0u, 0u, 1, reinterpret_cast<const unsigned long long*>(a.seeds), a.prompt_index};
}

// (b) The launch sequences.  Hoisted, once per call: time tables for every step, text cache, initial latents, step counter, first
// network input.  The time tables depend on (weights, schedule) only: a caller that re-runs with both unchanged in the same workspace
// may keep them (saves ~30 small GEMM launches per call).  The rest (~50 small launches) depends on this call's text and noise; with a
// sampler it is replayed as a graph so that the host does not pace the GPU through it.
int prologue(const Call& c, hipStream_t st) {
    const ReverseArgs& a = c.a;
    const ReverseWs& r = c.r;
    if (a.n_text > 1) LADIFF_TRY(denoiser_text_cache(c.W, a.text_emb, c.B2, r.tables, a.n_steps, r.cache, r.fwd, r.fwd_floats, st, a.n_text));
    else LADIFF_TRY(denoiser_text_static(c.W, a.text_emb, c.B2, r.cache, r.fwd, r.fwd_floats, st));      // the c table: per window, below
    if (c.edit())                                          // source latents noised to each prompt's start; the step counter starts at first_step
        LADIFF_TRY(launch_init_latents_from(a.z0, a.init_noise, a.init_noise == nullptr ? prompt_gen(a) : NoiseGen{0u, 0u, 0u, 0}, a.counts, a.coef,
                                            a.starts, a.first_step, r.latents, a.B, a.T, r.d_step, st));
    else if (a.draw_init_noise && a.init_noise == nullptr)      // a tensor still wins over the generator
        LADIFF_TRY(launch_init_latents_gen(prompt_gen(a), a.counts, a.init_noise_sigma, r.latents, a.B, a.T, st));
    else LADIFF_TRY(launch_init_latents(a.init_noise, a.counts, a.init_noise_sigma, r.latents, a.B, a.T, st));
    // [0] step index, [1] tail-kernel ticket, [2] window base.  A KERNEL, not hipMemsetAsync: this runs inside the captured prologue
    // graph, and a memset NODE is what an older exec replayed wrongly (see g_graph_epoch)
    if (!c.edit()) LADIFF_TRY(launch_zero_fill(reinterpret_cast<float*>(r.d_step), 4, st));
    // a recorded trajectory: the rows past each prompt's latent count, of every position this call runs, are zeroed here (a kernel too) -
    // no tail stores to them, and the pipeline's 16-row blocks do not even carry them
    LADIFF_TRY(launch_traj_zero_pad(c.end.traj_x, c.end.traj_counts, c.first(), a.n_steps, a.B, a.T, st));
    LADIFF_TRY(launch_traj_zero_pad(c.end.traj_x0, c.end.traj_counts, c.first(), a.n_steps, a.B, a.T, st));
    // One step = the nine denoiser layers + ONE tail launch (final LayerNorm of the guidance branches, guidance,
    // scheduler step, next step's network input, step counter).  The network input / last-layer output buffer of the
    // forward workspace is primed here.
    return launch_add_pe(r.latents, c.W.query_pe, a.B, 0, c.B2, a.T, c.xio, c.xios, st);
}

int one_step(const Call& c, hipStream_t st) {
    const ReverseArgs& a = c.a;
    const ReverseWs& r = c.r;
    LADIFF_TRY(denoiser_forward(c.W, c.WSp, r.tables, r.d_step, r.cache, r.window, r.latents, a.B, c.dup, a.T, a.counts, r.eps, r.fwd,
                                r.fwd_floats, st, 0, c.B2, 1, a.n_text, r.d_step + 2));
    return launch_step_tail(c.xio, c.xios, c.W.norm.g, c.W.norm.b, r.latents, r.d_step, c.W.query_pe, c.end, a.B, a.T, st);
}

// c-table rows of the window that starts at step `lo` (plain launches, outside the graphs: `lo` changes per window)
int open_window(const Call& c, int lo) {
    const ReverseWs& r = c.r;
    if (c.a.n_text > 1) return 0;
    LADIFF_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(r.d_step + 2), lo, 1, c.s));
    return denoiser_ctab(c.W, r.tables + (size_t)lo * DEN_STEP_STRIDE, r.window, r.cache, c.B2, r.cws, r.cws_floats, c.s, c.WSp);
}

// (c) The sampler's graphs (and, for the pipeline, the stage table in the workspace) are this call's: captured again when the key
// differs, or when another handle of the library has instantiated since (GraphSlot::newest).
int ensure_graphs(Sampler* sp, const Call& c) {
    const unsigned noise[4] = {c.end.gen.seed_lo, c.end.gen.seed_hi, c.end.gen.prompt0, (unsigned)c.end.gen.on};
    const GraphKey key = sampler_key(c.a, DEN_NPARAMS, c.pipeline, c.plan_mr, c.plan_nb, noise);
    const bool same = sp->setup && sp->slot.key == key;
    if (same && sp->slot.newest()) return 0;
    if (!same) {
        // replays of the old graphs may still be queued (the host never paces the GPU): drain before destroying them
        if (sp->exec || sp->setup || !sp->retired.empty()) LADIFF_HIP(hipStreamSynchronize(c.s));
        sp->drain_retired();
        if (sp->exec) { (void)hipGraphExecDestroy(sp->exec); sp->exec = nullptr; }
        if (sp->setup) { (void)hipGraphExecDestroy(sp->setup); sp->setup = nullptr; }
    } else {
        // same key, but another sampler has instantiated since: capture again.  No drain (a chunked batch alternates two
        // samplers launch after launch): the old graphs are set aside and destroyed at the next drain
        if (sp->retired.size() >= 8) { LADIFF_HIP(hipStreamSynchronize(c.s)); sp->drain_retired(); }
        if (sp->exec) { sp->retired.push_back(sp->exec); sp->exec = nullptr; }
        if (sp->setup) { sp->retired.push_back(sp->setup); sp->setup = nullptr; }
    }
    LADIFF_TRY(sp->cap.ensure());
    const hipStream_t cs = sp->cap.s;     // captured here, replayed on the caller's stream (see CaptureStream)
    LADIFF_TRY(capture_graph(cs, [&](hipStream_t st) { return prologue(c, st); }, &sp->setup));
    if (c.pipeline && same) {
        // only the prologue graph was renewed: the stage table in the workspace is this key's
    } else if (c.pipeline) {
        // stage table of the persistent pipeline (pointers of this call's weights and workspace): built and uploaded
        // once per key; the host copy stays alive in the sampler until the next rebuild
        LADIFF_TRY(sys_build_stages(c.W, c.WSp ? *c.WSp : c.W, c.r.sys, c.plan_mr, c.plan_nb, sp->stages));
        sp->blocks.clear();               // the descriptor area moved with the layout: upload again
        LADIFF_HIP(hipMemcpyAsync(c.r.sys, sp->stages.data(), sp->stages.size(), hipMemcpyHostToDevice, c.s));
        LADIFF_HIP(hipStreamSynchronize(c.s));
    } else {
        // several steps per graph launch (the step index lives in device memory): fewer ~9 us replay gaps
        // (a loop that starts at first_step replays from there: the unroll divides the steps of its first, partial window too - first_step
        // is part of this form's key)
        int unroll = 1;
        for (int u = 2; u <= 10; ++u) if (c.r.window % u == 0 && c.first() % u == 0) unroll = u;
        sp->unroll = unroll;
        LADIFF_TRY(capture_graph(cs, [&](hipStream_t st) {
            int rc = 0;
            for (int u = 0; u < unroll && rc == 0; ++u) rc = one_step(c, st);
            return rc;
        }, &sp->exec));
    }
    sp->slot.stamp(key);
    return 0;
}

// (d) this call's block descriptors (a few KB; the runtime stages a pageable source before it returns)
int upload_blocks(Sampler* sp, const Call& c) {
    if (!c.pipeline || (c.plan_mr == sp->plan_mr && c.plan_nb == sp->plan_nb && c.plan == sp->blocks)) return 0;
    if (!sp->blocks.empty()) LADIFF_HIP(hipStreamSynchronize(c.s));      // a copy from the old buffer may still be in flight
    sp->blocks = c.plan; sp->plan_mr = c.plan_mr; sp->plan_nb = c.plan_nb;
    LADIFF_HIP(hipMemcpyAsync(c.r.sys + sys_blocks_offset_floats(c.plan_mr, c.plan_nb), sp->blocks.data(), sp->blocks.size(),
                              hipMemcpyHostToDevice, c.s));
    return 0;
}

// (e) the N steps, window by window: one pipeline launch or window / unroll replays of the step graph each, between the sampler's events
int run_windows(Sampler* sp, const Call& c) {
    const ReverseArgs& a = c.a;
    const ReverseWs& r = c.r;
    sp->last_pipeline = c.pipeline ? 1 : 0;
    sp->n_windows = 0;
    // a loop from a source motion starts inside window first / window: that window is partial (positions from.. of it), the windows
    // before it are not opened, and every table keeps its full-schedule index
    const int first = c.first(), lo0 = first / r.window * r.window;
    for (int lo = lo0; lo < a.n_steps; lo += r.window) {
        const int from = lo < first ? first : lo, n = lo + r.window - from;
        LADIFF_TRY(open_window(c, lo));
        if (lo == lo0) LADIFF_HIP(hipEventRecord(sp->ev0, c.s));     // the loop itself: from the first step's first launch
        const int wi = (lo - lo0) / r.window;
        if (sp->time_windows) {
            while ((int)sp->wev.size() < 2 * (wi + 1)) { hipEvent_t e; LADIFF_HIP(hipEventCreate(&e)); sp->wev.push_back(e); }
            LADIFF_HIP(hipEventRecord(sp->wev[2 * wi], c.s));
        }
        if (c.pipeline) {
            // the c table's row of local step s of the launch is row from - lo + s of the window's
            const float* ctab = den_cache_ctab(r.cache, c.B2, 1) + (size_t)(from - lo) * (c.B2 + 1) * LADIFF_LATENT_DIM;
            LADIFF_TRY(launch_systolic_loop(c.W, r.sys, r.tables, den_cache_tkv(r.cache, c.B2, 1), ctab, r.window, r.latents, a.counts, c.end,
                                            a.B, a.T, from, n, c.WSp ? 0 : 1, c.plan_mr, c.plan_nb, c.s, sp->fault_wg, sp->timeout_ticks));
        } else {
            for (int i = 0; i < n / sp->unroll; ++i) LADIFF_HIP(hipGraphLaunch(sp->exec, c.s));
        }
        if (sp->time_windows) { LADIFF_HIP(hipEventRecord(sp->wev[2 * wi + 1], c.s)); sp->n_windows = wi + 1; }
    }
    LADIFF_HIP(hipEventRecord(sp->ev1, c.s));
    return 0;
}

}  // namespace

int diffusion_reverse(Sampler* sp, const DenoiserW& W, const DenoiserW* WSp, const ReverseArgs& a) {
    const int dup = a.cfg ? 2 : 1;
    // the sampler's generator stands in for a step-noise tensor the caller did not pass (schedules without noise never look at either)
    // A generator that is off is all zeros: its seed must not be part of any graph key (the Python loop owner draws a fresh seed per call,
    // also for deterministic schedules - a key that changed with it re-captured ~150-node graphs on every launch-per-stage call).
    NoiseGen gen{0u, 0u, 0u, 0};
    if (sp != nullptr && a.step_noise == nullptr && sp->gen.on) gen = sp->gen;
    // per-prompt seeds need no handle to carry them (they are arguments of the call) and replace the sampler's seed: the words that
    // enter the key are then constants, the arrays are keyed by pointer
    if (a.seeds != nullptr && a.step_noise == nullptr) gen = prompt_gen(a);
    Call c{W, WSp, a, carve_reverse(a.ws, a.B, a.T, a.n_steps, a.n_text), reinterpret_cast<hipStream_t>(a.stream), dup, dup * a.B,
           StepEnd{a.coef, a.step_noise, gen, a.guidance_scale, a.guidance_scales, a.cfg, a.x0_prev, a.z0 != nullptr, a.starts, a.first_step,
                   a.traj_x, a.traj_x0, a.final_counts},
           nullptr, nullptr, false, {}, 2, 0};
    if (a.ws_bytes < c.r.total_bytes) return LADIFF_ERR_WORKSPACE;
    den_loop_io(c.r.fwd, c.B2 * a.T, &c.xio, &c.xios);
    if (WSp == nullptr) c.xios = nullptr;
    // without guidance the pipeline runs one-branch 16-row blocks, which need the latent counts on the host (or no masking at all)
    // a call that records its trajectory AND starts from a source motion does not qualify either: the pipeline has no instantiation that
    // does both, it runs as step graphs
    c.pipeline = sp != nullptr && sp->loop == 1 && a.n_text == 1 && sys_supported(a.B, a.T, a.cfg, WSp != nullptr) &&
                 (a.cfg || a.counts == nullptr || a.h_counts != nullptr) && !(c.end.record() && c.edit());
    // Block geometry of the pipeline for THIS call's lengths.  16-row blocks carry only the valid latent rows of each prompt
    // (length-aware packing; needs the counts on the host), 32-row blocks the padded T rows.  A step costs the larger of (blocks x
    // the busiest stage's time per block) and one block's trip through the 59 stages: choose_plan() picks the cheaper plan.
    if (c.pipeline) choose_plan(a.B, a.T, a.h_counts, a.counts != nullptr, sp->loop_mode, WSp != nullptr, c.plan, &c.plan_mr, &c.plan_nb, a.cfg != 0);

    // abort / diagnostic words of the pipeline loop: cleared once per call (they are sticky over the call's windows; every
    // other loop form leaves them at "completed")
    LADIFF_TRY(sys_reset_status(c.r.sys, c.s));
    if (!a.reuse_time_tables) LADIFF_TRY(denoiser_time_tables(W, a.sinusoid, a.n_steps, c.r.tables, c.r.fwd, c.r.fwd_floats, c.s));
    if (sp == nullptr) {
        LADIFF_TRY(prologue(c, c.s));
        for (int i = c.first(); i < a.n_steps; ++i) {
            if (i % c.r.window == 0 || i == c.first()) LADIFF_TRY(open_window(c, i / c.r.window * c.r.window));
            LADIFF_TRY(one_step(c, c.s));
        }
    } else {
        LADIFF_TRY(ensure_graphs(sp, c));
        LADIFF_HIP(hipGraphLaunch(sp->setup, c.s));
        if (sp->ev0 == nullptr) { LADIFF_HIP(hipEventCreate(&sp->ev0)); LADIFF_HIP(hipEventCreate(&sp->ev1)); }
        LADIFF_TRY(upload_blocks(sp, c));
        LADIFF_TRY(run_windows(sp, c));
    }
    // (f) final zeroing of the rows past each motion's latent count: applied even when the denoiser ran unmasked
    // (TEST_EFFICIENCY), as ladiff.py:559-566 does.  An aborted pipeline launch leaves partial latents: z is then NaN.
    return launch_finalize_latents(c.r.latents, a.final_counts, a.z, a.B, a.T, c.s,
                                   reinterpret_cast<const unsigned*>(c.r.sys + sys_status_offset_floats(a.B, a.T)));
}

}  // namespace ladiff
