// The sampler handle of ladiff_diffusion_reverse: run by reverse.hip, created, configured and read by api.hip's ladiff_sampler_* entries.
#pragma once
#include <vector>

#include "graph_cache.h"
#include "noise_gen.h"

namespace ladiff {

struct Sampler {
    hipGraphExec_t exec = nullptr;
    hipGraphExec_t setup = nullptr;       // per-call prologue (text cache, initial latents, counter reset, first network input)
    int unroll = 1;                       // denoiser steps captured per graph launch
    int loop_mode = 1;                    // 1: pick per call, 2: 16-row length-aware blocks, 3: 32-row blocks
    std::vector<unsigned char> blocks;    // host copy of the block descriptors last uploaded (geometry of the previous call)
    int plan_mr = 0, plan_nb = 0;
    int loop = 1;                         // 1: persistent pipeline kernel when the call qualifies (systolic.hip), 0: launch per stage
    std::vector<unsigned char> stages;    // host copy of the pipeline's stage table (source of the upload)
    hipEvent_t ev0 = nullptr, ev1 = nullptr;   // bracket the N-step loop (pipeline kernel or graph replays) of the last call
    bool time_windows = false;            // measurement aid: one event pair per window of the schedule (ladiff_sampler_set_window_timing)
    std::vector<hipEvent_t> wev;          // [2 i], [2 i + 1]: around the loop launches of window i of the last call
    int n_windows = 0;
    int last_pipeline = 0;                // the last call ran the persistent pipeline kernel (1) or launch-per-stage graphs (0)
    // fault injection for the abort-path tests (ladiff_sampler_set_fault): THIS sampler's pipeline launches lose one workgroup right after
    // the start-up handshake and bound their waits; -1 / 0 = none / the default bound.  A field of the handle, not of the process.
    int fault_wg = -1;
    unsigned long long timeout_ticks = 0;
    // per-step noise drawn on the device (ladiff_sampler_set_noise_generator): used by the calls that pass step_noise = NULL
    NoiseGen gen = NoiseGen{0u, 0u, 0u, 0};
    GraphSlot slot;                       // capture key (sampler_key, graph_key.h) and epoch of `setup` / `exec`
    std::vector<hipGraphExec_t> retired;  // replaced while a launch of them could still be queued: destroyed at the next drain
    CaptureStream cap;

    void drain_retired() {                // call with the stream drained
        for (hipGraphExec_t g : retired) (void)hipGraphExecDestroy(g);
        retired.clear();
    }
};

}  // namespace ladiff
