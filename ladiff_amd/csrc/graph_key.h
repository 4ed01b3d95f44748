// The capture key of a hipGraph as a value.  A graph bakes pointers, shapes and scalars into its kernel nodes: it may be replayed only
// for a call that would bake in the same ones.  A key is the list of them, every entry added by name, compared entry by entry; a new
// input to a graph is one more add in its builder below.  Plain C++17 with no HIP header, like systolic_plan.h: tests/graph_key_check.cpp
// runs this header on the CPU under sanitizers (tests/test_graph_key.py).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <cstring>

namespace ladiff {

struct GraphKey {
    static constexpr int CAPACITY = 40;                  // entries; the sampler's key has 30, 31 with x0_prev, up to 34 with z0 / starts / first_step, up to 37 with traj_x / traj_x0, the decode graph's 22.  One too many aborts.
    uint64_t v[CAPACITY] = {0};
    int n = 0;

    GraphKey& add(uint64_t x) {
        if (n == CAPACITY) std::abort();                 // never a silently shorter key
        v[n++] = x;
        return *this;
    }
    GraphKey& add(const void* p) { return add((uint64_t) reinterpret_cast<uintptr_t>(p)); }
    GraphKey& add(int x) { return add((uint64_t)(int64_t)x); }
    GraphKey& add(unsigned x) { return add((uint64_t)x); }
    GraphKey& add(float x) {                             // by bit pattern: 0.0f and -0.0f are different keys
        uint32_t u;
        static_assert(sizeof(u) == sizeof(x), "float is 32 bits");
        std::memcpy(&u, &x, sizeof(u));
        return add((uint64_t)u);
    }
    bool operator==(const GraphKey& o) const { return n == o.n && std::equal(v, v + n, o.v); }
    bool operator!=(const GraphKey& o) const { return !(*this == o); }
};

// A weight table is identified by a hash over EVERY pointer of both tables plus the caller's generation id (bumped whenever a table is
// rebuilt), not by the address of the host array (which a rebuilt table can land on again).  FNV-1a over the pointer values.
inline uint64_t fnv1a_ptrs(const float* const* p, int n, uint64_t h) {
    for (int i = 0; i < n; ++i) {
        const uint64_t x = reinterpret_cast<uintptr_t>(p[i]);
        for (int b = 0; b < 8; ++b) { h ^= (x >> (8 * b)) & 0xff; h *= 1099511628211ull; }
    }
    return h;
}
inline uint64_t weights_hash(const float* const* w, const float* const* w_split, int n) {
    const uint64_t h = fnv1a_ptrs(w, n, 1469598103934665603ull);
    return w_split != nullptr ? fnv1a_ptrs(w_split, n, h ^ 0x9e3779b97f4a7c15ull) : h;
}

// The parameter list of ladiff_diffusion_reverse (include/ladiff_hip.h) as a record: api.hip fills it, the sampler's key reads it here,
// ladiff::diffusion_reverse (reverse.hip) runs it.
struct ReverseArgs {
    const float* const* w;
    const float* const* w_split;
    uint64_t weights_generation;
    const float *text_emb, *init_noise;
    const int32_t *counts, *final_counts, *h_counts;
    const float *sinusoid, *coef, *step_noise;
    float guidance_scale, init_noise_sigma;
    int cfg, B, T, n_text, n_steps;
    float* z;
    void* ws;
    size_t ws_bytes;
    int reuse_time_tables;
    void* stream;
    // ladiff_diffusion_reverse_prompts: what varies per prompt is device data ([B] arrays, null = the scalar of the call)
    const float* guidance_scales;
    const uint64_t* seeds;
    const uint32_t* prompt_index;
    int draw_init_noise;                  // the prologue draws the initial noise from `seeds` (schedule position -1) instead of reading init_noise
    // ladiff_diffusion_reverse_multistep: the caller's [B,T,256] buffer of the previous data prediction, or null (one-step rule)
    float* x0_prev;
    // ladiff_diffusion_reverse_from: the loop starts from source latents z0 [T,B,256] noised to each prompt's own schedule position
    // (starts [B] device, or null: all at first_step); positions first_step .. n_steps - 1 run.  z0 null: neither is looked at.
    const float* z0 = nullptr;
    const int32_t* starts = nullptr;
    int first_step = 0;
    // ladiff_diffusion_reverse_record: the caller's [n_steps,B,T,256] buffers for the latents after each position / each position's data
    // prediction, either or both null (nothing is recorded)
    float* traj_x = nullptr;
    float* traj_x0 = nullptr;
};

// Key of a sampler's graphs (prologue graph + step graph, or prologue graph + the pipeline's stage table).  n_params: pointers per weight
// table.  pipeline / plan_mr / plan_nb: the loop form of this call and its block plan (launch-per-stage: pass any plan, it is keyed as 0).
// noise[4]: the noise generator's words {seed_lo, seed_hi, prompt0, on}, baked into the step graphs' tail nodes.  The pipeline kernel takes
// them as launch arguments instead (nothing captured holds them), so a pipeline call keys four zeros: the loop owner draws a fresh seed per
// call and must not capture again for it.  The zeros cannot make a pipeline key equal a launch-per-stage key with the generator off:
// the `pipeline` and `plan_mr` entries (1 and 1 | 2 against 0 and 0) differ between any two such keys.
// The per-prompt arrays (guidance_scales, seeds, prompt_index) are keyed by POINTER: the prologue graph and the step graphs' tail nodes
// hold the pointers, the values are read when a graph runs - new scales or seeds in the same buffers replay what is there.
// x0_prev (the multistep form's state buffer) is baked into the step graphs' tail nodes: keyed by pointer as well, as an entry that only
// a call with the buffer has - a call without it keys exactly what it keyed before.
// z0 / starts (ladiff_diffusion_reverse_from): the prologue graph and the step graphs' tail nodes hold the pointers, the pipeline kernel takes
// them as launch arguments next to the captured prologue: keyed by pointer under a marker entry, again entries that only such a call has.
// first_step is baked in where a captured node holds it: the launch-per-stage form (its prologue sets the step counter) and a call without
// `starts` (the prologue kernel noises every prompt to first_step).  A pipeline call with `starts` passes it as a launch argument only: not
// keyed, new starts or a new first_step replay what is there.
// traj_x / traj_x0 (ladiff_diffusion_reverse_record): the prologue graph (its padding rows) and the step graphs' tail nodes hold the pointers,
// and a recording pipeline call runs other instantiations on another plan policy: keyed by pointer under a marker entry that only a recording
// call has - on or off, which kinds and where are all part of the key, so a plan never replays a graph of the other kind.
inline GraphKey sampler_key(const ReverseArgs& a, int n_params, bool pipeline, int plan_mr, int plan_nb, const unsigned noise[4]) {
    GraphKey k;
    k.add(a.ws);
    k.add(a.counts);
    k.add(a.final_counts);
    k.add(a.coef);
    k.add(a.step_noise);
    k.add(a.stream);
    k.add(a.text_emb);
    k.add(a.init_noise);
    k.add(a.z);
    k.add(a.B);
    k.add(a.T);
    k.add(a.n_steps);
    k.add(a.cfg);
    k.add(a.n_text);
    k.add(a.w_split != nullptr ? 1 : 0);
    k.add(pipeline ? 1 : 0);
    k.add(pipeline ? plan_mr : 0);
    k.add(pipeline ? plan_nb : 0);
    k.add(a.guidance_scale);
    k.add(a.init_noise_sigma);
    for (int i = 0; i < 4; ++i) k.add(pipeline ? 0u : noise[i]);
    k.add(weights_hash(a.w, a.w_split, n_params));
    k.add(a.weights_generation);
    k.add(a.guidance_scales);
    k.add(a.seeds);
    k.add(a.prompt_index);
    k.add(a.draw_init_noise);
    if (a.x0_prev != nullptr) k.add(a.x0_prev);          // one entry more, so never equal to a key without the buffer (operator== compares n)
    if (a.z0 != nullptr) {
        k.add(a.z0);
        k.add(a.starts);
        k.add(!pipeline || a.starts == nullptr ? a.first_step : -1);
    }
    if (a.traj_x != nullptr || a.traj_x0 != nullptr) {
        k.add((uint64_t)0x7472616a);                             // "traj": after it the two pointers, never a position an edit's entries take
        k.add(a.traj_x);
        k.add(a.traj_x0);
    }
    return k;
}

struct DecSwitches {              // one reading of the decoder's measurement switches (model.h, g_dec): each changes a decode's launch sequence
    int fused_mlp;                // ladiff_debug_set_decoder_fusion: 0 = linear1 / linear2 / LayerNorm as three launches, 1 = fused from dec_mlp_min_rows() rows, 2 = fused always
    int small_rows_path;          // (bit 2 clear / set): the small-M GEMM routing
    int final_split;              // (+ 8 clears it): final_layer on the large-M f16x3 kernel, else on the fp32 kernel as in round 2
    int out_cross;                // (+ 64 clears it): out_proj + cross-attention in one kernel, else the GEMM + the row kernel as two launches (the path before)
    int fused_attn;               // (+ 16 clears it, + 32 = always): in_proj inside the attention kernel, else GEMM + attention kernel as two launches (the path before)
    int mlp_variant;              // ladiff_debug_set_mlp_variant: workgroup form of the fused feed-forward kernel
    int post_off;                 // (+ 128 sets it): 0 = out_proj .. norm2 + the feed-forward in ONE kernel where both fused forms run, 1 = as two launches (the path before)
};
// Which launches a decode makes (decoder.hip), decided once per call; vae_decode branches on nothing else.  small: the GEMMs on the small-M
// kernels; fused_attn: in_proj inside the attention kernel; out_cross: out_proj .. norm2 in one kernel (never on the small route); fused_mlp: the
// feed-forward block in one kernel; final_split: final_layer on padded f16x3 tiles; post: out_cross and fused_mlp as ONE kernel (dec_post.hip).
// All false in fp32 mode (truth tables: tests/graph_key_check.cpp, tests/dec_post_route_check.cpp).
constexpr int DEC_SMALL_ROWS = 4096;
struct DecRoute { bool small, fused_attn, out_cross, fused_mlp, final_split, post; };
inline DecRoute dec_route(bool split_mode, int rows, const DecSwitches& sw, int mlp_min_rows) {
    DecRoute r;
    r.small = split_mode && rows < DEC_SMALL_ROWS && sw.small_rows_path;
    r.fused_attn = split_mode && sw.fused_attn && (rows >= DEC_SMALL_ROWS || sw.fused_attn == 2);
    r.out_cross = split_mode && !r.small && sw.out_cross;
    r.fused_mlp = split_mode && sw.fused_mlp && (rows >= mlp_min_rows || sw.fused_mlp == 2);
    r.final_split = split_mode && rows >= DEC_SMALL_ROWS && sw.final_split;
    r.post = r.out_cross && r.fused_mlp && !r.small && !sw.post_off;
    return r;
}
// Key of a decode graph (ladiff_vae_decode_graphed): EVERY field of the call's switch snapshot is part of it.
inline GraphKey decode_key(const float* const* w, const float* const* w_split, int n_params, uint64_t weights_generation, const float* z,
                           const int32_t* lengths, const int32_t* counts, const int32_t* row_off, int total_rows, int B, int F, int T, int C,
                           const float* feats, const void* ws, const void* stream, const DecSwitches& sw) {
    GraphKey k;
    k.add(z);
    k.add(lengths);
    k.add(counts);
    k.add(row_off);
    k.add(feats);
    k.add(ws);
    k.add(stream);
    k.add(B);
    k.add(F);
    k.add(T);
    k.add(C);
    k.add(total_rows);
    k.add(w_split != nullptr ? 1 : 0);
    k.add(sw.fused_mlp);
    k.add(sw.small_rows_path);
    k.add(sw.final_split);
    k.add(sw.mlp_variant);
    k.add(sw.fused_attn);
    k.add(sw.out_cross);
    k.add(sw.post_off);
    k.add(weights_hash(w, w_split, n_params));
    k.add(weights_generation);
    return k;
}

}  // namespace ladiff
