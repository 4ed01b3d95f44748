// The per-prompt arguments of ladiff_diffusion_reverse_prompts in the sampler's capture key (csrc/graph_key.h) on the CPU: plain C++17,
// built with AddressSanitizer + UBSan by tests/test_prompt_params.py and run as a child process.  Prints "prompt_params_key_check: ok"
// or the first failed property.
#include <cstdio>
#include <cstdlib>

#include "graph_key.h"

using namespace ladiff;

#define CHECK(cond) \
    do { if (!(cond)) { std::printf("prompt_params_key_check: FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); std::exit(1); } } while (0)

static float slab[64];                    // addresses for the pointer entries; never dereferenced
static uint64_t seeds_a[4], seeds_b[4];
static uint32_t index_a[4], index_b[4];
static const float* const W_TAB[3] = {slab + 10, slab + 11, slab + 12};
static const float* const S_TAB[3] = {slab + 20, slab + 21, slab + 22};

static ReverseArgs reverse_args() {
    ReverseArgs a{};
    a.w = W_TAB; a.w_split = S_TAB; a.weights_generation = 3;
    a.text_emb = slab + 30; a.init_noise = slab + 31; a.sinusoid = slab + 32; a.coef = slab + 33;
    a.guidance_scale = 7.5f; a.init_noise_sigma = 1.f;
    a.cfg = 1; a.B = 4; a.T = 5; a.n_text = 1; a.n_steps = 50;
    a.z = slab + 34; a.ws = slab + 35; a.ws_bytes = 1 << 20; a.stream = slab + 36;
    return a;
}

int main() {
    const unsigned off[4] = {0u, 0u, 0u, 0u}, on[4] = {0u, 0u, 0u, 1u};
    const ReverseArgs a = reverse_args();
    CHECK(a.guidance_scales == nullptr && a.seeds == nullptr && a.prompt_index == nullptr && a.draw_init_noise == 0);
    for (int pipeline = 0; pipeline < 2; ++pipeline) {
        auto key = [&](const ReverseArgs& x, const unsigned* noise = nullptr) { return sampler_key(x, 3, pipeline != 0, 1, 6, noise ? noise : off); };
        // null arrays: equal keys for equal scalar arguments, and the scalar still counts
        CHECK(key(a) == key(reverse_args()));
        ReverseArgs g = reverse_args();
        g.guidance_scale = 5.f;
        CHECK(key(g) != key(a));
        // each pointer and the flag is an entry of its own
        ReverseArgs s = reverse_args(), sd = reverse_args(), si = reverse_args(), d = reverse_args();
        s.guidance_scales = slab + 40;
        sd.seeds = seeds_a;
        si.seeds = seeds_a; si.prompt_index = index_a;
        d.seeds = seeds_a; d.draw_init_noise = 1;
        CHECK(key(s) != key(a) && key(sd) != key(a) && key(si) != key(sd) && key(d) != key(sd));
        CHECK(key(s) != key(sd) && key(s) != key(si) && key(si) != key(d));
        // another buffer is another key; the same buffer is the same key whatever it holds (the values are device data, never read here)
        ReverseArgs s2 = s, sd2 = sd, si2 = si;
        s2.guidance_scales = slab + 41; sd2.seeds = seeds_b; si2.prompt_index = index_b;
        CHECK(key(s2) != key(s) && key(sd2) != key(sd) && key(si2) != key(si));
        seeds_a[0] = 11; index_a[0] = 3; slab[40] = 2.5f;
        CHECK(key(s) == key(ReverseArgs(s)) && key(sd) == key(ReverseArgs(sd)) && key(si) == key(ReverseArgs(si)));
        seeds_a[0] = 0; index_a[0] = 0; slab[40] = 0.f;
        // a pointer in one slot is not the same pointer in another
        ReverseArgs x = reverse_args(), y = reverse_args();
        x.guidance_scales = reinterpret_cast<const float*>(seeds_a);
        y.seeds = seeds_a;
        CHECK(key(x) != key(y));
        // the generator's words of a launch-per-stage call with seeds are constants: they add nothing per call
        CHECK(key(sd, on) == key(ReverseArgs(sd), on));
        CHECK(key(d).n == 30 && key(a).n == 30 && key(a).n <= GraphKey::CAPACITY);
    }
    std::printf("prompt_params_key_check: ok\n");
    return 0;
}
