// The multistep form's state buffer in the sampler's capture key (csrc/graph_key.h) on the CPU: plain C++17, no HIP header.  The step
// graphs' tail nodes bake the x0_prev pointer in, so a call with another buffer - or without one - must not replay them.
#include <cstdio>

#include "graph_key.h"

using namespace ladiff;

#define CHECK(c)                                                                   \
    do {                                                                           \
        if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } \
    } while (0)

static float slab[64];
static const float* W_TAB[3] = {slab + 1, slab + 2, slab + 3};

int main() {
    ReverseArgs a{};
    a.w = W_TAB; a.weights_generation = 1; a.ws = slab + 10; a.coef = slab + 11; a.text_emb = slab + 12; a.init_noise = slab + 13;
    a.z = slab + 14; a.B = 2; a.T = 5; a.n_steps = 6; a.cfg = 1; a.n_text = 1; a.guidance_scale = 7.5f; a.init_noise_sigma = 1.f;
    const unsigned off[4] = {0u, 0u, 0u, 0u};
    for (int pipeline = 0; pipeline < 2; ++pipeline) {
        auto key = [&](const ReverseArgs& x) { return sampler_key(x, 3, pipeline != 0, 1, 6, off); };
        ReverseArgs m = a, m2 = a;
        m.x0_prev = slab + 20; m2.x0_prev = slab + 24;
        CHECK(a.x0_prev == nullptr && key(a) == key(ReverseArgs(a)));
        CHECK(key(m) != key(a) && key(m2) != key(a) && key(m) != key(m2));      // with / without a buffer, and two buffers
        CHECK(key(m) == key(ReverseArgs(m)));
        CHECK(key(m).n == key(a).n + 1 && key(m).n <= GraphKey::CAPACITY);      // a call without the buffer keys what it always keyed
        // no other pointer of the call can stand in for the buffer: the entry has a place of its own
        ReverseArgs s = a;
        s.prompt_index = reinterpret_cast<const uint32_t*>(slab + 20);
        CHECK(key(s) != key(m));
    }
    std::printf("ok\n");
    return 0;
}
