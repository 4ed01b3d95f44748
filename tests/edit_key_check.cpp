// The source latents and per-prompt starts of ladiff_diffusion_reverse_from in the sampler's capture key (csrc/graph_key.h) on the CPU:
// plain C++17, no HIP header.  The prologue graph and the step graphs' tail nodes bake the two pointers in; the pipeline kernel takes
// first_step as a launch argument, so a pipeline call with `starts` must replay for any first_step.
#include <cstdio>

#include "graph_key.h"

using namespace ladiff;

#define CHECK(c)                                                                   \
    do {                                                                           \
        if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } \
    } while (0)

static float slab[64];
static int32_t starts_a[4], starts_b[4];
static const float* W_TAB[3] = {slab + 1, slab + 2, slab + 3};

int main() {
    ReverseArgs a{};
    a.w = W_TAB; a.weights_generation = 1; a.ws = slab + 10; a.coef = slab + 11; a.text_emb = slab + 12; a.init_noise = slab + 13;
    a.z = slab + 14; a.B = 2; a.T = 5; a.n_steps = 6; a.cfg = 1; a.n_text = 1; a.guidance_scale = 7.5f; a.init_noise_sigma = 1.f;
    const unsigned off[4] = {0u, 0u, 0u, 0u};
    for (int pipeline = 0; pipeline < 2; ++pipeline) {
        auto key = [&](const ReverseArgs& x) { return sampler_key(x, 3, pipeline != 0, 1, 6, off); };
        // (1) a call without z0 / starts keys what it always keyed: 30 entries, 31 with x0_prev - whatever first_step says
        ReverseArgs m = a, f = a;
        m.x0_prev = slab + 20;
        f.first_step = 3;
        CHECK(a.z0 == nullptr && a.starts == nullptr && a.first_step == 0);
        CHECK(key(a).n == 30 && key(m).n == 31 && key(f) == key(a));
        // (2) the pointers enter the key, as entries of their own
        ReverseArgs e = a, e2 = a, es = a, es2 = a;
        e.z0 = slab + 30; e2.z0 = slab + 34;
        es.z0 = slab + 30; es.starts = starts_a;
        es2.z0 = slab + 30; es2.starts = starts_b;
        CHECK(key(e) != key(a) && key(e) != key(e2) && key(e) == key(ReverseArgs(e)));
        CHECK(key(es) != key(e) && key(es) != key(es2) && key(es) == key(ReverseArgs(es)));
        CHECK(key(e).n == key(a).n + 3 && key(es).n == key(e).n && key(es).n <= GraphKey::CAPACITY);
        ReverseArgs em = es;
        em.x0_prev = slab + 20;
        CHECK(key(em).n == key(a).n + 4 && key(em).n <= GraphKey::CAPACITY && key(em) != key(es) && key(em) != key(m));
        // no other pointer of the call can stand in for them
        ReverseArgs s = a;
        s.x0_prev = slab + 30;
        CHECK(key(s) != key(e));
        // (3) first_step: not part of a pipeline key with `starts` (a launch argument there); part of every key whose captured nodes
        // hold it - the launch-per-stage form, and a call without `starts`, whose prologue kernel noises every prompt to first_step
        ReverseArgs es3 = es, e3 = e;
        es3.first_step = 3; e3.first_step = 3;
        if (pipeline) CHECK(key(es3) == key(es));
        else CHECK(key(es3) != key(es));
        CHECK(key(e3) != key(e));
    }
    std::printf("ok\n");
    return 0;
}
