// The trajectory buffers of ladiff_diffusion_reverse_record in the sampler's capture key (csrc/graph_key.h) and the recording rows of the
// launch policy (csrc/systolic_plan.h's LoopKey) on the CPU: plain C++17, no HIP header.  The prologue graph (padding rows) and the step
// graphs' tail nodes bake both pointers in: recording on or off, which kinds and where must all tell two keys apart.
#include <cstdio>

#include "graph_key.h"

using namespace ladiff;

#define CHECK(c)                                                                   \
    do {                                                                           \
        if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } \
    } while (0)

static float slab[64];
static int32_t starts_a[4];
static const float* W_TAB[3] = {slab + 1, slab + 2, slab + 3};

int main() {
    ReverseArgs a{};
    a.w = W_TAB; a.weights_generation = 1; a.ws = slab + 10; a.coef = slab + 11; a.text_emb = slab + 12; a.init_noise = slab + 13;
    a.z = slab + 14; a.B = 2; a.T = 5; a.n_steps = 6; a.cfg = 1; a.n_text = 1; a.guidance_scale = 7.5f; a.init_noise_sigma = 1.f;
    const unsigned off[4] = {0u, 0u, 0u, 0u};
    for (int pipeline = 0; pipeline < 2; ++pipeline) {
        auto key = [&](const ReverseArgs& x) { return sampler_key(x, 3, pipeline != 0, 1, 6, off); };
        // (1) a call without the buffers keys what it always keyed
        CHECK(a.traj_x == nullptr && a.traj_x0 == nullptr && key(a).n == 30);
        // (2) on / off, which kinds, and where
        ReverseArgs x = a, x0 = a, both = a, moved = a, swapped = a;
        x.traj_x = slab + 40;
        x0.traj_x0 = slab + 40;                                         // the same address as the other kind
        both.traj_x = slab + 40; both.traj_x0 = slab + 44;
        moved.traj_x = slab + 48; moved.traj_x0 = slab + 44;
        swapped.traj_x = slab + 44; swapped.traj_x0 = slab + 40;
        const ReverseArgs all[] = {a, x, x0, both, moved, swapped};
        for (int i = 0; i < 6; ++i)
            for (int j = 0; j < 6; ++j) CHECK((key(all[i]) == key(all[j])) == (i == j));
        CHECK(key(x).n == key(a).n + 3 && key(both).n == key(x).n && key(both) == key(ReverseArgs(both)));
        // (3) beside the multistep buffer and an edit's entries: the longest key fits, and no other pointer of the call stands in
        ReverseArgs full = both;
        full.x0_prev = slab + 20; full.z0 = slab + 30; full.starts = starts_a; full.first_step = 2;
        CHECK(key(full).n == key(a).n + 7 && key(full).n <= GraphKey::CAPACITY);
        ReverseArgs edit = a, rec = a;
        edit.z0 = slab + 40; edit.starts = reinterpret_cast<const int32_t*>(slab + 44);      // three entries more, as a recording has
        rec.traj_x = slab + 40; rec.traj_x0 = slab + 44;
        CHECK(key(edit).n == key(rec).n && key(edit) != key(rec));
        ReverseArgs ms = a;
        ms.x0_prev = slab + 40;
        CHECK(key(ms) != key(x) && key(ms) != key(x0));
    }
    std::printf("ok\n");
    return 0;
}
