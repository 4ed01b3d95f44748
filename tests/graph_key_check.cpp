// The capture keys of the library's hipGraphs (csrc/graph_key.h) on the CPU: plain C++17, built with AddressSanitizer + UBSan by
// tests/test_graph_key.py and run as a child process.  Prints "graph_key_check: ok" or the first failed property.
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <vector>

#include "graph_key.h"

using namespace ladiff;

#define CHECK(cond) \
    do { if (!(cond)) { std::printf("graph_key_check: FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); std::exit(1); } } while (0)

static float slab[64];                    // addresses for the pointer entries; never dereferenced
static const float* P(int i) { return slab + i; }

// one entry of every type; `change` (0 .. 4) replaces one of them
static GraphKey mixed(int change = -1) {
    GraphKey k;
    k.add((const void*)P(change == 0 ? 1 : 0));
    k.add(change == 1 ? -7 : 7);
    k.add(change == 2 ? 0x80000001u : 0x80000000u);
    k.add(change == 3 ? 1.5f : 0.5f);
    k.add(change == 4 ? (uint64_t(1) << 40) + 1 : uint64_t(1) << 40);
    return k;
}

static uint64_t fnv_restated(const std::vector<const float*>& w, const std::vector<const float*>* ws) {
    uint64_t h = 1469598103934665603ull;
    auto eat = [&](const std::vector<const float*>& t) {
        for (const float* p : t)
            for (int b = 0; b < 8; ++b) { h ^= ((uint64_t) reinterpret_cast<uintptr_t>(p) >> (8 * b)) & 0xff; h *= 1099511628211ull; }
    };
    eat(w);
    if (ws) { h ^= 0x9e3779b97f4a7c15ull; eat(*ws); }
    return h;
}

static const float* const W_TAB[3] = {slab + 10, slab + 11, slab + 12};
static const float* const S_TAB[3] = {slab + 20, slab + 21, slab + 22};

static ReverseArgs reverse_args(int n_text = 1) {
    ReverseArgs a{};
    a.w = W_TAB; a.w_split = S_TAB; a.weights_generation = 3;
    a.text_emb = P(30); a.init_noise = P(31); a.sinusoid = P(32); a.coef = P(33); a.step_noise = nullptr;
    a.guidance_scale = 7.5f; a.init_noise_sigma = 1.f;
    a.cfg = 1; a.B = 2; a.T = 5; a.n_text = n_text; a.n_steps = 50;
    a.z = slab + 34; a.ws = slab + 35; a.ws_bytes = 1 << 20; a.stream = slab + 36;
    return a;
}

int main() {
    // equality: field-wise, order-sensitive, by bit pattern
    CHECK(mixed() == mixed() && !(mixed() != mixed()));
    for (int c = 0; c < 5; ++c) CHECK(mixed(c) != mixed() && !(mixed(c) == mixed()));
    CHECK(GraphKey().add(1).add(2) != GraphKey().add(2).add(1));
    CHECK(GraphKey().add(0.0f) != GraphKey().add(-0.0f));
    CHECK(GraphKey().add(1).add(2) != GraphKey().add(1));              // a prefix is another key
    CHECK(GraphKey() == GraphKey() && GraphKey() != mixed() && GraphKey() != GraphKey().add(0));     // an empty key equals no filled one
    {
        GraphKey full;
        for (int i = 0; i < GraphKey::CAPACITY; ++i) full.add(i);     // exactly the capacity fits (one more aborts: not run here)
        CHECK(full.n == GraphKey::CAPACITY && full == full);
    }

    // weights_hash: FNV-1a over the pointer values of both tables
    const std::vector<const float*> w(W_TAB, W_TAB + 3), s(S_TAB, S_TAB + 3);
    CHECK(weights_hash(W_TAB, nullptr, 3) == fnv_restated(w, nullptr));
    CHECK(weights_hash(W_TAB, S_TAB, 3) == fnv_restated(w, &s));
    CHECK(weights_hash(W_TAB, S_TAB, 3) != weights_hash(W_TAB, nullptr, 3));      // split table present / absent
    CHECK(weights_hash(W_TAB, S_TAB, 3) != weights_hash(S_TAB, W_TAB, 3));        // the two tables swapped
    CHECK(weights_hash(W_TAB, W_TAB, 3) != weights_hash(W_TAB, nullptr, 3));
    for (int i = 0; i < 3; ++i) {
        const float* w2[3] = {W_TAB[0], W_TAB[1], W_TAB[2]};
        w2[i] = slab + 40;
        CHECK(weights_hash(w2, S_TAB, 3) != weights_hash(W_TAB, S_TAB, 3));       // one pointer of either table changed
        CHECK(weights_hash(W_TAB, w2, 3) != weights_hash(W_TAB, S_TAB, 3));
    }

    // the sampler's key and the noise generator's words
    const unsigned off[4] = {0u, 0u, 0u, 0u}, seed_a[4] = {11u, 12u, 0u, 1u}, seed_b[4] = {21u, 12u, 0u, 1u};
    const ReverseArgs a = reverse_args();
    CHECK(sampler_key(a, 3, true, 1, 6, seed_a) == sampler_key(a, 3, true, 1, 6, seed_b));       // pipeline: the seed is a launch argument
    CHECK(sampler_key(a, 3, false, 2, 0, seed_a) != sampler_key(a, 3, false, 2, 0, seed_b));     // launch per stage: baked into the step graph
    CHECK(sampler_key(a, 3, false, 2, 0, seed_a) == sampler_key(a, 3, false, 1, 9, seed_a));     // ... whose key ignores the unused block plan
    for (int n_text : {1, 4, 77})
        for (int mr : {1, 2})
            for (int other_mr : {1, 2})
                for (const unsigned* noise : {off, seed_a})
                    CHECK(sampler_key(reverse_args(n_text), 3, true, mr, 6, seed_a) != sampler_key(reverse_args(n_text), 3, false, other_mr, 6, noise));
    CHECK(sampler_key(a, 3, true, 1, 6, off) != sampler_key(a, 3, true, 2, 6, off) && sampler_key(a, 3, true, 1, 6, off) != sampler_key(a, 3, true, 1, 7, off));
    // every argument a graph bakes in changes the key (h_counts, sinusoid, ws_bytes and reuse_time_tables are used outside the graphs)
    const std::vector<std::function<void(ReverseArgs&)>> changes = {
        [](ReverseArgs& x) { x.ws = slab + 50; }, [](ReverseArgs& x) { x.counts = (const int32_t*)(slab + 50); },
        [](ReverseArgs& x) { x.final_counts = (const int32_t*)(slab + 50); }, [](ReverseArgs& x) { x.coef = P(50); },
        [](ReverseArgs& x) { x.step_noise = P(50); }, [](ReverseArgs& x) { x.stream = slab + 50; }, [](ReverseArgs& x) { x.text_emb = P(50); },
        [](ReverseArgs& x) { x.init_noise = P(50); }, [](ReverseArgs& x) { x.z = slab + 50; }, [](ReverseArgs& x) { x.B = 3; },
        [](ReverseArgs& x) { x.T = 4; }, [](ReverseArgs& x) { x.n_steps = 20; }, [](ReverseArgs& x) { x.cfg = 0; }, [](ReverseArgs& x) { x.n_text = 4; },
        [](ReverseArgs& x) { x.w_split = nullptr; }, [](ReverseArgs& x) { x.w = S_TAB; }, [](ReverseArgs& x) { x.weights_generation = 4; },
        [](ReverseArgs& x) { x.guidance_scale = 5.f; }, [](ReverseArgs& x) { x.init_noise_sigma = -1.f; }};
    for (bool pipeline : {false, true})
        for (const auto& change : changes) {
            ReverseArgs b = reverse_args();
            change(b);
            CHECK(sampler_key(b, 3, pipeline, 1, 6, off) != sampler_key(a, 3, pipeline, 1, 6, off));
        }

    // the decode graph's key: every field of the switch snapshot is an entry of its own
    auto dkey = [&](int sw, int v) {
        int q[6] = {1, 1, 1, 1, 1, 0};      // fused_mlp, small_rows_path, final_split, out_cross, fused_attn, mlp_variant
        if (sw >= 0) q[sw] = v;
        return decode_key(W_TAB, S_TAB, 3, 1, P(30), (const int32_t*)P(31), (const int32_t*)P(32), nullptr, 0, 2, 60, 5, 263, P(33), slab + 34,
                          slab + 35, DecSwitches{q[0], q[1], q[2], q[3], q[4], q[5]});
    };
    CHECK(dkey(-1, 0) == dkey(-1, 0));
    for (int sw = 0; sw < 6; ++sw) CHECK(dkey(sw, 2) != dkey(-1, 0));
    CHECK(dkey(0, 0) != dkey(1, 0));          // switches that the multiplied-up sum could have folded together stay apart
    {
        // two snapshots that differ only in out_cross (ladiff_debug_set_decoder_fusion + 64) give different keys
        DecSwitches a0{1, 1, 1, 1, 1, 0}, a1 = a0;
        a1.out_cross = 0;
        auto key_of = [&](const DecSwitches& q) {
            return decode_key(W_TAB, S_TAB, 3, 1, P(30), (const int32_t*)P(31), (const int32_t*)P(32), nullptr, 0, 2, 60, 5, 263, P(33), slab + 34,
                              slab + 35, q);
        };
        CHECK(key_of(a0) != key_of(a1) && key_of(a0) == key_of(a0) && key_of(a1) == key_of(a1));
    }
    CHECK(dkey(-1, 0) != sampler_key(a, 3, true, 1, 6, off));

    // dec_route: which launches a decode makes, decided once from (mode, rows, switches).  The rule restated: nothing is routed in fp32
    // mode; the small-M GEMMs below 4,096 rows if switched on; in_proj inside the attention kernel from 4,096 rows or always (2);
    // out_proj + cross-attention in one kernel only on the large-M side; the fused feed-forward from mlp_min_rows or always (2);
    // final_layer on padded tiles from 4,096 rows.
    int routes = 0;
    for (bool split_mode : {false, true})
        for (int rows : {1, 4095, 4096, 9999, 10000})
            for (int fused_mlp : {0, 1, 2})
                for (int small_rows_path : {0, 1})
                    for (int final_split : {0, 1})
                        for (int out_cross : {0, 1})
                            for (int fused_attn : {0, 1, 2}) {
                                const DecSwitches sw{fused_mlp, small_rows_path, final_split, out_cross, fused_attn, 0};
                                const DecRoute r = dec_route(split_mode, rows, sw, 10000);
                                const bool big = rows >= 4096;
                                const bool small = split_mode && !big && small_rows_path == 1;
                                CHECK(r.small == small);
                                CHECK(r.fused_attn == (split_mode && (fused_attn == 2 || (fused_attn == 1 && big))));
                                CHECK(r.out_cross == (split_mode && !small && out_cross == 1));
                                CHECK(r.fused_mlp == (split_mode && (fused_mlp == 2 || (fused_mlp == 1 && rows >= 10000))));
                                CHECK(r.final_split == (split_mode && big && final_split == 1));
                                if (!split_mode) CHECK(!r.small && !r.fused_attn && !r.out_cross && !r.fused_mlp && !r.final_split);
                                CHECK(!(r.out_cross && r.small));
                                ++routes;
                            }
    CHECK(routes == 720);
    CHECK(DEC_SMALL_ROWS == 4096);
    {   // the threshold of the fused feed-forward is the caller's argument, not a constant of the rule
        const DecSwitches sw{1, 1, 1, 1, 1, 0};
        CHECK(dec_route(true, 5000, sw, 5000).fused_mlp && !dec_route(true, 4999, sw, 5000).fused_mlp);
    }
    std::printf("graph_key_check: ok\n");
    return 0;
}
