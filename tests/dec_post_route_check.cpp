// DecRoute::post and its switch (csrc/graph_key.h) on the CPU: plain C++17, built with AddressSanitizer + UBSan by
// tests/test_dec_post_route.py and run as a child process.  Prints "dec_post_route_check: ok" or the first failed property.
#include <cstdio>
#include <cstdlib>

#include "graph_key.h"

using namespace ladiff;

#define CHECK(cond) \
    do { if (!(cond)) { std::printf("dec_post_route_check: FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); std::exit(1); } } while (0)

static float slab[64];                    // addresses for the pointer entries; never dereferenced
static const float* const W_TAB[3] = {slab + 10, slab + 11, slab + 12};
static const float* const S_TAB[3] = {slab + 20, slab + 21, slab + 22};

static GraphKey key_of(const DecSwitches& q) {
    return decode_key(W_TAB, S_TAB, 3, 1, slab + 30, (const int32_t*)(slab + 31), (const int32_t*)(slab + 32), nullptr, 0, 2, 60, 5, 263, slab + 33,
                      slab + 34, slab + 35, q);
}

int main() {
    // the enumeration of tests/graph_key_check.cpp, with the new switch both ways
    int posts = 0, cases = 0;
    for (int split_mode : {0, 1})
        for (int rows : {0, 1, 480, 4095, 4096, 9999, 10000, 25088})
            for (int fused_mlp : {0, 1, 2})
                for (int small_rows_path : {0, 1})
                    for (int final_split : {0, 1})
                        for (int out_cross : {0, 1})
                            for (int fused_attn : {0, 1, 2}) {
                                const DecSwitches six{fused_mlp, small_rows_path, final_split, out_cross, fused_attn, 0};
                                CHECK(six.post_off == 0);                  // six initialisers: the switch at its default, the fused form on
                                DecRoute r[2];
                                for (int off : {0, 1}) {
                                    DecSwitches sw = six;
                                    sw.post_off = off;
                                    r[off] = dec_route(split_mode != 0, rows, sw, 10000);
                                }
                                // the old five fields: the rule restated, and untouched by the new switch
                                const bool big = rows >= 4096;
                                const bool small = split_mode && !big && small_rows_path == 1;
                                const bool mlp = split_mode && fused_mlp != 0 && (rows >= 10000 || fused_mlp == 2);
                                const bool oc = split_mode && !small && out_cross == 1;
                                for (int off : {0, 1}) {
                                    CHECK(r[off].small == small);
                                    CHECK(r[off].fused_attn == (split_mode && fused_attn != 0 && (big || fused_attn == 2)));
                                    CHECK(r[off].out_cross == oc);
                                    CHECK(r[off].fused_mlp == mlp);
                                    CHECK(r[off].final_split == (split_mode && big && final_split == 1));
                                }
                                // post: both fused forms run, not the small route, switch on
                                CHECK(r[0].post == (oc && mlp && !small));
                                CHECK(!r[1].post);
                                CHECK(!r[0].post || split_mode);
                                posts += r[0].post; ++cases;
                            }
    CHECK(posts > 0 && posts < cases);                                    // the rule is neither vacuous nor constant
    {   // the headline shape routes to the new kernel by default, config c1's 480 rows never
        const DecSwitches def{1, 1, 1, 1, 1, 0};
        CHECK(dec_route(true, 25088, def, 10000).post && !dec_route(true, 480, def, 10000).post && !dec_route(false, 25088, def, 10000).post);
        CHECK(!dec_route(true, 9999, def, 10000).post && dec_route(true, 10000, def, 10000).post);
        DecSwitches forced = def;
        forced.fused_mlp = 2;                                              // fused forms at every size: 3 rows - but never on the small route
        CHECK(!dec_route(true, 3, forced, 10000).post);
        forced.small_rows_path = 0;
        CHECK(dec_route(true, 3, forced, 10000).post);
    }
    {   // the switch is an entry of the decode graph's key
        DecSwitches a0{1, 1, 1, 1, 1, 0}, a1 = a0;
        a1.post_off = 1;
        CHECK(key_of(a0) == key_of(a0) && key_of(a1) == key_of(a1) && key_of(a0) != key_of(a1));
        CHECK(key_of(a0).n == 22 && key_of(a0).n <= GraphKey::CAPACITY);
        DecSwitches a2 = a0;
        a2.out_cross = 0;
        CHECK(key_of(a2) != key_of(a0) && key_of(a2) != key_of(a1));      // an entry of its own: not folded into a neighbour
    }
    std::printf("dec_post_route_check: ok\n");
    return 0;
}
