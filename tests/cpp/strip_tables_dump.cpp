// Prints the strip tables (strip_tables, csrc/kernels_arc.hip) of every strip geometry the recogniser's dispatch reaches over the launch space
// of conv_plan_dump.cpp: the eight unit shapes x the launch descriptions x batches 1 .. 256.  Host only: neither planning nor strip_tables calls
// a HIP function.  Per distinct geometry one header line
//   geom H W compact linear nt R n_img nslot threads first last period ppx stride
// (first / last: the smallest and the largest batch that reached the geometry) and then one line of `stride` integers per strip position.
// tests/test_strip_tables.py compares every integer with a restatement of its own.
#include <array>
#include <cstdio>
#include <map>

#include "arc_conv_describe.hpp"
#include "frt_kernels.h"

int main() {
    using namespace arc_describe;
    typedef std::array<int, 9> Key;
    std::map<Key, std::array<int, 2>> seen;  // geometry -> first and last batch
    for (int i = 0; i < kNumShapes; ++i)
        for (int d = 0; d < kNumDesc; ++d)
            for (int F = 1; F <= 256; ++F) {
                ConvMfmaArgs a;
                if (!describe(kShapes[i], i == 0, d, F, a)) continue;
                ConvPlan p = conv_plan(a);
                for (int twin = 0; twin < 2; ++twin) {
                    StripGeometry g;
                    if (twin) {
                        if (!p.se_fused()) break;
                        p.take_se_tail();
                    }
                    if (!conv_strip_geometry(a, p, g)) continue;
                    const Key k = {g.H, g.W, g.compact, g.linear, g.nt, g.R, g.n_img, g.nslot, g.threads};
                    auto it = seen.find(k);
                    if (it == seen.end()) seen[k] = {F, F};
                    else it->second[0] = F < it->second[0] ? F : it->second[0], it->second[1] = F > it->second[1] ? F : it->second[1];
                }
            }
    for (const auto &kv : seen) {
        const Key &k = kv.first;
        const StripGeometry g{k[0], k[1], k[2], k[3], k[4], k[5], k[6], k[7], k[8]};
        const StripTables t = strip_tables(g);
        if ((int)t.data.size() != t.period * t.stride || t.stride != strip_table_stride(g)) return 1;
        printf("geom %d %d %d %d %d %d %d %d %d %d %d %d %d %d\n", g.H, g.W, g.compact, g.linear, g.nt, g.R, g.n_img, g.nslot, g.threads, kv.second[0], kv.second[1],
               t.period, t.ppx, t.stride);
        for (int sp = 0; sp < t.period; ++sp) {
            for (int i = 0; i < t.stride; ++i) printf(i ? " %d" : "%d", t.data[(size_t)sp * t.stride + i]);
            printf("\n");
        }
    }
    return 0;
}
