// Prints what the recogniser's dispatch (conv_plan, csrc/kernels_arc.hip) decides over the whole space of launches the IR / IR-SE backbones
// make: the eight unit shapes x the launch descriptions frt_embedder::forward() fills x batches 1 .. 256, as maximal batch ranges over which
// (label, consumes the fused shortcut, can carry the SE tail) is constant.  Host only: planning calls no HIP function.
// tests/test_conv_plan.py compares the output with tests/golden/arc_conv_plan.txt.
#include <cstdint>
#include <cstdio>
#include <string>

#include "arc_conv_describe.hpp"
#include "frt_kernels.h"

namespace {

using namespace arc_describe;

std::string probe(const ConvMfmaArgs &a) {
    const ConvPlan p = conv_plan(a);
    return std::string(p.label) + " scx=" + (p.uses_scx ? "1" : "0") + " se=" + (p.se_fused() ? "1" : "0");
}

}  // namespace

int main() {
    for (size_t i = 0; i < sizeof(kShapes) / sizeof(kShapes[0]); ++i)
        for (int d = 0; d < 6; ++d) {
            const Shape &u = kShapes[i];
            ConvMfmaArgs a;
            if (!describe(u, i == 0, d, 1, a)) continue;
            std::string cur;
            int from = 1;
            for (int F = 1; F <= 257; ++F) {
                std::string now;
                if (F <= 256) {
                    describe(u, i == 0, d, F, a);
                    now = probe(a);
                }
                if (F > 1 && now != cur) {
                    printf("%d->%d %dx%d s%d %s F=%d..%d %s\n", u.cin, u.depth, u.h, u.h, u.stride, kDesc[d], from, F - 1, cur.c_str());
                    from = F;
                }
                cur = now;
            }
        }
    return 0;
}
