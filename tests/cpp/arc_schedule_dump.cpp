// Prints what one residual unit launches (arc_unit_schedule, csrc/frt_arc_launches.hpp - the function frt_embedder::forward() runs per unit)
// over the eight unit shapes x network with / without SE x SE tail allowed in conv2's epilogue or not x batches 1 .. 256.  Host only.
// Tab-separated lines:
//   sched <shape> <se> <fuse> <from> <to> <launch> ...   maximal batch ranges over which the launches are the same; a conv launch is
//                                                        "<description>;<planned label>;<SE tail taken 0/1>;<final label>", the stand-alone
//                                                        SE tail behind the convs is "launch_se"
//   twin <shape> <from> <to> <se_label>                  where conv_plan, asked directly about the conv2_se description, names an SE twin
//   geom H W compact linear nt R n_img nslot threads     every strip geometry a scheduled launch reads a table of
// tests/test_arc_schedule.py derives the expected lines from tests/golden/arc_conv_plan.txt and the schedule rule.
#include <array>
#include <cstdio>
#include <set>
#include <string>

#include "arc_conv_describe.hpp"

using namespace arc_describe;

namespace {

// prints `key <from> <to> <value>` for the maximal ranges of equal non-empty values
struct Ranges {
    std::string key, cur;
    int from = 1;
    void next(int F, const std::string &now) {
        if (F > 1 && now != cur) {
            if (!cur.empty()) printf("%s\t%d\t%d\t%s\n", key.c_str(), from, F - 1, cur.c_str());
            from = F;
        }
        cur = now;
    }
};

}  // namespace

int main() {
    std::set<std::array<int, 9>> geoms;
    for (int i = 0; i < kNumShapes; ++i) {
        const Shape &sh = kShapes[i];
        char shape[64];
        snprintf(shape, sizeof shape, "%d->%d %dx%d s%d", sh.cin, sh.depth, sh.h, sh.h, sh.stride);
        const ArcUnit u = unit_of(sh);
        for (int se = 0; se < 2; ++se)
            for (int fuse = 0; fuse < 2; ++fuse) {
                Ranges r{std::string("sched\t") + shape + "\t" + std::to_string(se) + "\t" + std::to_string(fuse)};
                for (int F = 1; F <= 257; ++F) {
                    std::string now;
                    if (F <= 256) {
                        const ArcUnitSchedule s = arc_unit_schedule(u, i == 0, buffers(), F, se != 0, fuse != 0);
                        for (int k = 0; k < s.n; ++k) {
                            const ArcLaunch &l = s.conv[k];
                            const bool tail = l.args.mode == EPI_BN_SE;
                            if (tail != (s.se_fused && k == s.n - 1)) return 1;
                            now += std::string(k ? "\t" : "") + kDesc[l.desc] + ";" + l.planned + ";" + (tail ? "1" : "0") + ";" + l.plan.label;
                            StripGeometry g;
                            if (conv_strip_geometry(l.args, l.plan, g)) geoms.insert({g.H, g.W, g.compact, g.linear, g.nt, g.R, g.n_img, g.nslot, g.threads});
                        }
                        if (s.se_tail) now += "\tlaunch_se";
                    }
                    r.next(F, now);
                }
            }
        Ranges t{std::string("twin\t") + shape};
        for (int F = 1; F <= 257; ++F) {
            ConvMfmaArgs a;
            std::string now;
            if (F <= 256 && describe(sh, i == 0, ARC_CONV2_SE, F, a)) {
                const ConvPlan p = conv_plan(a);
                if (p.se_fused()) now = p.se_label;
            }
            t.next(F, now);
        }
    }
    for (const auto &g : geoms) printf("geom %d %d %d %d %d %d %d %d %d\n", g[0], g[1], g[2], g[3], g[4], g[5], g[6], g[7], g[8]);
    return 0;
}
