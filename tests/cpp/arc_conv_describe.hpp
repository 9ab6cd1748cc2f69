// The recogniser's launch space: the eight unit shapes and, per unit, the launch descriptions it can make - described by the product's own
// functions (csrc/frt_arc_launches.hpp, the text frt_embedder::forward() compiles); no description rule lives here.  Shared by
// conv_plan_dump.cpp, strip_tables_dump.cpp, arc_schedule_dump.cpp (which enumerate) and arc_launch_check.cpp (which runs the launches one at a
// time).  Every pointer describe() sets is a non-null dummy: a program that launches replaces each of them.
#pragma once
#include <cstdint>

#include "frt_arc_launches.hpp"

namespace arc_describe {

struct Shape {
    int cin, depth, h, stride;
};
constexpr int kNumShapes = 8, kNumDesc = 6;
const Shape kShapes[kNumShapes] = {{64, 64, 112, 2}, {64, 64, 56, 1}, {64, 128, 56, 2}, {128, 128, 28, 1}, {128, 256, 28, 2}, {256, 256, 14, 1}, {256, 512, 14, 2}, {512, 512, 7, 1}};
const char *const kDesc[kNumDesc] = {"conv1", "conv2", "conv2_scx", "conv2_se", "conv2_res", "shortcut1x1"};

template <class T>
T *dummy(int k) {  // non-null, never dereferenced
    return reinterpret_cast<T *>((uintptr_t)0x10000 * (k + 1));
}

static_assert(kNumDesc == ARC_NUM_DESC, "kDesc names the product's descriptions, in their order");

// a unit of shape `s` with the weight copies build() gives such a unit (and SE weights: every shape can be asked for its IR-SE launches)
inline ArcUnit unit_of(const Shape &s) {
    ArcUnit u;
    u.cin = s.cin; u.depth = s.depth; u.stride = s.stride; u.h_in = s.h;
    const ArcUnitCopies c = arc_unit_copies(s.cin, s.depth, s.stride);
    u.w1 = dummy<half_t>(2); u.w2 = dummy<half_t>(3);
    if (c.w1f) u.w1f = dummy<half_t>(4);
    if (c.w2f) u.w2f = dummy<half_t>(5);
    if (c.w2f2) u.w2f2 = dummy<half_t>(6);
    if (c.wsc) u.wsc = dummy<half_t>(7), u.wscf = dummy<half_t>(8), u.ssc = dummy<float>(9), u.bsc = dummy<float>(10);
    u.prelu = dummy<float>(11); u.s2 = dummy<float>(12); u.b2 = dummy<float>(13); u.sn = dummy<float>(14); u.bn = dummy<float>(15);
    u.se_w1 = dummy<float>(16); u.se_w2 = dummy<float>(17);
    return u;
}
// an activation set of an embedder with max_batch 256
inline ArcUnitBuffers buffers() {
    return {dummy<half_t>(20), dummy<half_t>(21), dummy<half_t>(22), dummy<half_t>(23), dummy<half_t>(24), dummy<half_t>(25), dummy<half_t>(26),
            dummy<float>(27), dummy<float>(28), dummy<int>(29), 256, dummy<int>(30), dummy<half_t>(0)};
}

// the launch description `d` of a unit of shape `s` for a pass of F faces; false: the unit has no such launch
inline bool describe(const Shape &s, bool first_unit, int d, int F, ConvMfmaArgs &a) { return kArcDescribe[d](unit_of(s), first_unit, buffers(), F, a); }

}  // namespace arc_describe
