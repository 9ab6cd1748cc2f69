// The recogniser's launch space as frt_embedder::forward() fills it: the eight unit shapes and, per unit, the launch descriptions it makes.
// Shared by conv_plan_dump.cpp (which enumerates the plans) and arc_launch_check.cpp (which runs the launches one at a time), so that the two
// cannot describe a launch differently.  Every pointer describe() sets is a non-null dummy: a program that launches replaces each of them.
#pragma once
#include <cstdint>

#include "frt_kernels.h"

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

// the launch description `d` of a unit of shape `u` for a pass of F faces, filled the way forward() fills it; false: the unit has no such launch
inline bool describe(const Shape &u, bool first_unit, int d, int F, ConvMfmaArgs &a) {
    const int h = u.h, ho = h / u.stride;
    const bool has_sc_conv = u.cin != u.depth;  // build(): wsc / wscf exist for these units only
    a = ConvMfmaArgs{};
    a.B = F;
    a.splits = 1;
    a.zeros = dummy<half_t>(0);
    if (d == 0) {
        a.x = dummy<half_t>(1);
        a.w = dummy<half_t>(2);
        a.wf = dummy<half_t>(3);  // conv1 is stride 1: always a fragment-ordered copy
        a.H = h; a.W = h; a.Cin = u.cin; a.Ho = h; a.Wo = h; a.Cout = u.depth; a.ks = 3; a.stride = 1; a.pad = 1;
        a.mode = EPI_PRELU;
        a.p0 = dummy<float>(4);
        a.out0 = dummy<half_t>(5);
        return true;
    }
    if (d == 5) {
        if (!has_sc_conv) return false;
        a.x = dummy<half_t>(1);
        a.w = dummy<half_t>(2);
        a.H = h; a.W = h; a.Cin = u.cin; a.Ho = ho; a.Wo = ho; a.Cout = u.depth; a.ks = 1; a.stride = u.stride; a.pad = 0;
        a.mode = EPI_BN;
        a.p0 = dummy<float>(4);
        a.p1 = dummy<float>(6);
        a.out0 = dummy<half_t>(5);
        return true;
    }
    a.x = dummy<half_t>(1);
    a.w = dummy<half_t>(2);
    (u.stride == 1 ? a.wf : a.wf2) = dummy<half_t>(3);  // build() packs one of the two
    a.H = h; a.W = h; a.Cin = u.depth; a.Ho = ho; a.Wo = ho; a.Cout = u.depth; a.ks = 3; a.stride = u.stride; a.pad = 1;
    a.p0 = dummy<float>(4);
    a.p1 = dummy<float>(6);
    a.p2 = dummy<float>(7);
    a.p3 = dummy<float>(8);
    a.mode = EPI_BN_ADD_BN;
    a.sc = dummy<half_t>(9);
    a.sc_h = h; a.sc_w = h; a.sc_stride = u.stride;
    if (first_unit) a.sc_h = ho, a.sc_w = ho, a.sc_stride = 1;
    a.out0 = dummy<half_t>(5);
    a.out1 = dummy<half_t>(10);
    if (d == 2) {
        if (!(has_sc_conv && u.stride == 2)) return false;
        a.sc = nullptr;
        a.scx = dummy<half_t>(9); a.wscf = dummy<half_t>(11); a.psc0 = dummy<float>(12); a.psc1 = dummy<float>(13); a.Csc = u.cin;
        return true;
    }
    if (has_sc_conv) a.sc_h = ho, a.sc_w = ho, a.sc_stride = 1;  // the 1x1 launch's output
    if (d == 3 || d == 4) {
        a.se_pool = dummy<float>(14);
        a.se_w1 = dummy<float>(15);
        a.se_w2 = dummy<float>(16);
        a.se_counter = dummy<int>(17);
        a.se_flag_off = 256;
        a.se_error = dummy<int>(18);
    }
    if (d == 4) {
        a.mode = EPI_BN;
        a.out0 = dummy<half_t>(19);
        a.out1 = nullptr;
        a.sc = nullptr;
    }
    return true;
}

}  // namespace arc_describe
