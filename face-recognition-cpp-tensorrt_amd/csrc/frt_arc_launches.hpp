// The launches of one residual unit of the recogniser (model_irse.py:48-90), stated once: which packed weight copies a unit has, the
// ConvMfmaArgs description of each launch it can make, and the order and form in which one pass makes them.  Host only - no HIP call,
// every function inline - so frt_embedder::forward(), frt_embedder::warm_strip_tables() and the host programs under tests/cpp compile this
// very text: what the plan golden, the strip-table dump and the per-launch float64 checks describe is what the product launches.  The fp32
// mode's launches (frt_embedder::forward_f32) are described the same way at the end of this file.
#pragma once
#include "frt_kernels.h"

struct ArcUnit {
    int cin, depth, stride, h_in;  // input spatial size (square)
    half_t *w1 = nullptr, *w2 = nullptr, *wsc = nullptr;
    half_t *w1f = nullptr, *w2f = nullptr;  // fragment-ordered copies for the strip kernel (stride-1 3x3 convs)
    half_t *w2f2 = nullptr;                 // ... for the stride-2 strip kernel (conv2 of the first unit of a stage)
    half_t *wscf = nullptr;                 // 1x1 shortcut weights in fragment order (the stride-2 strip kernel computes the shortcut conv itself)
    float *prelu = nullptr, *s2 = nullptr, *b2 = nullptr, *ssc = nullptr, *bsc = nullptr;
    float *s2f32 = nullptr;              // closing BatchNorm's scale WITHOUT the load-time conditioning factor (the fp32 path multiplies the blob's own weights)
    float *sn = nullptr, *bn = nullptr;  // BatchNorm that consumes this unit's output (next unit's leading BN / output_layer.0)
    float *se_w1 = nullptr, *se_w2 = nullptr;
};

// The weight copies a unit of this shape has besides w1 / w2 (frt_embedder::build() packs exactly these): conv1 is always stride 1, conv2
// is stride 1 or 2 and has the copy of the strip kernel that runs it, and only a unit that changes the width has a shortcut conv.
struct ArcUnitCopies {
    bool w1f, w2f, w2f2;
    bool wsc;  // the 1x1 shortcut conv: wsc and wscf, with its BatchNorm ssc / bsc
};
inline ArcUnitCopies arc_unit_copies(int cin, int depth, int stride) { return {true, stride == 1, stride == 2, cin != depth}; }

// the buffers a unit's launches touch: an activation set at one parity (frt_embedder::unit_buffers)
struct ArcUnitBuffers {
    const half_t *z_in, *y_in;  // the unit's input: behind its leading BatchNorm, and raw (the shortcut's source)
    half_t *T, *SC, *RES;       // conv1's output; the 1x1 shortcut launch's; IR-SE: BN(conv2) in front of a stand-alone SE tail
    half_t *y_out, *z_out;      // the unit's output, raw and behind the next BatchNorm
    float *se_pool, *se_gate;   // IR-SE scratch (frt_embedder::ActSet) ...
    int *se_counter, se_flag_off, *se_error;  // ... the gate-ready flags' offset behind the counters, the fused tail's error word
    const half_t *zeros;
};

// ---- one description per launch a unit can make.  false: the unit has no such launch (`a` is then unspecified).
enum ArcDesc { ARC_CONV1, ARC_CONV2, ARC_CONV2_SCX, ARC_CONV2_SE, ARC_CONV2_RES, ARC_SHORTCUT1X1, ARC_NUM_DESC };

// conv1: BN(x) [already applied -> Z] -> conv3x3 s1 -> PReLU
inline bool arc_conv1(const ArcUnit &u, bool, const ArcUnitBuffers &b, int F, ConvMfmaArgs &a) {
    const int h = u.h_in;
    a = ConvMfmaArgs{};
    a.x = b.z_in; a.w = u.w1; a.wf = u.w1f;
    a.B = F; a.H = h; a.W = h; a.Cin = u.cin; a.Ho = h; a.Wo = h; a.Cout = u.depth; a.ks = 3; a.stride = 1; a.pad = 1;
    a.mode = EPI_PRELU;
    a.p0 = u.prelu;
    a.out0 = b.T;
    a.splits = 1; a.zeros = b.zeros;
    return true;
}

// conv1x1 stride s + BN on the raw input, as a launch of its own into SC
inline bool arc_shortcut1x1(const ArcUnit &u, bool, const ArcUnitBuffers &b, int F, ConvMfmaArgs &a) {
    if (!u.wsc) return false;
    const int h = u.h_in, ho = h / u.stride;
    a = ConvMfmaArgs{};
    a.x = b.y_in; a.w = u.wsc;
    a.B = F; a.H = h; a.W = h; a.Cin = u.cin; a.Ho = ho; a.Wo = ho; a.Cout = u.depth; a.ks = 1; a.stride = u.stride; a.pad = 0;
    a.mode = EPI_BN;
    a.p0 = u.ssc; a.p1 = u.bsc;
    a.out0 = b.SC;
    a.splits = 1; a.zeros = b.zeros;
    return true;
}

// conv2: conv3x3 stride s -> BN -> + shortcut; also emits BN_next(y).  Here with the identity shortcut every form below starts from.
inline void arc_conv2_identity(const ArcUnit &u, bool first_unit, const ArcUnitBuffers &b, int F, ConvMfmaArgs &a) {
    const int h = u.h_in, ho = h / u.stride;
    a = ConvMfmaArgs{};
    a.x = b.T; a.w = u.w2; a.wf = u.w2f; a.wf2 = u.w2f2;
    a.B = F; a.H = h; a.W = h; a.Cin = u.depth; a.Ho = ho; a.Wo = ho; a.Cout = u.depth; a.ks = 3; a.stride = u.stride; a.pad = 1;
    a.splits = 1; a.zeros = b.zeros;
    a.mode = EPI_BN_ADD_BN;
    a.p0 = u.s2; a.p1 = u.b2; a.p2 = u.sn; a.p3 = u.bn;
    a.sc = b.y_in;  // identity shortcut: MaxPool2d(1, stride) of the unit's input
    a.sc_h = h; a.sc_w = h; a.sc_stride = u.stride;
    if (first_unit) a.sc_h = ho, a.sc_w = ho, a.sc_stride = 1;  // the input layer already wrote its raw output at the even positions only
    a.out0 = b.y_out; a.out1 = b.z_out;
}

// conv2 as the plain unit tail: the shortcut is the unit's input, or the 1x1 launch's output where the unit has a shortcut conv
inline bool arc_conv2(const ArcUnit &u, bool first_unit, const ArcUnitBuffers &b, int F, ConvMfmaArgs &a) {
    arc_conv2_identity(u, first_unit, b, F, a);
    if (u.wsc) a.sc = b.SC, a.sc_h = a.sc_w = u.h_in / u.stride, a.sc_stride = 1;
    return true;
}

// IR-50: the stride-2 strip kernel (and the small-batch kernel) computes the 1x1 stride-2 shortcut conv itself (its input pixels are the
// (even, even) phase plane) - no launch, no shortcut tensor
inline bool arc_conv2_scx(const ArcUnit &u, bool first_unit, const ArcUnitBuffers &b, int F, ConvMfmaArgs &a) {
    if (!(u.wsc && u.wscf && u.stride == 2)) return false;
    arc_conv2_identity(u, first_unit, b, F, a);
    a.sc = nullptr;
    a.scx = b.y_in; a.wscf = u.wscf; a.psc0 = u.ssc; a.psc1 = u.bsc; a.Csc = u.cin;
    return true;
}

// IR-SE: the plain tail with the SE scratch - what is planned; launched only as its twin with the SE tail in the epilogue (arc_unit_schedule)
inline bool arc_conv2_se(const ArcUnit &u, bool first_unit, const ArcUnitBuffers &b, int F, ConvMfmaArgs &a) {
    if (!u.se_w1) return false;
    arc_conv2(u, first_unit, b, F, a);
    a.se_pool = b.se_pool; a.se_w1 = u.se_w1; a.se_w2 = u.se_w2;
    a.se_counter = b.se_counter; a.se_flag_off = b.se_flag_off; a.se_error = b.se_error;
    return true;
}

// IR-SE: conv2 + BN into RES, the SE tail as launches of its own behind it
inline bool arc_conv2_res(const ArcUnit &u, bool first_unit, const ArcUnitBuffers &b, int F, ConvMfmaArgs &a) {
    if (!arc_conv2_se(u, first_unit, b, F, a)) return false;
    a.mode = EPI_BN;
    a.out0 = b.RES; a.out1 = nullptr; a.sc = nullptr;
    return true;
}

typedef bool (*ArcDescribeFn)(const ArcUnit &, bool first_unit, const ArcUnitBuffers &, int F, ConvMfmaArgs &);
constexpr ArcDescribeFn kArcDescribe[ARC_NUM_DESC] = {arc_conv1, arc_conv2, arc_conv2_scx, arc_conv2_se, arc_conv2_res, arc_shortcut1x1};

// ---- what one unit launches in a pass of F faces, in order
struct ArcLaunch {
    ConvMfmaArgs args;
    ConvPlan plan;
    int desc;             // ArcDesc
    const char *planned;  // the label conv_plan gave; plan.label is another only where the SE tail was taken
    double flops;         // the figure the launch's profiling bracket gets
};
struct ArcUnitSchedule {
    int n = 0;
    ArcLaunch conv[3];
    bool se_fused = false;  // the last conv runs the SE tail in its epilogue (mode EPI_BN_SE): the launcher gives it its se_epoch
    bool se_tail = false;   // `se` runs behind the last conv
    SeArgs se;
    void add(int desc, const ConvMfmaArgs &a, const ConvPlan &p, double flops) { conv[n++] = ArcLaunch{a, p, desc, p.label, flops}; }
};

// se: the network has SE (the gate multiplies the residual branch only, so IR-SE keeps the shortcut tensor).  fuse: the SE tail may run in
// conv2's epilogue (frt_embedder_set_se_fused and the per-device occupancy gate conv_se_fits_device, which stays outside the plan).
inline ArcUnitSchedule arc_unit_schedule(const ArcUnit &u, bool first_unit, const ArcUnitBuffers &b, int F, bool se, bool fuse) {
    ArcUnitSchedule s;
    const int h = u.h_in, ho = h / u.stride;
    ConvMfmaArgs a;
    arc_conv1(u, first_unit, b, F, a);
    s.add(ARC_CONV1, a, conv_plan(a), 2.0 * 9 * u.cin * u.depth * (double)F * h * h);
    const double flops2 = 2.0 * 9 * u.depth * u.depth;
    if (!se && arc_conv2_scx(u, first_unit, b, F, a)) {
        const ConvPlan plan = conv_plan(a);
        if (plan.uses_scx) {
            s.add(ARC_CONV2_SCX, a, plan, (flops2 + 2.0 * u.cin * u.depth) * (double)F * ho * ho);
            return s;
        }
    }
    if (arc_shortcut1x1(u, first_unit, b, F, a)) s.add(ARC_SHORTCUT1X1, a, conv_plan(a), 2.0 * u.cin * u.depth * (double)F * ho * ho);
    if (!se) {
        arc_conv2(u, first_unit, b, F, a);
        s.add(ARC_CONV2, a, conv_plan(a), flops2 * (double)F * ho * ho);
        return s;
    }
    arc_conv2_se(u, first_unit, b, F, a);
    ConvPlan plan = conv_plan(a);
    if (fuse && plan.se_fused()) {  // the strip kernel runs the whole tail in its epilogue
        // The plan made for the EPI_BN_ADD_BN description IS the plan of this launch: the arguments are not planned again under the new mode
        // (no planner has to treat the two modes alike) - the plan only moves to its twin instantiation, same geometry.
        s.add(ARC_CONV2_SE, a, plan, flops2 * (double)F * ho * ho);
        ArcLaunch &l = s.conv[s.n - 1];
        l.args.mode = EPI_BN_SE;
        l.plan.take_se_tail();
        s.se_fused = true;
        return s;
    }
    // another description - conv2 + BN into RES - and so another plan
    s.se = SeArgs{b.RES, u.se_w1, u.se_w2, a.sc, a.sc_h, a.sc_w, a.sc_stride, u.sn, u.bn, a.out0, a.out1, b.se_pool, b.se_gate, F, ho, ho, u.depth, b.se_counter};
    s.se_tail = true;
    arc_conv2_res(u, first_unit, b, F, a);
    s.add(ARC_CONV2_RES, a, conv_plan(a), flops2 * (double)F * ho * ho);
    return s;
}

// ---- the fp32 mode (frt_embedder_set_precision(e, 1); kernels_arc_f32.hip).  One unit makes conv1, the 1x1 shortcut where it has one, and
// conv2 - plain, or (IR-SE) into RES with launch_se32 behind it.  frt_embedder::forward_f32() and tests/cpp/arc32_launch_check.cpp compile
// this text.  The per-channel parameters are the ArcUnit's fp32 arrays; the weights are this mode's own packed copies.
struct Arc32Weights {
    float *w1 = nullptr, *w2 = nullptr, *wsc = nullptr;  // [Cout][tap][Cin] fp32 in conv32_kernel's fragment order (frt::conv32_w_frag)
};
// the activation buffers of the mode, in floats, for passes of up to `chunk` faces (frt_embedder::build_f32)
struct Arc32BufferSizes {
    size_t act, sc, res, gate, fc_out;  // A[0] / A[1] / T; the 1x1 shortcut launch's output; RES; the SE gates; the Linear's sums
};
inline Arc32BufferSizes arc32_buffer_sizes(int chunk) {
    const size_t C = (size_t)chunk;
    return {C * 112 * 112 * 64, C * 56 * 56 * 128, C * 56 * 56 * 64, C * 512, C * 512};
}
struct Arc32Buffers {
    const float *x;                // the unit's raw input (its leading BatchNorm is applied by conv1 on load)
    const float *lead_s, *lead_b;  // that BatchNorm
    float *T, *SC, *RES, *gate;    // conv1's output; the 1x1 shortcut launch's; IR-SE: BN(conv2); the SE gates [F][C]
    float *y;                      // the unit's output
};
enum Arc32Desc { ARC32_CONV1, ARC32_SHORTCUT1X1, ARC32_CONV2, ARC32_CONV2_RES, ARC32_NUM_DESC };

// conv1: BN(x) (on load; the zero padding pads the normalised tensor) -> conv3x3 s1 -> PReLU
inline bool arc32_conv1(const ArcUnit &u, const Arc32Weights &w, const Arc32Buffers &b, int F, Conv32Args &a) {
    const int h = u.h_in;
    a = Conv32Args{b.x, w.w1, b.lead_s, b.lead_b, b.T, F, h, h, u.cin, h, h, u.depth, 3, 1, 1, 0, u.prelu, nullptr, nullptr, 0, 0, 0};
    return true;
}
// conv1x1 stride s + BN on the raw input, into SC
inline bool arc32_shortcut1x1(const ArcUnit &u, const Arc32Weights &w, const Arc32Buffers &b, int F, Conv32Args &a) {
    if (!w.wsc) return false;
    const int h = u.h_in, ho = h / u.stride;
    a = Conv32Args{b.x, w.wsc, nullptr, nullptr, b.SC, F, h, h, u.cin, ho, ho, u.depth, 1, u.stride, 0, 1, u.ssc, u.bsc, nullptr, 0, 0, 0};
    return true;
}
// the unit's shortcut tensor: MaxPool2d(1, stride) of the raw input, or the 1x1 launch's output
struct Arc32Shortcut {
    const float *sc;
    int sc_h, sc_stride;
};
inline Arc32Shortcut arc32_shortcut(const ArcUnit &u, const Arc32Weights &w, const Arc32Buffers &b) {
    if (w.wsc) return {b.SC, u.h_in / u.stride, 1};
    return {b.x, u.h_in, u.stride};
}
// conv2 as the plain unit tail: conv3x3 stride s -> BN -> + shortcut
inline bool arc32_conv2(const ArcUnit &u, const Arc32Weights &w, const Arc32Buffers &b, int F, Conv32Args &a) {
    const int h = u.h_in, ho = h / u.stride;
    const Arc32Shortcut sc = arc32_shortcut(u, w, b);
    a = Conv32Args{b.T, w.w2, nullptr, nullptr, b.y, F, h, h, u.depth, ho, ho, u.depth, 3, u.stride, 1, 2, u.s2f32, u.b2, sc.sc, sc.sc_h, sc.sc_h, sc.sc_stride};
    return true;
}
// IR-SE: conv2 + BN into RES, launch_se32 behind it
inline bool arc32_conv2_res(const ArcUnit &u, const Arc32Weights &w, const Arc32Buffers &b, int F, Conv32Args &a) {
    if (!u.se_w1) return false;
    const int h = u.h_in, ho = h / u.stride;
    a = Conv32Args{b.T, w.w2, nullptr, nullptr, b.RES, F, h, h, u.depth, ho, ho, u.depth, 3, u.stride, 1, 1, u.s2f32, u.b2, nullptr, 0, 0, 0};
    return true;
}
typedef bool (*Arc32DescribeFn)(const ArcUnit &, const Arc32Weights &, const Arc32Buffers &, int F, Conv32Args &);
constexpr Arc32DescribeFn kArc32Describe[ARC32_NUM_DESC] = {arc32_conv1, arc32_shortcut1x1, arc32_conv2, arc32_conv2_res};

// the arguments of launch_se32, in its order: y = RES * gate + shortcut
struct Se32Args {
    const float *res, *w1, *w2;
    float *gate;
    const float *sc;
    float *out;
    int F, Ho, Wo, C, sc_h, sc_w, sc_stride;
};
inline Se32Args arc32_se(const ArcUnit &u, const Arc32Weights &w, const Arc32Buffers &b, int F) {
    const int ho = u.h_in / u.stride;
    const Arc32Shortcut sc = arc32_shortcut(u, w, b);
    return {b.RES, u.se_w1, u.se_w2, b.gate, sc.sc, b.y, F, ho, ho, u.depth, sc.sc_h, sc.sc_h, sc.sc_stride};
}
inline void launch_se32(const Se32Args &a, hipStream_t s) { launch_se32(a.res, a.w1, a.w2, a.gate, a.sc, a.out, a.F, a.Ho, a.Wo, a.C, a.sc_h, a.sc_w, a.sc_stride, s); }
