// Runs the recogniser's launches ONE AT A TIME, outside any network.  Convs: for each case of a list written by tests/arc_launch_ref.py it fills
// ConvMfmaArgs through the same describe() the plan golden is enumerated with (arc_conv_describe.hpp), packs the case's plain fp32 weights with
// the product's own packers (csrc/frt_arc_pack.hpp), calls conv_plan() and launch_conv_mfma() once and writes out0 / out1 and the planned label
// back.  tests/test_gpu_arc_launches.py compares them with a float64 restatement of the operation that only ever sees [Cout][Cin][3][3]
// weights.
//
//   arc_launch_check DIR          run every case of DIR/cases.txt on the current device; stops at the first HIP error (exit 1)
//   arc_launch_check --plan DIR   print "<id>\t<label>" per case (conv2_se: the twin that runs); no HIP call (runs on a machine without a device)
//
// DIR/cases.txt: one line per case.  "conv <id> <unit shape 0..7> <description 0..5> <F>" is a conv launch, with the little-endian arrays
//   <id>.x    fp16 [F][H][W][Cin]                   <id>.w    fp32 [Cout][Cin][ks][ks]
//   <id>.sc   fp16 shortcut tensor, or the raw unit input of the fused 1x1 shortcut conv (absent: the launch has none)
//   <id>.wsc  fp32 [Cout][Csc] (fused shortcut conv only)
//   <id>.p    fp32 [6][Cout]: p0 p1 p2 p3 psc0 psc1
// Written: <id>.out0 / <id>.out1 (fp16, the logical tensors) and one line "<id>\t<changed slack elements>\t<label>" in DIR/results.txt.
// Description 3 (conv2_se) is the IR-SE conv2 with the whole SE tail in its epilogue (run_conv_se below), with three more arrays
//   <id>.se   fp32 fc1 weights [Cout/16][Cout], then fc2 weights [Cout][Cout/16]
//   <id>.x0 / <id>.sc0   fp16, the tensors of the primer launch (the geometry of <id>.x / <id>.sc, other values)
// and the line "<id>\t<twin label>\t<conv_se_fits_device>\t<n_parts>\t<changed slack halves>\t<changed scratch words outside the partial sums,
// counters and flags>\t<partial sums not written>\t<counters not zero>\t<flags not at the epoch>\t<halves the third launch wrote differently>".
// "conv_plain <id> <unit shape> <description> <F>" launches the description AS IT IS PLANNED, with the files and the result line of "conv": the
// same for every description but conv2_se, whose se=0 plan lines are the plain tail (with the SE scratch) and have no twin to move to.
// The three small launches go through the same buffers and checks (label: the launcher's name):
//   "input <id> <F>"                   launch_arc_input: <id>.x fp32 [F][3][112][112], <id>.w fp32 [64][27], <id>.p fp32 [5][64] s0 b0 slope s1 b1
//                                      -> out0 = z [F][112][112][64], out1 = y [F][56][56][64] (the even positions)
//   "fc <id> <F>"                      launch_fc_slices + launch_fc_finalize: <id>.x fp16 [F][25088] (NHWC flatten), <id>.w fp32 [512][25088] (NCHW
//                                      flatten, as the blob has it), <id>.p fp32 [3][512] bias s b, <id>.valid int32 [F]
//                                      -> out0 = fp32 [F][512], out1 = the slice sums fp32 [49][F][512]
//   "se <id> <H> <C> <F> <sc_stride>"  launch_se: <id>.x fp16 res [F][H][H][C], <id>.sc fp16 [F][H*sc_stride][H*sc_stride][C], <id>.w fp32 w1 [C/16][C]
//                                      then w2 [C][C/16], <id>.p fp32 [2][C] s1 b1 -> out0 = y, out1 = z, <id>.gate fp32 [F][C]; arrival counters
//                                      that are not back at zero count as changed slack
//
// Buffers are sized the way frt_embedder::alloc_act_set sizes them for max_batch = F (the kernels were written against that sizing: compact
// strips compute pixel slots of images that do not exist), each with 1 MiB in front.  Inputs are filled with a large finite fp16 value outside
// the logical tensor - a kernel that accumulated slack into a stored value cannot pass the comparison - and outputs with a fixed bit pattern,
// which must still be there after the launch everywhere outside the logical tensor.
#define CHECK_PROGRAM "arc_launch_check"
#include "check_common.hpp"

#include "arc_conv_describe.hpp"
#include "frt_arc_pack.hpp"
#include "frt_kernels.h"

namespace {

using namespace arc_describe;
using namespace check;

constexpr size_t kMarginBytes = (size_t)1 << 20;  // in front of every activation buffer
constexpr uint16_t kInFill = 0x7800;              // 32768.0: large, finite
constexpr uint16_t kOutFill = 0x5a5a;
constexpr uint32_t kInFill32 = 0x7149f2ca;        // 1e30f
constexpr uint32_t kOutFill32 = 0x5a5a5a5a;

typedef MarginBuf<uint16_t> ActBuf;

// the device memory of one case: every buffer behind kMarginBytes, nothing behind it but the product's own slack
struct Dev : DeviceCase {
    explicit Dev(const std::string &id) : DeviceCase(id, kMarginBytes, 0, "elements") {}
    ActBuf act(size_t cap, size_t logical, uint16_t fill, const std::vector<uint16_t> *init) { return buf<uint16_t>(cap, logical, fill, init ? init->data() : nullptr); }
};

void run_conv(const std::string &dir, const Case &c, FILE *results) {
    const Shape &u = kShapes[c.shape];
    ConvMfmaArgs a;
    if (!describe(u, c.shape == 0, c.d, c.F, a)) die("case " + c.id + ": the unit has no such launch");
    const std::string pre = dir + "/" + c.id;
    Dev dc(c.id);
    const size_t F = (size_t)c.F, big = F * 112 * 112 * 64, sc_cap = F * 28 * 28 * 128;  // alloc_act_set: Y / Z / T, and SC
    const bool has_sc_conv = u.cin != u.depth;

    const size_t nx = F * a.H * a.W * a.Cin, nout = F * a.Ho * a.Wo * a.Cout, nw = (size_t)a.Cout * a.Cin * a.ks * a.ks;
    const std::vector<uint16_t> x = read_exact<uint16_t>(pre + ".x", nx);
    const std::vector<float> w = read_exact<float>(pre + ".w", nw);
    const std::vector<float> par = read_exact<float>(pre + ".p", (size_t)6 * a.Cout);
    a.x = dc.act(big, nx, kInFill, &x).ptr<half_t>();
    a.w = reinterpret_cast<half_t *>(dc.upload(frt::conv_w_f16(w.data(), a.Cout, a.Cin, a.ks)));
    if (a.wf) a.wf = reinterpret_cast<half_t *>(dc.upload(frt::conv_w_f16_frag(w.data(), a.Cout, a.Cin)));
    // build(): the 64 -> 64 stride-2 layer's kernel walks the taps in tap order
    if (a.wf2) a.wf2 = reinterpret_cast<half_t *>(dc.upload(frt::conv_w_f16_frag(w.data(), a.Cout, a.Cin, u.depth != 64)));
    float *dpar = dc.upload(par);
    if (a.p0) a.p0 = dpar;
    if (a.p1) a.p1 = dpar + a.Cout;
    if (a.p2) a.p2 = dpar + 2 * a.Cout;
    if (a.p3) a.p3 = dpar + 3 * a.Cout;
    if (a.sc) {  // the unit's input (Y), or the 1x1 launch's output (SC) in the units that have a shortcut conv
        const size_t nsc = F * a.sc_h * a.sc_w * a.Cout;
        const std::vector<uint16_t> sc = read_exact<uint16_t>(pre + ".sc", nsc);
        a.sc = dc.act(has_sc_conv ? sc_cap : big, nsc, kInFill, &sc).ptr<half_t>();
    }
    if (a.scx) {
        const size_t nsc = F * a.H * a.W * a.Csc;
        const std::vector<uint16_t> sc = read_exact<uint16_t>(pre + ".sc", nsc);
        const std::vector<float> wsc = read_exact<float>(pre + ".wsc", (size_t)a.Cout * a.Csc);
        a.scx = dc.act(big, nsc, kInFill, &sc).ptr<half_t>();
        a.wscf = reinterpret_cast<half_t *>(dc.upload(frt::conv1x1_w_f16_frag(wsc.data(), a.Cout, a.Csc)));
        a.psc0 = dpar + 4 * a.Cout;
        a.psc1 = dpar + 5 * a.Cout;
    }
    a.zeros = reinterpret_cast<half_t *>(dc.upload(std::vector<uint16_t>(256, 0)));
    if (a.se_pool) {  // conv2_res is described with the embedder's SE scratch: real memory, sized as alloc_act_set sizes it
        float *pool = dc.upload(std::vector<float>(F * 512 * 4 + 2 * F, 0.f));
        a.se_pool = pool;
        a.se_counter = reinterpret_cast<int *>(pool + F * 512 * 4);
        a.se_flag_off = c.F;
        a.se_w1 = dc.upload(std::vector<float>((size_t)a.Cout / 16 * a.Cout, 0.f));
        a.se_w2 = dc.upload(std::vector<float>((size_t)a.Cout * (a.Cout / 16), 0.f));
        a.se_error = dc.upload(std::vector<int>(1, 0));
    }
    ActBuf o0, o1;
    o0 = dc.act(c.d == 5 ? sc_cap : big, nout, kOutFill, nullptr);
    a.out0 = o0.ptr<half_t>();
    if (a.out1) {
        o1 = dc.act(big, nout, kOutFill, nullptr);
        a.out1 = o1.ptr<half_t>();
    }

    const ConvPlan plan = conv_plan(a);
    launch_conv_mfma(a, plan, nullptr);
    sync_and_check();
    size_t changed = dc.download(o0, pre + ".out0");
    if (o1.base) changed += dc.download(o1, pre + ".out1");
    fprintf(results, "%s\t%zu\t%s\n", c.id.c_str(), changed, plan.label);
}

// IR-SE conv2 with the SE tail in its epilogue (csrc/frt_se_device.h), launched the way arc_unit_schedule (csrc/frt_arc_launches.hpp) builds it:
// the arc_conv2_se description is planned, the plan must offer the tail, then the mode becomes EPI_BN_SE and the plan moves to its twin.  The SE
// scratch is the embedder's (alloc_act_set): [4][F][512] partial sums, F arrival counters, F gate-ready flags - here behind a margin and, but for
// the zeroed counters and flags, filled with a pattern.  Three launches on the same scratch and outputs, which is what consecutive units of
// a pass are: a primer with other tensors at epoch e (a workgroup of the next launch that accepted a stale flag, or read the partial sums before
// every part had arrived, would pool the primer's values or the pattern), the case at e + 1, and the case again at e + 2, which must write the
// same bits (the gate does not depend on arrival order).  A raised error word ends the process like a HIP error.
void run_conv_se(const std::string &dir, const Case &c, FILE *results) {
    constexpr int kEpoch = 7;
    const Shape &u = kShapes[c.shape];
    ConvMfmaArgs a;
    if (!describe(u, c.shape == 0, ARC_CONV2_SE, c.F, a)) die("case " + c.id + ": the unit has no such launch");
    const std::string pre = dir + "/" + c.id;
    Dev dc(c.id);
    const size_t F = (size_t)c.F, C = (size_t)a.Cout, big = F * 112 * 112 * 64, sc_cap = F * 28 * 28 * 128;  // alloc_act_set: Y / Z / T, and SC
    const size_t nx = F * a.H * a.W * a.Cin, nout = F * a.Ho * a.Wo * C, nsc = F * a.sc_h * a.sc_w * C;
    const std::vector<uint16_t> x = read_exact<uint16_t>(pre + ".x", nx), x0 = read_exact<uint16_t>(pre + ".x0", nx);
    const std::vector<uint16_t> sc = read_exact<uint16_t>(pre + ".sc", nsc), sc0 = read_exact<uint16_t>(pre + ".sc0", nsc);
    const std::vector<float> w = read_exact<float>(pre + ".w", C * a.Cin * 9), par = read_exact<float>(pre + ".p", 6 * C), se = read_exact<float>(pre + ".se", 2 * (C / 16) * C);
    const ActBuf dx = dc.act(big, nx, kInFill, &x0), dsc = dc.act(u.cin != u.depth ? sc_cap : big, nsc, kInFill, &sc0);
    a.x = dx.ptr<half_t>();
    a.sc = dsc.ptr<half_t>();
    a.w = reinterpret_cast<half_t *>(dc.upload(frt::conv_w_f16(w.data(), a.Cout, a.Cin, a.ks)));
    if (a.wf) a.wf = reinterpret_cast<half_t *>(dc.upload(frt::conv_w_f16_frag(w.data(), a.Cout, a.Cin)));
    if (a.wf2) a.wf2 = reinterpret_cast<half_t *>(dc.upload(frt::conv_w_f16_frag(w.data(), a.Cout, a.Cin, u.depth != 64)));
    float *dpar = dc.upload(par), *dse = dc.upload(se);
    a.p0 = dpar; a.p1 = dpar + C; a.p2 = dpar + 2 * C; a.p3 = dpar + 3 * C;
    a.se_w1 = dse;
    a.se_w2 = dse + (C / 16) * C;
    a.zeros = reinterpret_cast<half_t *>(dc.upload(std::vector<uint16_t>(256, 0)));
    const size_t pool_words = F * 512 * 4;
    const MarginBuf<uint32_t> scratch = dc.buf<uint32_t>(pool_words + 2 * F, pool_words + 2 * F, kOutFill32, nullptr);
    HIPCHK(hipMemset(scratch.ptr<uint32_t>() + pool_words, 0, 2 * F * sizeof(uint32_t)));
    a.se_pool = scratch.ptr<float>();
    a.se_counter = scratch.ptr<int>() + pool_words;
    a.se_flag_off = c.F;
    struct Mapped {  // the error word: mapped host memory, as frt_embedder::build() allocates it
        int *host = nullptr;
        ~Mapped() { (void)hipHostFree(host); }
    } err;
    HIPCHK(hipHostMalloc(reinterpret_cast<void **>(&err.host), sizeof(int), hipHostMallocMapped));
    *err.host = 0;
    HIPCHK(hipHostGetDevicePointer(reinterpret_cast<void **>(&a.se_error), err.host, 0));
    const ActBuf o0 = dc.act(big, nout, kOutFill, nullptr), o1 = dc.act(big, nout, kOutFill, nullptr);
    a.out0 = o0.ptr<half_t>();
    a.out1 = o1.ptr<half_t>();

    ConvPlan plan = conv_plan(a);
    if (!plan.se_fused()) die("case " + c.id + ": planned as " + plan.label + ", which has no twin with the SE tail");
    a.mode = EPI_BN_SE;
    plan.take_se_tail();
    const int n_parts = plan.n_img == 1 ? (a.Ho + plan.R - 1) / plan.R : 1;  // strips of one image: the parts its channel sums arrive in
    if (!conv_se_fits_device()) {  // the embedder would run the stand-alone tail here: nothing is launched, the test reports it
        fprintf(results, "%s\t%s\t0\t%d\t0\t0\t0\t0\t0\t0\n", c.id.c_str(), plan.label, n_parts);
        return;
    }
    size_t slack = 0, outside = 0, unwritten = 0, counters = 0, flags = 0;
    auto launch = [&](int epoch, const std::string &keep, std::vector<uint16_t> *y, std::vector<uint16_t> *z) {
        a.se_epoch = epoch;
        launch_conv_mfma(a, plan, nullptr);
        sync_and_check();
        if (*err.host) die("case " + c.id + ": a hand-over wait of the SE tail timed out (error word " + std::to_string(*err.host) + ", epoch " + std::to_string(epoch) + ")");
        if (y) slack += dc.download(o0, keep.empty() ? keep : keep + ".out0", y) + dc.download(o1, keep.empty() ? keep : keep + ".out1", z);
        const std::vector<uint32_t> h = dc.fetch(scratch);
        const uint32_t *s = h.data() + scratch.front;
        const size_t live = n_parts * F * C;  // se_pool[part][face][channel]: every word written, none behind them
        outside += changed_outside(h.data(), scratch.front + pool_words, scratch.front, live, kOutFill32);
        for (size_t i = 0; i < live; ++i) unwritten += s[i] == kOutFill32;
        for (size_t f = 0; f < F; ++f) counters += s[pool_words + f] != 0, flags += s[pool_words + F + f] != (uint32_t)epoch;
    };
    launch(kEpoch, "", nullptr, nullptr);
    HIPCHK(hipMemcpy(dx.ptr<void>(), x.data(), nx * 2, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dsc.ptr<void>(), sc.data(), nsc * 2, hipMemcpyHostToDevice));
    dc.refill(o0);
    dc.refill(o1);
    std::vector<uint16_t> y2, z2, y3, z3;
    launch(kEpoch + 1, pre, &y2, &z2);
    dc.refill(o0);
    dc.refill(o1);
    launch(kEpoch + 2, "", &y3, &z3);
    size_t repeat = 0;
    for (size_t i = 0; i < nout; ++i) repeat += (y2[i] != y3[i]) + (z2[i] != z3[i]);
    fprintf(results, "%s\t%s\t1\t%d\t%zu\t%zu\t%zu\t%zu\t%zu\t%zu\n", c.id.c_str(), plan.label, n_parts, slack, outside, unwritten, counters, flags, repeat);
}

void run_input(const std::string &dir, const Case &c, FILE *results) {
    const std::string pre = dir + "/" + c.id;
    Dev dc(c.id);
    const size_t F = (size_t)c.F, big = F * 112 * 112 * 64;
    const std::vector<float> x = read_exact<float>(pre + ".x", F * 3 * 112 * 112), w = read_exact<float>(pre + ".w", 64 * 27), par = read_exact<float>(pre + ".p", 5 * 64);
    std::vector<float> wt(27 * 64);  // build(): [27][64] for the scalar kernel
    for (int co = 0; co < 64; ++co)
        for (int k = 0; k < 27; ++k) wt[k * 64 + co] = w[co * 27 + k];
    const MarginBuf<uint32_t> dx = dc.buf<uint32_t>(x.size(), x.size(), kInFill32, x.data());  // d_in has no slack
    float *dpar = dc.upload(par);
    const ActBuf z = dc.act(big, big, kOutFill, nullptr), y = dc.act(big, big / 4, kOutFill, nullptr);  // Z[0], Y[0]
    ArcInputArgs a{dx.ptr<float>(), dc.upload(wt), dpar, dpar + 64, dpar + 128, dpar + 192, dpar + 256, y.ptr<half_t>(), z.ptr<half_t>(), c.F, 112, 112,
                   reinterpret_cast<half_t *>(dc.upload(frt::arc_input_w_f16(w.data(), par.data(), par.data() + 64)))};
    launch_arc_input(a, nullptr);
    sync_and_check();
    const size_t changed = dc.download(z, pre + ".out0") + dc.download(y, pre + ".out1");
    fprintf(results, "%s\t%zu\tlaunch_arc_input\n", c.id.c_str(), changed);
}

void run_fc(const std::string &dir, const Case &c, FILE *results) {
    const std::string pre = dir + "/" + c.id;
    Dev dc(c.id);
    const size_t F = (size_t)c.F;
    const std::vector<uint16_t> zin = read_exact<uint16_t>(pre + ".x", F * 25088);
    const std::vector<float> w = read_exact<float>(pre + ".w", (size_t)512 * 25088), par = read_exact<float>(pre + ".p", 3 * 512);
    const std::vector<int> valid = read_exact<int>(pre + ".valid", F);
    const ActBuf z = dc.act(F * 112 * 112 * 64, zin.size(), kInFill, &zin);
    const MarginBuf<uint32_t> partial = dc.buf<uint32_t>(49 * F * 512, 49 * F * 512, kOutFill32, nullptr), out = dc.buf<uint32_t>(F * 512, F * 512, kOutFill32, nullptr);
    float *dpar = dc.upload(par);
    launch_fc_slices(z.ptr<half_t>(), reinterpret_cast<half_t *>(dc.upload(frt::fc_w_f16_frag(w.data()))), c.F, partial.ptr<float>(), nullptr);
    launch_fc_finalize(partial.ptr<float>(), 49, c.F, dpar, dpar + 512, dpar + 1024, dc.upload(valid), out.ptr<float>(), nullptr);
    sync_and_check();
    const size_t changed = dc.download(out, pre + ".out0") + dc.download(partial, pre + ".out1");
    fprintf(results, "%s\t%zu\tlaunch_fc\n", c.id.c_str(), changed);
}

void run_se(const std::string &dir, const Case &c, FILE *results) {
    const std::string pre = dir + "/" + c.id;
    Dev dc(c.id);
    const size_t F = (size_t)c.F, C = c.C, n = F * c.H * c.H * C, big = F * 112 * 112 * 64, sh = (size_t)c.H * c.sc_stride;
    const std::vector<uint16_t> res = read_exact<uint16_t>(pre + ".x", n), sc = read_exact<uint16_t>(pre + ".sc", F * sh * sh * C);
    const std::vector<float> w = read_exact<float>(pre + ".w", 2 * (C / 16) * C), par = read_exact<float>(pre + ".p", 2 * C);
    // alloc_act_set: RES, Y (the shortcut), Y / Z of the other parity, se_pool with the arrival counters and flags behind it, se_gate
    const ActBuf dres = dc.act(F * 56 * 56 * 64, n, kInFill, &res), dsc = dc.act(big, sc.size(), kInFill, &sc);
    const ActBuf y = dc.act(big, n, kOutFill, nullptr), z = dc.act(big, n, kOutFill, nullptr);
    const MarginBuf<uint32_t> gate = dc.buf<uint32_t>(F * 512, F * C, kOutFill32, nullptr);
    float *pool = dc.upload(std::vector<float>(F * 512 * 4 + 2 * F, 0.f));
    int *counter = reinterpret_cast<int *>(pool + F * 512 * 4);
    float *dw = dc.upload(w), *dpar = dc.upload(par);
    SeArgs a{dres.ptr<half_t>(), dw, dw + (C / 16) * C, dsc.ptr<half_t>(), (int)sh, (int)sh, c.sc_stride, dpar, dpar + C, y.ptr<half_t>(), z.ptr<half_t>(), pool, gate.ptr<float>(),
             c.F, c.H, c.H, c.C, counter};
    launch_se(a, nullptr);
    sync_and_check();
    size_t changed = dc.download(y, pre + ".out0") + dc.download(z, pre + ".out1") + dc.download(gate, pre + ".gate");
    std::vector<int> cnt(2 * F);
    HIPCHK(hipMemcpy(cnt.data(), counter, cnt.size() * sizeof(int), hipMemcpyDeviceToHost));
    for (int v : cnt) changed += v != 0;  // the next launch on this scratch counts from zero
    fprintf(results, "%s\t%zu\tlaunch_se\n", c.id.c_str(), changed);
}

void run_case(const std::string &dir, const Case &c, FILE *results) {
    if ((c.kind == "conv" && c.d != ARC_CONV2_SE) || c.kind == "conv_plain") run_conv(dir, c, results);
    if (c.kind == "conv" && c.d == ARC_CONV2_SE) run_conv_se(dir, c, results);
    if (c.kind == "input") run_input(dir, c, results);
    if (c.kind == "fc") run_fc(dir, c, results);
    if (c.kind == "se") run_se(dir, c, results);
    fflush(results);
}

}  // namespace

int main(int argc, char **argv) {
    const bool plan_only = argc == 3 && std::string(argv[1]) == "--plan";
    if (argc != 2 && !plan_only) die("usage: arc_launch_check [--plan] DIR");
    const std::string dir = argv[argc - 1];
    const std::vector<Case> cases = read_cases(dir, kNumShapes, kNumDesc, 256);
    if (plan_only) {
        for (const Case &c : cases) {
            ConvMfmaArgs a;
            if (c.kind != "conv" && c.kind != "conv_plain") continue;  // only the convs are planned
            if (!describe(kShapes[c.shape], c.shape == 0, c.d, c.F, a)) die("case " + c.id + ": the unit has no such launch");
            const ConvPlan p = conv_plan(a);
            const bool twin = c.kind == "conv" && c.d == ARC_CONV2_SE;
            if (twin && !p.se_fused()) die("case " + c.id + ": planned as " + p.label + ", which has no twin with the SE tail");
            printf("%s\t%s\n", c.id.c_str(), twin ? p.se_label : p.label);  // the fused launch runs the twin
        }
        return 0;
    }
    FILE *results = fopen((dir + "/results.txt").c_str(), "w");
    if (!results) die("cannot write " + dir + "/results.txt");
    for (const Case &c : cases) run_case(dir, c, results);
    fclose(results);
    return 0;
}
