// Runs the launches of the recogniser's fp32 mode (frt_embedder::forward_f32, csrc/kernels_arc_f32.hip) ONE AT A TIME, outside any network: the
// sibling of arc_launch_check.cpp for the path the others are judged against.  Convs: for each case of a list written by tests/arc_launch_ref.py
// it fills Conv32Args through the descriptions forward_f32 itself compiles (csrc/frt_arc_launches.hpp: arc32_conv1, arc32_shortcut1x1,
// arc32_conv2, arc32_conv2_res), packs the case's plain weights with the product's packer (frt::conv32_w_frag -> pack_conv32_weights), calls
// launch_conv32 once and writes the output back.  tests/test_gpu_arc32_launches.py compares it with a float64 restatement of the operation that
// only ever sees [Cout][Cin][ks][ks] weights and [F][H][W][C] tensors.
//
//   arc32_launch_check DIR            run every case of DIR/cases.txt on the current device; stops at the first HIP error (exit 1)
//   arc32_launch_check --describe DIR print "<id>\t<the Conv32Args' integers>" per conv case; no HIP call (runs on a machine without a device)
//
// DIR/cases.txt, one line per case; all arrays little-endian fp32 unless said otherwise:
//   "conv <id> <unit shape 0..7> <description 0..3> <F>"   <id>.x [F][H][W][Cin], <id>.w [Cout][Cin][ks][ks], <id>.p [2][Cout] p0 p1,
//                                      <id>.pro [2][Cin] the leading BatchNorm (conv1 only), <id>.sc the shortcut tensor (conv2 only) -> <id>.out0
//   "input <id> <F>"                   launch_arc32_input: <id>.x [F][3][112][112], <id>.w [64][27], <id>.p [3][64] s0 b0 slope -> out0 [F][112][112][64]
//   "fc <id> <F>"                      launch_fc32 + launch_fc_finalize(splits = 1): <id>.x [F][25088] (NHWC flatten), <id>.w [512][25088] (NCHW
//                                      flatten, as the blob has it), <id>.pro [2][512] the BatchNorm applied on load, <id>.p [3][512] bias s b,
//                                      <id>.valid int32 [F] -> out0 = the embeddings [F][512], out1 = the Linear's sums [F][512]
//   "se <id> <H> <C> <F> <sc_stride>"  launch_se32: <id>.x res [F][H][H][C], <id>.sc [F][H*sc_stride][H*sc_stride][C], <id>.w w1 [C/16][C] then
//                                      w2 [C][C/16] -> out0 [F][H][H][C], <id>.gate [F][C]
// One line "<id>\t<floats outside the logical outputs that changed>\t<description / launcher>" per case goes to DIR/results.txt.
//
// Every buffer has the size frt_embedder::build_f32 gives it for passes of F faces (arc32_buffer_sizes), between two margins of 1 MiB.  Input
// buffers are NaN everywhere outside the logical tensor, margins included: a read at a wrong but nearby address shows as a NaN in the output
// instead of passing as a zero (the margins are longer than (W + 1) * Cin floats for every shape).  Output buffers hold a fixed bit pattern,
// which must still be there after the launch everywhere outside the logical tensor, in front and behind.
#define CHECK_PROGRAM "arc32_launch_check"
#include "check_common.hpp"

#include "arc_conv_describe.hpp"
#include "frt_arc_pack.hpp"
#include "frt_kernels.h"

namespace {

using namespace arc_describe;
using namespace check;

constexpr size_t kMargin = ((size_t)1 << 20) / sizeof(float);  // floats in front of and behind every activation buffer
constexpr uint32_t kNaN = 0x7fc00000u, kOutFill = 0x5a5a5a5au;
const char *const kDesc32[ARC32_NUM_DESC] = {"conv1", "shortcut1x1", "conv2", "conv2_res"};

typedef MarginBuf<uint32_t> Buf;

// the device memory of one case: `cap` floats between two margins, all filled; the first `logical` floats behind the front margin are the tensor
struct Dev : DeviceCase {
    explicit Dev(const std::string &id) : DeviceCase(id, kMargin * sizeof(float), kMargin * sizeof(float), "floats") {}
    Buf in(size_t cap, const std::vector<float> &v) { return buf<uint32_t>(cap, v.size(), kNaN, v.data()); }
    Buf out(size_t cap, size_t logical) { return buf<uint32_t>(cap, logical, kOutFill, nullptr); }
};

// the description `d` of a unit of shape `s` as forward_f32 builds it, every pointer a dummy that names its buffer
struct Described {
    ArcUnit u;
    Arc32Weights w;
    Arc32Buffers b;
    Conv32Args a;
};
bool describe32(const Shape &s, int d, int F, Described &o) {
    o.u = unit_of(s);
    o.u.s2f32 = dummy<float>(18);
    o.w.w1 = dummy<float>(40);
    o.w.w2 = dummy<float>(41);
    o.w.wsc = arc_unit_copies(s.cin, s.depth, s.stride).wsc ? dummy<float>(42) : nullptr;
    o.b = Arc32Buffers{dummy<float>(50), dummy<float>(51), dummy<float>(52), dummy<float>(53), dummy<float>(54), dummy<float>(55), dummy<float>(56), dummy<float>(57)};
    return kArc32Describe[d](o.u, o.w, o.b, F, o.a);
}

void run_conv(const std::string &dir, const Case &c, FILE *results) {
    Described ds;
    if (!describe32(kShapes[c.shape], c.d, c.F, ds)) die("case " + c.id + ": the unit has no such launch");
    Conv32Args a = ds.a;
    const Arc32Buffers &b = ds.b;
    const Arc32BufferSizes sz = arc32_buffer_sizes(c.F);
    const std::string pre = dir + "/" + c.id;
    Dev dc(c.id);
    // the capacity of the buffer a described pointer names
    auto cap_of = [&](const float *p) -> size_t {
        if (p == b.x || p == b.T || p == b.y) return sz.act;
        if (p == b.SC) return sz.sc;
        if (p == b.RES) return sz.res;
        die("case " + c.id + ": the description names a buffer the harness does not know");
    };
    const size_t F = (size_t)c.F, nx = F * a.H * a.W * a.Cin, nout = F * a.Ho * a.Wo * a.Cout;
    if (kMargin < (size_t)(a.W + 1) * a.Cin) die("case " + c.id + ": the margins are shorter than a row of the input");
    const std::vector<float> x = read_exact<float>(pre + ".x", nx), w = read_exact<float>(pre + ".w", (size_t)a.Cout * a.Cin * a.ks * a.ks);
    const std::vector<float> par = read_exact<float>(pre + ".p", (size_t)2 * a.Cout);
    a.x = dc.in(cap_of(ds.a.x), x).ptr<float>();
    a.w = dc.upload(frt::conv32_w_frag(w.data(), a.Cout, a.Cin, a.ks));
    if (a.ps) {
        float *pro = dc.upload(read_exact<float>(pre + ".pro", (size_t)2 * a.Cin));
        a.ps = pro;
        a.pb = pro + a.Cin;
    }
    float *dpar = dc.upload(par);
    a.p0 = dpar;
    if (a.p1) a.p1 = dpar + a.Cout;
    if (a.sc) a.sc = dc.in(cap_of(ds.a.sc), read_exact<float>(pre + ".sc", F * a.sc_h * a.sc_w * a.Cout)).ptr<float>();
    const Buf o = dc.out(cap_of(ds.a.out), nout);
    a.out = o.ptr<float>();
    launch_conv32(a, nullptr);
    sync_and_check();
    fprintf(results, "%s\t%zu\t%s\n", c.id.c_str(), dc.download(o, pre + ".out0"), kDesc32[c.d]);
}

void run_input(const std::string &dir, const Case &c, FILE *results) {
    const std::string pre = dir + "/" + c.id;
    Dev dc(c.id);
    const size_t F = (size_t)c.F;
    const std::vector<float> x = read_exact<float>(pre + ".x", F * 3 * 112 * 112), w = read_exact<float>(pre + ".w", 64 * 27), par = read_exact<float>(pre + ".p", 3 * 64);
    std::vector<float> wt(27 * 64);  // build(): [27][64]
    for (int co = 0; co < 64; ++co)
        for (int k = 0; k < 27; ++k) wt[k * 64 + co] = w[co * 27 + k];
    const Buf dx = dc.in(x.size(), x);  // d_in has no slack
    float *dpar = dc.upload(par);
    const Buf y = dc.out(arc32_buffer_sizes(c.F).act, F * 112 * 112 * 64);
    launch_arc32_input(dx.ptr<float>(), dc.upload(wt), dpar, dpar + 64, dpar + 128, y.ptr<float>(), c.F, nullptr);
    sync_and_check();
    fprintf(results, "%s\t%zu\tlaunch_arc32_input\n", c.id.c_str(), dc.download(y, pre + ".out0"));
}

void run_fc(const std::string &dir, const Case &c, FILE *results) {
    const std::string pre = dir + "/" + c.id;
    Dev dc(c.id);
    const size_t F = (size_t)c.F;
    const Arc32BufferSizes sz = arc32_buffer_sizes(c.F);
    const std::vector<float> yin = read_exact<float>(pre + ".x", F * 25088), w = read_exact<float>(pre + ".w", (size_t)512 * 25088);
    const std::vector<float> pro = read_exact<float>(pre + ".pro", 2 * 512), par = read_exact<float>(pre + ".p", 3 * 512);
    const std::vector<int> valid = read_exact<int>(pre + ".valid", F);
    const Buf y = dc.in(sz.act, yin), sums = dc.out(sz.fc_out, F * 512), out = dc.out(F * 512, F * 512);
    float *dpro = dc.upload(pro), *dpar = dc.upload(par);
    launch_fc32(y.ptr<float>(), dpro, dpro + 512, dc.upload(frt::fc32_w_nhwc(w.data())), sums.ptr<float>(), c.F, nullptr);
    launch_fc_finalize(sums.ptr<float>(), 1, c.F, dpar, dpar + 512, dpar + 1024, dc.upload(valid), out.ptr<float>(), nullptr);
    sync_and_check();
    const size_t changed = dc.download(out, pre + ".out0") + dc.download(sums, pre + ".out1");
    fprintf(results, "%s\t%zu\tlaunch_fc32\n", c.id.c_str(), changed);
}

void run_se(const std::string &dir, const Case &c, FILE *results) {
    const std::string pre = dir + "/" + c.id;
    Dev dc(c.id);
    const size_t F = (size_t)c.F, C = c.C, n = F * c.H * c.H * C, sh = (size_t)c.H * c.sc_stride;
    const Arc32BufferSizes sz = arc32_buffer_sizes(c.F);
    const std::vector<float> res = read_exact<float>(pre + ".x", n), sc = read_exact<float>(pre + ".sc", F * sh * sh * C), w = read_exact<float>(pre + ".w", 2 * (C / 16) * C);
    const Buf dres = dc.in(sz.res, res), dsc = dc.in(sz.act, sc), y = dc.out(sz.act, n), gate = dc.out(sz.gate, F * C);
    float *dw = dc.upload(w);
    const Se32Args a{dres.ptr<float>(), dw, dw + (C / 16) * C, gate.ptr<float>(), dsc.ptr<float>(), y.ptr<float>(), c.F, c.H, c.H, c.C, (int)sh, (int)sh, c.sc_stride};
    launch_se32(a, nullptr);
    sync_and_check();
    const size_t changed = dc.download(y, pre + ".out0") + dc.download(gate, pre + ".gate");
    fprintf(results, "%s\t%zu\tlaunch_se32\n", c.id.c_str(), changed);
}

}  // namespace

int main(int argc, char **argv) {
    const bool describe_only = argc == 3 && std::string(argv[1]) == "--describe";
    if (argc != 2 && !describe_only) die("usage: arc32_launch_check [--describe] DIR");
    const std::string dir = argv[argc - 1];
    const std::vector<Case> cases = read_cases(dir, kNumShapes, ARC32_NUM_DESC, 8);  // 8: the mode's chunk
    if (describe_only) {
        for (const Case &c : cases) {
            if (c.kind != "conv") continue;
            Described ds;
            if (!describe32(kShapes[c.shape], c.d, c.F, ds)) die("case " + c.id + ": the unit has no such launch");
            const Conv32Args &a = ds.a;
            const char *sc = !a.sc ? "none" : a.sc == ds.b.x ? "x" : a.sc == ds.b.SC ? "SC" : "?";
            printf("%s\t%s F=%d H=%d Cin=%d Ho=%d Cout=%d ks=%d stride=%d pad=%d mode=%d pro=%d sc=%s sc_h=%d sc_stride=%d\n", c.id.c_str(), kDesc32[c.d], a.F, a.H, a.Cin,
                   a.Ho, a.Cout, a.ks, a.stride, a.pad, a.mode, a.ps != nullptr, sc, a.sc_h, a.sc_stride);
        }
        return 0;
    }
    FILE *results = fopen((dir + "/results.txt").c_str(), "w");
    if (!results) die("cannot write " + dir + "/results.txt");
    for (const Case &c : cases) {
        if (c.kind == "conv") run_conv(dir, c, results);
        if (c.kind == "input") run_input(dir, c, results);
        if (c.kind == "fc") run_fc(dir, c, results);
        if (c.kind == "se") run_se(dir, c, results);
        fflush(results);
    }
    fclose(results);
    return 0;
}
