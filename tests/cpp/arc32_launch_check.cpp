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
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "arc_conv_describe.hpp"
#include "frt_arc_pack.hpp"
#include "frt_kernels.h"

namespace {

using namespace arc_describe;

constexpr size_t kMargin = ((size_t)1 << 20) / sizeof(float);  // floats in front of and behind every activation buffer
constexpr uint32_t kNaN = 0x7fc00000u, kOutFill = 0x5a5a5a5au;
const char *const kDesc32[ARC32_NUM_DESC] = {"conv1", "shortcut1x1", "conv2", "conv2_res"};

[[noreturn]] void die(const std::string &msg) {
    fprintf(stderr, "arc32_launch_check: %s\n", msg.c_str());
    exit(1);
}
void hipchk(hipError_t e, const char *what, const std::string &id) {
    if (e != hipSuccess) die("case " + id + ": " + what + ": " + hipGetErrorString(e));
}
#define HIPCHK(x) hipchk((x), #x, id)

template <class T>
std::vector<T> read_file(const std::string &path, size_t n) {
    FILE *f = fopen(path.c_str(), "rb");
    if (!f) die("cannot open " + path);
    std::vector<T> v(n);
    const size_t got = fread(v.data(), sizeof(T), n, f);
    char extra;
    const bool more = fread(&extra, 1, 1, f) == 1;
    fclose(f);
    if (got != n || more) die(path + ": expected " + std::to_string(n) + " elements");
    return v;
}
void write_file(const std::string &path, const void *p, size_t bytes) {
    FILE *f = fopen(path.c_str(), "wb");
    if (!f || fwrite(p, 1, bytes, f) != bytes) die("cannot write " + path);
    fclose(f);
}

struct Case {
    std::string kind, id;
    int shape = 0, d = 0, F = 0, H = 0, C = 0, sc_stride = 0;
};
std::vector<Case> read_cases(const std::string &dir) {
    FILE *f = fopen((dir + "/cases.txt").c_str(), "r");
    if (!f) die("cannot open " + dir + "/cases.txt");
    std::vector<Case> cs;
    char kind[32], id[256];
    while (fscanf(f, "%31s %255s", kind, id) == 2) {
        Case c;
        c.kind = kind;
        c.id = id;
        bool ok = false;
        if (c.kind == "conv")
            ok = fscanf(f, "%d %d %d", &c.shape, &c.d, &c.F) == 3 && c.shape >= 0 && c.shape < kNumShapes && c.d >= 0 && c.d < ARC32_NUM_DESC;
        else if (c.kind == "input" || c.kind == "fc")
            ok = fscanf(f, "%d", &c.F) == 1;
        else if (c.kind == "se")
            ok = fscanf(f, "%d %d %d %d", &c.H, &c.C, &c.F, &c.sc_stride) == 4 && c.H >= 1 && c.H <= 56 && c.C >= 64 && c.C <= 512 && c.C % 64 == 0 &&
                 (size_t)c.H * c.H * c.C <= 56 * 56 * 64 && (c.sc_stride == 1 || c.sc_stride == 2);
        if (!ok || c.F < 1 || c.F > 8) die("bad case line for " + c.id);  // 8: the mode's chunk
        cs.push_back(c);
    }
    fclose(f);
    return cs;
}

// `cap` floats between two margins, all filled with `fill`; the first `logical` floats behind the front margin are the tensor
struct Buf {
    uint32_t *base = nullptr;
    size_t cap = 0, logical = 0;
    uint32_t fill = 0;
    float *ptr() const { return reinterpret_cast<float *>(base + kMargin); }
};

struct DeviceCase {
    std::string id;
    std::vector<void *> owned;
    ~DeviceCase() {
        for (void *p : owned) (void)hipFree(p);
    }
    Buf buf(size_t cap, size_t logical, uint32_t fill, const float *init) {
        if (logical > cap) die("case " + id + ": a tensor of " + std::to_string(logical) + " floats does not fit the product's buffer of " + std::to_string(cap));
        Buf b;
        b.cap = cap;
        b.logical = logical;
        b.fill = fill;
        HIPCHK(hipMalloc(reinterpret_cast<void **>(&b.base), (2 * kMargin + cap) * sizeof(uint32_t)));
        owned.push_back(b.base);
        HIPCHK(hipMemsetD32(reinterpret_cast<hipDeviceptr_t>(b.base), (int)fill, 2 * kMargin + cap));
        if (init) HIPCHK(hipMemcpy(b.base + kMargin, init, logical * sizeof(float), hipMemcpyHostToDevice));
        return b;
    }
    Buf in(size_t cap, const std::vector<float> &v) { return buf(cap, v.size(), kNaN, v.data()); }
    Buf out(size_t cap, size_t logical) { return buf(cap, logical, kOutFill, nullptr); }
    template <class T>
    T *upload(const std::vector<T> &v) {
        T *d = nullptr;
        HIPCHK(hipMalloc(reinterpret_cast<void **>(&d), v.size() * sizeof(T)));
        owned.push_back(d);
        HIPCHK(hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
        return d;
    }
    // the logical tensor -> `path`; returns the number of floats outside it, margins included, that no longer hold the fill pattern
    size_t download(const Buf &b, const std::string &path) {
        std::vector<uint32_t> h(2 * kMargin + b.cap);
        HIPCHK(hipMemcpy(h.data(), b.base, h.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
        write_file(path, h.data() + kMargin, b.logical * sizeof(uint32_t));
        size_t changed = 0;
        for (size_t i = 0; i < kMargin; ++i) changed += h[i] != b.fill;
        for (size_t i = kMargin + b.logical; i < h.size(); ++i) changed += h[i] != b.fill;
        return changed;
    }
    void finish() {
        HIPCHK(hipGetLastError());
        HIPCHK(hipDeviceSynchronize());
        HIPCHK(hipGetLastError());
    }
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
    DeviceCase dc;
    dc.id = c.id;
    // the capacity of the buffer a described pointer names
    auto cap_of = [&](const float *p) -> size_t {
        if (p == b.x || p == b.T || p == b.y) return sz.act;
        if (p == b.SC) return sz.sc;
        if (p == b.RES) return sz.res;
        die("case " + c.id + ": the description names a buffer the harness does not know");
    };
    const size_t F = (size_t)c.F, nx = F * a.H * a.W * a.Cin, nout = F * a.Ho * a.Wo * a.Cout;
    if (kMargin < (size_t)(a.W + 1) * a.Cin) die("case " + c.id + ": the margins are shorter than a row of the input");
    const std::vector<float> x = read_file<float>(pre + ".x", nx), w = read_file<float>(pre + ".w", (size_t)a.Cout * a.Cin * a.ks * a.ks);
    const std::vector<float> par = read_file<float>(pre + ".p", (size_t)2 * a.Cout);
    a.x = dc.in(cap_of(ds.a.x), x).ptr();
    a.w = dc.upload(frt::conv32_w_frag(w.data(), a.Cout, a.Cin, a.ks));
    if (a.ps) {
        float *pro = dc.upload(read_file<float>(pre + ".pro", (size_t)2 * a.Cin));
        a.ps = pro;
        a.pb = pro + a.Cin;
    }
    float *dpar = dc.upload(par);
    a.p0 = dpar;
    if (a.p1) a.p1 = dpar + a.Cout;
    if (a.sc) a.sc = dc.in(cap_of(ds.a.sc), read_file<float>(pre + ".sc", F * a.sc_h * a.sc_w * a.Cout)).ptr();
    const Buf o = dc.out(cap_of(ds.a.out), nout);
    a.out = o.ptr();
    launch_conv32(a, nullptr);
    dc.finish();
    fprintf(results, "%s\t%zu\t%s\n", c.id.c_str(), dc.download(o, pre + ".out0"), kDesc32[c.d]);
}

void run_input(const std::string &dir, const Case &c, FILE *results) {
    const std::string pre = dir + "/" + c.id;
    DeviceCase dc;
    dc.id = c.id;
    const size_t F = (size_t)c.F;
    const std::vector<float> x = read_file<float>(pre + ".x", F * 3 * 112 * 112), w = read_file<float>(pre + ".w", 64 * 27), par = read_file<float>(pre + ".p", 3 * 64);
    std::vector<float> wt(27 * 64);  // build(): [27][64]
    for (int co = 0; co < 64; ++co)
        for (int k = 0; k < 27; ++k) wt[k * 64 + co] = w[co * 27 + k];
    const Buf dx = dc.in(x.size(), x);  // d_in has no slack
    float *dpar = dc.upload(par);
    const Buf y = dc.out(arc32_buffer_sizes(c.F).act, F * 112 * 112 * 64);
    launch_arc32_input(dx.ptr(), dc.upload(wt), dpar, dpar + 64, dpar + 128, y.ptr(), c.F, nullptr);
    dc.finish();
    fprintf(results, "%s\t%zu\tlaunch_arc32_input\n", c.id.c_str(), dc.download(y, pre + ".out0"));
}

void run_fc(const std::string &dir, const Case &c, FILE *results) {
    const std::string pre = dir + "/" + c.id;
    DeviceCase dc;
    dc.id = c.id;
    const size_t F = (size_t)c.F;
    const Arc32BufferSizes sz = arc32_buffer_sizes(c.F);
    const std::vector<float> yin = read_file<float>(pre + ".x", F * 25088), w = read_file<float>(pre + ".w", (size_t)512 * 25088);
    const std::vector<float> pro = read_file<float>(pre + ".pro", 2 * 512), par = read_file<float>(pre + ".p", 3 * 512);
    const std::vector<int> valid = read_file<int>(pre + ".valid", F);
    const Buf y = dc.in(sz.act, yin), sums = dc.out(sz.fc_out, F * 512), out = dc.out(F * 512, F * 512);
    float *dpro = dc.upload(pro), *dpar = dc.upload(par);
    launch_fc32(y.ptr(), dpro, dpro + 512, dc.upload(frt::fc32_w_nhwc(w.data())), sums.ptr(), c.F, nullptr);
    launch_fc_finalize(sums.ptr(), 1, c.F, dpar, dpar + 512, dpar + 1024, dc.upload(valid), out.ptr(), nullptr);
    dc.finish();
    const size_t changed = dc.download(out, pre + ".out0") + dc.download(sums, pre + ".out1");
    fprintf(results, "%s\t%zu\tlaunch_fc32\n", c.id.c_str(), changed);
}

void run_se(const std::string &dir, const Case &c, FILE *results) {
    const std::string pre = dir + "/" + c.id;
    DeviceCase dc;
    dc.id = c.id;
    const size_t F = (size_t)c.F, C = c.C, n = F * c.H * c.H * C, sh = (size_t)c.H * c.sc_stride;
    const Arc32BufferSizes sz = arc32_buffer_sizes(c.F);
    const std::vector<float> res = read_file<float>(pre + ".x", n), sc = read_file<float>(pre + ".sc", F * sh * sh * C), w = read_file<float>(pre + ".w", 2 * (C / 16) * C);
    const Buf dres = dc.in(sz.res, res), dsc = dc.in(sz.act, sc), y = dc.out(sz.act, n), gate = dc.out(sz.gate, F * C);
    float *dw = dc.upload(w);
    const Se32Args a{dres.ptr(), dw, dw + (C / 16) * C, gate.ptr(), dsc.ptr(), y.ptr(), c.F, c.H, c.H, c.C, (int)sh, (int)sh, c.sc_stride};
    launch_se32(a, nullptr);
    dc.finish();
    const size_t changed = dc.download(y, pre + ".out0") + dc.download(gate, pre + ".gate");
    fprintf(results, "%s\t%zu\tlaunch_se32\n", c.id.c_str(), changed);
}

}  // namespace

int main(int argc, char **argv) {
    const bool describe_only = argc == 3 && std::string(argv[1]) == "--describe";
    if (argc != 2 && !describe_only) die("usage: arc32_launch_check [--describe] DIR");
    const std::string dir = argv[argc - 1];
    const std::vector<Case> cases = read_cases(dir);
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
