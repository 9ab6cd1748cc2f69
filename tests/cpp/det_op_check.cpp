// Runs the detector's ops ONE AT A TIME: frt_detector_create on a blob the test wrote, then for every op of frt_detector::ops the op's input(s)
// are copied from the work directory into the op's own `in` pointer(s), frt_detector::run_op(i, B, stream) - the call forward() makes - runs
// once, and the op's logical output(s) are written back.  tests/test_gpu_det_ops.py compares them with the float64 restatement of
// tests/det_op_ref.py.  Nothing about the launches is decided here: which kernel runs is launch_dwpw / launch_conv3x3_multi / ...'s business.
//
//   det_op_check DIR      DIR/job.txt: "<frame_w> <frame_h> <in_h> <in_w> <B> <u8: 0 | 1>", then "<op> <tag>" per extra run of one op on
//                         op<i>.p<k>.in.<tag> (outputs and results line carry the tag); DIR/blob.frtw
//
// The detector is created with max_batch = B + 1: every activation buffer has one frame slot behind the B frames in use.  Before each op
// every buffer an op reads or writes (the distinct in / out / add / out2 pointers of the op list, d_loc / d_conf / d_ldm, d_tmp) is filled
// with a sentinel - a large finite float, so that a kernel which accumulated slack into a stored value cannot pass the comparison - and
// after the op every word outside the op's logical output (frame slot B, the other channels of a concat target, every other buffer, the
// op's own inputs) must still hold what was put there.  d_loc / d_conf / d_ldm are written whole for frames 0 .. B-1: the anchors of levels
// the op does not own are checked by the test, which knows the anchor table.
//
// Read per op i and problem k (one per pyramid level / RFB branch; all little-endian fp32):
//   op<i>.p<k>.in   [B][Cin][H][W]        op<i>.p<k>.add  [B][Cout][add_h][add_w] (ops with an upsample-add)       op<i>.p<k>.in1  (RFB tail: the shortcut)
// Written:
//   oplist.txt      one line per problem: kind, every dimension, the device addresses (tests rebuild the graph from them)
//   op<i>.p<k>.out / .out2 [B][channels][Ho][Wo], op<i>.loc / .conf / .ldm [B][A][4 | 2 | 10]
//   results.txt     "<name>\t<changed sentinel / input words>" per op that ran; u8conv / u8stem: launch_det_conv1_u8 and launch_det_stem on
//                   DIR/frames.u8 [B][frame_h][frame_w][3] (u8 = 1; "n/a" where the launcher declined), outputs u8conv.out (op 0's) and u8stem.out (op 2's)
// Exit status 1 on any HIP error; what was written before it stays.
#include <algorithm>

#include "frt_detector.hpp"
#undef HIPCHK  // the host library's own (csrc/frt_host.hpp), which returns a status: here a HIP error ends the process
#define CHECK_PROGRAM "det_op_check"
#include "check_common.hpp"

namespace {

using namespace check;

constexpr uint32_t kFill = 0x7149f2ca;  // 1e30f

// channels [coff, coff + cn) of a [frames][ctotal][h][w] tensor at ptr; flat: [frames][ctotal] words per frame (d_loc / d_conf / d_ldm)
struct Ref {
    std::string name;
    const float *ptr;
    int ctotal, coff, cn, h, w;
    size_t frame_words() const { return (size_t)ctotal * h * w; }
};
struct OpDesc {
    std::string kind, dump;  // dump: the oplist.txt lines
    std::vector<Ref> ins, outs;
    const float *tmp = nullptr;  // the depthwise scratch an op may write
    size_t tmp_words = 0;
};

std::string kv(const char *k, long v) { return std::string(" ") + k + "=" + std::to_string(v); }
std::string kp(const char *k, const void *p) { return std::string(" ") + k + "=" + std::to_string((unsigned long long)reinterpret_cast<uintptr_t>(p)); }

struct Describe {
    frt_detector *d;
    int B;
    size_t i = 0;
    OpDesc o;
    std::string head(int k) const { return "op " + std::to_string(i) + " " + o.kind + " p " + std::to_string(k); }
    std::string nm(int k, const char *what) const { return "op" + std::to_string(i) + ".p" + std::to_string(k) + "." + what; }
    void flat_outs(float *ldm) {
        const int A = d->g.A;
        o.outs.push_back({"op" + std::to_string(i) + ".loc", d->d_loc, A * 4, 0, A * 4, 1, 1});
        o.outs.push_back({"op" + std::to_string(i) + ".conf", d->d_conf, A * 2, 0, A * 2, 1, 1});
        if (ldm) o.outs.push_back({"op" + std::to_string(i) + ".ldm", ldm, A * 10, 0, A * 10, 1, 1});
    }
    void operator()(DwPwArgs &a) {
        o.kind = "dwpw";
        o.ins.push_back({nm(0, "in"), a.in, a.Cin, 0, a.Cin, a.H, a.W});
        if (a.add) o.ins.push_back({nm(0, "add"), a.add, a.Cout, 0, a.Cout, a.add_h, a.add_w});
        o.outs.push_back({nm(0, "out"), a.out, a.Cout, 0, a.Cout, a.Ho, a.Wo});
        if (a.wd && a.tmp) {
            o.tmp = a.tmp;
            o.tmp_words = (size_t)B * a.Cin * a.Ho * a.Wo;
        }
        o.dump = head(0) + kp("in", a.in) + kp("out", a.out) + kp("add", a.add) + kv("Cin", a.Cin) + kv("H", a.H) + kv("W", a.W) + kv("Cout", a.Cout) + kv("Ho", a.Ho) +
                 kv("Wo", a.Wo) + kv("stride", a.stride) + kv("relu", a.relu) + kv("add_h", a.add_h) + kv("add_w", a.add_w) + kv("dw", a.wd != nullptr) +
                 kv("wph", a.wph != nullptr) + kv("wpf", a.wpf != nullptr) + kv("tmp", a.tmp != nullptr) + "\n";
    }
    void operator()(frt_detector::Conv3Op &c) {
        o.kind = "conv3";
        for (int k = 0; k < c.n; ++k) {
            const Conv3Args &a = c.p[k];
            const int c1 = a.out2 ? a.split : a.Cout;
            o.ins.push_back({nm(k, "in"), a.in, a.Cin, 0, a.Cin, a.H, a.W});
            o.outs.push_back({nm(k, "out"), a.out, a.out_ctotal, a.out_coff, c1, a.Ho, a.Wo});
            if (a.out2) o.outs.push_back({nm(k, "out2"), a.out2, a.out2_ctotal, a.out2_coff, a.Cout - a.split, a.Ho, a.Wo});
            o.dump += head(k) + kp("in", a.in) + kp("out", a.out) + kp("out2", a.out2) + kv("Cin", a.Cin) + kv("H", a.H) + kv("W", a.W) + kv("Cout", a.Cout) +
                      kv("Ho", a.Ho) + kv("Wo", a.Wo) + kv("stride", a.stride) + kv("relu", a.relu) + kv("out_ctotal", a.out_ctotal) + kv("out_coff", a.out_coff) +
                      kv("split", a.out2 ? a.split : a.Cout) + kv("out2_ctotal", a.out2_ctotal) + kv("out2_coff", a.out2_coff) + kv("wh", a.wh != nullptr) + "\n";
        }
    }
    void operator()(frt_detector::HeadsOp &h) {
        o.kind = "heads";
        for (int k = 0; k < h.n; ++k) {
            const HeadArgs &a = h.p[k];
            o.ins.push_back({nm(k, "in"), a.in, a.C, 0, a.C, a.H, a.W});
            o.dump += head(k) + kp("in", a.in) + kp("loc", a.loc) + kp("conf", a.conf) + kp("ldm", a.ldm) + kv("C", a.C) + kv("H", a.H) + kv("W", a.W) + kv("A", a.A) +
                      kv("base", a.base) + kv("na", 2) + "\n";
        }
        flat_outs(h.p[0].ldm);
    }
    void operator()(frt_detector::SlimHeadsOp &h) {
        o.kind = "slim_heads";
        for (int k = 0; k < h.n; ++k) {
            const SlimHeadArgs &a = h.a.lv[k];
            o.ins.push_back({nm(k, "in"), a.in, a.C, 0, a.C, a.H, a.W});
            o.dump += head(k) + kp("in", a.in) + kp("loc", h.a.loc) + kp("conf", h.a.conf) + kp("ldm", h.a.ldm) + kv("C", a.C) + kv("H", a.H) + kv("W", a.W) + kv("A", h.a.A) +
                      kv("base", a.base) + kv("na", a.na) + "\n";
        }
        flat_outs(h.a.ldm);
    }
    void operator()(DenseHeadArgs &a) {
        o.kind = "dense_head";
        o.ins.push_back({nm(0, "in"), a.in, a.C, 0, a.C, a.H, a.W});
        o.dump = head(0) + kp("in", a.in) + kp("loc", a.loc) + kp("conf", a.conf) + kp("ldm", a.ldm) + kv("C", a.C) + kv("H", a.H) + kv("W", a.W) + kv("A", a.A) +
                 kv("base", a.base) + kv("na", a.na) + kv("cout", a.cout) + "\n";
        flat_outs(a.ldm);
    }
    void operator()(RfbProjArgs &a) {
        o.kind = "rfb_proj";
        o.ins.push_back({nm(0, "in"), a.in, 64, 0, 64, a.H, a.W});
        o.outs.push_back({nm(0, "out"), a.red, 24, 0, 24, a.H, a.W});
        o.outs.push_back({nm(0, "out2"), a.sc, 64, 0, 64, a.H, a.W});
        o.dump = head(0) + kp("in", a.in) + kp("out", a.red) + kp("out2", a.sc) + kv("H", a.H) + kv("W", a.W) + "\n";
    }
    void operator()(frt_detector::RfbConvOp &c) {
        o.kind = "rfb_conv";
        for (int k = 0; k < c.n; ++k) {
            const RfbConvArgs &a = c.a.p[k];
            o.ins.push_back({nm(k, "in"), a.in, a.in_ctotal, a.in_coff, a.Cin, c.a.H, c.a.W});
            o.outs.push_back({nm(k, "out"), a.out, a.out_ctotal, a.out_coff, a.Cout, c.a.H, c.a.W});
            o.dump += head(k) + kp("in", a.in) + kp("out", a.out) + kv("Cin", a.Cin) + kv("Cout", a.Cout) + kv("H", c.a.H) + kv("W", c.a.W) + kv("dil", a.dil) + kv("relu", a.relu) +
                      kv("in_ctotal", a.in_ctotal) + kv("in_coff", a.in_coff) + kv("out_ctotal", a.out_ctotal) + kv("out_coff", a.out_coff) + "\n";
        }
    }
    void operator()(RfbTailArgs &a) {
        o.kind = "rfb_tail";
        o.ins.push_back({nm(0, "in"), a.cat, 48, 0, 48, a.H, a.W});
        o.ins.push_back({nm(0, "in1"), a.sc, 64, 0, 64, a.H, a.W});
        o.outs.push_back({nm(0, "out"), a.out, 64, 0, 64, a.H, a.W});
        o.dump = head(0) + kp("in", a.cat) + kp("in1", a.sc) + kp("out", a.out) + kv("H", a.H) + kv("W", a.W) + "\n";
    }
};

// every buffer the ops touch, B + 1 frame slots each, and a host image of what it must hold
struct Buffers {
    std::map<const float *, std::vector<uint32_t>> want;  // base pointer -> expected words
    std::map<const float *, std::vector<uint8_t>> open;   // 1: the running op may write this word
    void add(const float *p, size_t words) {
        auto &v = want[p];
        if (v.size() < words) v.resize(words);
    }
    struct Range {
        const float *p;
        size_t off, n;
    };
    std::vector<Range> dirty;  // what place() changed in the host images since the last fill()
    void fill() {
        for (auto &b : want) {
            if (open[b.first].size() != b.second.size()) {  // first use
                std::fill(b.second.begin(), b.second.end(), kFill);
                open[b.first].assign(b.second.size(), 0);
            }
            HIPCHK(hipMemsetD32(reinterpret_cast<hipDeviceptr_t>(const_cast<float *>(b.first)), (int)kFill, b.second.size()));
        }
        for (const Range &r : dirty) {
            std::fill(want.at(r.p).begin() + r.off, want.at(r.p).begin() + r.off + r.n, kFill);
            std::memset(open.at(r.p).data() + r.off, 0, r.n);
        }
        dirty.clear();
    }
    void open_words(const float *p, size_t off, size_t n) {
        std::memset(open.at(p).data() + off, 1, n);
        dirty.push_back({p, off, n});
    }
    // the logical tensor r of `frames` frames: uploaded from `src` (inputs) or opened for writing (outputs)
    void place(const Ref &r, int frames, const uint32_t *src) {
        auto &w = want.at(r.ptr);
        const size_t hw = (size_t)r.h * r.w, n = (size_t)r.cn * hw;
        for (int b = 0; b < frames; ++b) {
            const size_t off = (size_t)b * r.frame_words() + (size_t)r.coff * hw;
            if (off + n > w.size()) die(g_where + ": " + r.name + " does not fit its buffer");
            if (src) {
                std::memcpy(w.data() + off, src + (size_t)b * n, n * 4);
                dirty.push_back({r.ptr, off, n});
                HIPCHK(hipMemcpy(const_cast<float *>(r.ptr) + off, src + (size_t)b * n, n * 4, hipMemcpyHostToDevice));
            } else {
                open_words(r.ptr, off, n);
            }
        }
    }
    // words that may not have changed and did; the buffers' contents land in `got`
    size_t check(std::map<const float *, std::vector<uint32_t>> &got) {
        size_t changed = 0;
        for (auto &b : want) {
            auto &g = got[b.first];
            g.resize(b.second.size());
            HIPCHK(hipMemcpy(g.data(), b.first, g.size() * 4, hipMemcpyDeviceToHost));
            bool touched = false;
            for (const Range &r : dirty) touched = touched || r.p == b.first;
            if (!touched) {
                changed += changed_outside(g.data(), g.size(), 0, 0, kFill);
                continue;
            }
            const auto &o = open.at(b.first);
            for (size_t k = 0; k < g.size(); ++k) changed += !o[k] && g[k] != b.second[k];
        }
        return changed;
    }
};

void write_ref(const std::string &dir, const Ref &r, int frames, const std::vector<uint32_t> &buf) {
    const size_t hw = (size_t)r.h * r.w, n = (size_t)r.cn * hw;
    std::vector<uint32_t> out((size_t)frames * n);
    for (int b = 0; b < frames; ++b) std::memcpy(out.data() + (size_t)b * n, buf.data() + (size_t)b * r.frame_words() + (size_t)r.coff * hw, n * 4);
    write_file(dir + "/" + r.name, out.data(), out.size() * 4);
}

}  // namespace

int main(int argc, char **argv) {
    if (argc != 2) die("usage: det_op_check DIR");
    const std::string dir = argv[1];
    int frame_w, frame_h, in_h, in_w, B, u8;
    std::vector<std::pair<size_t, std::string>> extras;  // further lines of job.txt: "<op> <tag>"
    {
        FILE *f = fopen((dir + "/job.txt").c_str(), "r");
        if (!f || fscanf(f, "%d %d %d %d %d %d", &frame_w, &frame_h, &in_h, &in_w, &B, &u8) != 6 || B < 1 || B > 64) die("bad " + dir + "/job.txt");
        char tag[64];
        int op;
        while (fscanf(f, "%d %63s", &op, tag) == 2) extras.push_back({(size_t)op, tag});
        fclose(f);
    }
    frt_detector *d = nullptr;
    if (frt_detector_create((dir + "/blob.frtw").c_str(), frame_w, frame_h, 3, in_h, in_w, B + 1, 4, 0.4f, 0.6f, 0, &d) != FRT_OK)
        die(std::string("frt_detector_create: ") + frt_last_error());
    hipStream_t s = d->stream;

    std::vector<OpDesc> ops;
    Buffers bufs;
    const size_t slots = (size_t)B + 1;
    {
        std::string list;
        for (size_t i = 0; i < d->ops.size(); ++i) {
            Describe ds{d, B, i, {}};
            std::visit([&](auto &a) { ds(a); }, d->ops[i]);
            list += ds.o.dump;
            for (const auto *refs : {&ds.o.ins, &ds.o.outs})
                for (const Ref &r : *refs) bufs.add(r.ptr, slots * r.frame_words());
            if (ds.o.tmp) bufs.add(ds.o.tmp, slots * (ds.o.tmp_words / B));
            ops.push_back(ds.o);
        }
        bufs.add(d->d_loc, slots * d->g.A * 4);
        bufs.add(d->d_conf, slots * d->g.A * 2);
        if (d->d_ldm) bufs.add(d->d_ldm, slots * d->g.A * 10);
        write_file(dir + "/oplist.txt", list.data(), list.size());
    }
    FILE *results = fopen((dir + "/results.txt").c_str(), "w");
    if (!results) die("cannot write " + dir + "/results.txt");
    std::map<const float *, std::vector<uint32_t>> got;

    // after the launch(es) of one step: synchronise, check, write the outputs
    auto finish = [&](const std::vector<Ref> &outs, const std::vector<std::string> &names) {
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(s));
        HIPCHK(hipGetLastError());
        const size_t changed = bufs.check(got);
        for (size_t k = 0; k < outs.size(); ++k) {
            Ref r = outs[k];
            if (!names.empty()) r.name = names[k];
            write_ref(dir, r, B, got.at(r.ptr));
        }
        fprintf(results, "%s\t%zu\n", g_where.c_str(), changed);
        fflush(results);
    };

    // op i alone; tag: the inputs are op<i>.p<k>.in.<tag> (an op's own input scaled, the range-edge cases) and the outputs carry the tag too
    auto run_alone = [&](size_t i, const std::string &tag) {
        const OpDesc &o = ops[i];
        g_where = "op" + std::to_string(i) + (tag.empty() ? "" : "." + tag);
        bufs.fill();
        for (const Ref &r : o.ins) {
            const bool scaled = !tag.empty() && r.name.size() > 3 && r.name.compare(r.name.size() - 3, 3, ".in") == 0;
            const std::vector<uint32_t> x = read_exact<uint32_t>(dir + "/" + r.name + (scaled ? "." + tag : ""), (size_t)B * r.cn * r.h * r.w, false, "words");
            bufs.place(r, B, x.data());
        }
        std::vector<std::string> names;
        for (const Ref &r : o.outs) {
            bufs.place(r, B, nullptr);
            names.push_back(r.name + (tag.empty() ? "" : "." + tag));
        }
        if (o.tmp) bufs.open_words(o.tmp, 0, o.tmp_words);
        d->run_op(i, B, s);
        finish(o.outs, names);
    };
    for (size_t i = 0; i < ops.size(); ++i) run_alone(i, "");
    for (const auto &e : extras) {
        if (e.first >= ops.size()) die("job.txt names op " + std::to_string(e.first));
        run_alone(e.first, e.second);
    }

    if (u8) {
        if (frame_w != in_w || frame_h != in_h) die("u8 = 1 needs frames of the network's input size");
        const frt_detector::Stem st = d->stem();
        const size_t tight = (size_t)frame_w * 3, fbytes = tight * frame_h;
        const std::vector<char> frames = read_all(dir + "/frames.u8");
        if (frames.size() < (size_t)B * fbytes) die("cannot read " + dir + "/frames.u8");
        g_where = "u8conv";
        HIPCHK(hipMemcpy(d->d_frames, frames.data(), (size_t)B * fbytes, hipMemcpyHostToDevice));
        if (st.c) {
            bufs.fill();
            bufs.place(ops[0].outs[0], B, nullptr);
            Conv3Args c = *st.c;
            c.B = B;
            if (launch_det_conv1_u8(d->d_frames, tight, fbytes, c, s)) finish({ops[0].outs[0]}, {"u8conv.out"});
            else fprintf(results, "%s\tn/a\n", g_where.c_str());
            g_where = "u8stem";
            bufs.fill();
            if (st.d1) {
                bufs.place(ops[2].outs[0], B, nullptr);
                if (launch_det_stem(d->d_frames, tight, fbytes, c, *st.d1, *st.d2, s)) finish({ops[2].outs[0]}, {"u8stem.out"});
                else fprintf(results, "%s\tn/a\n", g_where.c_str());
            } else {
                fprintf(results, "%s\tn/a\n", g_where.c_str());
            }
        }
    }
    fclose(results);
    frt_detector_destroy(d);
    return 0;
}
