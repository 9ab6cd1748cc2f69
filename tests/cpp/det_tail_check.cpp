// Runs the launches between the detector's heads and the recogniser's input ONE AT A TIME (candidate compaction, NMS, landmark decode, the two
// face cutters, the result records), or chained, through the launchers libfrt.so exports, on buffers whose every byte the test controls.
// tests/det_tail_ref.py writes the case directory and holds the references; tests/test_gpu_det_tail.py compares.  This program knows nothing
// about expected values.
//
//   det_tail_check DIR     run DIR/ops.txt on the current device; stops at the first HIP error (exit 1)
//
// DIR/ops.txt is a list of operations, one per line, on NAMED device buffers.  Every buffer is allocated with kGuard bytes in front and behind;
// the guards and every byte the case does not load are filled with the pattern 0x5a (as a float about 1.5e16, as an int 1515870810).  Numbers
// are decimal; floats travel as their 32-bit pattern (decimal); "-" is a null pointer.
//   case ID                            begins a case
//   buf NAME BYTES FILE|-              a buffer the launches may write (FILE: DIR/FILE is loaded at its start; it may be shorter than BYTES)
//   rbuf NAME BYTES FILE               an input: at `end` every byte of it must still be what was loaded
//   load NAME FILE                     DIR/FILE over the start of an existing buffer (an rbuf: the whole of it), nothing else touched
//   geom FAMILY LEVELS IN_W IN_H FRAME_W FRAME_H NMS_BITS BBOX_BITS MAX_FACES   det_geometry(...): the DetGeom of the launches that follow
//   dump_geom FILE                     the DetGeom's bytes -> DIR/FILE
//   decode CONF B CAND COUNT           launch_decode
//   nms CAND LOC COUNT B DEAD OUT NOUT KEPT|-      launch_nms
//   landmarks LDM KEPT NOUT B OUT      launch_landmark_decode
//   crop FRAMES NFRAMES FH FW ROW_STRIDE FRAME_STRIDE BOXES NBOXES|- MAX_FACES F SHARED OH OW CROPS|- CHW VALID    launch_crop_faces
//   align FRAMES NFRAMES FH FW ROW_STRIDE FRAME_STRIDE LM NBOXES|- MAX_FACES F SHARED CROPS|- CHW VALID            launch_align_faces
//   pack BOXES NBOXES VALID IDX|- SIM|- MAX_FACES F OUT               launch_pack_results
//   dump NAME FILE                     the buffer's bytes (without guards) -> DIR/FILE
//   end                                "ID\t<changed guard bytes + changed rbufs>" -> DIR/results.txt; frees every buffer
// Every launch is checked against the sizes of the buffers it is given before it runs, and followed by hipDeviceSynchronize and hipGetLastError.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <sstream>
#include <string>
#include <vector>

#include "frt_kernels.h"

// (csrc/frt_internal.hpp declares it among the host library's internals, which this program does not need)
void launch_pack_results(const frt_bbox *boxes, const int *n_boxes, const int *valid, const int32_t *idx, const float *sim, int max_faces, int F,
                         frt_face_result *out, hipStream_t s);

namespace {

constexpr size_t kGuard = (size_t)64 << 10;
constexpr int kFill = 0x5a;
constexpr size_t kCountStride = 32;  // ints between the frames' candidate counters (kernels_post.hip)

std::string g_case = "(none)";

[[noreturn]] void die(const std::string &msg) {
    fprintf(stderr, "det_tail_check: case %s: %s\n", g_case.c_str(), msg.c_str());
    exit(1);
}
void hipchk(hipError_t e, const char *what) {
    if (e != hipSuccess) die(std::string(what) + ": " + hipGetErrorString(e));
}
#define HIPCHK(x) hipchk((x), #x)

struct Buf {
    char *base = nullptr;
    size_t bytes = 0;
    std::vector<char> loaded;  // rbuf: what must still be there
    bool readonly = false;
};
std::map<std::string, Buf> g_bufs;
std::string g_dir;

std::vector<char> read_all(const std::string &path) {
    FILE *f = fopen(path.c_str(), "rb");
    if (!f) die("cannot open " + path);
    std::vector<char> v;
    char tmp[1 << 16];
    size_t n;
    while ((n = fread(tmp, 1, sizeof(tmp), f)) > 0) v.insert(v.end(), tmp, tmp + n);
    fclose(f);
    return v;
}

void load_buf(Buf &b, const std::string &name, const std::string &file) {
    std::vector<char> v = read_all(g_dir + "/" + file);
    if (v.size() > b.bytes || (b.readonly && v.size() != b.bytes)) die(file + " does not fit buffer " + name);
    if (!v.empty()) HIPCHK(hipMemcpy(b.base + kGuard, v.data(), v.size(), hipMemcpyHostToDevice));
    if (b.readonly) b.loaded.swap(v);
}

void make_buf(const std::string &name, size_t bytes, const std::string &file, bool readonly) {
    if (g_bufs.count(name)) die("buffer " + name + " exists");
    Buf b;
    b.bytes = bytes;
    b.readonly = readonly;
    HIPCHK(hipMalloc(reinterpret_cast<void **>(&b.base), bytes + 2 * kGuard));
    HIPCHK(hipMemset(b.base, kFill, bytes + 2 * kGuard));
    if (file != "-") load_buf(b, name, file);
    else if (readonly) die("rbuf " + name + " needs a file");
    g_bufs[name] = std::move(b);
}

template <class T>
T *ptr(const std::string &name, size_t need_bytes) {
    if (name == "-") return nullptr;
    auto it = g_bufs.find(name);
    if (it == g_bufs.end()) die("no buffer " + name);
    if (it->second.bytes < need_bytes) die("buffer " + name + " holds " + std::to_string(it->second.bytes) + " bytes, the launch needs " + std::to_string(need_bytes));
    return reinterpret_cast<T *>(it->second.base + kGuard);
}

void finish() {
    HIPCHK(hipGetLastError());
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipGetLastError());
}

size_t end_case() {
    size_t changed = 0;
    for (auto &kv : g_bufs) {
        Buf &b = kv.second;
        std::vector<char> h(b.bytes + 2 * kGuard);
        HIPCHK(hipMemcpy(h.data(), b.base, h.size(), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < kGuard; ++i) changed += (h[i] != (char)kFill) + (h[kGuard + b.bytes + i] != (char)kFill);
        if (b.readonly) changed += memcmp(h.data() + kGuard, b.loaded.data(), b.bytes) != 0 ? 1 : 0;
        HIPCHK(hipFree(b.base));
    }
    g_bufs.clear();
    return changed;
}

float from_bits(long long u) {
    const uint32_t v = (uint32_t)u;
    float f;
    memcpy(&f, &v, 4);
    return f;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: det_tail_check DIR\n");
        return 1;
    }
    g_dir = argv[1];
    FILE *ops = fopen((g_dir + "/ops.txt").c_str(), "r");
    if (!ops) die("cannot open " + g_dir + "/ops.txt");
    FILE *results = fopen((g_dir + "/results.txt").c_str(), "w");
    if (!results) die("cannot write " + g_dir + "/results.txt");
    DetGeom g{};
    bool have_geom = false;
    char linebuf[1024];
    while (fgets(linebuf, sizeof(linebuf), ops)) {
        std::istringstream in(linebuf);
        std::string op;
        if (!(in >> op)) continue;
        std::vector<std::string> a;
        for (std::string t; in >> t;) a.push_back(t);
        auto I = [&](size_t i) -> long long {
            if (i >= a.size()) die(op + ": too few arguments");
            return atoll(a[i].c_str());
        };
        auto S = [&](size_t i) -> const std::string & {
            if (i >= a.size()) die(op + ": too few arguments");
            return a[i];
        };
        auto need_geom = [&](long long B) {
            if (!have_geom) die(op + ": no geom");
            if (B < 1 || B > 65535) die(op + ": bad frame count");
        };
        // frames of `fh` rows of `fw` pixels, `rs` bytes from row to row and `fs` from frame to frame: the bytes the cutters may read
        auto frame_bytes = [&](long long n, long long fh, long long fw, long long rs, long long fs) -> size_t {
            if (n < 1 || fh < 1 || fw < 1 || rs < fw * 3 || fs < fh * rs) die(op + ": bad frame layout");
            return (size_t)((n - 1) * fs + (fh - 1) * rs + fw * 3);
        };
        auto slots_ok = [&](long long n, long long maxf, long long F, long long shared) {
            if (maxf < 1 || F < 1 || F > 65535) die(op + ": bad slot count");
            if (!shared && F > n * maxf) die(op + ": more face slots than the frames hold");
        };
        if (op == "case") {
            g_case = S(0);
        } else if (op == "buf" || op == "rbuf") {
            make_buf(S(0), (size_t)I(1), S(2), op == "rbuf");
        } else if (op == "load") {
            auto it = g_bufs.find(S(0));
            if (it == g_bufs.end()) die("no buffer " + S(0));
            load_buf(it->second, S(0), S(1));
        } else if (op == "geom") {
            if (I(1) < 1 || I(1) > DET_MAX_LEVELS || I(2) < 8 || I(3) < 8 || I(4) < 1 || I(5) < 1 || I(8) < 1) die("geom: bad arguments");
            g = det_geometry((int)I(0), (int)I(1), (int)I(2), (int)I(3), (int)I(4), (int)I(5), from_bits(I(6)), from_bits(I(7)), (int)I(8));
            have_geom = true;
        } else if (op == "dump_geom") {
            FILE *f = fopen((g_dir + "/" + S(0)).c_str(), "wb");
            if (!f || fwrite(&g, 1, sizeof(g), f) != sizeof(g)) die("cannot write " + S(0));
            fclose(f);
        } else if (op == "decode") {
            const long long B = I(1);
            need_geom(B);
            launch_decode(nullptr, ptr<float>(S(0), (size_t)B * g.A * 8), (int)B, g, ptr<Candidate>(S(2), (size_t)B * g.A * sizeof(Candidate)),
                          ptr<int>(S(3), ((size_t)(B - 1) * kCountStride + 1) * 4), nullptr);
            finish();
        } else if (op == "nms") {
            const long long B = I(3);
            need_geom(B);
            // the candidate count is read from the device's own counter: a case that injects one keeps it <= A (checked here, before the launch)
            std::vector<int> cc((size_t)(B - 1) * kCountStride + 1);
            int *d_count = ptr<int>(S(2), cc.size() * 4);
            HIPCHK(hipMemcpy(cc.data(), d_count, cc.size() * 4, hipMemcpyDeviceToHost));
            for (long long f = 0; f < B; ++f)
                if (cc[(size_t)f * kCountStride] < 0 || cc[(size_t)f * kCountStride] > g.A) die("nms: a candidate count outside [0, A]: not launched");
            launch_nms(ptr<Candidate>(S(0), (size_t)B * g.A * sizeof(Candidate)), ptr<float>(S(1), (size_t)B * g.A * 16), d_count, (int)B, g,
                       ptr<uint8_t>(S(4), (size_t)B * g.A), ptr<frt_bbox>(S(5), (size_t)B * g.max_faces * sizeof(frt_bbox)), ptr<int>(S(6), (size_t)B * 4),
                       ptr<int>(S(7), (size_t)B * g.max_faces * 4), nullptr);
            finish();
        } else if (op == "landmarks") {
            const long long B = I(3);
            need_geom(B);
            launch_landmark_decode(ptr<float>(S(0), (size_t)B * g.A * 40), ptr<int>(S(1), (size_t)B * g.max_faces * 4), ptr<int>(S(2), (size_t)B * 4), (int)B, g,
                                   ptr<float>(S(4), (size_t)B * g.max_faces * 40), nullptr);
            finish();
        } else if (op == "crop") {
            const long long n = I(1), fh = I(2), fw = I(3), rs = I(4), fs = I(5), maxf = I(8), F = I(9), shared = I(10), oh = I(11), ow = I(12);
            slots_ok(n, maxf, F, shared);
            if (oh < 1 || ow < 1) die("crop: bad output size");
            launch_crop_faces(ptr<uint8_t>(S(0), frame_bytes(n, fh, fw, rs, fs)), (int)fh, (int)fw, (size_t)rs, (size_t)fs, ptr<frt_bbox>(S(6), (size_t)F * sizeof(frt_bbox)),
                              ptr<int>(S(7), (size_t)((F + maxf - 1) / maxf) * 4), (int)maxf, (int)F, (int)shared, (int)oh, (int)ow, ptr<uint8_t>(S(13), (size_t)F * oh * ow * 3),
                              ptr<float>(S(14), (size_t)F * oh * ow * 12), ptr<int>(S(15), (size_t)F * 4), nullptr);
            finish();
        } else if (op == "align") {
            const long long n = I(1), fh = I(2), fw = I(3), rs = I(4), fs = I(5), maxf = I(8), F = I(9), shared = I(10);
            slots_ok(n, maxf, F, shared);
            launch_align_faces(ptr<uint8_t>(S(0), frame_bytes(n, fh, fw, rs, fs)), (int)fh, (int)fw, (size_t)rs, (size_t)fs, ptr<float>(S(6), (size_t)F * 40),
                               ptr<int>(S(7), (size_t)((F + maxf - 1) / maxf) * 4), (int)maxf, (int)F, (int)shared, ptr<uint8_t>(S(11), (size_t)F * 112 * 112 * 3),
                               ptr<float>(S(12), (size_t)F * 112 * 112 * 12), ptr<int>(S(13), (size_t)F * 4), nullptr);
            finish();
        } else if (op == "pack") {
            const long long maxf = I(5), F = I(6);
            if (maxf < 1 || F < 1) die("pack: bad slot count");
            launch_pack_results(ptr<frt_bbox>(S(0), (size_t)F * sizeof(frt_bbox)), ptr<int>(S(1), (size_t)((F + maxf - 1) / maxf) * 4), ptr<int>(S(2), (size_t)F * 4),
                                ptr<int32_t>(S(3), (size_t)F * 4), ptr<float>(S(4), (size_t)F * 4), (int)maxf, (int)F,
                                ptr<frt_face_result>(S(7), (size_t)F * sizeof(frt_face_result)), nullptr);
            finish();
        } else if (op == "dump") {
            auto it = g_bufs.find(S(0));
            if (it == g_bufs.end()) die("no buffer " + S(0));
            std::vector<char> h(it->second.bytes);
            HIPCHK(hipMemcpy(h.data(), it->second.base + kGuard, h.size(), hipMemcpyDeviceToHost));
            FILE *f = fopen((g_dir + "/" + S(1)).c_str(), "wb");
            if (!f || fwrite(h.data(), 1, h.size(), f) != h.size()) die("cannot write " + S(1));
            fclose(f);
        } else if (op == "end") {
            fprintf(results, "%s\t%zu\n", g_case.c_str(), end_case());
            fflush(results);
        } else {
            die("unknown operation " + op);
        }
    }
    fclose(ops);
    fclose(results);
    if (!g_bufs.empty()) die("ops.txt ends inside a case");
    return 0;
}
