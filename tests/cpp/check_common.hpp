// The shared core of the launch-alone check programs (det_tail_check, match_stage_check, match_exact_check, arc_launch_check, arc32_launch_check, det_op_check):
// what they all need to stop at the first error, to read and write the files of a case directory, and to count what a launch changed outside
// the memory it was given.  Two buffer models sit on top of the small utilities:
//   * NAMED GUARDED BUFFERS driven by an op list (run_ops: DIR/ops.txt): every buffer between two guards of kGuard bytes, the guards and every
//     byte the case does not load filled with 0x5a; an `rbuf` must be byte-identical at `end`.  The program supplies the launches.
//   * MARGIN BUFFERS driven by a case list (read_cases: DIR/cases.txt, DeviceCase): a buffer of the product's capacity behind (and, where the
//     program asks for it, in front of) a margin, everything outside the logical tensor filled with a pattern the program chooses.
// Every count of changed guard / margin / slack elements goes through changed_outside(), a pure host function (tests/cpp/changed_outside_test.cpp).
// A program defines CHECK_PROGRAM, its name in messages, before it includes this file.  Nothing here makes a HIP call unless it is called.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <sstream>
#include <string>
#include <vector>

#ifndef CHECK_PROGRAM
#error "define CHECK_PROGRAM, the program's name, before including check_common.hpp"
#endif

namespace check {

// ------------------------------------------------------------------------------------------------ small utilities
inline std::string g_case = "(none)";  // the op list's current case: in front of every message of an op-list program
inline bool g_case_in_messages = false;
inline std::string g_where;            // in front of a HIP error only: "case ID" (DeviceCase) or the step's name (det_op_check)

[[noreturn]] inline void die(const std::string &msg) {
    if (g_case_in_messages) fprintf(stderr, CHECK_PROGRAM ": case %s: %s\n", g_case.c_str(), msg.c_str());
    else fprintf(stderr, CHECK_PROGRAM ": %s\n", msg.c_str());
    exit(1);
}
inline void hipchk(hipError_t e, const char *what) {
    if (e != hipSuccess) die((g_where.empty() ? "" : g_where + ": ") + what + ": " + hipGetErrorString(e));
}
#define HIPCHK(x) ::check::hipchk((x), #x)

// after the launch(es) of one step
inline void sync_and_check() {
    HIPCHK(hipGetLastError());
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipGetLastError());
}

inline std::vector<char> read_all(const std::string &path) {
    FILE *f = fopen(path.c_str(), "rb");
    if (!f) die("cannot open " + path);
    std::vector<char> v;
    char tmp[1 << 16];
    size_t n;
    while ((n = fread(tmp, 1, sizeof(tmp), f)) > 0) v.insert(v.end(), tmp, tmp + n);
    fclose(f);
    return v;
}

// exactly n elements, no trailing byte; optional: an absent file is an empty vector
template <class T>
std::vector<T> read_exact(const std::string &path, size_t n, bool optional = false, const char *unit = "elements") {
    FILE *f = fopen(path.c_str(), "rb");
    if (!f) {
        if (optional) return {};
        die("cannot open " + path);
    }
    std::vector<T> v(n);
    const size_t got = fread(v.data(), sizeof(T), n, f);
    char extra;
    const bool more = fread(&extra, 1, 1, f) == 1;
    fclose(f);
    if (got != n || more) die(path + ": expected " + std::to_string(n) + " " + unit);
    return v;
}

inline void write_file(const std::string &path, const void *p, size_t bytes) {
    FILE *f = fopen(path.c_str(), "wb");
    if (!f || fwrite(p, 1, bytes, f) != bytes) die("cannot write " + path);
    fclose(f);
}

inline float from_bits(long long u) {
    const uint32_t v = (uint32_t)u;
    float f;
    memcpy(&f, &v, 4);
    return f;
}

// `total` host elements, of which [front, front + logical) are the launch's to write: how many of the others no longer hold `fill`
template <class T>
size_t changed_outside(const T *h, size_t total, size_t front, size_t logical, T fill) {
    size_t changed = 0;
    for (size_t i = 0; i < front && i < total; ++i) changed += h[i] != fill;
    for (size_t i = front + logical; i < total; ++i) changed += h[i] != fill;
    return changed;
}

// ------------------------------------------------------------------------------------------------ named guarded buffers, driven by an op list
constexpr size_t kGuard = (size_t)64 << 10;
constexpr int kGuardFill = 0x5a;

struct GuardedBuf {
    char *base = nullptr;
    size_t bytes = 0;
    std::vector<char> loaded;  // rbuf: what must still be there
    bool readonly = false;
};
inline std::map<std::string, GuardedBuf> g_bufs;
inline std::string g_dir;

inline GuardedBuf &find_buf(const std::string &name) {
    auto it = g_bufs.find(name);
    if (it == g_bufs.end()) die("no buffer " + name);
    return it->second;
}

inline void load_buf(GuardedBuf &b, const std::string &name, const std::string &file) {
    std::vector<char> v = read_all(g_dir + "/" + file);
    if (v.size() > b.bytes || (b.readonly && v.size() != b.bytes)) die(file + " does not fit buffer " + name);
    if (!v.empty()) HIPCHK(hipMemcpy(b.base + kGuard, v.data(), v.size(), hipMemcpyHostToDevice));
    if (b.readonly) b.loaded.swap(v);
}

inline void make_buf(const std::string &name, size_t bytes, const std::string &file, bool readonly) {
    if (g_bufs.count(name)) die("buffer " + name + " exists");
    GuardedBuf b;
    b.bytes = bytes;
    b.readonly = readonly;
    HIPCHK(hipMalloc(reinterpret_cast<void **>(&b.base), bytes + 2 * kGuard));
    HIPCHK(hipMemset(b.base, kGuardFill, bytes + 2 * kGuard));
    if (file != "-") load_buf(b, name, file);
    else if (readonly) die("rbuf " + name + " needs a file");
    g_bufs[name] = std::move(b);
}

// the start of buffer `name` ("-": a null pointer), which must hold what the launch needs
template <class T>
T *ptr(const std::string &name, size_t need_bytes = 0) {
    if (name == "-") return nullptr;
    GuardedBuf &b = find_buf(name);
    if (b.bytes < need_bytes) die("buffer " + name + " holds " + std::to_string(b.bytes) + " bytes, the launch needs " + std::to_string(need_bytes));
    return reinterpret_cast<T *>(b.base + kGuard);
}

// changed guard bytes + changed rbufs; frees every buffer
inline size_t end_case() {
    size_t changed = 0;
    for (auto &kv : g_bufs) {
        GuardedBuf &b = kv.second;
        std::vector<char> h(b.bytes + 2 * kGuard);
        HIPCHK(hipMemcpy(h.data(), b.base, h.size(), hipMemcpyDeviceToHost));
        changed += changed_outside(h.data(), h.size(), kGuard, b.bytes, (char)kGuardFill);
        if (b.readonly) changed += memcmp(h.data() + kGuard, b.loaded.data(), b.bytes) != 0 ? 1 : 0;
        HIPCHK(hipFree(b.base));
    }
    g_bufs.clear();
    return changed;
}

// one line of ops.txt: the operation and its arguments
struct OpLine {
    std::string op;
    std::vector<std::string> a;
    const std::string &S(size_t i) const {
        if (i >= a.size()) die(op + ": too few arguments");
        return a[i];
    }
    long long I(size_t i) const { return atoll(S(i).c_str()); }
};

// main() of an op-list program: runs DIR/ops.txt on the current device and stops at the first HIP error (exit 1).  Owned here:
//   case ID                 begins a case
//   buf NAME BYTES FILE|-   a buffer the launches may write (FILE: DIR/FILE is loaded at its start; it may be shorter than BYTES)
//   rbuf NAME BYTES FILE    an input: at `end` every byte of it must still be what was loaded
//   load NAME FILE          DIR/FILE over the start of an existing buffer (an rbuf: the whole of it), nothing else touched
//   dump NAME FILE          the buffer's bytes (without guards) -> DIR/FILE
//   end                     "ID\t<changed guard bytes + changed rbufs>" -> DIR/results.txt; frees every buffer; then at_end()
// Every other line goes to launch(line), which returns false for an operation it does not know.
template <class Launch, class AtEnd>
int run_ops(int argc, char **argv, Launch &&launch, AtEnd &&at_end) {
    if (argc != 2) {
        fprintf(stderr, "usage: " CHECK_PROGRAM " DIR\n");
        return 1;
    }
    g_case_in_messages = true;
    g_dir = argv[1];
    FILE *ops = fopen((g_dir + "/ops.txt").c_str(), "r");
    if (!ops) die("cannot open " + g_dir + "/ops.txt");
    FILE *results = fopen((g_dir + "/results.txt").c_str(), "w");
    if (!results) die("cannot write " + g_dir + "/results.txt");
    char linebuf[1024];
    while (fgets(linebuf, sizeof(linebuf), ops)) {
        std::istringstream in(linebuf);
        OpLine l;
        if (!(in >> l.op)) continue;
        for (std::string t; in >> t;) l.a.push_back(t);
        if (l.op == "case") {
            g_case = l.S(0);
        } else if (l.op == "buf" || l.op == "rbuf") {
            make_buf(l.S(0), (size_t)l.I(1), l.S(2), l.op == "rbuf");
        } else if (l.op == "load") {
            load_buf(find_buf(l.S(0)), l.S(0), l.S(1));
        } else if (l.op == "dump") {
            const GuardedBuf &b = find_buf(l.S(0));
            std::vector<char> h(b.bytes);
            HIPCHK(hipMemcpy(h.data(), b.base + kGuard, h.size(), hipMemcpyDeviceToHost));
            write_file(g_dir + "/" + l.S(1), h.data(), h.size());
        } else if (l.op == "end") {
            fprintf(results, "%s\t%zu\n", g_case.c_str(), end_case());
            fflush(results);
            at_end();
        } else if (!launch(l)) {
            die("unknown operation " + l.op);
        }
    }
    fclose(ops);
    fclose(results);
    if (!g_bufs.empty()) die("ops.txt ends inside a case");
    return 0;
}

// ------------------------------------------------------------------------------------------------ margin buffers, driven by a case list
struct Case {
    std::string kind, id;
    int shape = 0, d = 0, F = 0, H = 0, C = 0, sc_stride = 0;
};

// DIR/cases.txt: "conv <id> <unit shape> <description> <F>" (or "conv_plain ..."), "input <id> <F>", "fc <id> <F>", "se <id> <H> <C> <F> <sc_stride>"
inline std::vector<Case> read_cases(const std::string &dir, int n_shapes, int n_desc, int max_F) {
    FILE *f = fopen((dir + "/cases.txt").c_str(), "r");
    if (!f) die("cannot open " + dir + "/cases.txt");
    std::vector<Case> cs;
    char kind[32], id[256];
    while (fscanf(f, "%31s %255s", kind, id) == 2) {
        Case c;
        c.kind = kind;
        c.id = id;
        bool ok = false;
        if (c.kind == "conv" || c.kind == "conv_plain")
            ok = fscanf(f, "%d %d %d", &c.shape, &c.d, &c.F) == 3 && c.shape >= 0 && c.shape < n_shapes && c.d >= 0 && c.d < n_desc;
        else if (c.kind == "input" || c.kind == "fc")
            ok = fscanf(f, "%d", &c.F) == 1;
        else if (c.kind == "se")
            ok = fscanf(f, "%d %d %d %d", &c.H, &c.C, &c.F, &c.sc_stride) == 4 && c.H >= 1 && c.H <= 56 && c.C >= 64 && c.C <= 512 && c.C % 64 == 0 &&
                 (size_t)c.H * c.H * c.C <= 56 * 56 * 64 && (c.sc_stride == 1 || c.sc_stride == 2);
        if (!ok || c.F < 1 || c.F > max_F) die("bad case line for " + c.id);
        cs.push_back(c);
    }
    fclose(f);
    return cs;
}

// `cap` elements (T = uint16_t: halves, uint32_t: floats / ints) between a front and a back margin, all filled with `fill`; the first `logical`
// elements behind the front margin are the tensor
template <class T>
struct MarginBuf {
    T *base = nullptr;
    size_t front = 0, back = 0, cap = 0, logical = 0;
    T fill = 0;
    size_t total() const { return front + cap + back; }
    template <class P>
    P *ptr() const { return reinterpret_cast<P *>(base + front); }
};

// the device memory of one case; margins in bytes, `unit` what the "does not fit" message calls an element
struct DeviceCase {
    const std::string id;
    const size_t front_bytes, back_bytes;
    const char *const unit;
    std::vector<void *> owned;
    DeviceCase(const std::string &id, size_t front_bytes, size_t back_bytes, const char *unit) : id(id), front_bytes(front_bytes), back_bytes(back_bytes), unit(unit) {
        g_where = "case " + id;
    }
    DeviceCase(const DeviceCase &) = delete;
    ~DeviceCase() {
        for (void *p : owned) (void)hipFree(p);
    }
    template <class T>
    void refill(const MarginBuf<T> &b) {
        static_assert(sizeof(T) == 2 || sizeof(T) == 4, "halves or words");
        if (sizeof(T) == 2)
            HIPCHK(hipMemsetD16(reinterpret_cast<hipDeviceptr_t>(b.base), (unsigned short)b.fill, b.total()));
        else
            HIPCHK(hipMemsetD32(reinterpret_cast<hipDeviceptr_t>(b.base), (int)b.fill, b.total()));
    }
    template <class T>
    MarginBuf<T> buf(size_t cap, size_t logical, T fill, const void *init) {
        if (logical > cap) die("case " + id + ": a tensor of " + std::to_string(logical) + " " + unit + " does not fit the product's buffer of " + std::to_string(cap));
        MarginBuf<T> b;
        b.front = front_bytes / sizeof(T);
        b.back = back_bytes / sizeof(T);
        b.cap = cap;
        b.logical = logical;
        b.fill = fill;
        HIPCHK(hipMalloc(reinterpret_cast<void **>(&b.base), b.total() * sizeof(T)));
        owned.push_back(b.base);
        refill(b);
        if (init) HIPCHK(hipMemcpy(b.base + b.front, init, logical * sizeof(T), hipMemcpyHostToDevice));
        return b;
    }
    template <class T>
    T *upload(const std::vector<T> &v) {
        T *d = nullptr;
        HIPCHK(hipMalloc(reinterpret_cast<void **>(&d), v.size() * sizeof(T)));
        owned.push_back(d);
        HIPCHK(hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
        return d;
    }
    template <class T>
    std::vector<T> fetch(const MarginBuf<T> &b) {  // margins and slack included
        std::vector<T> h(b.total());
        HIPCHK(hipMemcpy(h.data(), b.base, h.size() * sizeof(T), hipMemcpyDeviceToHost));
        return h;
    }
    // the logical tensor -> `path` (empty: not kept); returns the number of elements outside it, margins included, that no longer hold the fill pattern
    template <class T>
    size_t download(const MarginBuf<T> &b, const std::string &path, std::vector<T> *keep = nullptr) {
        const std::vector<T> h = fetch(b);
        if (!path.empty()) write_file(path, h.data() + b.front, b.logical * sizeof(T));
        if (keep) keep->assign(h.begin() + b.front, h.begin() + b.front + b.logical);
        return changed_outside(h.data(), h.size(), b.front, b.logical, b.fill);
    }
};

}  // namespace check
