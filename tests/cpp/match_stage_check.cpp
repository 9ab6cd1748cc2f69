// Runs the stages of the matcher's screened search ONE AT A TIME (shadow build, coarse scan, k-th entry, pair selection, exact re-rank + unpack),
// or chained, through the launchers libfrt.so exports, on buffers whose every byte the test controls.  tests/match_stage_ref.py writes the case
// directory and holds the float64 references; tests/test_gpu_match_stages.py compares.  This program knows nothing about expected values.
//
//   match_stage_check DIR     run DIR/ops.txt on the current device; stops at the first HIP error (exit 1)
//
// DIR/ops.txt is a list of operations, one per line, on NAMED device buffers.  Every buffer is allocated with kGuard bytes in front and behind;
// the guards and every byte the case does not load are filled with the pattern 0x5a.  Numbers are decimal; floats travel as their 32-bit pattern
// (decimal) so that inf / NaN / exact values arrive unchanged; "-" is a null pointer.
//   case ID                            begins a case
//   buf NAME BYTES FILE|-              a buffer the stage may write (FILE: DIR/FILE is loaded at its start; it may be shorter than BYTES)
//   rbuf NAME BYTES FILE               an input: at `end` every byte of it must still be what was loaded
//   shadow8 GAL N G8 SCALE BITS        launch_gallery_shadow8 (D = 512); BITS: int[2] = max_err2_bits, max_norm2_bits
//   shadow8_rows ROWS ROW0 NROWS G8 SCALE BITS   launch_gallery_shadow8_rows
//   shadow16 GAL N D G16 BITS          launch_gallery_shadow (max_norm2_bits = BITS[1])
//   norm16 G16 ROW0 NROWS D BITS       launch_rows_norm<half_t> (-> BITS[1])
//   bounds BITS                        gerr = sqrt(BITS[0]), gmax_norm = sqrt(BITS[1]): what frt_matcher::read_bounds does
//   bounds_set GERR GMAX               the two as given bit patterns
//   scratch TILEMAX WGMAX PAIRS PAIR_CAP CTL QKEY G8|- SCALE|-     the ScreenScratch of the following launches (gerr: the current value)
//   coarse G16|- N D Q F               launch_match_coarse
//   select_kth N D Q F K KTH|- I8      launch_match_select_kth (K > 1 runs match_kth_kernel first)
//   select_thr N D Q F THR TILE_MIN I8 launch_match_select_threshold
//   screened GAL|- G16|- N D Q F K KTH|- PARTIAL PBLOCKS IDX SIM ROW_OFFSET      launch_match_screened
//   rerank_excl GAL|- G16|- N D Q F PARTIAL PBLOCKS LABELS EXCLUDED IDX SIM OVF  launch_match_top1_excluding(screened = true)
//   dump NAME FILE                     the buffer's bytes (without guards) -> DIR/FILE
//   end                                "ID\t<changed guard bytes + changed rbuf bytes>" -> DIR/results.txt; frees every buffer
// Every launch is followed by hipDeviceSynchronize and hipGetLastError.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <sstream>
#include <string>
#include <vector>

#include "frt_kernels.h"

namespace {

constexpr size_t kGuard = (size_t)64 << 10;
constexpr int kFill = 0x5a;

std::string g_case = "(none)";

[[noreturn]] void die(const std::string &msg) {
    fprintf(stderr, "match_stage_check: case %s: %s\n", g_case.c_str(), msg.c_str());
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

void make_buf(const std::string &name, size_t bytes, const std::string &file, bool readonly) {
    if (g_bufs.count(name)) die("buffer " + name + " exists");
    Buf b;
    b.bytes = bytes;
    b.readonly = readonly;
    HIPCHK(hipMalloc(reinterpret_cast<void **>(&b.base), bytes + 2 * kGuard));
    HIPCHK(hipMemset(b.base, kFill, bytes + 2 * kGuard));
    if (file != "-") {
        std::vector<char> v = read_all(g_dir + "/" + file);
        if (v.size() > bytes || (readonly && v.size() != bytes)) die(file + " does not fit buffer " + name);
        if (!v.empty()) HIPCHK(hipMemcpy(b.base + kGuard, v.data(), v.size(), hipMemcpyHostToDevice));
        if (readonly) b.loaded.swap(v);
    } else if (readonly) {
        die("rbuf " + name + " needs a file");
    }
    g_bufs[name] = std::move(b);
}

template <class T>
T *ptr(const std::string &name, size_t need_bytes = 0) {
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

float from_bits(unsigned long long u) {
    const uint32_t v = (uint32_t)u;
    float f;
    memcpy(&f, &v, 4);
    return f;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: match_stage_check DIR\n");
        return 1;
    }
    g_dir = argv[1];
    FILE *ops = fopen((g_dir + "/ops.txt").c_str(), "r");
    if (!ops) die("cannot open " + g_dir + "/ops.txt");
    FILE *results = fopen((g_dir + "/results.txt").c_str(), "w");
    if (!results) die("cannot write " + g_dir + "/results.txt");
    ScreenScratch w{};
    float gerr = 0.f, gmax = 0.f;
    size_t n_tilemax = 0;  // what the scratch buffers hold, for the size checks below
    std::string names[7];
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
        auto tiles_of = [](long long N) { return (size_t)((N + 127) / 128); };
        // the launches below write [F][tiles][4] coarse maxima, [256][F] workgroup maxima, F keys and the control words: the scratch must hold them
        auto need_scratch = [&](long long N, long long F) {
            n_tilemax = (size_t)F * tiles_of(N) * 4;
            (void)ptr<float>(names[0], n_tilemax * 4);
            (void)ptr<float>(names[1], (size_t)FRT_MATCH_COARSE_WG * F * 4);
            (void)ptr<char>(names[2], (size_t)w.pair_cap * sizeof(MatchPair));
            (void)ptr<int>(names[3], FRT_MATCH_CTL_WORDS * 4);
            (void)ptr<char>(names[4], (size_t)F * 8);
            if (w.pair_cap <= 0 || w.pair_cap % FRT_MATCH_SEL_SUB) die("pair_cap must be a positive multiple of the sub-list count");
        };
        if (op == "case") {
            g_case = S(0);
        } else if (op == "buf" || op == "rbuf") {
            make_buf(S(0), (size_t)I(1), S(2), op == "rbuf");
        } else if (op == "shadow8") {
            const long long N = I(1);
            const size_t rows = tiles_of(N) * 128;
            launch_gallery_shadow8(ptr<float>(S(0), (size_t)N * 512 * 4), (int)N, 512, ptr<uint8_t>(S(2), rows * 512), ptr<float>(S(3), rows * 4), ptr<int>(S(4), 8),
                                   ptr<int>(S(4), 8) + 1, nullptr);
            finish();
        } else if (op == "shadow8_rows") {
            const long long row0 = I(1), n = I(2);
            if (row0 < 0 || n < 0) die("bad row range");
            const size_t rows = tiles_of(row0 + n) * 128;
            launch_gallery_shadow8_rows(ptr<float>(S(0), (size_t)n * 512 * 4), (int)row0, (int)n, ptr<uint8_t>(S(3), rows * 512), ptr<float>(S(4), rows * 4),
                                        ptr<int>(S(5), 8), ptr<int>(S(5), 8) + 1, nullptr);
            finish();
        } else if (op == "shadow16") {
            const long long N = I(1), D = I(2);
            if (D % 16) die("bad D");
            launch_gallery_shadow(ptr<float>(S(0), (size_t)N * D * 4), (int)N, (int)D, ptr<half_t>(S(3), gallery16_elems((int)N, (int)D) * 2), ptr<int>(S(4), 8) + 1, nullptr);
            finish();
        } else if (op == "norm16") {
            const long long row0 = I(1), n = I(2), D = I(3);
            if (row0 < 0 || n < 0 || D % 16) die("bad row range");
            launch_rows_norm<half_t>(ptr<half_t>(S(0), gallery16_elems((int)(row0 + n), (int)D) * 2), (int)row0, (int)n, (int)D, ptr<int>(S(4), 8) + 1, nullptr);
            finish();
        } else if (op == "bounds") {
            int bits[2];
            HIPCHK(hipMemcpy(bits, ptr<int>(S(0), 8), 8, hipMemcpyDeviceToHost));
            gerr = std::sqrt(from_bits((uint32_t)bits[0]));
            gmax = std::sqrt(from_bits((uint32_t)bits[1]));
            w.gerr = gerr;
        } else if (op == "bounds_set") {
            gerr = from_bits(I(0));
            gmax = from_bits(I(1));
            w.gerr = gerr;
        } else if (op == "scratch") {
            for (int i = 0; i < 3; ++i) names[i] = S(i);
            names[3] = S(4);
            names[4] = S(5);
            names[5] = S(6);
            names[6] = S(7);
            w.tilemax = ptr<float>(S(0));
            w.wgmax = ptr<float>(S(1));
            w.pairs = ptr<void>(S(2));
            w.pair_cap = (int)I(3);
            w.ctl = ptr<int>(S(4));
            w.qkey = ptr<unsigned long long>(S(5));
            w.g8 = ptr<uint8_t>(S(6));
            w.g8_scale = ptr<float>(S(7));
            w.gerr = gerr;
        } else if (op == "coarse") {
            const long long N = I(1), D = I(2), F = I(4);
            if (!match_screen_supported((int)D) || tiles_of(N) < (size_t)FRT_MATCH_COARSE_WG || F < 1) die("coarse: unsupported shape");
            need_scratch(N, F);
            if (w.g8 && D == 512) {  // the int8 scan reads whole tiles of bytes and scales
                (void)ptr<uint8_t>(names[5], tiles_of(N) * 128 * 512);
                if (!ptr<float>(names[6], tiles_of(N) * 128 * 4)) die("coarse: an int8 shadow without scales");
            }
            const half_t *g16 = ptr<half_t>(S(0), gallery16_elems((int)N, (int)D) * 2);
            if (!g16 && !(w.g8 && D == 512)) die("coarse: no shadow to scan");
            launch_match_coarse(g16, (int)N, (int)D, ptr<float>(S(3), (size_t)F * D * 4), (int)F, w, nullptr);
            finish();
        } else if (op == "select_kth") {
            const long long N = I(0), D = I(1), F = I(3), K = I(4);
            need_scratch(N, F);
            if (K < 1 || K > match_topk_max()) die("select_kth: bad k");
            launch_match_select_kth((int)N, (int)D, ptr<float>(S(2), (size_t)F * D * 4), (int)F, (int)K, gmax, w, ptr<float>(S(5), (size_t)F * 4), I(6) != 0, nullptr);
            finish();
        } else if (op == "select_thr") {
            const long long N = I(0), D = I(1), F = I(3);
            need_scratch(N, F);
            launch_match_select_threshold((int)N, (int)D, ptr<float>(S(2), (size_t)F * D * 4), (int)F, from_bits(I(4)), (int)I(5), gmax, w, I(6) != 0, nullptr);
            finish();
        } else if (op == "screened") {
            const long long N = I(2), D = I(3), F = I(5), K = I(6), pb = I(9);
            need_scratch(N, F);
            if (K < 1 || K > match_topk_max() || pb < 1) die("screened: bad k");
            const size_t fb = (size_t)(pb < 128 ? pb : 128);
            launch_match_screened(ptr<float>(S(0), (size_t)N * D * 4), ptr<half_t>(S(1), gallery16_elems((int)N, (int)D) * 2), (int)N, (int)D,
                                  ptr<float>(S(4), (size_t)F * D * 4), (int)F, (int)K, gmax, w, ptr<float>(S(7), (size_t)F * 4),
                                  ptr<MatchPartial>(S(8), fb * F * sizeof(MatchPartial)), (int)pb, ptr<int32_t>(S(10), (size_t)F * K * 4), ptr<float>(S(11), (size_t)F * K * 4),
                                  (int)I(12), nullptr);
            finish();
        } else if (op == "rerank_excl") {
            const long long N = I(2), D = I(3), F = I(5), pb = I(7);
            need_scratch(N, F);
            const size_t fb = (size_t)(pb < 128 ? pb : 128);
            launch_match_top1_excluding(ptr<float>(S(0), (size_t)N * D * 4), ptr<half_t>(S(1), gallery16_elems((int)N, (int)D) * 2), (int)N, (int)D,
                                        ptr<float>(S(4), (size_t)F * D * 4), (int)F, true, w, ptr<MatchPartial>(S(6), fb * F * sizeof(MatchPartial)), (int)pb,
                                        ptr<int32_t>(S(8), (size_t)N * 4), ptr<int32_t>(S(9), (size_t)F * 4), ptr<int32_t>(S(10), (size_t)F * 4), ptr<float>(S(11), (size_t)F * 4),
                                        ptr<int>(S(12), 4), nullptr);
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
            w = ScreenScratch{};
        } else {
            die("unknown operation " + op);
        }
    }
    fclose(ops);
    fclose(results);
    if (!g_bufs.empty()) die("ops.txt ends inside a case");
    return 0;
}
