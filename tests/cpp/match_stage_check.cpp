// Runs the stages of the matcher's screened search ONE AT A TIME (shadow build, coarse scan, k-th entry, pair selection, exact re-rank + unpack),
// or chained, through the launchers libfrt.so exports, on buffers whose every byte the test controls.  tests/match_stage_ref.py writes the case
// directory and holds the float64 references; tests/test_gpu_match_stages.py compares.  This program knows nothing about expected values.
//
//   match_stage_check DIR     run DIR/ops.txt on the current device; stops at the first HIP error (exit 1)
//
// DIR/ops.txt is a list of operations, one per line, on NAMED device buffers (read by run_ops, check_common.hpp, which owns case / buf / rbuf /
// load / dump / end; this file holds the launches and their size checks).  Every buffer is allocated with kGuard bytes in front and behind;
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

#define CHECK_PROGRAM "match_stage_check"
#include "check_common.hpp"
#include "frt_kernels.h"

using namespace check;

int main(int argc, char **argv) {
    ScreenScratch w{};
    float gerr = 0.f, gmax = 0.f;
    size_t n_tilemax = 0;  // what the scratch buffers hold, for the size checks below
    std::string names[7];
    auto launch = [&](const OpLine &l) -> bool {
        const std::string &op = l.op;
        auto I = [&](size_t i) { return l.I(i); };
        auto S = [&](size_t i) -> const std::string & { return l.S(i); };
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
        if (op == "shadow8") {
            const long long N = I(1);
            const size_t rows = tiles_of(N) * 128;
            launch_gallery_shadow8(ptr<float>(S(0), (size_t)N * 512 * 4), (int)N, 512, ptr<uint8_t>(S(2), rows * 512), ptr<float>(S(3), rows * 4), ptr<int>(S(4), 8),
                                   ptr<int>(S(4), 8) + 1, nullptr);
            sync_and_check();
        } else if (op == "shadow8_rows") {
            const long long row0 = I(1), n = I(2);
            if (row0 < 0 || n < 0) die("bad row range");
            const size_t rows = tiles_of(row0 + n) * 128;
            launch_gallery_shadow8_rows(ptr<float>(S(0), (size_t)n * 512 * 4), (int)row0, (int)n, ptr<uint8_t>(S(3), rows * 512), ptr<float>(S(4), rows * 4),
                                        ptr<int>(S(5), 8), ptr<int>(S(5), 8) + 1, nullptr);
            sync_and_check();
        } else if (op == "shadow16") {
            const long long N = I(1), D = I(2);
            if (D % 16) die("bad D");
            launch_gallery_shadow(ptr<float>(S(0), (size_t)N * D * 4), (int)N, (int)D, ptr<half_t>(S(3), gallery16_elems((int)N, (int)D) * 2), ptr<int>(S(4), 8) + 1, nullptr);
            sync_and_check();
        } else if (op == "norm16") {
            const long long row0 = I(1), n = I(2), D = I(3);
            if (row0 < 0 || n < 0 || D % 16) die("bad row range");
            launch_rows_norm<half_t>(ptr<half_t>(S(0), gallery16_elems((int)(row0 + n), (int)D) * 2), (int)row0, (int)n, (int)D, ptr<int>(S(4), 8) + 1, nullptr);
            sync_and_check();
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
            sync_and_check();
        } else if (op == "select_kth") {
            const long long N = I(0), D = I(1), F = I(3), K = I(4);
            need_scratch(N, F);
            if (K < 1 || K > match_topk_max()) die("select_kth: bad k");
            launch_match_select_kth((int)N, (int)D, ptr<float>(S(2), (size_t)F * D * 4), (int)F, (int)K, gmax, w, ptr<float>(S(5), (size_t)F * 4), I(6) != 0, nullptr);
            sync_and_check();
        } else if (op == "select_thr") {
            const long long N = I(0), D = I(1), F = I(3);
            need_scratch(N, F);
            launch_match_select_threshold((int)N, (int)D, ptr<float>(S(2), (size_t)F * D * 4), (int)F, from_bits(I(4)), (int)I(5), gmax, w, I(6) != 0, nullptr);
            sync_and_check();
        } else if (op == "screened") {
            const long long N = I(2), D = I(3), F = I(5), K = I(6), pb = I(9);
            need_scratch(N, F);
            if (K < 1 || K > match_topk_max() || pb < 1) die("screened: bad k");
            const size_t fb = (size_t)(pb < 128 ? pb : 128);
            launch_match_screened(ptr<float>(S(0), (size_t)N * D * 4), ptr<half_t>(S(1), gallery16_elems((int)N, (int)D) * 2), (int)N, (int)D,
                                  ptr<float>(S(4), (size_t)F * D * 4), (int)F, (int)K, gmax, w, ptr<float>(S(7), (size_t)F * 4),
                                  ptr<MatchPartial>(S(8), fb * F * sizeof(MatchPartial)), (int)pb, ptr<int32_t>(S(10), (size_t)F * K * 4), ptr<float>(S(11), (size_t)F * K * 4),
                                  (int)I(12), nullptr);
            sync_and_check();
        } else if (op == "rerank_excl") {
            const long long N = I(2), D = I(3), F = I(5), pb = I(7);
            need_scratch(N, F);
            const size_t fb = (size_t)(pb < 128 ? pb : 128);
            launch_match_top1_excluding(ptr<float>(S(0), (size_t)N * D * 4), ptr<half_t>(S(1), gallery16_elems((int)N, (int)D) * 2), (int)N, (int)D,
                                        ptr<float>(S(4), (size_t)F * D * 4), (int)F, true, w, ptr<MatchPartial>(S(6), fb * F * sizeof(MatchPartial)), (int)pb,
                                        ptr<int32_t>(S(8), (size_t)N * 4), ptr<int32_t>(S(9), (size_t)F * 4), ptr<int32_t>(S(10), (size_t)F * 4), ptr<float>(S(11), (size_t)F * 4),
                                        ptr<int>(S(12), 4), nullptr);
            sync_and_check();
        } else {
            return false;
        }
        return true;
    };
    return run_ops(argc, argv, launch, [&] { w = ScreenScratch{}; });
}
