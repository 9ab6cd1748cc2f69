// Runs the launchers of the matcher's EXACT fp32 scan (match_kernel + match_reduce_kernel in every instantiation) and the two device merges ONE AT A
// TIME, through what libfrt.so exports, on buffers whose every byte the test controls.  tests/match_exact_ref.py writes the case directory and
// holds the references (the fma chain restated in NumPy, float64, the ranking); tests/test_gpu_match_exact.py compares.  This program knows nothing
// about expected values.
//
//   match_exact_check DIR     run DIR/ops.txt on the current device; stops at the first HIP error (exit 1)
//
// DIR/ops.txt: operations on NAMED guarded device buffers (run_ops, check_common.hpp, owns case / buf / rbuf / load / dump / end; this file holds
// the launches and their size checks).  GAL G16: exactly one of the two is a buffer, the other "-": fp32 row-major rows [N][D], or the
// fragment-ordered fp16 rows padded to whole 128-row tiles - the launcher's own rule for the row type.
//   top1 GAL G16 N D Q F PARTIAL PBLOCKS IDX SIM ROW_OFFSET                              launch_match_top1
//   full GAL G16 N D Q F OUT                                                             launch_match_full (sizes its own grid)
//   topk GAL G16 N D Q F K PARTIAL PBLOCKS IDX SIM ROW_OFFSET                            launch_match_topk(screen = false)
//   topk_labels GAL G16 N D Q F K PARTIAL PBLOCKS LABELS CTL LAB IDX SIM ROW_OFFSET      launch_match_topk_labels(kth_count = 0); CTL: the control words
//   top1_excl GAL G16 N D Q F PARTIAL PBLOCKS LABELS EXCLUDED CTL IDX SIM OVF            launch_match_top1_excluding(screened = false)
//   merge IDX_ALL SIM_ALL SHARDS N K IDX SIM                                             launch_merge_topk
//   merge_labels LAB_ALL IDX_ALL SIM_ALL SHARDS N K LAB IDX SIM                          launch_merge_topk_labels
// Every launch is followed by hipDeviceSynchronize and hipGetLastError.
#define CHECK_PROGRAM "match_exact_check"
#include "check_common.hpp"
#include "frt_kernels.h"

using namespace check;

int main(int argc, char **argv) {
    auto launch = [&](const OpLine &l) -> bool {
        const std::string &op = l.op;
        auto I = [&](size_t i) { return l.I(i); };
        auto S = [&](size_t i) -> const std::string & { return l.S(i); };
        // the shape every scan shares: arguments 0 - 5 = GAL G16 N D Q F
        struct Scan {
            const float *gal;
            const half_t *g16;
            const float *q;
            int N, D, F;
        };
        auto scan = [&]() {
            const long long N = I(2), D = I(3), F = I(5);
            if (N < 1 || N > (1 << 24) || D < 32 || D > 4096 || D % 32 || F < 1 || F > 4096) die(op + ": unsupported shape");
            Scan c{ptr<float>(S(0), (size_t)N * D * 4), ptr<half_t>(S(1), gallery16_elems((int)N, (int)D) * 2), ptr<float>(S(4), (size_t)F * D * 4), (int)N, (int)D, (int)F};
            if (!c.gal == !c.g16 || !c.q) die(op + ": exactly one of the fp32 rows and the fp16 rows, and the queries");
            return c;
        };
        auto B = [&](size_t i) -> const std::string & {  // every buffer but GAL / G16 must exist
            if (S(i) == "-") die(op + ": argument " + std::to_string(i) + " must be a buffer");
            return S(i);
        };
        auto blocks = [&](size_t i) {
            const long long pb = I(i);
            if (pb < 1 || pb > 4096) die(op + ": bad partial_blocks");
            return (int)pb;
        };
        auto topk_k = [&](size_t i) {
            const long long k = I(i);
            if (k < 1 || k > match_topk_max()) die(op + ": bad k");
            return (int)k;
        };
        if (op == "top1") {
            const Scan c = scan();
            const int pb = blocks(7);
            MatchPartial *partial = ptr<MatchPartial>(B(6), (size_t)pb * c.F * sizeof(MatchPartial));
            int32_t *idx = ptr<int32_t>(B(8), (size_t)c.F * 4);
            float *sim = ptr<float>(B(9), (size_t)c.F * 4);
            if (c.gal) launch_match_top1(c.gal, c.N, c.D, c.q, c.F, partial, pb, idx, sim, (int)I(10), nullptr);
            else launch_match_top1(c.g16, c.N, c.D, c.q, c.F, partial, pb, idx, sim, (int)I(10), nullptr);
            sync_and_check();
        } else if (op == "full") {
            const Scan c = scan();
            float *out = ptr<float>(B(6), (size_t)c.F * c.N * 4);
            if (c.gal) launch_match_full(c.gal, c.N, c.D, c.q, c.F, out, nullptr);
            else launch_match_full(c.g16, c.N, c.D, c.q, c.F, out, nullptr);
            sync_and_check();
        } else if (op == "topk") {
            const Scan c = scan();
            const int k = topk_k(6), pb = blocks(8);
            launch_match_topk(c.gal, c.g16, c.N, c.D, c.q, c.F, k, false, 0.f, ScreenScratch{}, nullptr, ptr<MatchPartial>(B(7), (size_t)pb * c.F * sizeof(MatchPartial)), pb,
                              ptr<int32_t>(B(9), (size_t)c.F * k * 4), ptr<float>(B(10), (size_t)c.F * k * 4), (int)I(11), nullptr);
            sync_and_check();
        } else if (op == "topk_labels") {
            const Scan c = scan();
            const int k = topk_k(6), pb = blocks(8);
            ScreenScratch w{};
            w.ctl = ptr<int>(B(10), FRT_MATCH_CTL_WORDS * 4);  // the launcher forms w.ctl + FRT_MATCH_CTL_OVERFLOW; no kernel of an unscreened call reads it
            launch_match_topk_labels(c.gal, c.g16, c.N, c.D, c.q, c.F, k, 0, 0.f, w, nullptr, ptr<MatchPartial>(B(7), (size_t)pb * c.F * sizeof(MatchPartial)), pb,
                                     ptr<int32_t>(B(9), (size_t)c.N * 4), ptr<int32_t>(B(11), (size_t)c.F * k * 4), ptr<int32_t>(B(12), (size_t)c.F * k * 4),
                                     ptr<float>(B(13), (size_t)c.F * k * 4), (int)I(14), nullptr);
            sync_and_check();
        } else if (op == "top1_excl") {
            const Scan c = scan();
            const int pb = blocks(7);
            ScreenScratch w{};
            w.ctl = ptr<int>(B(10), FRT_MATCH_CTL_WORDS * 4);
            launch_match_top1_excluding(c.gal, c.g16, c.N, c.D, c.q, c.F, false, w, ptr<MatchPartial>(B(6), (size_t)pb * c.F * sizeof(MatchPartial)), pb,
                                        ptr<int32_t>(B(8), (size_t)c.N * 4), ptr<int32_t>(B(9), (size_t)c.F * 4), ptr<int32_t>(B(11), (size_t)c.F * 4),
                                        ptr<float>(B(12), (size_t)c.F * 4), ptr<int>(B(13), 4), nullptr);
            sync_and_check();
        } else if (op == "merge" || op == "merge_labels") {
            const size_t o = op == "merge" ? 0 : 1;  // merge_labels carries a label buffer in front of each group
            const long long shards = I(o + 2), n = I(o + 3);
            if (shards < 1 || shards > 64 || n < 1 || n > (1 << 20)) die(op + ": unsupported shape");
            const int k = topk_k(o + 4);
            const size_t in_bytes = (size_t)shards * n * k * 4, out_bytes = (size_t)n * k * 4;
            if (op == "merge")
                launch_merge_topk(ptr<int32_t>(B(0), in_bytes), ptr<float>(B(1), in_bytes), (int)shards, (int)n, k, ptr<int32_t>(B(5), out_bytes), ptr<float>(B(6), out_bytes),
                                  nullptr);
            else
                launch_merge_topk_labels(ptr<int32_t>(B(0), in_bytes), ptr<int32_t>(B(1), in_bytes), ptr<float>(B(2), in_bytes), (int)shards, (int)n, k,
                                         ptr<int32_t>(B(6), out_bytes), ptr<int32_t>(B(7), out_bytes), ptr<float>(B(8), out_bytes), nullptr);
            sync_and_check();
        } else {
            return false;
        }
        return true;
    };
    return run_ops(argc, argv, launch, [] {});
}
