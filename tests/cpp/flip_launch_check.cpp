// Runs the two launches of the recogniser's flip mode (csrc/kernels_arc_flip.hip; frt_embedder::forward with flip on) ONE AT A TIME, outside any
// network, on named guarded buffers (run_ops, check_common.hpp: case / buf / rbuf / load / dump / end).  tests/test_gpu_flip_launches.py writes
// the op list and compares what is dumped with tests/flip_ref.py.  The launches:
//   pair_up IN OUT N                       launch_arc_flip_pair: IN fp32 [N][3][112][112] -> OUT [2N][3][112][112]
//   mirror IN OUT N                        launch_arc_flip_mirror: -> OUT [N][3][112][112]
//   finalize PARTIAL PAR VALID OUT N SPLITS  launch_fc_finalize_pair on one 2N-face pass: PARTIAL fp32 [SPLITS][2N][512], PAR [3][512] bias s b,
//                                          VALID int32 [N] -> OUT [N][512]
//   finalize2 PA PB PAR VALID OUT N SPLITS   ... on two N-face passes kept apart: PA, PB [SPLITS][N][512]
// Every buffer must hold exactly what its launch reads or writes (checked here, before the launch), so a write past 2N faces or N rows lands in
// a guard and is counted at `end`.
#define CHECK_PROGRAM "flip_launch_check"
#include "check_common.hpp"

#include "frt_kernels.h"

using namespace check;

namespace {

constexpr size_t kFace = (size_t)3 * 112 * 112 * sizeof(float);

// the buffer's start; it must hold exactly `bytes`
template <class T>
T *exact(const std::string &name, size_t bytes) {
    if (find_buf(name).bytes != bytes) die("buffer " + name + " holds " + std::to_string(find_buf(name).bytes) + " bytes, the launch covers " + std::to_string(bytes));
    return ptr<T>(name, bytes);
}

}  // namespace

int main(int argc, char **argv) {
    auto launch = [&](const OpLine &l) -> bool {
        if (l.op == "pair_up" || l.op == "mirror") {
            const long long n = l.I(2);
            if (n < 1 || n > 64) die("bad face count");
            const float *in = exact<float>(l.S(0), (size_t)n * kFace);
            if (l.op == "pair_up") launch_arc_flip_pair(in, exact<float>(l.S(1), 2 * (size_t)n * kFace), (int)n, nullptr);
            else launch_arc_flip_mirror(in, exact<float>(l.S(1), (size_t)n * kFace), (int)n, nullptr);
            sync_and_check();
        } else if (l.op == "finalize" || l.op == "finalize2") {
            const bool two = l.op == "finalize2";
            const size_t o = two ? 1 : 0;
            const long long n = l.I(4 + o), splits = l.I(5 + o);
            if (n < 1 || n > 64 || splits < 1 || splits > 49) die("bad finalize shape");
            const size_t rows = two ? (size_t)n : 2 * (size_t)n, pbytes = (size_t)splits * rows * 512 * sizeof(float);
            const float *pa = exact<float>(l.S(0), pbytes);
            const float *pb = two ? exact<float>(l.S(1), pbytes) : pa + (size_t)n * 512;
            const float *par = exact<float>(l.S(1 + o), 3 * 512 * sizeof(float));
            const int *valid = exact<int>(l.S(2 + o), (size_t)n * sizeof(int));
            float *out = exact<float>(l.S(3 + o), (size_t)n * 512 * sizeof(float));
            launch_fc_finalize_pair(pa, pb, (int)splits, (int)rows, (int)n, par, par + 512, par + 1024, valid, out, nullptr);
            sync_and_check();
        } else {
            return false;
        }
        return true;
    };
    return run_ops(argc, argv, launch, [] {});
}
