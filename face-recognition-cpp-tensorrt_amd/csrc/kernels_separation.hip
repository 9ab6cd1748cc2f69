// Leave-one-out genuine / impostor scores of a labelled gallery (frt_matcher_separation) for gfx950: the genuine side and the
// reduction.  The impostor side is the label-excluded top-1 search of kernels_match.hip (launch_match_top1_excluding), one call per chunk
// of 128 stored rows used as queries.
//
// Genuine side.  For row i the candidates are the other rows of its own identity; S(i, j) is evaluated by exact_row_dot (frt_kernels.h),
// the chain of the pair re-rank, so it has the bits of the exact scan.  ONE WAVE per query row, rows taken in the order of the identity ->
// rows grouping (group_rows): the wave stages its query row in LDS once (2 KB at D = 512, every lane then reads the same address: a
// broadcast, no bank conflict), and walks the identity's members in blocks of 64, lane = one member = one dependent D-term chain.  An
// identity of n rows is therefore spread over n waves of ceil(n / 64) blocks each - no workgroup owns an identity, nothing is buffered per
// identity, and no atomic is needed because a row's winner is decided inside its own wave.  The work is latency-bound (one chain per pair),
// so what counts is waves in flight: the 16 row loads per thread that exact_row_dot keeps in flight cost 96 VGPRs with fp32 rows and 118
// with fp16 rows (5 / 4 waves per SIMD); the 8 KB of LDS per workgroup at 512 columns are far from limiting.
#include <limits.h>

#include "frt_kernels.h"

namespace {

__device__ __forceinline__ bool better(float v, int i, float bv, int bi) { return (v > bv) || (v == bv && i < bi); }

// group_off [I + 1], group_rows [N]: frt_templates.hpp (rows ascend inside an identity); pos_ident [N]: the identity of position p of group_rows
template <typename GT>
__global__ __launch_bounds__(256) void separation_genuine_kernel(const GT *__restrict__ G, int N, int D, const int *__restrict__ group_off,
                                                                 const int *__restrict__ group_rows, const int *__restrict__ pos_ident,
                                                                 float *__restrict__ gen_sim, int32_t *__restrict__ gen_row) {
    extern __shared__ __attribute__((aligned(16))) char smem_s[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float *qs = reinterpret_cast<float *>(smem_s) + (size_t)wave * D;  // this wave's query row
    for (long base = (long)blockIdx.x * 4; base < N; base += (long)gridDim.x * 4) {  // (block-uniform trip count: the barriers below)
        const long p = base + wave;
        int i = -1, b0 = 0, n = 0;
        __syncthreads();  // the previous row's readers of qs are done
        if (p < N) {
            i = group_rows[p];
            const int id = pos_ident[p];
            b0 = group_off[id];
            n = group_off[id + 1] - b0;
            for (int k = lane * 4; k < D; k += 256) *reinterpret_cast<floatx4 *>(qs + k) = load_g4(G, (long)i, D, k);
        }
        __syncthreads();
        if (p >= N) continue;  // (no barrier behind this point in the iteration)
        float v = -INFINITY;
        int r = INT_MAX;
        for (int m0 = 0; m0 < n; m0 += 64) {
            const int mj = m0 + lane;
            if (mj < n && b0 + mj != p) {  // a member of the identity other than the query itself
                const int j = group_rows[b0 + mj];
                const float sim = exact_row_dot(G, (long)j, D, qs);
                if (sim == sim && better(sim, j, v, r)) {  // a NaN similarity is no candidate
                    v = sim;
                    r = j;
                }
            }
        }
        for (int off = 32; off > 0; off >>= 1) {
            const float ov = __shfl_xor(v, off);
            const int oi = __shfl_xor(r, off);
            if (better(ov, oi, v, r)) {
                v = ov;
                r = oi;
            }
        }
        if (lane == 0) {
            gen_sim[i] = v;
            gen_row[i] = r == INT_MAX ? -1 : r;
        }
    }
}

struct SepThresholds {
    float t[FRT_SEPARATION_MAX_THRESHOLDS];
};

// stats[0..2] and counts [nt][2] from the four arrays: ballots -> per-workgroup sums in LDS -> one 64-bit atomic per counter and workgroup.
// Workgroup 0 also turns the chunks' overflow flags into stats[3] / stats[4].  stats and counts are zero when the kernel starts.
__global__ __launch_bounds__(256) void separation_reduce_kernel(const float *__restrict__ gen_sim, const int32_t *__restrict__ gen_row,
                                                                const float *__restrict__ imp_sim, const int32_t *__restrict__ imp_row, int N,
                                                                SepThresholds thr, int nt, const int *__restrict__ chunk_overflow, int chunks, int screened,
                                                                unsigned long long *__restrict__ counts, unsigned long long *__restrict__ stats) {
    __shared__ unsigned part[4 + 2 * FRT_SEPARATION_MAX_THRESHOLDS];  // [0..2] stats, [3] overflowed chunks, [4 + 2 k + side] counts
    const int tid = threadIdx.x, lane = tid & 63;
    for (int c = tid; c < 4 + 2 * FRT_SEPARATION_MAX_THRESHOLDS; c += 256) part[c] = 0u;
    __syncthreads();
    auto count = [&](bool hit, int slot) {
        const unsigned long long bal = __ballot(hit);
        if (bal && lane == 0) atomicAdd(&part[slot], (unsigned)__popcll(bal));
    };
    for (long base = (long)blockIdx.x * 256; base < N; base += (long)gridDim.x * 256) {  // (whole waves reach the ballots)
        const long i = base + tid;
        bool hg = false, hi = false;
        float gs = 0.f, is = 0.f;
        if (i < N) {
            hg = gen_row[i] >= 0;
            hi = imp_row[i] >= 0;
            gs = gen_sim[i];
            is = imp_sim[i];
        }
        count(hg, 0);
        count(hi, 1);
        count(hg && hi && is >= gs, 2);
        for (int k = 0; k < nt; ++k) {
            count(hg && gs < thr.t[k], 4 + 2 * k);
            count(hi && is >= thr.t[k], 5 + 2 * k);
        }
    }
    if (blockIdx.x == 0 && screened)
        for (int c0 = 0; c0 < chunks; c0 += 256) count(c0 + tid < chunks && chunk_overflow[c0 + tid] != 0, 3);
    __syncthreads();
    if (tid < 3 && part[tid]) atomicAdd(&stats[tid], (unsigned long long)part[tid]);
    if (tid >= 4 && tid < 4 + 2 * nt && part[tid]) atomicAdd(&counts[tid - 4], (unsigned long long)part[tid]);
    if (blockIdx.x == 0 && tid == 0) {
        const unsigned exact = screened ? part[3] : (unsigned)chunks;
        stats[3] = (unsigned long long)chunks - exact;
        stats[4] = exact;
    }
}

}  // namespace

template <typename GT>
void launch_separation_genuine(const GT *rows, int N, int D, const int *group_off, const int *group_rows, const int *pos_ident, float *gen_sim,
                               int32_t *gen_row, hipStream_t s) {
    if (N <= 0) return;
    const long blocks = ((long)N + 3) / 4;
    const size_t lds = (size_t)4 * D * sizeof(float);
    if (lds > 65536) (void)hipFuncSetAttribute(reinterpret_cast<const void *>(&separation_genuine_kernel<GT>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL((separation_genuine_kernel<GT>), dim3((unsigned)(blocks < 16384 ? blocks : 16384)), dim3(256), lds, s, rows, N, D,
                       group_off, group_rows, pos_ident, gen_sim, gen_row);
}
template void launch_separation_genuine(const float *, int, int, const int *, const int *, const int *, float *, int32_t *, hipStream_t);
template void launch_separation_genuine(const half_t *, int, int, const int *, const int *, const int *, float *, int32_t *, hipStream_t);

void launch_separation_reduce(const float *gen_sim, const int32_t *gen_row, const float *imp_sim, const int32_t *imp_row, int N, const float *thresholds,
                              int n_thresholds, const int *chunk_overflow, int chunks, bool screened, long long *counts, long long *stats, hipStream_t s) {
    SepThresholds thr = {};
    for (int k = 0; k < n_thresholds; ++k) thr.t[k] = thresholds[k];
    (void)hipMemsetAsync(stats, 0, 5 * sizeof(long long), s);
    if (n_thresholds > 0) (void)hipMemsetAsync(counts, 0, (size_t)n_thresholds * 2 * sizeof(long long), s);
    const long blocks = ((long)N + 255) / 256;
    hipLaunchKernelGGL(separation_reduce_kernel, dim3((unsigned)(blocks < 1024 ? (blocks > 0 ? blocks : 1) : 1024)), dim3(256), 0, s, gen_sim, gen_row, imp_sim,
                       imp_row, N, thr, n_thresholds, chunk_overflow, chunks, screened ? 1 : 0, reinterpret_cast<unsigned long long *>(counts),
                       reinterpret_cast<unsigned long long *>(stats));
}
