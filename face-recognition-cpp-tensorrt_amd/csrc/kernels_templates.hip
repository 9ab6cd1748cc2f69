// Template gallery for gfx950: one row per identity, the re-normalised mean of that identity's rows (include/frt.h,
// frt_matcher_build_templates).
//
// One streaming pass over the stored rows, N * D * (4 | 2) bytes read and I * D * 4 written: HBM-bound.  One WAVE per identity:
//   - a row is D consecutive floats, lane l holds columns 4 l .. 4 l + 3 of every 256-column group: one fully coalesced 16-byte load per
//     lane and group (fp16-stored rows come through load_g4 in their fragment order: 8-byte loads, see the cost note in DESIGN §3.27);
//   - the loads of ROWS_IN_FLIGHT rows are issued before the first add, the adds then run in ascending row order - the order is part of
//     the definition, so no atomics and no tree over rows;
//   - one wave reduction gives ||s||^2; the template is scaled in registers and written once;
//   - the member dots <g, t> come from the registers the rows were loaded into while the identity has at most ROWS_IN_FLIGHT rows (and the
//     row fits one column chunk); a larger identity reads its rows a second time, which the L2 serves (they were read microseconds ago).
// Widths beyond 256 * NV columns are walked in chunks of that size with the unnormalised sum parked in the output row between the passes,
// so any width the matcher accepts works without a per-thread array that would have to live in scratch.
#include "frt_kernels.h"

namespace {

constexpr int ROWS_IN_FLIGHT = 4;

__device__ __forceinline__ float wave_sum(float v) {  // xor butterfly: every lane ends with the same bits
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}
__device__ __forceinline__ float dot4(floatx4 a, floatx4 b, float acc) { return fmaf(a[3], b[3], fmaf(a[2], b[2], fmaf(a[1], b[1], fmaf(a[0], b[0], acc)))); }

// group_off [I + 1], group_rows: local row indices, ascending inside an identity (frt_templates.hpp).  templates is read back by the lane
// that wrote it when the width takes more than one chunk, hence no __restrict__ on it.
template <typename GT, int NV>
__global__ __launch_bounds__(256) void template_build_kernel(const GT *__restrict__ G, int D, const int *__restrict__ group_off,
                                                             const int *__restrict__ group_rows, int I, int row_offset, float *templates,
                                                             float *__restrict__ min_sim, int32_t *__restrict__ min_row) {
    constexpr int R = ROWS_IN_FLIGHT, CW = 256 * NV;  // columns per chunk
    const int lane = threadIdx.x & 63;
    const int id = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
    if (id >= I) return;  // (wave-uniform; the kernel has no barrier)
    const int b = group_off[id], M = group_off[id + 1] - b;
    const int *my_rows = group_rows + b;
    const bool single = D <= CW;
    float *t_out = templates + (long)id * D;

    floatx4 v[R][NV];
    auto load_batch = [&](int j0, int c0) {  // rows j0 .. j0 + R - 1 of the identity, columns of chunk c0; zeros past either end
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const bool live = j0 + r < M;
            const long g = my_rows[live ? j0 + r : 0];
#pragma unroll
            for (int n = 0; n < NV; ++n) {
                const int k = c0 + n * 256 + lane * 4;
                v[r][n] = (live && k < D) ? load_g4(G, g, D, k) : floatx4{0.f, 0.f, 0.f, 0.f};
            }
        }
    };

    // ---- the sum, in ascending row order (0 + g_r1 is g_r1; the zeros of a short last batch change nothing), and its squared norm
    floatx4 acc[NV];
    float n2 = 0.f;
    for (int c0 = 0; c0 < D; c0 += CW) {
#pragma unroll
        for (int n = 0; n < NV; ++n) acc[n] = floatx4{0.f, 0.f, 0.f, 0.f};
        for (int j0 = 0; j0 < M; j0 += R) {
            load_batch(j0, c0);
#pragma unroll
            for (int r = 0; r < R; ++r)
#pragma unroll
                for (int n = 0; n < NV; ++n) acc[n] += v[r][n];
        }
#pragma unroll
        for (int n = 0; n < NV; ++n) {
            n2 = dot4(acc[n], acc[n], n2);
            const int k = c0 + n * 256 + lane * 4;
            if (!single && k < D) *reinterpret_cast<floatx4 *>(t_out + k) = acc[n];
        }
    }
    n2 = wave_sum(n2);
    const bool zero = n2 == 0.f;
    const float nrm = sqrtf(n2);
    auto scaled = [&](floatx4 s) { return zero ? floatx4{0.f, 0.f, 0.f, 0.f} : s / nrm; };

    // ---- the template
    floatx4 t[NV];
    for (int c0 = 0; c0 < D; c0 += CW) {
#pragma unroll
        for (int n = 0; n < NV; ++n) {
            const int k = c0 + n * 256 + lane * 4;
            if (!single && k < D) acc[n] = *reinterpret_cast<const floatx4 *>(t_out + k);
            t[n] = scaled(acc[n]);
            if (k < D) *reinterpret_cast<floatx4 *>(t_out + k) = t[n];
        }
    }

    // ---- the member that agrees least with it (rows ascend, so `<` keeps the lowest row among equals)
    float best = INFINITY;
    int best_row = my_rows[0];
    for (int j0 = 0; j0 < M; j0 += R) {
        float d[R];
#pragma unroll
        for (int r = 0; r < R; ++r) d[r] = 0.f;
        for (int c0 = 0; c0 < D; c0 += CW) {
            if (!single) {
#pragma unroll
                for (int n = 0; n < NV; ++n) {
                    const int k = c0 + n * 256 + lane * 4;
                    t[n] = k < D ? *reinterpret_cast<const floatx4 *>(t_out + k) : floatx4{0.f, 0.f, 0.f, 0.f};
                }
            }
            if (!single || M > R) load_batch(j0, c0);  // otherwise v still holds the identity's only batch
#pragma unroll
            for (int r = 0; r < R; ++r)
#pragma unroll
                for (int n = 0; n < NV; ++n) d[r] = dot4(v[r][n], t[n], d[r]);
        }
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const float s = wave_sum(d[r]);
            if (j0 + r < M && s < best) {
                best = s;
                best_row = my_rows[j0 + r];
            }
        }
    }
    if (lane == 0) {
        min_sim[id] = zero ? 0.f : best;
        min_row[id] = best_row + row_offset;
    }
}

}  // namespace

template <typename GT>
void launch_template_build(const GT *rows, int D, const int *group_off, const int *group_rows, int I, int row_offset, float *templates, float *min_sim,
                           int32_t *min_row, hipStream_t s) {
    if (I <= 0) return;
    const dim3 grid((unsigned)((I + 3) / 4)), block(256);  // 4 waves = 4 identities per workgroup
    if (D <= 256)
        hipLaunchKernelGGL((template_build_kernel<GT, 1>), grid, block, 0, s, rows, D, group_off, group_rows, I, row_offset, templates, min_sim, min_row);
    else
        hipLaunchKernelGGL((template_build_kernel<GT, 2>), grid, block, 0, s, rows, D, group_off, group_rows, I, row_offset, templates, min_sim, min_row);
}
template void launch_template_build(const float *, int, const int *, const int *, int, int, float *, float *, int32_t *, hipStream_t);
template void launch_template_build(const half_t *, int, const int *, const int *, int, int, float *, float *, int32_t *, hipStream_t);
