// Face quality for gfx950: one record of integer sums, three float32 values and the gate's flags per u8 BGR 112x112 crop (include/frt.h
// "Face quality"; tests/quality_ref.py is the contract, to the byte).
//
// face_quality_kernel, one workgroup of four waves per face slot:
//   - an absent slot (records given, valid == 0) leaves 14 zero dwords and never touches its crop: the test is uniform over the workgroup;
//   - the crop's 37 632 bytes come in as 2352 16-byte loads: a thread takes 48 consecutive bytes - 16 pixels, three loads - per turn,
//     784 turns in all, a thread's twelve loads issued together - and leaves their 16 luma bytes in LDS with one 16-byte store (12 544
//     bytes);
//   - behind ONE barrier a thread walks the luma plane a dword - four pixels of one row - at a time (3136 dwords, 28 per row): the dword
//     itself, the ones above and below and the two neighbouring bytes give the four Laplacians; the six sums and the two counts stay in
//     32-bit registers (a thread sees at most 52 pixels: 52 * 1020^2 < 2^26), sum_lap2 widens to 64 bits for the reduction;
//   - xor butterflies over the wave, one LDS row per wave, a second barrier, and thread 0 adds the four rows, derives mean / luma_var /
//     sharpness - the exact integer numerator, ONE float64 division, one rounding to float32 - and the flags, and stores the record.
// Integer sums: the order of the reduction cannot change a bit.  No atomics, no scratch.  This file is compiled without fp contraction
// (Makefile: EXACT), though there is nothing to contract: every float is a division or a comparison.
// Bounds: a slot is blockIdx.x < n; a turn is clamped to 783, so its bytes end at 784 * 48 = 37 632; a luma dword is < 3136 and its vertical
// neighbours are read for rows 1 .. 110 only, the bytes left and right of it only inside its row.
#include "frt_kernels.h"

namespace {

constexpr int Q_THREADS = 256, Q_WAVES = Q_THREADS / 64;
constexpr int Q_SIDE = 112, Q_PIX = Q_SIDE * Q_SIDE, Q_INNER = (Q_SIDE - 2) * (Q_SIDE - 2);  // N = 12544, M = 12100
constexpr int Q_TURNS = Q_PIX / 16, Q_DWORDS = Q_PIX / 4, Q_ROW_DWORDS = Q_SIDE / 4;       // 784, 3136, 28
constexpr int Q_TURNS_PER_THREAD = (Q_TURNS + Q_THREADS - 1) / Q_THREADS;                   // 4: three whole rounds and 16 turns of a fourth
static_assert(Q_TURNS * 48 == Q_PIX * 3 && Q_ROW_DWORDS * 4 == Q_SIDE, "a crop is whole turns and a row whole dwords");
static_assert(sizeof(struct frt_face_quality) == 56 && offsetof(struct frt_face_quality, sum_lap2) == 24 && offsetof(struct frt_face_quality, present) == 52,
              "frt_face_quality is 14 dwords as include/frt.h states them");

__device__ __forceinline__ unsigned luma(unsigned b, unsigned g, unsigned r) { return (29u * b + 150u * g + 77u * r + 128u) >> 8; }
__device__ __forceinline__ unsigned byte_of(const unsigned (&w)[12], int i) {  // byte i of 48, i a compile-time constant after unrolling
    return (w[i >> 2] >> ((i & 3) * 8)) & 255u;
}
__device__ __forceinline__ unsigned wave_sum_u32(unsigned v) {  // xor butterfly: every lane ends with the sum
    for (int off = 32; off > 0; off >>= 1) v += (unsigned)__shfl_xor((int)v, off);
    return v;
}
__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned lo = __shfl_xor((unsigned)v, off), hi = __shfl_xor((unsigned)(v >> 32), off);
        v += ((unsigned long long)hi << 32) | lo;
    }
    return v;
}

__global__ __launch_bounds__(Q_THREADS) void face_quality_kernel(const uint8_t *__restrict__ crops, const frt_face_result *__restrict__ results, int n,
                                                                 frt_quality_options opt, struct frt_face_quality *__restrict__ out) {
    __shared__ __attribute__((aligned(16))) uint8_t s_y[Q_PIX];
    __shared__ unsigned s_part[Q_WAVES][8];
    const int slot = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (slot >= n) return;
    int valid = 1, size = 0;
    float score = 0.f;
    if (results) {
        const frt_face_result r = results[slot];
        valid = r.valid;
        const int dx = r.box.x2 - r.box.x1, dy = r.box.y2 - r.box.y1;
        size = dx < dy ? dx : dy;
        score = r.box.score;
    }
    if (valid == 0) {  // (the same in every thread)
        if (tid < (int)(sizeof(struct frt_face_quality) / 4)) reinterpret_cast<unsigned *>(out + slot)[tid] = 0u;
        return;
    }

    const uint4 *__restrict__ src = reinterpret_cast<const uint4 *>(crops + (size_t)slot * (Q_PIX * 3));
    uint4 *s_y16 = reinterpret_cast<uint4 *>(s_y);
    // all of a thread's loads first, so that they are in flight together: a turn past the end (the last 240 threads' fourth) loads the last
    // turn's bytes again - in bounds, a cache hit - and stores nothing
    uint4 in[Q_TURNS_PER_THREAD][3];
#pragma unroll
    for (int i = 0; i < Q_TURNS_PER_THREAD; ++i) {
        const int t = tid + i * Q_THREADS < Q_TURNS ? tid + i * Q_THREADS : Q_TURNS - 1;
#pragma unroll
        for (int j = 0; j < 3; ++j) in[i][j] = src[3 * t + j];
    }
#pragma unroll
    for (int i = 0; i < Q_TURNS_PER_THREAD; ++i) {
        const int t = tid + i * Q_THREADS;
        if (t >= Q_TURNS) break;
        const uint4 a = in[i][0], b = in[i][1], c = in[i][2];
        const unsigned v[12] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x, c.y, c.z, c.w};
        unsigned y[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int p = 0; p < 16; ++p) y[p >> 2] |= luma(byte_of(v, 3 * p), byte_of(v, 3 * p + 1), byte_of(v, 3 * p + 2)) << ((p & 3) * 8);
        s_y16[t] = make_uint4(y[0], y[1], y[2], y[3]);
    }
    __syncthreads();

    const unsigned *s_y32 = reinterpret_cast<const unsigned *>(s_y);
    unsigned sum_y = 0u, sum_y2 = 0u, n_dark = 0u, n_bright = 0u, lap2 = 0u;
    int sum_lap = 0;
    for (int q = tid; q < Q_DWORDS; q += Q_THREADS) {
        const int row = q / Q_ROW_DWORDS, cq = q - row * Q_ROW_DWORDS;
        const unsigned c = s_y32[q];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const unsigned y = (c >> (8 * k)) & 255u;
            sum_y += y;
            sum_y2 += y * y;
            n_dark += y < 32u ? 1u : 0u;
            n_bright += y > 223u ? 1u : 0u;
        }
        if (row >= 1 && row <= Q_SIDE - 2) {
            const unsigned up = s_y32[q - Q_ROW_DWORDS], dn = s_y32[q + Q_ROW_DWORDS];
            const int left = cq > 0 ? (int)s_y[4 * q - 1] : 0, right = cq < Q_ROW_DWORDS - 1 ? (int)s_y[4 * q + 4] : 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int col = 4 * cq + k;
                if (col >= 1 && col <= Q_SIDE - 2) {
                    const int y = (int)((c >> (8 * k)) & 255u), u = (int)((up >> (8 * k)) & 255u), d = (int)((dn >> (8 * k)) & 255u);
                    const int l = k > 0 ? (int)((c >> (8 * (k - 1))) & 255u) : left;
                    const int r = k < 3 ? (int)((c >> ((8 * (k + 1)) & 31)) & 255u) : right;
                    const int L = 4 * y - u - d - l - r;
                    sum_lap += L;
                    lap2 += (unsigned)(L * L);
                }
            }
        }
    }
    sum_y = wave_sum_u32(sum_y);
    sum_y2 = wave_sum_u32(sum_y2);
    n_dark = wave_sum_u32(n_dark);
    n_bright = wave_sum_u32(n_bright);
    sum_lap = (int)wave_sum_u32((unsigned)sum_lap);  // (two's complement: the wrapped sum of the parts is the sum)
    const unsigned long long lap2w = wave_sum_u64((unsigned long long)lap2);
    if (lane == 0) {
        s_part[wave][0] = sum_y;
        s_part[wave][1] = sum_y2;
        s_part[wave][2] = (unsigned)sum_lap;
        s_part[wave][3] = n_dark;
        s_part[wave][4] = n_bright;
        s_part[wave][5] = (unsigned)lap2w;
        s_part[wave][6] = (unsigned)(lap2w >> 32);
    }
    __syncthreads();
    if (tid != 0) return;

    struct frt_face_quality o;
    o.sum_y = o.sum_y2 = o.n_dark = o.n_bright = 0u;
    o.sum_lap = 0;
    o.sum_lap2 = 0ull;
#pragma unroll
    for (int w = 0; w < Q_WAVES; ++w) {
        o.sum_y += s_part[w][0];
        o.sum_y2 += s_part[w][1];
        o.sum_lap += (int)s_part[w][2];
        o.n_dark += s_part[w][3];
        o.n_bright += s_part[w][4];
        o.sum_lap2 += ((unsigned long long)s_part[w][6] << 32) | s_part[w][5];
    }
    o.size = size;
    o.score = score;
    // exact integer numerators (N * sum_y2 <= 1.03e13, M * sum_lap2 <= 1.6e14), one IEEE division each, one rounding to float32
    const long long N = Q_PIX, M = Q_INNER;
    const long long var_num = N * (long long)o.sum_y2 - (long long)o.sum_y * (long long)o.sum_y;
    const long long lap_num = M * (long long)o.sum_lap2 - (long long)o.sum_lap * (long long)o.sum_lap;
    o.mean = (float)((double)o.sum_y / (double)N);
    o.luma_var = (float)((double)var_num / (double)(N * N));
    o.sharpness = (float)((double)lap_num / (double)(M * M));
    unsigned flags = 0u;
    if (results) {
        if (size < opt.min_size) flags |= FRT_QUALITY_SMALL;
        if (score < opt.min_score) flags |= FRT_QUALITY_LOW_SCORE;
    }
    if (o.sharpness < opt.min_sharpness) flags |= FRT_QUALITY_BLURRED;
    if (o.luma_var < opt.min_luma_var) flags |= FRT_QUALITY_FLAT;
    if (o.mean < opt.min_mean) flags |= FRT_QUALITY_DARK;
    if (o.mean > opt.max_mean) flags |= FRT_QUALITY_BRIGHT;
    if (o.n_dark + o.n_bright > (unsigned)opt.max_clipped) flags |= FRT_QUALITY_CLIPPED;
    o.flags = flags;
    o.present = 1;
    out[slot] = o;
}

}  // namespace

void launch_face_quality(const uint8_t *crops, const frt_face_result *results, int n, const frt_quality_options &opt, struct frt_face_quality *out,
                         hipStream_t s) {
    if (n < 1) return;
    hipLaunchKernelGGL(face_quality_kernel, dim3(n), dim3(Q_THREADS), 0, s, crops, results, n, opt, out);
}
