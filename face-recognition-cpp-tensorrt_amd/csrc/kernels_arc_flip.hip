// Recogniser, flip-augmented embeddings (frt_embedder_set_flip): out = normalize(pre(x) + pre(mirror x)), pre = BN1d(Linear(...)) before the
// L2 normalisation.  Two kernels around the unchanged network:
//   * pair-up: n faces [n][3][112][112] -> a 2n-face network input, faces 0 .. n-1 the originals, n .. 2n-1 the same images with the W axis
//     reversed.  Pure data movement, bit-exact; 16-byte accesses on both sides (a 112-float row is 28 float4: the mirrored store reverses the
//     float4 order and the lane order);
//   * pair finalize: the Linear's slice sums of the 2n-face pass -> for face f the two pre-normalisation vectors of rows f and n + f, each summed
//     in slice order exactly as fc_finalize_kernel does (kernels_arc.hip), their sum, L2 normalised.
#include "frt_kernels.h"

namespace {

constexpr int ROW4 = 112 / 4;            // float4 per image row
constexpr long FACE4 = 3L * 112 * ROW4;  // float4 per face

// One thread per float4 of the input.  orig (may be null: the caller runs the originals from where they are) and mirror are [n] faces each.
__global__ __launch_bounds__(256) void arc_flip_pair_kernel(const float4 *__restrict__ in, float4 *__restrict__ orig, float4 *__restrict__ mirror, long total4) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total4) return;
    const float4 v = in[i];
    if (orig) orig[i] = v;
    const long row = i / ROW4;
    const int q = (int)(i - row * ROW4);
    mirror[row * ROW4 + (ROW4 - 1 - q)] = make_float4(v.w, v.z, v.y, v.x);
}

// partial_a / partial_b: [splits][rows][512] slice sums, addressed at row f: the originals' and the mirror images' (one 2n-face pass: the same
// array, n rows apart; two one-face passes: two arrays).  One workgroup per output face; splits == 49 keeps all 2 x 49 loads in flight before
// the adds (128 blocks cannot hide a dependent load chain).
__global__ __launch_bounds__(512) void fc_finalize_pair_kernel(const float *__restrict__ partial_a, const float *__restrict__ partial_b, int splits, int rows,
                                                               const float *__restrict__ bias, const float *__restrict__ s, const float *__restrict__ b,
                                                               const int *__restrict__ valid, float *__restrict__ out) {
    const int f = blockIdx.x, o = threadIdx.x;
    float va = 0.f, vb = 0.f;
    if (splits == 49) {
        float ta[49], tb[49];
#pragma unroll
        for (int k = 0; k < 49; ++k) {
            ta[k] = partial_a[((long)k * rows + f) * 512 + o];
            tb[k] = partial_b[((long)k * rows + f) * 512 + o];
        }
#pragma unroll
        for (int k = 0; k < 49; ++k) va += ta[k];
#pragma unroll
        for (int k = 0; k < 49; ++k) vb += tb[k];
    } else {
        for (int k = 0; k < splits; ++k) {
            va += partial_a[((long)k * rows + f) * 512 + o];
            vb += partial_b[((long)k * rows + f) * 512 + o];
        }
    }
    va = (va + bias[o]) * s[o] + b[o];
    vb = (vb + bias[o]) * s[o] + b[o];
    const float v = va + vb;
    float sq = v * v;
    for (int off = 32; off > 0; off >>= 1) sq += __shfl_xor(sq, off);
    __shared__ float red[8];
    if ((o & 63) == 0) red[o >> 6] = sq;
    __syncthreads();
    float tot = 0.f;
#pragma unroll
    for (int w = 0; w < 8; ++w) tot += red[w];
    const float nrm = fmaxf(sqrtf(tot), 1e-12f);
    const bool ok = valid == nullptr || valid[f] != 0;
    out[(long)f * 512 + o] = ok ? v / nrm : 0.f;
}

void flip_launch(const float *in, float *orig, float *mirror, int n, hipStream_t s) {
    if (n < 1) return;
    const long total4 = (long)n * FACE4;
    hipLaunchKernelGGL(arc_flip_pair_kernel, dim3((unsigned)((total4 + 255) / 256)), dim3(256), 0, s, reinterpret_cast<const float4 *>(in),
                       reinterpret_cast<float4 *>(orig), reinterpret_cast<float4 *>(mirror), total4);
}

}  // namespace

void launch_arc_flip_pair(const float *chw, float *pair, int n, hipStream_t s) { flip_launch(chw, pair, pair + (size_t)n * 3 * 112 * 112, n, s); }

void launch_arc_flip_mirror(const float *chw, float *mirror, int n, hipStream_t s) { flip_launch(chw, nullptr, mirror, n, s); }

void launch_fc_finalize_pair(const float *partial_a, const float *partial_b, int splits, int rows, int n, const float *bias, const float *s, const float *b,
                             const int *valid, float *out, hipStream_t st) {
    if (n < 1) return;
    hipLaunchKernelGGL(fc_finalize_pair_kernel, dim3(n), dim3(512), 0, st, partial_a, partial_b, splits, rows, bias, s, b, valid, out);
}
