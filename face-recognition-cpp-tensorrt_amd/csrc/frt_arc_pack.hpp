// Host-side weight packers of the recogniser: plain fp32 weights -> the fp16 layouts its kernels read (and, at the end, the fp32 mode's).
// Host only (no HIP call): used by frt_embedder::build() / build_f32() and, so that a packing bug shows against a reference that only ever
// sees plain weights, by the stand-alone launch harnesses (tests/cpp/arc_launch_check.cpp, tests/cpp/arc32_launch_check.cpp).
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "frt_weights.hpp"

namespace frt {

inline std::vector<uint16_t> conv_w_f16(const float *src, int cout, int cin, int ks) {
    // [Cout][Cin][kh][kw] fp32 -> [Cout][kh][kw][Cin] fp16 (K index = tap*Cin + ci)
    std::vector<uint16_t> w((size_t)cout * cin * ks * ks);
    for (int co = 0; co < cout; ++co)
        for (int ci = 0; ci < cin; ++ci)
            for (int t = 0; t < ks * ks; ++t) w[((size_t)co * ks * ks + t) * cin + ci] = f32_to_f16(src[((size_t)co * cin + ci) * ks * ks + t]);
    return w;
}
// 3x3 weights in the order the strip kernel's MFMA A fragments consume them: [Cout/32][Cin/64][tap][kk][lane = (k half, cout row)][8]
// (kernels_arc.hip: conv_patch_kernel); a wave's load of one fragment is then one contiguous kilobyte.  Empty unless Cin % 64 == 0.
// stride2: taps in the step order of the stride-2 strip kernel (kernels_arc_s2.hip: phase planes (odd,odd) (even,even) (odd,even) (even,odd)).
inline std::vector<uint16_t> conv_w_f16_frag(const float *src, int cout, int cin, bool stride2 = false) {
    if (cin % 64 || cout % 32) return {};
    static const int s2_step_of_tap[9] = {0, 5, 1, 7, 4, 8, 2, 6, 3};  // inverse of the step -> tap table 0,2,6,8,4,1,7,3,5
    std::vector<uint16_t> w((size_t)cout * cin * 9);
    const int nch = cin / 64;
    for (int co = 0; co < cout; ++co)
        for (int ci = 0; ci < cin; ++ci)
            for (int t = 0; t < 9; ++t) {
                const int blk = co >> 5, r = co & 31, ch = ci >> 6, kk = (ci & 63) >> 4, hi = (ci & 15) >> 3, e = ci & 7;
                const int st = stride2 ? s2_step_of_tap[t] : t;
                const size_t off = (((((size_t)blk * nch + ch) * 9 + st) * 4 + kk) * 64 + hi * 32 + r) * 8 + e;
                w[off] = f32_to_f16(src[((size_t)co * cin + ci) * 9 + t]);
            }
    return w;
}
// 1x1 shortcut weights [Cout][Cin] in the stride-2 strip kernel's fragment order [Cout/32][Cin/64][kk][lane = (k half, cout row)][8]
inline std::vector<uint16_t> conv1x1_w_f16_frag(const float *src, int cout, int cin) {
    if (cin % 64 || cout % 32) return {};
    std::vector<uint16_t> w((size_t)cout * cin);
    const int nch = cin / 64;
    for (int co = 0; co < cout; ++co)
        for (int ci = 0; ci < cin; ++ci) {
            const int blk = co >> 5, r = co & 31, ch = ci >> 6, kk = (ci & 63) >> 4, hi = (ci & 15) >> 3, e = ci & 7;
            w[(((((size_t)blk * nch + ch) * 4 + kk) * 64) + hi * 32 + r) * 8 + e] = f32_to_f16(src[(size_t)co * cin + ci]);
        }
    return w;
}
// input layer 3 -> 64, weights [64][27] (k = ci*9 + kh*3 + kw) with the folded BN (s0, b0) behind it, in the matrix-core layout of
// kernels_arc_input.hip: [64][32] fp16, k < 27: w * s0, k == 27: b0 (multiplies a constant 1), else 0
inline std::vector<uint16_t> arc_input_w_f16(const float *src, const float *s0, const float *b0) {
    std::vector<uint16_t> wh(64 * 32, 0);
    for (int co = 0; co < 64; ++co) {
        for (int k = 0; k < 27; ++k) wh[co * 32 + k] = f32_to_f16(src[co * 27 + k] * s0[co]);
        wh[co * 32 + 27] = f32_to_f16(b0[co]);
    }
    return wh;
}
// output Linear [512][25088] over the NCHW flatten (index c*49 + hw), re-ordered to NHWC (k = hw*512 + c) and packed in MFMA-fragment order
// for kernels_arc_fc.hip: [output block o / 32][k step k / 16][lane = (k half, o % 32)][8]
inline std::vector<uint16_t> fc_w_f16_frag(const float *src) {
    std::vector<uint16_t> w((size_t)512 * 25088);
    for (int o = 0; o < 512; ++o)
        for (int c = 0; c < 512; ++c)
            for (int hw = 0; hw < 49; ++hw) {
                const size_t k = (size_t)hw * 512 + c;
                const size_t off = ((((size_t)(o >> 5) * (25088 / 16) + (k >> 4)) * 64) + ((k >> 3) & 1) * 32 + (o & 31)) * 8 + (k & 7);
                w[off] = f32_to_f16(src[(size_t)o * 25088 + (size_t)c * 49 + hw]);
            }
    return w;
}

}  // namespace frt

// ---- the fp32 mode (kernels_arc_f32.hip; frt_embedder::build_f32() and tests/cpp/arc32_launch_check.cpp)
void pack_conv32_weights(const float *w, int cout, int taps, int cin, float *out);  // frt_kernels.h

namespace frt {

// [Cout][Cin][ks][ks] fp32 -> [Cout][tap][Cin] -> conv32_kernel's fragment order
inline std::vector<float> conv32_w_frag(const float *src, int cout, int cin, int ks) {
    const int taps = ks * ks;
    std::vector<float> w((size_t)cout * cin * taps);
    for (int co = 0; co < cout; ++co)
        for (int ci = 0; ci < cin; ++ci)
            for (int t = 0; t < taps; ++t) w[((size_t)co * taps + t) * cin + ci] = src[((size_t)co * cin + ci) * taps + t];
    std::vector<float> wf(w.size());
    pack_conv32_weights(w.data(), cout, taps, cin, wf.data());
    return wf;
}
// output Linear [512][25088] over the NCHW flatten (index c*49 + hw), re-ordered to NHWC (k = hw*512 + c) for fc32_kernel
inline std::vector<float> fc32_w_nhwc(const float *src) {
    std::vector<float> w((size_t)512 * 25088);
    for (int o = 0; o < 512; ++o)
        for (int c = 0; c < 512; ++c)
            for (int hw = 0; hw < 49; ++hw) w[(size_t)o * 25088 + (size_t)hw * 512 + c] = src[(size_t)o * 25088 + (size_t)c * 49 + hw];
    return w;
}

}  // namespace frt
