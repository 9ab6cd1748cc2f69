// The parts of the Slim and RFB detectors (the "Face-Detector-1MB" nets of conversion/retina/models/net_slim.py / net_rfb.py) that the
// mnet kernels do not cover: the depth_conv2d heads of levels 0-2, the dense 3x3 head of level 3, and RFB's conv8 (BasicRFB).  The
// conv_dw body blocks and conv14 run on the DwPwArgs kernels of kernels_det.hip.  fp32 NCHW like the rest of the detector.
//
// Every kernel is one thread per output pixel with all of its output channels in registers and the weights read as wave-uniform scalar
// loads: these layers have 8 - 88 output channels and are bound by their input / output bytes, not by arithmetic.
#include "frt_kernels.h"

#include <algorithm>

namespace {

// ---------------------------------------------------------------- heads of levels 0-2 (net_slim.py:64-76, depth_conv2d x 3)
// Per pixel and input channel: the 3x3 neighbourhood is read ONCE, feeds the three heads' depthwise taps (+ bias, ReLU), whose results
// feed the three heads' 1x1 convs.  Output channels: loc 4*3 | conf 2*3 | ldm 10*3 (zero weights beyond the level's na anchors, never
// stored).  Writes straight into [B][A][4 | 2 | 10] at the level's anchor base; conf is the softmax over the two classes.
template <bool LDM>
__global__ __launch_bounds__(256) void slim_heads_kernel(SlimHeadsArgs m) {
    constexpr int NO = LDM ? 48 : 18;
    const SlimHeadArgs &a = m.lv[blockIdx.z];
    const long gp = (long)blockIdx.x * 256 + threadIdx.x;
    const int HW = a.H * a.W;
    if (gp >= (long)m.B * HW) return;
    const int b = (int)(gp / HW), p = (int)(gp - (long)b * HW);
    const int y = p / a.W, x = p - y * a.W;
    int off[9];
    bool ok[9];
#pragma unroll
    for (int t = 0; t < 9; ++t) {
        const int ih = y - 1 + t / 3, iw = x - 1 + t % 3;
        ok[t] = ih >= 0 && ih < a.H && iw >= 0 && iw < a.W;
        off[t] = ok[t] ? ih * a.W + iw : 0;
    }
    float acc[NO];
#pragma unroll
    for (int o = 0; o < NO; ++o) acc[o] = 0.f;
    const float *inb = a.in + (long)b * a.C * HW;
    for (int ci = 0; ci < a.C; ++ci) {
        const float *xc = inb + (long)ci * HW;
        float v[9];
#pragma unroll
        for (int t = 0; t < 9; ++t) v[t] = ok[t] ? xc[off[t]] : 0.f;
        const float *wd = a.wd + ci * 30;  // [3 heads][9 taps + bias]
        float d[3];
#pragma unroll
        for (int h = 0; h < 3; ++h) {
            float s = wd[h * 10 + 9];
#pragma unroll
            for (int t = 0; t < 9; ++t) s = fmaf(v[t], wd[h * 10 + t], s);
            d[h] = fmaxf(s, 0.f);
        }
        const float *wp = a.wp + ci * 48;
#pragma unroll
        for (int o = 0; o < NO; ++o) acc[o] = fmaf(d[o < 12 ? 0 : (o < 18 ? 1 : 2)], wp[o], acc[o]);
    }
    const long an = (long)b * m.A + a.base + (long)p * a.na;
    for (int k = 0; k < a.na; ++k) {  // (na: 3 or 2 anchors per cell; uniform over the launch's level)
        floatx4 l;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float o = 0.f;
#pragma unroll
            for (int q = 0; q < 3; ++q)
                if (q == k) o = acc[q * 4 + j];
            l[j] = o + a.bp[k * 4 + j];
        }
        *reinterpret_cast<floatx4 *>(m.loc + (an + k) * 4) = l;
        float c0 = 0.f, c1 = 0.f;
#pragma unroll
        for (int q = 0; q < 3; ++q)
            if (q == k) {
                c0 = acc[12 + q * 2];
                c1 = acc[12 + q * 2 + 1];
            }
        c0 += a.bp[12 + k * 2];
        c1 += a.bp[12 + k * 2 + 1];
        const float mx = fmaxf(c0, c1);
        const float e0 = expf(c0 - mx), e1 = expf(c1 - mx);
        const float sum = e0 + e1;
        m.conf[(an + k) * 2] = e0 / sum;
        m.conf[(an + k) * 2 + 1] = e1 / sum;
        if (LDM) {
#pragma unroll
            for (int j = 0; j < 10; ++j) {
                float o = 0.f;
#pragma unroll
                for (int q = 0; q < 3; ++q)
                    if (q == k) o = acc[(18 + q * 10 + j) % NO];
                m.ldm[(an + k) * 10 + j] = o + a.bp[18 + k * 10 + j];
            }
        }
    }
}

// ---------------------------------------------------------------- level-3 head: dense 3x3 (pad 1) C -> na*(4 | 2 | 10) + bias
// Thread = (pixel, DH_G output channels); the channels are loc 4na | conf 2na | ldm 10na and a conf pair never straddles a group (4na is
// even and the groups start at even channels).  The level is tiny (10 x 10 at 640 x 640): 4 channels per thread give 12 workgroups per 256
// pixels; with 16 per thread the 32-frame launch was 39 workgroups (and spilled scalar registers on 144 uniform weights per channel).
constexpr int DH_G = 4;
__global__ __launch_bounds__(256) void dense_head_kernel(DenseHeadArgs a) {
    const long gp = (long)blockIdx.x * 256 + threadIdx.x;
    const int HW = a.H * a.W;
    if (gp >= (long)a.B * HW) return;
    const int b = (int)(gp / HW), p = (int)(gp - (long)b * HW);
    const int y = p / a.W, x = p - y * a.W;
    const int co0 = blockIdx.y * DH_G;
    int off[9];
    bool ok[9];
#pragma unroll
    for (int t = 0; t < 9; ++t) {
        const int ih = y - 1 + t / 3, iw = x - 1 + t % 3;
        ok[t] = ih >= 0 && ih < a.H && iw >= 0 && iw < a.W;
        off[t] = ok[t] ? ih * a.W + iw : 0;
    }
    float acc[DH_G];
#pragma unroll
    for (int c = 0; c < DH_G; ++c) acc[c] = 0.f;
    const float *inb = a.in + (long)b * a.C * HW;
    // (nine taps x two channels of loads in flight per step: one tap per step was a chain of dependent memory round trips, 903 us)
#pragma unroll 2
    for (int ci = 0; ci < a.C; ++ci) {
        const float *xc = inb + (long)ci * HW;
        const float *w = a.w + (long)ci * 9 * a.cpad + co0;
        float v[9];
#pragma unroll
        for (int t = 0; t < 9; ++t) v[t] = ok[t] ? xc[off[t]] : 0.f;
#pragma unroll
        for (int t = 0; t < 9; ++t)
#pragma unroll
            for (int c = 0; c < DH_G; ++c) acc[c] = fmaf(v[t], w[t * a.cpad + c], acc[c]);
    }
    const long an = (long)b * a.A + a.base + (long)p * a.na;
    const int nl = 4 * a.na, nc = 6 * a.na;  // (channels [0, nl): loc, [nl, nc): conf, beyond: ldm)
#pragma unroll
    for (int c = 0; c < DH_G; ++c) {
        const int co = co0 + c;
        if (co >= a.cout) break;
        const float o = acc[c] + a.b[co];
        if (co < nl) {
            a.loc[(an + co / 4) * 4 + (co & 3)] = o;
        } else if (co < nc) {
            if (c + 1 < DH_G && !(co & 1)) {
                const float o1 = acc[c + 1] + a.b[co + 1];
                const float mx = fmaxf(o, o1);
                const float e0 = expf(o - mx), e1 = expf(o1 - mx);
                const float sum = e0 + e1;
                const long q = an + (co - nl) / 2;
                a.conf[q * 2] = e0 / sum;
                a.conf[q * 2 + 1] = e1 / sum;
            }
        } else if (a.ldm) {
            const int r = co - nc;
            a.ldm[(an + r / 10) * 10 + r % 10] = o;
        }
    }
}

// ---------------------------------------------------------------- BasicRFB (net_rfb.py:31-78), 64 channels at H/8
// (1) the four 1x1 convs that read x - three branch reductions 64 -> 8 and the shortcut 64 -> 64, BN folded, no ReLU - in one pass over x
//     (the weights are staged in LDS and read as broadcasts: as wave-uniform scalar loads, 88 per input channel spilled scalar registers)
__global__ __launch_bounds__(256) void rfb_proj_kernel(RfbProjArgs a) {
    __shared__ float s_w[64 * 88];
    for (int i = threadIdx.x; i < 64 * 88; i += 256) s_w[i] = a.w[i];
    __syncthreads();
    const long gp = (long)blockIdx.x * 256 + threadIdx.x;
    const int HW = a.H * a.W;
    if (gp >= (long)a.B * HW) return;
    const int b = (int)(gp / HW), p = (int)(gp - (long)b * HW);
    float acc[88];
#pragma unroll
    for (int o = 0; o < 88; ++o) acc[o] = a.b[o];
    const float *xb = a.in + (long)b * 64 * HW + p;
#pragma unroll 4
    for (int ci = 0; ci < 64; ++ci) {
        const float v = xb[(long)ci * HW];
        const float *w = s_w + ci * 88;
#pragma unroll
        for (int o = 0; o < 88; ++o) acc[o] = fmaf(v, w[o], acc[o]);
    }
    float *rb = a.red + (long)b * 24 * HW + p;
#pragma unroll
    for (int o = 0; o < 24; ++o) rb[(long)o * HW] = acc[o];
    float *sb = a.sc + (long)b * 64 * HW + p;
#pragma unroll
    for (int o = 0; o < 64; ++o) sb[(long)o * HW] = acc[24 + o];
}

// (2) the branches' 3x3 convs, plain (dil 1) or dilated (dil = pad = 2, 3, 5): up to three problems per launch (blockIdx.z), <= 16
//     output channels each (weights padded to 16), BN folded, optional ReLU, each reading / writing a channel slice
__global__ __launch_bounds__(256) void rfb_conv_kernel(RfbConvMulti m) {
    const RfbConvArgs &a = m.p[blockIdx.z];
    __shared__ float s_w[16 * 9 * 16];  // (LDS: see rfb_proj_kernel)
    for (int i = threadIdx.x; i < a.Cin * 9 * 16; i += 256) s_w[i] = a.w[i];
    __syncthreads();
    const long gp = (long)blockIdx.x * 256 + threadIdx.x;
    const int HW = m.H * m.W;
    if (gp >= (long)m.B * HW) return;
    const int b = (int)(gp / HW), p = (int)(gp - (long)b * HW);
    const int y = p / m.W, x = p - y * m.W;
    int off[9];
    bool ok[9];
#pragma unroll
    for (int t = 0; t < 9; ++t) {
        const int ih = y + (t / 3 - 1) * a.dil, iw = x + (t % 3 - 1) * a.dil;
        ok[t] = ih >= 0 && ih < m.H && iw >= 0 && iw < m.W;
        off[t] = ok[t] ? ih * m.W + iw : 0;
    }
    float acc[16];
#pragma unroll
    for (int c = 0; c < 16; ++c) acc[c] = 0.f;
    const float *inb = a.in + ((long)b * a.in_ctotal + a.in_coff) * HW;
    for (int ci = 0; ci < a.Cin; ++ci) {
        const float *xc = inb + (long)ci * HW;
        const float *w = s_w + ci * 9 * 16;
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            const float v = ok[t] ? xc[off[t]] : 0.f;
#pragma unroll
            for (int c = 0; c < 16; ++c) acc[c] = fmaf(v, w[t * 16 + c], acc[c]);
        }
    }
    float *ob = a.out + ((long)b * a.out_ctotal + a.out_coff) * HW + p;
#pragma unroll
    for (int c = 0; c < 16; ++c) {
        if (c >= a.Cout) break;
        float o = acc[c] + a.b[c];
        if (a.relu) o = fmaxf(o, 0.f);
        ob[(long)c * HW] = o;
    }
}

// (3) tail: ConvLinear 48 -> 64 + BN, then  * scale + shortcut, then ReLU
__global__ __launch_bounds__(256) void rfb_tail_kernel(RfbTailArgs a) {
    __shared__ float s_w[48 * 64];  // (LDS: see rfb_proj_kernel)
    for (int i = threadIdx.x; i < 48 * 64; i += 256) s_w[i] = a.w[i];
    __syncthreads();
    const long gp = (long)blockIdx.x * 256 + threadIdx.x;
    const int HW = a.H * a.W;
    if (gp >= (long)a.B * HW) return;
    const int b = (int)(gp / HW), p = (int)(gp - (long)b * HW);
    float acc[64];
#pragma unroll
    for (int o = 0; o < 64; ++o) acc[o] = 0.f;
    const float *cb = a.cat + (long)b * 48 * HW + p;
#pragma unroll 4
    for (int ci = 0; ci < 48; ++ci) {
        const float v = cb[(long)ci * HW];
        const float *w = s_w + ci * 64;
#pragma unroll
        for (int o = 0; o < 64; ++o) acc[o] = fmaf(v, w[o], acc[o]);
    }
    const float *sb = a.sc + (long)b * 64 * HW + p;
    float *ob = a.out + (long)b * 64 * HW + p;
#pragma unroll
    for (int o = 0; o < 64; ++o) {
        const float y = (acc[o] + a.b[o]) * a.scale + sb[(long)o * HW];
        ob[(long)o * HW] = fmaxf(y, 0.f);
    }
}

inline unsigned blocks_of(long threads) { return (unsigned)((threads + 255) / 256); }

}  // namespace

void launch_slim_heads(const SlimHeadsArgs &a, int n, hipStream_t s) {
    long max_total = 0;
    for (int i = 0; i < n; ++i) max_total = std::max(max_total, (long)a.B * a.lv[i].H * a.lv[i].W);
    const dim3 grid(blocks_of(max_total), 1, n);
    if (a.ldm) hipLaunchKernelGGL(slim_heads_kernel<true>, grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL(slim_heads_kernel<false>, grid, dim3(256), 0, s, a);
}

void launch_dense_head(const DenseHeadArgs &a, hipStream_t s) {
    const dim3 grid(blocks_of((long)a.B * a.H * a.W), a.cpad / DH_G);
    hipLaunchKernelGGL(dense_head_kernel, grid, dim3(256), 0, s, a);
}

void launch_rfb_proj(const RfbProjArgs &a, hipStream_t s) {
    hipLaunchKernelGGL(rfb_proj_kernel, dim3(blocks_of((long)a.B * a.H * a.W)), dim3(256), 0, s, a);
}

void launch_rfb_conv(const RfbConvMulti &a, int n, hipStream_t s) {
    hipLaunchKernelGGL(rfb_conv_kernel, dim3(blocks_of((long)a.B * a.H * a.W), 1, n), dim3(256), 0, s, a);
}

void launch_rfb_tail(const RfbTailArgs &a, hipStream_t s) {
    hipLaunchKernelGGL(rfb_tail_kernel, dim3(blocks_of((long)a.B * a.H * a.W)), dim3(256), 0, s, a);
}
