// ArcFace IR-50 stage 1: conv3x3 64 -> 64, stride 1, pad 1 at 112x112 / 56x56 (model_irse.py:58-66 inside units 0-2), fp16 NHWC.
//
// These five layers are 17 % of the network's FLOPs but took 22 % of its time: with only 64 output channels a B (pixel) fragment
// feeds two MFMAs, the generic strip kernel needs a 69 KB patch per strip (one workgroup per CU, 4 waves) and - having a single
// K chunk - runs patch load, MFMA loop and epilogue strictly one after the other: PMC showed the matrix pipe 12.5 % busy and
// the LDS 12 % busy, i.e. a latency-bound kernel.  This kernel is built for exactly this shape:
//   * persistent 2-wave workgroups (wave = one 32-cout block); the wave's whole weight slice [32 cout][576 k] lives in 144
//     VGPRs for the lifetime of the kernel - no weight traffic at all after the first microsecond;
//   * a work item is a strip of 2 image rows x 56 columns (112 pixels = 3.5 MFMA pixel tiles, 4 accumulators): its halo patch
//     (4 x 58 pixels x 144-byte rows) is 34 KB, double-buffered in LDS -> two workgroups per CU; the NEXT strip's patch is
//     DMA'd global -> LDS (global_load_lds, 17 instructions per wave), one instruction per step of the first K loop, so
//     staging costs no VGPRs and no burst in front of the MFMAs;
//   * the strip's four pixel tiles are two halves with a K loop each (36 steps of 2 MFMAs on the same 144 weight registers:
//     a single accumulation chain of this MFMA issues back to back, the four tiles need not advance together).  While half 1
//     accumulates, half 0 of the same strip drains - the epilogue below, cut into operations of a few instructions that are
//     dealt into the gaps behind the MFMAs; while half 0 of the NEXT strip accumulates, half 1 drains.  No second accumulator
//     set: 32 of the 64 accumulator registers accumulate, 32 drain; after the last strip one half drains alone;
//   * per (tap, 16-channel step) one A fragment from registers and two ds_read_b128 B fragments, prefetched four steps ahead
//     through a 5-deep register ring that runs through both halves; every B address is one per-tile base register plus an immediate;
//   * epilogue through a wave-private fp32 LDS tile: the lane-owns-a-pixel accumulator becomes 64-byte NHWC half-rows, the
//     per-channel parameters a lane needs (8 channels) sit in registers; same arithmetic and rounding points as the generic
//     epilogue (fp32 BN / PReLU / shortcut add, one rounding to fp16 per output);
//   * one wave per SIMD, so nothing hides a wait: the hand-over between strips is a counted vmcnt (this wave's DMAs, not the
//     drain's stores behind them) and a bare s_barrier.
// At 128 faces the 112x112 launch now moves its 410 MB at 3.1 TB/s (0.86 of what conv_s2c64_kernel reaches on the same tensors)
// and runs its MFMAs at 0.68 of the sustained peak: it is bound by the patch traffic with ONE patch in flight per workgroup -
// all that 160 KB of LDS hold at two workgroups per CU - not by LDS read bandwidth.
#include <cstdlib>
#include <type_traits>

#include "frt_kernels.h"

namespace {

constexpr int SW = 56;                 // strip width (pixels)
constexpr int PW = SW + 2;             // patch width
constexpr int PROWB = 144;             // bytes per patch pixel (128 data + 16 pad: conflict-free ds_read_b128)
constexpr int NDMA = (4 * PW * 9 + 127) / 128;  // LDS-DMA instructions per wave per patch (2088 16-byte slots / 2 waves / 64 lanes) = 17
constexpr int PATCH_B = NDMA * 2 * 1024;        // 34816: whole DMA slots
constexpr int RING = 5;                // B-fragment register ring: fragments are requested RING-1 steps (64 clk each) ahead
constexpr int EROW = 36;               // floats per pixel row of the epilogue tile (32 + 4 pad)
constexpr int STEPS = 36;              // (tap, 16-channel step) pairs of one half
constexpr int GAPS = 2 * STEPS;        // MFMAs of one half: the gaps the other half's drain is dealt into

// f(integral_constant<int, I>) for I = LO .. HI - 1: a loop whose index is a constant expression in its body
template <int LO, int HI, class F>
__device__ __forceinline__ void static_for(F &&f) {
    if constexpr (LO < HI) {
        f(std::integral_constant<int, LO>{});
        static_for<LO + 1, HI>(f);
    }
}

// Drain of one half (pixel tiles 2h, 2h + 1) as a list of small operations, dealt evenly over the MFMA gaps of the other half's K loop:
//   4 tile-writes of tile 2h, 2 read-backs, 4 tile-writes of tile 2h + 1, 2 read-backs (the LDS is in order, so the second tile may be
//   written as soon as the first one's read-backs are issued), then per live (tile, pixel group): one operation per channel (two in the
//   shortcut-add form: y, then z) and one for the stores.  (tile 3, group 1) is pixels 112..127 of a 112-pixel strip: never drained.
template <int MODE>
struct DrainOps {
    static constexpr int PER = (MODE == EPI_BN_ADD_BN ? 16 : 8) + 1;
    static constexpr int count(int h) { return 12 + (h == 0 ? 4 : 3) * PER; }
};

template <int MODE>
__global__ __launch_bounds__(128) void conv64_kernel(ConvMfmaArgs p, int n_strips) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char *patch = smem;                                           // [2][PATCH_B]
    float *etile = reinterpret_cast<float *>(smem + 2 * PATCH_B); // [2 waves][32][EROW]
    const int tid = threadIdx.x, lane = tid & 63, cb = tid >> 6;
    const int r = lane & 31, hi = lane >> 5;
    const int H = p.H, W = p.W;
    const int strips_x = W / SW, strips_per_img = (H / 2) * strips_x;

    // ---- persistent strip walk: XCD-contiguous full rounds, remainder dealt round-robin over the XCDs
    const int nwg = gridDim.x;
    const int bq = nwg >> 3, brem = nwg & 7;
    const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
    const int wid = (xcd < brem ? xcd * (bq + 1) : brem * (bq + 1) + (xcd - brem) * bq) + slot;
    const int k_full = n_strips / nwg, rem_strips = n_strips - k_full * nwg;
    auto strip_of = [&](int k) {
        if (k < k_full) return wid + k * nwg;
        return (k == k_full && (int)blockIdx.x < rem_strips) ? k_full * nwg + (int)blockIdx.x : n_strips;
    };

    // ---- weights: lane (cout cb*32 + r, half hi) holds k = tap*64 + kk*16 + 8*hi .. +7 for every (tap, kk)
    half8 wreg[9][4];
    {
        const half_t *wrow = p.w + (long)(cb * 32 + r) * 576 + 8 * hi;
#pragma unroll
        for (int tap = 0; tap < 9; ++tap)
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) wreg[tap][kk] = *reinterpret_cast<const half8 *>(wrow + tap * 64 + kk * 16);
    }
    // ---- epilogue parameters of this lane's 8 channels (after the transpose a lane always handles the same channel octet)
    const int ec0 = cb * 32 + (lane & 3) * 8;
    float q0[8], q1[8], q2[8], q3[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        q0[e] = p.p0[ec0 + e];
        q1[e] = MODE == EPI_PRELU ? 0.f : p.p1[ec0 + e];
        q2[e] = (MODE == EPI_BN_ADD_BN && p.out1) ? p.p2[ec0 + e] : 1.f;
        q3[e] = (MODE == EPI_BN_ADD_BN && p.out1) ? p.p3[ec0 + e] : -0.f;
    }
    // the second output of the shortcut-add form is optional: without it the second store repeats the first one (z = y * 1 + -0 is y
    // bit for bit, signed zeros included; same place), so that every strip issues the same number of stores and the counted wait below holds
    half_t *const out1 = (MODE == EPI_BN_ADD_BN && p.out1) ? p.out1 : p.out0;

    // ---- B fragment bases: tile t, lane pixel q = 32 t + r (q >= 112: dead slot, clamped to pixel 0)
    int bbase[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int q = 32 * t + r;
        const int qq = q < 2 * SW ? q : 0;
        const int row = qq / SW, col = qq - row * SW;
        bbase[t] = (row * PW + col) * PROWB + hi * 16;
    }
    // ---- output / shortcut offsets of the drain, in halves from the strip's first pixel: after the transpose lane l handles pixel
    //      32 t + 16 i + (l >> 2) of the strip and its channel octet.  Only (tile 1, group 1) - pixels 48..63 - straddles the two rows.
    const int lane_off = (lane >> 2) * 64 + ec0;
    const int lane_off11 = lane_off + ((lane >> 2) >= SW - 48 ? (W - SW) * 64 : 0);
    // (one scalar base per tensor and strip, the group's part of the offset added per lane: a base per group would hold 28 scalar registers)
    auto group_off = [&](int h, int j, int i) __attribute__((always_inline)) {
        const int q0s = 64 * h + 32 * j + 16 * i;  // first pixel of the group; row 1 from pixel 56 on
        return (unsigned)(((h == 0 && j == 1 && i == 1) ? lane_off11 : lane_off) + (q0s + (q0s >= SW ? W - SW : 0)) * 64);
    };

    // ---- patch staging by LDS-DMA (global_load_lds: no VGPR round trip, no ds_write, completion counted by vmcnt).  The DMA
    //      writes wave-base + lane*16, so the patch image is slot-linear: slot = pixel*9 + part (part 8 = the 16-byte pad, fed
    //      from the zero buffer like every out-of-image pixel).  Wave w issues DMA q for slots (2q + w)*64 + lane.  Everything
    //      that does not depend on the strip is precomputed: rel = offset inside the strip's window, need = which borders the
    //      slot's pixel touches (bit0 top halo row, bit1 bottom halo row, bit2 left halo column, bit3 right, bit4 always zero,
    //      bit5 every slot: set in `edge` when there is no next strip, so that the same 17 DMAs are issued - all from the zero buffer).
    unsigned prel[NDMA];
#pragma unroll
    for (int q = 0; q < NDMA; ++q) {
        const int slot = (2 * q + cb) * 64 + lane;
        const int pix = slot / 9, part = slot - pix * 9;
        const int pr = pix / PW, pc = pix - pr * PW;
        const bool dead = part == 8 || pix >= 4 * PW;
        const unsigned need = 32u | (dead ? 16u : ((pr == 0 ? 1u : 0u) | (pr == 3 ? 2u : 0u) | (pc == 0 ? 4u : 0u) | (pc == PW - 1 ? 8u : 0u)));
        const unsigned rel = dead ? 0u : (unsigned)((pr * W + pc) * 128 + part * 16);  // bytes, relative to (y0, x0)
        prel[q] = rel | (need << 26);
    }
    // a strip's decode, once per strip and wave-uniform: its first pixel, its window (one row up, one pixel left: may point before the
    // image, only used with rel of valid pixels) and the borders its window crosses
    struct Strip {
        long pix0;
        const char *win;
        unsigned edge;
    };
    auto decode = [&](int strip, bool valid) __attribute__((always_inline)) {
        const int b = strip / strips_per_img, rem = strip - b * strips_per_img;
        const int sy = rem / strips_x, sx = rem - sy * strips_x;
        const int y0 = sy * 2 - 1, x0 = sx * SW - 1;
        Strip s;
        s.pix0 = (long)b * H * W + (long)(sy * 2) * W + sx * SW;
        s.win = reinterpret_cast<const char *>(p.x + (s.pix0 - W - 1) * 64);
        s.edge = 16u | (valid ? 0u : 32u) | (y0 < 0 ? 1u : 0u) | (y0 + 3 >= H ? 2u : 0u) | (x0 < 0 ? 4u : 0u) | (x0 + PW - 1 >= W ? 8u : 0u);
        return s;
    };
    // DMA q in two parts, so that the loop can put them into different gaps: the lanes' source addresses, then the instruction.  It is
    // issued from inline assembly on purpose: behind the builtin the compiler treats every later wait for an LDS read or a load as a
    // wait for everything (lgkmcnt(0) / vmcnt(0)), which would empty the B ring's prefetch all through the steps that issue DMAs.
    // Its completion is therefore waited for by hand (the counted vmcnt at the hand-over below).  The statement sets M0 (the DMA's LDS
    // base), which nothing else in this kernel reads: gfx950's LDS instructions do not use it.
    const unsigned patch_lds = (unsigned)(size_t)(__attribute__((address_space(3))) char *)patch + __builtin_amdgcn_readfirstlane(cb) * 1024;
    auto dma_src = [&](int q, const Strip &s) __attribute__((always_inline)) {
        const bool live = ((prel[q] >> 26) & s.edge) == 0;
        return live ? s.win + (prel[q] & 0x3ffffffu) : reinterpret_cast<const char *>(p.zeros);
    };
    auto dma_issue = [&](int q, const char *src, int buf) __attribute__((always_inline)) {
        asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off" ::"s"(patch_lds + buf * PATCH_B + q * 2048), "v"(src) : "memory");
    };

    int k = 0;
    if (strip_of(0) >= n_strips) return;
    Strip cs = decode(strip_of(0), true), ns = cs;  // the strip being accumulated, the next one
    long prev_pix0 = 0;                             // the strip whose second half is still in its accumulators
    bool has_next = false;
#pragma unroll
    for (int q = 0; q < NDMA; ++q) dma_issue(q, dma_src(q, cs), 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    int cur = 0;

    float *et = etile + cb * 32 * EROW;
    floatx16 acc[2][2];      // [half][tile of the half]: one half accumulates while the other drains
    half8 scv[2][2][2];      // shortcut values [half][tile][pixel group], requested one half-loop ahead of their drain
    floatx4 vb[2][2][2];     // read-backs of the transposed tiles [tile][pixel group][channel quad]
    half8 oy, oz;            // the outputs of the (tile, pixel group) being converted

    // operation n of the drain of half h (accumulators a, strip at pix0), in the order DrainOps describes; h and n are types, so that
    // what a gap holds is decided while the code is instantiated
    auto drain_op = [&](auto hc, auto nc, floatx16 (&a)[2], long pix0) __attribute__((always_inline)) {
        constexpr int h = decltype(hc)::value, n = decltype(nc)::value, PER = DrainOps<MODE>::PER;
        if constexpr (n < 12) {
            constexpr int j = n / 6, w = n % 6;
            if constexpr (w < 4) {
                // lane (r, hi) owns pixel r of the tile and channels (e&3) + 8*(e>>2) + 4*hi of this wave's 32
                floatx4 v = {a[j][4 * w], a[j][4 * w + 1], a[j][4 * w + 2], a[j][4 * w + 3]};
                *reinterpret_cast<floatx4 *>(et + r * EROW + 8 * w + 4 * hi) = v;
            } else {
                // read back as 128 octets (32 pixels x 4), two per lane: lane -> pixel (lane >> 2) + 16 i, channel octet lane & 3
                constexpr int i = w - 4;
                const int px = (lane >> 2) + 16 * i;
                vb[j][i][0] = *reinterpret_cast<const floatx4 *>(et + px * EROW + (lane & 3) * 8);
                vb[j][i][1] = *reinterpret_cast<const floatx4 *>(et + px * EROW + (lane & 3) * 8 + 4);
            }
        } else {
            constexpr int grp = (n - 12) / PER, w = (n - 12) % PER, j = grp >> 1, i = grp & 1;
            static_assert(!(h == 1 && j == 1 && i == 1), "pixels 112..127 are never drained");
            if constexpr (w < 8) {
                constexpr int e = w;
                float v = vb[j][i][e >> 2][e & 3];
                if (MODE == EPI_PRELU) v = v > 0.f ? v : v * q0[e];
                else v = v * q0[e] + q1[e];
                if (MODE == EPI_BN_ADD_BN) v += (float)scv[h][j][i][e];
                // (an empty statement the vectoriser cannot see through: it would otherwise pair this channel's arithmetic with the next
                // one's and move both into one gap, leaving every other gap empty)
                asm("" : "+v"(v));
                oy[e] = (half_t)v;
                vb[j][i][e >> 2][e & 3] = v;
            } else if constexpr (w < PER - 1) {
                constexpr int e = w - 8;
                float z = vb[j][i][e >> 2][e & 3] * q2[e] + q3[e];
                asm("" : "+v"(z));
                oz[e] = (half_t)z;
            } else {
                const unsigned off = group_off(h, j, i);
                *reinterpret_cast<half8 *>((p.out0 + pix0 * 64) + off) = oy;
                if (MODE == EPI_BN_ADD_BN) *reinterpret_cast<half8 *>((out1 + pix0 * 64) + off) = oz;
            }
        }
    };
    // operations [LO, HI) of that drain
    auto drain = [&](auto hc, auto lo, auto hi_, floatx16 (&a)[2], long pix0) __attribute__((always_inline)) {
        static_for<decltype(lo)::value, decltype(hi_)::value>([&](auto nc) __attribute__((always_inline)) { drain_op(hc, nc, a, pix0); });
    };
    // (plain loads: the compiler waits for them itself, with counted waits - it does not see the DMAs, so its counts err on the early side)
    auto load_sc = [&](int h, int j, int i, long pix0) __attribute__((always_inline)) {
        scv[h][j][i] = *reinterpret_cast<const half8 *>((p.sc + pix0 * 64) + group_off(h, j, i));
    };

    // One strip: 72 steps of 2 MFMAs, tiles 0 / 1 in the first 36 (half 0), tiles 2 / 3 in the last 36 (half 1), one ring of B fragments
    // through both.  The gaps behind the MFMAs of half 0 take the drain of the PREVIOUS strip's half 1, the 17 patch DMAs of the next
    // strip and the shortcut requests of this strip's half 0; the gaps of half 1 take the drain of this strip's half 0 and the shortcut
    // requests of its half 1.  first: no previous strip.
    auto strip_body = [&](auto first) __attribute__((always_inline)) {
        const int next = strip_of(k + 1);
        has_next = next < n_strips;
        ns = decode(next, has_next);
        const char *src = nullptr;  // the next DMA's source addresses
        const char *pb = patch + cur * PATCH_B;
        half8 bf[RING][2];
        auto read_b = [&](int u, half8 (&d)[2]) __attribute__((always_inline)) {
            const int h = u / STEPS, s = u - h * STEPS;
            const int tap = s >> 2, kk = s & 3;
            const int kh = tap / 3, kw = tap - kh * 3;
            const int off = (kh * PW + kw) * PROWB + kk * 32;
#pragma unroll
            for (int j = 0; j < 2; ++j) d[j] = *reinterpret_cast<const half8 *>(pb + bbase[2 * h + j] + off);
        };
#pragma unroll
        for (int u = 0; u < RING - 1; ++u) read_b(u, bf[u]);
        static_for<0, 2 * STEPS>([&](auto uc) __attribute__((always_inline)) {
            constexpr int u = decltype(uc)::value, h = u / STEPS, s = u - h * STEPS;
            if constexpr (u + RING - 1 < 2 * STEPS) read_b(u + RING - 1, bf[(u + RING - 1) % RING]);
            __builtin_amdgcn_sched_barrier(0);
            static_for<0, 2>([&](auto jc) __attribute__((always_inline)) {
                constexpr int j = decltype(jc)::value;
                constexpr int g = 2 * s + j;  // the gap behind this MFMA
                const floatx16 zero = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
                acc[h][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wreg[s >> 2][s & 3], bf[u % RING][j], s == 0 ? zero : acc[h][j], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
                if constexpr (MODE == EPI_BN_ADD_BN && g < 8 && !(g & 1) && !(h == 1 && g == 6)) load_sc(h, g >> 2, (g >> 1) & 1, cs.pix0);
                if constexpr (h == 0) {
                    // the next strip's patch goes into the other buffer: its readers retired at the last barrier
                    if constexpr (!(g & 1) && (g >> 1) < NDMA) src = dma_src(g >> 1, ns);
                    if constexpr ((g & 1) && (g >> 1) < NDMA) dma_issue(g >> 1, src, cur ^ 1);
                    constexpr int N = DrainOps<MODE>::count(1);
                    if constexpr (!decltype(first)::value)
                        drain(std::integral_constant<int, 1>{}, std::integral_constant<int, g * N / GAPS>{}, std::integral_constant<int, (g + 1) * N / GAPS>{}, acc[1], prev_pix0);
                } else {
                    constexpr int N = DrainOps<MODE>::count(0);
                    drain(std::integral_constant<int, 0>{}, std::integral_constant<int, g * N / GAPS>{}, std::integral_constant<int, (g + 1) * N / GAPS>{}, acc[0], cs.pix0);
                }
                __builtin_amdgcn_sched_barrier(0);
            });
        });
        // Hand-over.  vmcnt counts in issue order: behind this wave's DMAs came the rest of the previous half-1 drain's stores, the
        // shortcut requests of half 1 and the stores of the half-0 drain - 4 of them, or 8 in the shortcut-add form, all issued in
        // the last 36 steps.  Leaving exactly those outstanding waits for the DMAs (and the shortcut values), not for the stores.
        if (MODE == EPI_BN_ADD_BN) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
        // both waves are past the last read of this patch and have their share of the next one in LDS
        __builtin_amdgcn_s_barrier();
    };

    strip_body(std::true_type{});
    while (has_next) {
        prev_pix0 = cs.pix0;
        cs = ns;
        cur ^= 1;
        ++k;
        strip_body(std::false_type{});
    }
    // the last strip's half 1 drains with nothing above it
    drain(std::integral_constant<int, 1>{}, std::integral_constant<int, 0>{}, std::integral_constant<int, DrainOps<MODE>::count(1)>{}, acc[1], cs.pix0);
}

// Round 4, built, measured and parked in tools/experiments/conv64_in_unit0_input_layer_fused.hip: this kernel computing its own input
// patch from the 3-channel crop (the input layer - 4 MFMAs, 16 gathers and a 64-value fp32 PReLU / BN epilogue per 32 patch pixels - inside
// the strip loop, so that the 205 MB tensor z is never written or read).  Bit-identical to the two-kernel path (goldens green) and
// SLOWER: 379 us at 128 faces against 78 (arc_input_mfma_kernel) + 169 (this kernel) = 247 us (profiles/r04/r04k_unit0_fused_in.txt).  The
// strip loop runs one wave per SIMD; the patch build is ~ 3 000 VALU / LDS / store instructions per strip and wave in the same in-order
// stream as the 144 MFMAs (7 261 instructions in the kernel, 800 of them AGPR moves at 498 registers), where the stand-alone input
// kernel spreads the same work over sixteen waves per CU and is bound by its 256 MB of HBM writes.  410 MB of traffic saved, 132 us lost.

// Round 3, measured and removed: a variant in which a wave owns BOTH 32-cout blocks (288 weight registers) and half of the strip's
// pixel tiles, so that every B fragment read from LDS feeds two MFMAs (half the LDS traffic per MFMA, which was taken for the bound then).  Correct,
// no spills in the PReLU / BN forms - and slower (profiles/r03/r03b_embed_ab.txt, one box, rocprofv3 averages at 128 faces): the three PReLU
// layers 92.2 -> 108.3 us per launch (the 56x56 ones 48.8 -> 57.8), the shortcut-add form 57.4 -> 79.6 us.  At 464 - 512 registers per
// lane the A operands of half the MFMAs come out of the accumulator file, and the kernel can no longer share a SIMD with another
// wave.  The kernel above stays.

template <int MODE>
void launch_c64_t(const ConvMfmaArgs &a, const ConvPlan &, hipStream_t s) {
    const int n_strips = a.B * (a.H / 2) * (a.W / SW);
    int grid = 512;
    if (grid > n_strips) grid = n_strips;
    const size_t lds = 2 * PATCH_B + 2 * 32 * EROW * sizeof(float);
    static bool attr_done[FRT_MAX_DEVICES] = {};
    if (frt_first_use_on_device(attr_done))  // > 64 KB of dynamic LDS needs the opt-in
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(&conv64_kernel<MODE>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL((conv64_kernel<MODE>), dim3(grid), dim3(128), lds, s, a, n_strips);
}

// row = the epilogue: PReLU, BN, everything else the shortcut-add form
const ConvRow kC64[] = {
    {"conv64_kernel<0>", launch_c64_t<EPI_PRELU>, -1},
    {"conv64_kernel<1>", launch_c64_t<EPI_BN>, -1},
    {"conv64_kernel<2>", launch_c64_t<EPI_BN_ADD_BN>, -1},
};

}  // namespace

// Cin == Cout == 64, 3x3, stride 1, pad 1, H even, W a multiple of 56.  false: not this shape (use the generic kernels).
bool plan_c64(const ConvMfmaArgs &a, ConvPlan &p) {
    if (a.Cin != 64 || a.Cout != 64 || a.ks != 3 || a.stride != 1 || a.pad != 1 || a.Ho != a.H || a.Wo != a.W) return false;
    if ((a.H & 1) || a.W % SW || a.mode == EPI_PARTIAL) return false;
    if (a.mode == EPI_BN_ADD_BN && !(a.sc && a.sc_stride == 1 && a.sc_h == a.H && a.sc_w == a.W)) return false;
    conv_plan_row(p, CONV_C64, kC64, a.mode == EPI_PRELU ? 0 : (a.mode == EPI_BN ? 1 : 2));
    return true;
}

void launch_c64(const ConvMfmaArgs &a, const ConvPlan &p, hipStream_t s) { kC64[p.row].launch(a, p, s); }
