// libfrt.so: the recogniser object (weights, fp16 and fp32 networks) and its C ABI (frt_embedder_*, frt_crop_faces, frt_align_faces).
// All device work is hand-written HIP (kernels_*.hip); there is no CPU fallback anywhere in this file: without a HIP
// device every entry point that needs one fails with FRT_ERR_DEVICE.
#include <array>
#include <set>

#include "frt_embedder.hpp"
#include "frt_arc_pack.hpp"
#include "frt_matcher.hpp"

namespace {

using frt::conv_w_f16;
using frt::conv_w_f16_frag;
using frt::conv1x1_w_f16_frag;
std::vector<uint16_t> conv_w_f16(const frt::Blob &b, const std::string &name, int cout, int cin, int ks) {
    return conv_w_f16(b.get(name, (size_t)cout * cin * ks * ks).data, cout, cin, ks);
}
std::vector<float> vec_of(const frt::Blob &b, const std::string &name, size_t n) {
    const float *p = b.get(name, n).data;
    return std::vector<float>(p, p + n);
}


// Residual-stream conditioning of the deep IR backbones.  The fp16 stream (Y / Z / SC) adds one branch per unit: on the same
// kind of weights IR-100 / IR-152 peak 11 / 16 times higher than IR-50 (545 / 783 vs 48), so a stream scale IR-50 holds (1e3) overflows
// them.  Where the stream BatchNorms' running statistics say the stream is large (sigma >= 2^6), such a blob runs with the stream scaled by
// ds = 2^-4, which gives back exactly the headroom the depth costs (and no more: what overflows IR-50 still overflows them, loudly).
// PReLU, MaxPool and the convs are positively homogeneous, so with input_layer.1 and every closing BN scale and bias * ds, every
// shortcut BN's bias * ds and every BN that reads the stream (res_layer.0, output_layer.0) scale / ds the network computes the same function;
// every factor is a power of two, exact in binary floating point.  IR-50 (24 units) and the IR-SE family (its gates damp the branches:
// peaks 5 / 9 / 11) are never touched.
float residual_stream_scale(const frt::Blob &b, const frt::ArcLayout &layout, bool se) {
    if (se || layout.units.size() <= 24) return 1.0f;
    double var = 0.0;
    for (size_t i = 0; i <= layout.units.size(); ++i) {
        const std::string p = i < layout.units.size() ? "body." + std::to_string(i) + ".res_layer.0" : std::string("output_layer.0");
        const frt::Tensor &v = b.get(p + ".running_var", i < layout.units.size() ? layout.units[i].cin : 512);
        for (size_t c = 0; c < v.numel; ++c) var = std::max(var, (double)v.data[c]);
    }
    return std::sqrt(var + 1e-5) >= 64.0 ? 0.0625f : 1.0f;
}

// Conditioning of the branch conv1 -> PReLU -> conv2 -> BN (round 5; model_irse.py:57-66).  conv1's accumulators leave as the fp16
// tensor T and both convs multiply fp16 weights: a trained backbone (conversion/arcface/torch2trt.py:21-22 loads one nobody here
// has seen) may keep that branch orders of magnitude away from 1 - tools/dynamic_range_sweep.py: a branch 1e-4 times smaller pushes
// T and conv1's weights into fp16's subnormals and conv2's towards its overflow, SILENTLY (1 - cos 4.8e-4).  PReLU is positively
// homogeneous, so for powers of two c_j, d_k > 0 the unit computes exactly the same function with
//     conv1 row j * c_j      conv2 column j / c_j, row k * d_k      BN scale k / d_k        (every scaling exact in binary fp)
// c_j brings conv1's row norm to ~ 1 (T = O(1) behind a normalised input), d_k conv2's largest row entry into [0.5, 1).  A branch
// that is in range already is left bit for bit as it was (the scalings commute with every rounding).
// Returns 1 / d_k, the factors the closing BN's scale takes.
std::vector<float> condition_branch(std::vector<float> &w1v, std::vector<float> &w2v, int cin, int depth) {
    std::vector<float> dinv(depth, 1.f);
    auto pow2_inv = [](double v) {  // 2^-round(log2 v), clamped; 1 for zero / non-finite rows
        if (!(v > 0.0) || !std::isfinite(v)) return 1.0;
        const double e = std::max(-60.0, std::min(60.0, -std::nearbyint(std::log2(v))));
        return std::exp2(e);
    };
    for (int j = 0; j < depth; ++j) {
        double n2 = 0.0;
        float *row = &w1v[(size_t)j * cin * 9];
        for (int i = 0; i < cin * 9; ++i) n2 += (double)row[i] * row[i];
        const double c = pow2_inv(std::sqrt(n2));
        if (c == 1.0) continue;
        for (int i = 0; i < cin * 9; ++i) row[i] = (float)(row[i] * c);
        for (int k = 0; k < depth; ++k)
            for (int t = 0; t < 9; ++t) {
                float &v = w2v[((size_t)k * depth + j) * 9 + t];
                v = (float)(v / c);
            }
    }
    for (int k = 0; k < depth; ++k) {
        double mx = 0.0;
        float *row = &w2v[(size_t)k * depth * 9];
        for (int i = 0; i < depth * 9; ++i) mx = std::max(mx, (double)std::fabs(row[i]));
        double d = 1.0;
        if (mx > 0.0 && std::isfinite(mx) && (mx >= 2.0 || mx < 0.03125)) d = std::exp2(std::max(-60.0, std::min(60.0, -std::ceil(std::log2(mx)))));
        if (d == 1.0) continue;   // (entries already inside [2^-5, 2): nothing to gain, keep the trained numbers as they are)
        for (int i = 0; i < depth * 9; ++i) row[i] = (float)(row[i] * d);
        dinv[k] = (float)(1.0 / d);
    }
    return dinv;
}

}  // namespace

void frt_embedder::build(const frt::Blob &b) {
    std::vector<float> sc, bi;
    stream_scale = residual_stream_scale(b, layout, se);
    const float ds = stream_scale;
    // input layer (model_irse.py:139-141)
    {
        const float *src = b.get("input_layer.0.weight", 64 * 27).data;
        std::vector<float> w(27 * 64);
        for (int co = 0; co < 64; ++co)
            for (int k = 0; k < 27; ++k) w[k * 64 + co] = src[co * 27 + k];
        in_w = arena.upload(w);
        frt::bn_fold(b, "input_layer.1", 64, sc, bi);
        for (int co = 0; co < 64; ++co) sc[co] *= ds, bi[co] *= ds;
        in_s0 = arena.upload(sc);
        in_b0 = arena.upload(bi);
        const std::vector<uint16_t> wh = frt::arc_input_w_f16(src, sc.data(), bi.data());  // matrix-core layout: BN folded
        in_wh = reinterpret_cast<half_t *>(arena.upload(wh));
        in_slope = arena.upload(vec_of(b, "input_layer.2.weight", 64));
        frt::bn_fold(b, "body.0.res_layer.0", 64, sc, bi);
        for (int co = 0; co < 64; ++co) sc[co] /= ds;
        in_s1 = arena.upload(sc);
        in_b1 = arena.upload(bi);
        flops_per_face += 2.0 * 27 * 64 * 112 * 112;
    }
    // units (model_irse.py:48-90), in the order and shapes frt::arc_layout read from the blob (IR-50 / IR-100 / IR-152, with or without SE)
    size_t idx = 0;
    for (int st = 0; st < 4; ++st)
        for (int u = 0; u < layout.stage_units[st]; ++u, ++idx) {
            const frt::ArcUnitShape &shape = layout.units[idx];
            const int h = shape.h_in;
            ArcUnit a;
            a.cin = shape.cin;
            a.depth = shape.depth;
            a.stride = shape.stride;
            a.h_in = h;
            const std::string p = "body." + std::to_string(idx);
            std::vector<float> w1v = vec_of(b, p + ".res_layer.1.weight", (size_t)a.depth * a.cin * 9);
            std::vector<float> w2v = vec_of(b, p + ".res_layer.3.weight", (size_t)a.depth * a.depth * 9);
            const std::vector<float> dinv = condition_branch(w1v, w2v, a.cin, a.depth);
            a.w1 = reinterpret_cast<half_t *>(arena.upload(conv_w_f16(w1v.data(), a.depth, a.cin, 3)));
            const ArcUnitCopies copies = arc_unit_copies(a.cin, a.depth, a.stride);  // (arc_layout's widths are multiples of 64: no packer declines)
            if (copies.w1f) a.w1f = reinterpret_cast<half_t *>(arena.upload(conv_w_f16_frag(w1v.data(), a.depth, a.cin)));
            if (copies.w2f) a.w2f = reinterpret_cast<half_t *>(arena.upload(conv_w_f16_frag(w2v.data(), a.depth, a.depth)));
            // the 64 -> 64 stride-2 layer has its own kernel that stages rows in natural order and walks the taps in tap order
            if (copies.w2f2) a.w2f2 = reinterpret_cast<half_t *>(arena.upload(conv_w_f16_frag(w2v.data(), a.depth, a.depth, a.depth != 64)));
            a.prelu = arena.upload(vec_of(b, p + ".res_layer.2.weight", a.depth));
            a.w2 = reinterpret_cast<half_t *>(arena.upload(conv_w_f16(w2v.data(), a.depth, a.depth, 3)));
            frt::bn_fold(b, p + ".res_layer.4", a.depth, sc, bi);
            for (int k = 0; k < a.depth; ++k) sc[k] *= ds, bi[k] *= ds;
            a.s2f32 = arena.upload(sc);   // (the fp32 path multiplies the blob's own weights: the unconditioned scale)
            for (int k = 0; k < a.depth; ++k) sc[k] *= dinv[k];
            a.s2 = arena.upload(sc);
            a.b2 = arena.upload(bi);
            if (copies.wsc) {
                a.wsc = reinterpret_cast<half_t *>(arena.upload(conv_w_f16(b, p + ".shortcut_layer.0.weight", a.depth, a.cin, 1)));
                a.wscf = reinterpret_cast<half_t *>(arena.upload(conv1x1_w_f16_frag(b.get(p + ".shortcut_layer.0.weight", (size_t)a.depth * a.cin).data, a.depth, a.cin)));
                frt::bn_fold(b, p + ".shortcut_layer.1", a.depth, sc, bi);
                for (int k = 0; k < a.depth; ++k) bi[k] *= ds;
                a.ssc = arena.upload(sc);
                a.bsc = arena.upload(bi);
            }
            if (se) {
                a.se_w1 = arena.upload(vec_of(b, p + ".res_layer.5.fc1.weight", (size_t)a.depth / 16 * a.depth));
                a.se_w2 = arena.upload(vec_of(b, p + ".res_layer.5.fc2.weight", (size_t)a.depth * (a.depth / 16)));
            }
            const bool last = idx + 1 == layout.units.size();
            frt::bn_fold(b, last ? std::string("output_layer.0") : "body." + std::to_string(idx + 1) + ".res_layer.0", a.depth, sc, bi);
            for (int k = 0; k < a.depth; ++k) sc[k] /= ds;
            a.sn = arena.upload(sc);
            a.bn = arena.upload(bi);
            const int ho = h / a.stride;
            flops_per_face += 2.0 * 9 * a.cin * a.depth * h * h + 2.0 * 9 * a.depth * a.depth * ho * ho;
            if (a.wsc) flops_per_face += 2.0 * a.cin * a.depth * ho * ho;
            units.push_back(a);
        }
    // output layer (model_irse.py:143-147): Linear over the NCHW flatten (index c*49 + hw) re-ordered to NHWC (hw*512 + c)
    {
        const float *src = b.get("output_layer.3.weight", (size_t)512 * 25088).data;
        // ... and packed in MFMA-fragment order for kernels_arc_fc.hip (frt_arc_pack.hpp)
        wfc = reinterpret_cast<half_t *>(arena.upload(frt::fc_w_f16_frag(src)));
        fc_bias = arena.upload(vec_of(b, "output_layer.3.bias", 512));
        frt::bn_fold(b, "output_layer.4", 512, sc, bi);
        bn_s = arena.upload(sc);
        bn_b = arena.upload(bi);
        flops_per_face += 2.0 * 25088 * 512;
    }
    const size_t F = (size_t)max_batch;
    d_in = arena.alloc<float>(F * 3 * 112 * 112);
    alloc_act_set(act[0]);
    if (se) {
        HIPCHK(hipHostMalloc(reinterpret_cast<void **>(&h_se_error), sizeof(int), hipHostMallocMapped));
        *h_se_error = 0;
        HIPCHK(hipHostGetDevicePointer(reinterpret_cast<void **>(&d_se_error), h_se_error, 0));
    }
    d_out = arena.alloc<float>(F * 512);
    d_crops = arena.alloc<uint8_t>(F * 112 * 112 * 3);
    d_valid = arena.alloc<int>(F);
    d_boxes = arena.alloc<frt_bbox>(F);
    d_lm = arena.alloc<float>((size_t)F * 10);
    zeros = arena.alloc<half_t>(256);
    HIPCHK(hipMemset(zeros, 0, 256 * sizeof(half_t)));
    warm_strip_tables();
}

// The strip kernels read per-geometry tables whose first use on a device allocates and copies (kernels_arc.hip).  Every launch forward() can
// make - the unit schedule of every distinct unit shape, for every batch up to max_batch and either setting of frt_embedder_set_se_fused -
// is asked for its table here, so that first use happens now: never in steady state, never inside a captured graph.
void frt_embedder::warm_strip_tables() {
    const ArcUnitBuffers bufs = unit_buffers(act[0], 0);
    std::set<std::array<int, 5>> seen;  // IR-152: 49 units in 8 shapes
    for (const ArcUnit &u : units) {
        const bool first = &u == &units[0];
        if (!seen.insert({u.cin, u.depth, u.stride, u.h_in, first}).second) continue;
        for (int F = 1; F <= max_batch; ++F)
            for (int fuse = 0; fuse <= (se ? 1 : 0); ++fuse) {
                const ArcUnitSchedule sch = arc_unit_schedule(u, first, bufs, F, se, fuse != 0);
                for (int i = 0; i < sch.n; ++i) conv_strip_tables_warm(sch.conv[i].args, sch.conv[i].plan);
            }
    }
}

void frt_embedder::alloc_act_set(ActSet &a) {
    const size_t F = (size_t)max_batch;
    const size_t big = F * 112 * 112 * 64;
    for (int i = 0; i < 2; ++i) {
        a.Y[i] = arena.alloc<half_t>(big);
        a.Z[i] = arena.alloc<half_t>(big);
    }
    a.T = arena.alloc<half_t>(big);
    a.SC = arena.alloc<half_t>(F * 28 * 28 * 128);  // largest conv-shortcut output (56->28, 128 ch)
    if (se) {
        a.RES = arena.alloc<half_t>(F * 56 * 56 * 64);
        a.se_pool = arena.alloc<float>(F * 512 * 4 + 2 * F);  // SE_SPLIT partial sums per (face, channel) + per-face arrival counters + gate-ready flags
        a.se_counter = reinterpret_cast<int *>(a.se_pool + F * 512 * 4);
        HIPCHK(hipMemset(a.se_counter, 0, 2 * F * sizeof(int)));  // (kept at zero between launches by the kernel)
        a.se_gate = arena.alloc<float>(F * 512);
    }
    a.fc_partial = arena.alloc<float>((size_t)FC_SPLITS * std::max<size_t>(F, 2) * 512);  // (flip mode at max_batch 1: two one-face passes, kept apart)
    if (flip) a.pair = arena.alloc<float>(F * 3 * 112 * 112);
}

void frt_embedder::ensure_alt() {
    if (has_alt) return;
    alloc_act_set(act[1]);
    has_alt = true;
}

void frt_embedder::set_flip(bool on) {
    if (on)
        for (int i = 0; i < (has_alt ? 2 : 1); ++i)
            if (!act[i].pair) act[i].pair = arena.alloc<float>((size_t)max_batch * 3 * 112 * 112);
    flip = on;
}

// fp32 weights: 3x3 [Cout][Cin][3][3] -> [Cout][tap][Cin]; 1x1 and Linear as described at the kernels
void frt_embedder::build_f32() {
    if (!f32.units.empty()) return;
    frt::Blob b;
    std::string err;
    const int rc = b.load(blob_path.c_str(), err);
    if (rc) raise(rc, "fp32 mode: cannot re-read the weight blob: " + err);
    auto up = [&](const std::vector<float> &v) {
        float *d = nullptr;
        HIPCHK(hipMalloc(reinterpret_cast<void **>(&d), v.size() * sizeof(float)));
        f32.owned.push_back(d);
        HIPCHK(hipMemcpy(d, v.data(), v.size() * sizeof(float), hipMemcpyHostToDevice));
        return d;
    };
    auto dev = [&](size_t n) {
        float *d = nullptr;
        HIPCHK(hipMalloc(reinterpret_cast<void **>(&d), n * sizeof(float)));
        f32.owned.push_back(d);
        return d;
    };
    auto w3 = [&](const std::string &name, int cout, int cin) { return up(frt::conv32_w_frag(b.get(name, (size_t)cout * cin * 9).data, cout, cin, 3)); };
    auto w1x1 = [&](const std::string &name, int cout, int cin) { return up(frt::conv32_w_frag(b.get(name, (size_t)cout * cin).data, cout, cin, 1)); };
    int idx = 0;
    for (const ArcUnit &u : units) {
        const std::string p = "body." + std::to_string(idx++);
        F32Unit fu;
        fu.w1 = w3(p + ".res_layer.1.weight", u.depth, u.cin);
        fu.w2 = w3(p + ".res_layer.3.weight", u.depth, u.depth);
        if (u.wsc) fu.wsc = w1x1(p + ".shortcut_layer.0.weight", u.depth, u.cin);
        f32.units.push_back(fu);
    }
    f32.wfc = up(frt::fc32_w_nhwc(b.get("output_layer.3.weight", (size_t)512 * 25088).data));
    f32.chunk = std::min(max_batch, 8);
    const Arc32BufferSizes n = arc32_buffer_sizes(f32.chunk);
    f32.A[0] = dev(n.act);
    f32.A[1] = dev(n.act);
    f32.T = dev(n.act);
    f32.SCb = dev(n.sc);
    if (se) {
        f32.RES = dev(n.res);
        f32.gate = dev(n.gate);
    }
    f32.fc_out = dev(std::max(n.fc_out, (size_t)2 * 512));  // (flip mode at chunk 1: two one-face passes, kept apart)
    f32.pair = dev((size_t)f32.chunk * 3 * 112 * 112);
    HIPCHK(hipEventCreateWithFlags(&f32.done, hipEventDisableTiming));
}

// Backbone.forward in fp32 (model_irse.py:166-173), CHUNK faces at a time.  The per-channel parameters (folded BatchNorms, PReLU slopes, SE
// weights, Linear bias) are the fp32 arrays the default path's epilogues use.
void frt_embedder::forward_f32(const float *chw_dev, int F, const int *valid_dev, float *out_dev, hipStream_t s) {
    ProfScope ps(2, "embed_network", flops_per_face * F * (flip ? 2 : 1), s);
    if (f32.busy) HIPCHK(hipStreamWaitEvent(s, f32.done, 0));
    constexpr size_t IN = (size_t)3 * 112 * 112;
    // the network up to the Linear's sums: x [n][3][112][112] -> sums [n][512]
    auto network = [&](const float *x, int n, float *sums) {
        launch_arc32_input(x, in_w, in_s0, in_b0, in_slope, f32.A[0], n, s);
        int cur = 0;
        const float *lead_s = in_s1, *lead_b = in_b1;  // the leading BatchNorm of the unit about to run
        for (size_t i = 0; i < units.size(); ++i) {
            const ArcUnit &u = units[i];
            const F32Unit &fu = f32.units[i];
            // the unit's launches as csrc/frt_arc_launches.hpp describes them: conv1, the 1x1 shortcut where the unit has one, conv2 (-> SE)
            const Arc32Buffers bufs{f32.A[cur], lead_s, lead_b, f32.T, f32.SCb, f32.RES, f32.gate, f32.A[cur ^ 1]};
            Conv32Args a;
            arc32_conv1(u, fu, bufs, n, a);
            launch_conv32(a, s);
            if (arc32_shortcut1x1(u, fu, bufs, n, a)) launch_conv32(a, s);
            if (se) {
                arc32_conv2_res(u, fu, bufs, n, a);
                launch_conv32(a, s);
                launch_se32(arc32_se(u, fu, bufs, n), s);
            } else {
                arc32_conv2(u, fu, bufs, n, a);
                launch_conv32(a, s);
            }
            lead_s = u.sn;
            lead_b = u.bn;
            cur ^= 1;
        }
        // output_layer: BN2d (on load) -> Flatten -> Linear (-> BN1d -> L2 normalise: the finalize launches below)
        launch_fc32(f32.A[cur], lead_s, lead_b, f32.wfc, sums, n, s);
    };
    if (!flip) {
        for (int f0 = 0; f0 < F; f0 += f32.chunk) {
            const int n = std::min(f32.chunk, F - f0);
            network(chw_dev + (size_t)f0 * IN, n, f32.fc_out);
            launch_fc_finalize(f32.fc_out, 1, n, fc_bias, bn_s, bn_b, valid_dev ? valid_dev + f0 : nullptr, out_dev + (size_t)f0 * 512, s);
        }
    } else if (f32.chunk == 1) {  // the face and its mirror image as two one-face passes
        for (int f = 0; f < F; ++f) {
            network(chw_dev + (size_t)f * IN, 1, f32.fc_out);
            launch_arc_flip_mirror(chw_dev + (size_t)f * IN, f32.pair, 1, s);
            network(f32.pair, 1, f32.fc_out + 512);
            launch_fc_finalize_pair(f32.fc_out, f32.fc_out + 512, 1, 1, 1, fc_bias, bn_s, bn_b, valid_dev ? valid_dev + f : nullptr, out_dev + (size_t)f * 512, s);
        }
    } else {
        const int half = f32.chunk / 2;
        for (int f0 = 0; f0 < F; f0 += half) {
            const int n = std::min(half, F - f0);
            launch_arc_flip_pair(chw_dev + (size_t)f0 * IN, f32.pair, n, s);
            network(f32.pair, 2 * n, f32.fc_out);
            launch_fc_finalize_pair(f32.fc_out, f32.fc_out + (size_t)n * 512, 1, 2 * n, n, fc_bias, bn_s, bn_b, valid_dev ? valid_dev + f0 : nullptr,
                                    out_dev + (size_t)f0 * 512, s);
        }
    }
    HIPCHK(hipEventRecord(f32.done, s));
    f32.busy = true;
    HIPCHK(hipGetLastError());
}

void frt_embedder::run_network(const ActSet &A, const float *chw_dev, int F, float *partial, hipStream_t s) {
    ArcInputArgs ia{chw_dev, in_w, in_s0, in_b0, in_slope, in_s1, in_b1, A.Y[0], A.Z[0], F, 112, 112, in_wh};
    launch_arc_input(ia, s);
    int cur = 0;
    const bool fuse = se && se_fused && conv_se_fits_device();
    for (const ArcUnit &u : units) {
        ArcUnitSchedule sch = arc_unit_schedule(u, &u == &units[0], unit_buffers(A, cur), F, se, fuse);
        if (sch.se_fused) {
            if (se_epoch >= (1 << 30)) {  // the flags carry launch numbers: start over with clean flags (every allocated set)
                for (int i = 0; i < (has_alt ? 2 : 1); ++i) HIPCHK(hipMemsetAsync(act[i].se_counter + max_batch, 0, (size_t)max_batch * sizeof(int), s));
                se_epoch = 0;
            }
            sch.conv[sch.n - 1].args.se_epoch = ++se_epoch;
        }
        for (int i = 0; i < sch.n; ++i) {
            const ArcLaunch &l = sch.conv[i];
            if (l.desc == ARC_SHORTCUT1X1) {  // (not bracketed: the recorded label sequences hold conv1 and conv2 of every unit)
                launch_conv_mfma(l.args, l.plan, s);
                continue;
            }
            ProfScope pk(1, l.plan.label, l.flops, s);
            launch_conv_mfma(l.args, l.plan, s);
        }
        if (sch.se_tail) launch_se(sch.se, s);
        cur ^= 1;
    }
    // Linear 25088 -> 512 as 49 K-slices over the NHWC-flattened BN2d output (Z); the finalize launch adds the slices
    launch_fc_slices(A.Z[cur], wfc, F, partial, s);
}

void frt_embedder::forward(int set, const float *chw_dev, int F, const int *valid_dev, float *out_dev, hipStream_t s) {
    if (fp32_mode) return forward_f32(chw_dev, F, valid_dev, out_dev, s);
    ProfScope ps(2, "embed_network", flops_per_face * F * (flip ? 2 : 1), s);
    const ActSet &A = act[set];
    constexpr size_t IN = (size_t)3 * 112 * 112;
    if (!flip) {
        run_network(A, chw_dev, F, A.fc_partial, s);
        launch_fc_finalize(A.fc_partial, FC_SPLITS, F, fc_bias, bn_s, bn_b, valid_dev, out_dev, s);  // slice sum + bias + BN1d + L2 norm
    } else if (max_batch == 1) {  // the face and its mirror image as two one-face passes, their slice sums kept apart
        float *partial_m = A.fc_partial + (size_t)FC_SPLITS * 512;
        for (int f = 0; f < F; ++f) {
            run_network(A, chw_dev + (size_t)f * IN, 1, A.fc_partial, s);
            launch_arc_flip_mirror(chw_dev + (size_t)f * IN, A.pair, 1, s);
            run_network(A, A.pair, 1, partial_m, s);
            launch_fc_finalize_pair(A.fc_partial, partial_m, FC_SPLITS, 1, 1, fc_bias, bn_s, bn_b, valid_dev ? valid_dev + f : nullptr, out_dev + (size_t)f * 512, s);
        }
    } else {  // sub-passes of max_batch / 2 faces: one network pass over the faces and, behind them, their mirror images
        const int half = max_batch / 2;
        for (int f0 = 0; f0 < F; f0 += half) {
            const int n = std::min(half, F - f0);
            {
                ProfScope pk(1, "flip_pair_up", (double)n * IN, s);
                launch_arc_flip_pair(chw_dev + (size_t)f0 * IN, A.pair, n, s);
            }
            run_network(A, A.pair, 2 * n, A.fc_partial, s);
            ProfScope pk(1, "fc_finalize_pair", (double)n * 512, s);
            launch_fc_finalize_pair(A.fc_partial, A.fc_partial + (size_t)n * 512, FC_SPLITS, 2 * n, n, fc_bias, bn_s, bn_b, valid_dev ? valid_dev + f0 : nullptr,
                                    out_dev + (size_t)f0 * 512, s);
        }
    }
    HIPCHK(hipGetLastError());
}

namespace {

// One-shot crop / alignment (frt_crop_faces, frt_align_faces): frame up, `launch(arena, d_frame, tight, d_crops, d_chw, d_valid)`, crops down
// into crops_host [n][out_h][out_w][3]; returns the validity flags.
template <class Launch>
std::vector<int> crops_one_shot(const uint8_t *bgr, int rows, int cols, size_t row_stride, int n, int out_h, int out_w, int device, uint8_t *crops_host,
                                Launch launch) {
    if (device >= 0) use_device(device);
    Arena a;
    struct Guard {
        Arena &a;
        ~Guard() { a.release(); }
    } guard{a};
    const size_t tight = (size_t)cols * 3, crop_bytes = (size_t)n * out_h * out_w * 3;
    uint8_t *d_frame = a.alloc<uint8_t>((size_t)rows * tight);
    uint8_t *d_crops = a.alloc<uint8_t>(crop_bytes);
    float *d_chw = a.alloc<float>(crop_bytes);
    int *d_valid = a.alloc<int>(n);
    HIPCHK(hipMemcpy2D(d_frame, tight, bgr, row_stride, tight, rows, hipMemcpyHostToDevice));
    launch(a, d_frame, tight, d_crops, d_chw, d_valid);
    std::vector<int> valid(n);
    HIPCHK(hipMemcpy(valid.data(), d_valid, sizeof(int) * n, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(crops_host, d_crops, crop_bytes, hipMemcpyDeviceToHost));
    return valid;
}

// frt_embedder_forward / _forward_aligned: frame up once, then per pass of at most max_batch faces `stage(f0, nf, tight, stream)` (boxes or landmarks
// up, crop or alignment into d_crops / d_in / d_valid) -> network -> embeddings (and crops) down.  Returns whether a face was invalid.
template <class Stage>
bool forward_frame(frt_embedder *e, const uint8_t *bgr, int rows, int cols, size_t row_stride, int n, float *embeds_out, uint8_t *crops_out, Stage stage) {
    std::lock_guard<std::mutex> lk(e->mu);
    use_device(e->device);
    hipStream_t s = e->stream;
    e->wait_idle(s);
    const size_t tight = (size_t)cols * 3, need = (size_t)rows * tight;
    e->d_frame.reserve(need);
    HIPCHK(hipMemcpy2DAsync(e->d_frame.get(), tight, bgr, row_stride, tight, rows, hipMemcpyHostToDevice, s));
    bool bad = false;
    for (int f0 = 0; f0 < n; f0 += e->max_batch) {
        const int nf = std::min(e->max_batch, n - f0);
        stage(f0, nf, tight, s);
        e->forward(0, e->d_in, nf, e->d_valid, e->d_out, s);
        HIPCHK(hipMemcpyAsync(embeds_out + (size_t)f0 * 512, e->d_out, sizeof(float) * 512 * nf, hipMemcpyDeviceToHost, s));
        if (crops_out) HIPCHK(hipMemcpyAsync(crops_out + (size_t)f0 * 112 * 112 * 3, e->d_crops, (size_t)nf * 112 * 112 * 3, hipMemcpyDeviceToHost, s));
        std::vector<int> valid(nf);
        HIPCHK(hipMemcpyAsync(valid.data(), e->d_valid, sizeof(int) * nf, hipMemcpyDeviceToHost, s));
        sync_stream_spinning(s);
        e->check_se_error();
        for (int v : valid) bad = bad || !v;
    }
    return bad;
}

}  // namespace

// ---- face images instead of frames (include/frt.h "Face images instead of frames")
// every argument of a face-image entry point that can be checked on the host, before any device work
void check_face_images(const frt_face_image *faces, int n, const char *what) {
    if (n < 0) raise(FRT_ERR_INVALID, std::string(what) + ": n < 0");
    if (n > 0 && !faces) raise(FRT_ERR_INVALID, std::string(what) + ": null image list");
    for (int i = 0; i < n; ++i) {
        const frt_face_image &f = faces[i];
        const char *why = !f.bgr ? "null pixel pointer"
                          : f.rows < 1 || f.cols < 1 ? "rows < 1 or cols < 1"
                          : f.cols > INT32_MAX / 3 ? "more columns than a row of int32 bytes holds"
                          : f.row_stride < (size_t)f.cols * 3 ? "row_stride < cols * 3"
                                                              : nullptr;
        if (why) raise(FRT_ERR_INVALID, std::string(what) + ": image " + std::to_string(i) + ": " + why);
    }
}

// images [first, first + count) with their row strides removed, each at its descriptor's offset behind `arena`
void pack_face_images(const frt_face_image *faces, const frt_face_desc *desc, int first, int count, uint8_t *arena) {
    for (int i = first; i < first + count; ++i) {
        const frt_face_image &f = faces[i];
        const size_t tight = (size_t)f.cols * 3;
        uint8_t *dst = arena + desc[i].offset;
        if (f.row_stride == tight) {
            std::memcpy(dst, f.bgr, tight * f.rows);
        } else {
            for (int r = 0; r < f.rows; ++r) std::memcpy(dst + (size_t)r * tight, f.bgr + (size_t)r * f.row_stride, tight);
        }
    }
}

std::vector<frt_face_desc> face_descs(const frt_face_image *faces, int n) {
    std::vector<frt_face_desc> desc((size_t)n);
    for (int i = 0; i < n; ++i) desc[(size_t)i] = frt_face_desc{0, faces[i].rows, faces[i].cols};
    return desc;
}

namespace {

// The loop of gen / /insert/face / /recognize (app.cpp:69-99, :148-162, :243-287) for n images, under e->mu: chunk i + 1 is packed and
// uploaded on the copy stream while chunk i's prepare kernel and network pass run on e->stream.  Embeddings go to embeds_out (host, may be
// null) per chunk and, when `collect` (device, [n][512]) is given, are written there by the network pass itself.
void embed_face_images(frt_embedder *e, const frt_face_image *faces, int n, float *embeds_out, uint8_t *crops_out, float *collect) {
    frt_embedder::FaceStage &fs = e->faces;
    hipStream_t s = e->stream;
    std::vector<frt_face_desc> desc = face_descs(faces, n);
    const std::vector<frt_face_chunk> chunks = frt_plan_face_chunks(desc.data(), n, e->max_batch, FRT_FACES_STAGE_CAP);
    const size_t hdr = ((size_t)e->max_batch * sizeof(frt_face_desc) + 255) & ~(size_t)255;  // descriptor table in front of the arena: one upload
    size_t need = 0;
    for (const frt_face_chunk &c : chunks) need = std::max(need, c.bytes);
    if (!fs.copy) {
        HIPCHK(hipStreamCreateWithFlags(&fs.copy, hipStreamNonBlocking));
        for (int b = 0; b < 2; ++b) {
            HIPCHK(hipEventCreateWithFlags(&fs.uploaded[b], hipEventDisableTiming));
            HIPCHK(hipEventCreateWithFlags(&fs.read[b], hipEventDisableTiming));
        }
    }
    for (PackPair &pk : fs.pack) pk.reserve(hdr, need);  // (both idle: every call ends with its streams drained)
    e->wait_idle(s);
    bool used[2] = {false, false};
    auto stage = [&](size_t ci) {
        const int b = (int)(ci & 1);
        const frt_face_chunk &c = chunks[ci];
        if (used[b]) wait_event_spinning(fs.uploaded[b]);  // the pinned buffer is rewritten only after its upload
        std::memcpy(fs.pack[b].h.get(), &desc[(size_t)c.first], (size_t)c.count * sizeof(frt_face_desc));
        pack_face_images(faces, desc.data(), c.first, c.count, fs.pack[b].h.get() + hdr);
        if (used[b]) HIPCHK(hipStreamWaitEvent(fs.copy, fs.read[b], 0));  // the arena only after the prepare kernel that read it
        HIPCHK(hipMemcpyAsync(fs.pack[b].d.get(), fs.pack[b].h.get(), hdr + c.bytes, hipMemcpyHostToDevice, fs.copy));
        HIPCHK(hipEventRecord(fs.uploaded[b], fs.copy));
        used[b] = true;
    };
    try {
        stage(0);
        for (size_t ci = 0; ci < chunks.size(); ++ci) {
            if (ci + 1 < chunks.size()) stage(ci + 1);  // (before this chunk's downloads: a copy into pageable memory holds the host)
            const int b = (int)(ci & 1);
            const frt_face_chunk &c = chunks[ci];
            HIPCHK(hipStreamWaitEvent(s, fs.uploaded[b], 0));
            {
                ProfScope ps(2, "faces_prepare", (double)c.count * 112 * 112, s);
                ProfScope pk(1, "faces_prepare_kernel", (double)c.count * 112 * 112, s);
                launch_faces_prepare(fs.pack[b].d.get() + hdr, reinterpret_cast<const frt_face_desc *>(fs.pack[b].d.get()), c.count,
                                     crops_out ? e->d_crops : nullptr, e->d_in, s);  // (d_in is shared: behind the previous chunk's pass on s)
            }
            HIPCHK(hipEventRecord(fs.read[b], s));
            float *out = collect ? collect + (size_t)c.first * 512 : e->d_out;
            e->forward(0, e->d_in, c.count, nullptr, out, s);
            if (embeds_out) HIPCHK(hipMemcpyAsync(embeds_out + (size_t)c.first * 512, out, sizeof(float) * 512 * c.count, hipMemcpyDeviceToHost, s));
            if (crops_out)
                HIPCHK(hipMemcpyAsync(crops_out + (size_t)c.first * 112 * 112 * 3, e->d_crops, (size_t)c.count * 112 * 112 * 3, hipMemcpyDeviceToHost, s));
        }
        sync_stream_spinning(s);
    } catch (...) {  // leave nothing in flight that reads the staging of a call that has returned
        (void)hipStreamSynchronize(fs.copy);
        (void)hipStreamSynchronize(s);
        throw;
    }
    e->check_se_error();
}

}  // namespace

extern "C" {

// ---------------------------------------------------------------------------------------------------------------- crop
int frt_crop_faces(const uint8_t *bgr, int rows, int cols, size_t row_stride, const frt_bbox *boxes, int n, int out_w, int out_h,
                   uint8_t *crops_out, int device) {
    return guarded([&] {
        if (!bgr || !boxes || !crops_out || n < 0 || out_w < 1 || out_h < 1) raise(FRT_ERR_INVALID, "getCroppedFaces: bad argument");
        if (n == 0) return;
        std::vector<uint8_t> tmp((size_t)n * out_h * out_w * 3);
        const std::vector<int> valid = crops_one_shot(bgr, rows, cols, row_stride, n, out_h, out_w, device, tmp.data(),
                                                      [&](Arena &a, const uint8_t *d_frame, size_t tight, uint8_t *d_crops, float *d_chw, int *d_valid) {
            frt_bbox *d_boxes = a.alloc<frt_bbox>(n);
            HIPCHK(hipMemcpy(d_boxes, boxes, sizeof(frt_bbox) * n, hipMemcpyHostToDevice));
            launch_crop_faces(d_frame, rows, cols, tight, 0, d_boxes, nullptr, 1, n, 1, out_h, out_w, d_crops, d_chw, d_valid, nullptr);
        });
        bool bad = false;
        for (int i = 0; i < n; ++i) {
            if (valid[i])
                std::memcpy(crops_out + (size_t)i * out_h * out_w * 3, tmp.data() + (size_t)i * out_h * out_w * 3, (size_t)out_h * out_w * 3);
            else
                bad = true;
        }
        if (bad) raise(FRT_ERR_EMPTY_ROI, "getCroppedFaces: empty or out-of-frame ROI");
    });
}

// ------------------------------------------------------------------------------------------------------------ embedder
int frt_embedder_create(const char *weights_path, int in_c, int in_h, int in_w, int out_dim, int max_batch, int device, frt_embedder **out) {
    return guarded([&] {
        if (!out || !weights_path) raise(FRT_ERR_INVALID, "null argument");
        *out = nullptr;
        if (in_c != 3 || in_h != 112 || in_w != 112 || out_dim != 512 || max_batch < 1)
            raise(FRT_ERR_INVALID, "embedder: only rec_inputShape [3,112,112] and rec_outputDim 512 are supported");
        frt::Blob blob;
        std::string err;
        const int rc = blob.load(weights_path, err);
        if (rc) raise(rc, err);
        if (blob.kind != 2 && blob.kind != 3) raise(FRT_ERR_FORMAT, "embedder: weight blob is not an ArcFace IR / IR-SE blob");
        const frt::ArcLayout layout = frt::arc_layout(blob, blob.kind == 3);  // (host only: a malformed blob fails before any HIP call)
        use_device(device);
        std::unique_ptr<frt_embedder> e(new frt_embedder);
        e->device = device;
        e->max_batch = max_batch;
        e->se = blob.kind == 3;
        e->layout = layout;
        e->blob_path = weights_path;
        HIPCHK(hipStreamCreate(&e->stream));
        HIPCHK(hipEventCreateWithFlags(&e->ev_busy[0], hipEventDisableTiming));
        HIPCHK(hipEventCreateWithFlags(&e->ev_busy[1], hipEventDisableTiming));
        e->build(blob);
        HIPCHK(hipDeviceSynchronize());
        *out = e.release();
    });
}

int frt_embedder_describe(const char *weights_path, int *num_layers, int *se, int *units_per_stage) {
    return guarded([&] {
        if (!weights_path) raise(FRT_ERR_INVALID, "null argument");
        frt::Blob blob;
        std::string err;
        const int rc = blob.load(weights_path, err);
        if (rc) raise(rc, err);
        if (blob.kind != 2 && blob.kind != 3) raise(FRT_ERR_FORMAT, "embedder: weight blob is not an ArcFace IR / IR-SE blob");
        const frt::ArcLayout layout = frt::arc_layout(blob, blob.kind == 3);
        if (num_layers) *num_layers = layout.num_layers;
        if (se) *se = layout.se ? 1 : 0;
        if (units_per_stage)
            for (int i = 0; i < 4; ++i) units_per_stage[i] = layout.stage_units[i];
    });
}

void frt_embedder_destroy(frt_embedder *e) {
    if (!e) return;
    (void)hipSetDevice(e->device);
    if (e->stream) {
        (void)hipStreamSynchronize(e->stream);
        (void)hipStreamDestroy(e->stream);
    }
    if (e->faces.copy) {
        (void)hipStreamSynchronize(e->faces.copy);
        (void)hipStreamDestroy(e->faces.copy);
    }
    for (int b = 0; b < 2; ++b) {
        if (e->faces.uploaded[b]) (void)hipEventDestroy(e->faces.uploaded[b]);
        if (e->faces.read[b]) (void)hipEventDestroy(e->faces.read[b]);
    }
    for (void *p : e->f32.owned) (void)hipFree(p);
    if (e->f32.done) (void)hipEventDestroy(e->f32.done);
    if (e->h_se_error) (void)hipHostFree(e->h_se_error);
    for (hipEvent_t ev : e->ev_busy)
        if (ev) (void)hipEventDestroy(ev);
    e->arena.release();
    delete e;  // d_frame and the face stage's buffers free themselves, on the device set above
}

int frt_embedder_set_se_fused(frt_embedder *e, int enable) {
    return guarded([&] {
        if (!e) raise(FRT_ERR_INVALID, "null argument");
        std::lock_guard<std::mutex> lk(e->mu);
        e->se_fused = enable != 0;
    });
}

int frt_embedder_set_precision(frt_embedder *e, int fp32) {
    return guarded([&] {
        if (!e) raise(FRT_ERR_INVALID, "null argument");
        std::lock_guard<std::mutex> lk(e->mu);
        use_device(e->device);
        if (fp32) {
            HIPCHK(hipStreamSynchronize(e->stream));
            e->build_f32();
            HIPCHK(hipDeviceSynchronize());
        }
        e->fp32_mode = fp32 != 0;
    });
}

int frt_embedder_set_flip(frt_embedder *e, int enable) {
    return guarded([&] {
        if (!e) raise(FRT_ERR_INVALID, "null argument");
        std::lock_guard<std::mutex> lk(e->mu);
        use_device(e->device);
        e->wait_idle(e->stream);  // the pipeline's passes in flight on either activation set
        HIPCHK(hipStreamSynchronize(e->stream));
        e->set_flip(enable != 0);
    });
}

int frt_embedder_get_flip(const frt_embedder *e, int *enabled_out) {
    return guarded([&] {
        if (!e || !enabled_out) raise(FRT_ERR_INVALID, "null argument");
        std::lock_guard<std::mutex> lk(const_cast<frt_embedder *>(e)->mu);
        *enabled_out = e->flip ? 1 : 0;
    });
}

int frt_embedder_preprocess_face(frt_embedder *e, const uint8_t *bgr_crop, float *chw_out) {
    return guarded([&] {
        if (!e || !bgr_crop || !chw_out) raise(FRT_ERR_INVALID, "null argument");
        std::lock_guard<std::mutex> lk(e->mu);
        use_device(e->device);
        hipStream_t s = e->stream;
        e->wait_idle(s);
        HIPCHK(hipMemcpyAsync(e->d_crops, bgr_crop, 112 * 112 * 3, hipMemcpyHostToDevice, s));
        launch_face_normalize(e->d_crops, 1, 112, 112, e->d_in, s);
        HIPCHK(hipMemcpyAsync(chw_out, e->d_in, sizeof(float) * 3 * 112 * 112, hipMemcpyDeviceToHost, s));
        sync_stream_spinning(s);
    });
}

int frt_embedder_infer(frt_embedder *e, const float *chw, int batch, float *embeds_out) {
    return guarded([&] {
        if (!e || !chw || !embeds_out || batch < 1) raise(FRT_ERR_INVALID, "doInference: bad argument");
        std::lock_guard<std::mutex> lk(e->mu);
        use_device(e->device);
        hipStream_t s = e->stream;
        e->wait_idle(s);
        const size_t in_elems = (size_t)3 * 112 * 112;
        for (int f0 = 0; f0 < batch; f0 += e->max_batch) {
            const int nf = std::min(e->max_batch, batch - f0);
            HIPCHK(hipMemcpyAsync(e->d_in, chw + (size_t)f0 * in_elems, sizeof(float) * in_elems * nf, hipMemcpyHostToDevice, s));
            e->forward(0, e->d_in, nf, nullptr, e->d_out, s);
            HIPCHK(hipMemcpyAsync(embeds_out + (size_t)f0 * 512, e->d_out, sizeof(float) * 512 * nf, hipMemcpyDeviceToHost, s));
            sync_stream_spinning(s);
            e->check_se_error();
        }
    });
}

int frt_embedder_forward(frt_embedder *e, const uint8_t *bgr, int rows, int cols, size_t row_stride, const frt_bbox *boxes, int n,
                         float *embeds_out, uint8_t *crops_out) {
    return guarded([&] {
        if (!e || !bgr || !boxes || !embeds_out || n < 0 || rows < 1 || cols < 1) raise(FRT_ERR_INVALID, "forward: bad argument");
        if (n == 0) return;
        const bool bad = forward_frame(e, bgr, rows, cols, row_stride, n, embeds_out, crops_out, [&](int f0, int nf, size_t tight, hipStream_t s) {
            HIPCHK(hipMemcpyAsync(e->d_boxes, boxes + f0, sizeof(frt_bbox) * nf, hipMemcpyHostToDevice, s));
            launch_crop_faces(e->d_frame.get(), rows, cols, tight, 0, e->d_boxes, nullptr, 1, nf, 1, 112, 112, e->d_crops, e->d_in, e->d_valid, s);
        });
        if (bad) raise(FRT_ERR_EMPTY_ROI, "forward: empty or out-of-frame ROI (embedding set to zeros)");
    });
}

int frt_align_faces(const uint8_t *bgr, int rows, int cols, size_t row_stride, const float *landmarks, int n, uint8_t *crops_out, int device) {
    return guarded([&] {
        if (!bgr || !landmarks || !crops_out || n < 0 || rows < 1 || cols < 1) raise(FRT_ERR_INVALID, "alignFaces: bad argument");
        if (n == 0) return;
        const std::vector<int> valid = crops_one_shot(bgr, rows, cols, row_stride, n, 112, 112, device, crops_out,
                                                      [&](Arena &a, const uint8_t *d_frame, size_t tight, uint8_t *d_crops, float *d_chw, int *d_valid) {
            float *d_lm = a.alloc<float>((size_t)n * 10);
            HIPCHK(hipMemcpy(d_lm, landmarks, sizeof(float) * 10 * n, hipMemcpyHostToDevice));
            launch_align_faces(d_frame, rows, cols, tight, 0, d_lm, nullptr, 1, n, 1, d_crops, d_chw, d_valid, nullptr);
        });
        for (int v : valid)
            if (!v) raise(FRT_ERR_EMPTY_ROI, "alignFaces: degenerate landmarks (crop set to zeros)");
    });
}

int frt_embedder_forward_aligned(frt_embedder *e, const uint8_t *bgr, int rows, int cols, size_t row_stride, const float *landmarks, int n,
                                 float *embeds_out, uint8_t *crops_out) {
    return guarded([&] {
        if (!e || !bgr || !landmarks || !embeds_out || n < 0 || rows < 1 || cols < 1) raise(FRT_ERR_INVALID, "forwardAligned: bad argument");
        if (n == 0) return;
        const bool bad = forward_frame(e, bgr, rows, cols, row_stride, n, embeds_out, crops_out, [&](int f0, int nf, size_t tight, hipStream_t s) {
            HIPCHK(hipMemcpyAsync(e->d_lm, landmarks + (size_t)f0 * 10, sizeof(float) * 10 * nf, hipMemcpyHostToDevice, s));
            launch_align_faces(e->d_frame.get(), rows, cols, tight, 0, e->d_lm, nullptr, 1, nf, 1, e->d_crops, e->d_in, e->d_valid, s);
        });
        if (bad) raise(FRT_ERR_EMPTY_ROI, "forwardAligned: degenerate landmarks (embedding set to zeros)");
    });
}

// ---------------------------------------------------------------------------------------------- face images instead of frames
int frt_preprocess_faces(const frt_face_image *faces, int n, uint8_t *crops_out, float *chw_out, int device) {
    return guarded([&] {
        check_face_images(faces, n, "preprocessFaces");
        if (n == 0 || (!crops_out && !chw_out)) return;
        std::vector<frt_face_desc> desc = face_descs(faces, n);
        const std::vector<frt_face_chunk> chunks = frt_plan_face_chunks(desc.data(), n, n, SIZE_MAX);  // one chunk: one arena, one launch
        const size_t hdr = ((size_t)n * sizeof(frt_face_desc) + 255) & ~(size_t)255, px = (size_t)n * 112 * 112 * 3;
        std::vector<uint8_t> pack(hdr + chunks[0].bytes);
        std::memcpy(pack.data(), desc.data(), (size_t)n * sizeof(frt_face_desc));
        pack_face_images(faces, desc.data(), 0, n, pack.data() + hdr);
        if (device >= 0) use_device(device);
        Arena a;
        struct Guard {
            Arena &a;
            ~Guard() { a.release(); }
        } guard{a};
        uint8_t *d_pack = a.alloc<uint8_t>(pack.size());
        uint8_t *d_crops = crops_out ? a.alloc<uint8_t>(px) : nullptr;
        float *d_chw = chw_out ? a.alloc<float>(px) : nullptr;
        HIPCHK(hipMemcpy(d_pack, pack.data(), pack.size(), hipMemcpyHostToDevice));
        launch_faces_prepare(d_pack + hdr, reinterpret_cast<const frt_face_desc *>(d_pack), n, d_crops, d_chw, nullptr);
        HIPCHK(hipGetLastError());
        if (crops_out) HIPCHK(hipMemcpy(crops_out, d_crops, px, hipMemcpyDeviceToHost));
        if (chw_out) HIPCHK(hipMemcpy(chw_out, d_chw, px * sizeof(float), hipMemcpyDeviceToHost));
    });
}

int frt_embedder_embed_faces(frt_embedder *e, const frt_face_image *faces, int n, float *embeds_out, uint8_t *crops_out) {
    return guarded([&] {
        if (!e) raise(FRT_ERR_INVALID, "embedFaces: null argument");
        check_face_images(faces, n, "embedFaces");
        if (n > 0 && !embeds_out) raise(FRT_ERR_INVALID, "embedFaces: null argument");
        if (n == 0) return;
        std::lock_guard<std::mutex> lk(e->mu);
        use_device(e->device);
        embed_face_images(e, faces, n, embeds_out, crops_out, nullptr);
    });
}

int frt_embedder_enrol_faces(frt_embedder *e, frt_matcher *m, const frt_face_image *faces, int n, const int32_t *labels, float *embeds_out,
                             int *first_row_out) {
    return guarded([&] {
        if (!e || !m) raise(FRT_ERR_INVALID, "enrolFaces: null argument");
        check_face_images(faces, n, "enrolFaces");
        if (n > 65536) raise(FRT_ERR_CAPACITY, "enrolFaces: more than 65536 images in one call");
        if (e->device != m->device) raise(FRT_ERR_INVALID, "enrolFaces: the embedder and the matcher live on different devices");
        for (int i = 0; labels && i < n; ++i)
            if (labels[i] < 0) raise(FRT_ERR_INVALID, "enrolFaces: image " + std::to_string(i) + ": negative label");
        std::lock_guard<std::mutex> lk(e->mu);  // lock order: embedder, then matcher
        int rows = 0;
        {  // what the edit will refuse is refused before the images are embedded (the add below checks again: the gallery may change in between)
            std::lock_guard<std::mutex> lm(m->mu);
            rows = m->N;
            if (m->D != 512) raise(FRT_ERR_INVALID, "enrolFaces: the gallery does not hold 512-column rows (frt_matcher_init or gallery_begin + commit first)");
            if (m->N > 0 && m->labelled != (labels != nullptr))
                raise(FRT_ERR_INVALID, m->labelled ? "enrolFaces: the gallery is labelled (one label per image)"
                                                   : "enrolFaces: the gallery has no labels (frt_matcher_set_labels first)");
        }
        if (n == 0) {
            if (first_row_out) *first_row_out = rows;
            return;
        }
        use_device(e->device);
        frt_embedder::FaceStage &fs = e->faces;
        fs.d_embeds.reserve((size_t)n * 512);
        embed_face_images(e, faces, n, embeds_out, nullptr, fs.d_embeds.get());
        // one edit: all n rows or none (it takes the matcher's lock itself and checks the gallery's state again)
        const int rc = labels ? frt_matcher_gallery_add_labeled_dev(m, fs.d_embeds.get(), labels, n) : frt_matcher_gallery_add_dev(m, fs.d_embeds.get(), n);
        if (rc != FRT_OK) raise(rc, std::string(frthost::last_error()));
        if (first_row_out) *first_row_out = frt_matcher_num_rows(m) - n;
    });
}


}  // extern "C"
