// libfrt.so: the detector object (weights, network, post-processing) and its C ABI (frt_detector_*, frame ingest).
// All device work is hand-written HIP (kernels_*.hip); there is no CPU fallback anywhere in this file: without a HIP
// device every entry point that needs one fails with FRT_ERR_DEVICE.
#include "frt_detector.hpp"

namespace {

// conv weight [Cout][Cin][3][3] (+BN) -> transposed [Cin][9][Cout] fp32 with the BN scale folded, bias [Cout]
void fold_conv3(const frt::Blob &b, const std::string &conv, const std::string &bn, int cout, int cin, std::vector<float> &w, std::vector<float> &bias) {
    const float *src = b.get(conv + ".weight", (size_t)cout * cin * 9).data;
    std::vector<float> sc, bi;
    frt::bn_fold(b, bn, cout, sc, bi);
    w.assign((size_t)cin * 9 * cout, 0.f);
    for (int co = 0; co < cout; ++co)
        for (int ci = 0; ci < cin; ++ci)
            for (int t = 0; t < 9; ++t) w[((size_t)ci * 9 + t) * cout + co] = src[((size_t)co * cin + ci) * 9 + t] * sc[co];
    bias = bi;
}
void fold_dw(const frt::Blob &b, const std::string &conv, const std::string &bn, int c, std::vector<float> &w, std::vector<float> &bias) {
    const float *src = b.get(conv + ".weight", (size_t)c * 9).data;
    std::vector<float> sc, bi;
    frt::bn_fold(b, bn, c, sc, bi);
    w.resize((size_t)c * 9);
    for (int i = 0; i < c; ++i)
        for (int t = 0; t < 9; ++t) w[(size_t)i * 9 + t] = src[(size_t)i * 9 + t] * sc[i];
    bias = bi;
}
void fold_pw(const frt::Blob &b, const std::string &conv, const std::string &bn, int cout, int cin, std::vector<float> &w, std::vector<float> &bias) {
    const float *src = b.get(conv + ".weight", (size_t)cout * cin).data;
    std::vector<float> sc, bi;
    frt::bn_fold(b, bn, cout, sc, bi);
    w.resize((size_t)cin * cout);
    for (int co = 0; co < cout; ++co)
        for (int ci = 0; ci < cin; ++ci) w[(size_t)ci * cout + co] = src[(size_t)co * cin + ci] * sc[co];
    bias = bi;
}
// bias-only convs (Slim / RFB heads and conv14) as BN-free folds: depthwise [C][9] + bias, pointwise transposed [Cin][Cout] + bias
void dw_bias(const frt::Blob &b, const std::string &conv, int c, std::vector<float> &w, std::vector<float> &bias) {
    const float *src = b.get(conv + ".weight", (size_t)c * 9).data, *bs = b.get(conv + ".bias", c).data;
    w.assign(src, src + (size_t)c * 9);
    bias.assign(bs, bs + c);
}
void pw_bias(const frt::Blob &b, const std::string &conv, int cout, int cin, std::vector<float> &w, std::vector<float> &bias) {
    const float *src = b.get(conv + ".weight", (size_t)cout * cin).data, *bs = b.get(conv + ".bias", cout).data;
    w.resize((size_t)cin * cout);
    for (int co = 0; co < cout; ++co)
        for (int ci = 0; ci < cin; ++ci) w[(size_t)ci * cout + co] = src[(size_t)co * cin + ci];
    bias.assign(bs, bs + cout);
}
// two 3x3 convs (+BN) of the same input as one: fold_conv3 of each, concatenated along Cout (a's channels first)
void fold_conv3_pair(const frt::Blob &b, const std::string &a, int couta, const std::string &c, int coutc, int cin, std::vector<float> &w,
                     std::vector<float> &bias) {
    std::vector<float> wa, wc, bc;
    fold_conv3(b, a + ".0", a + ".1", couta, cin, wa, bias);
    fold_conv3(b, c + ".0", c + ".1", coutc, cin, wc, bc);
    bias.insert(bias.end(), bc.begin(), bc.end());
    const int cout = couta + coutc;
    w.resize((size_t)cin * 9 * cout);
    for (size_t row = 0; row < (size_t)cin * 9; ++row) {
        std::copy(wa.begin() + row * couta, wa.begin() + (row + 1) * couta, w.begin() + row * cout);
        std::copy(wc.begin() + row * coutc, wc.begin() + (row + 1) * coutc, w.begin() + row * cout + couta);
    }
}
inline int conv_out(int x, int stride) { return (x + 2 - 3) / stride + 1; }
inline float f16_to_f32(uint16_t h) {  // exact
    _Float16 x;
    std::memcpy(&x, &h, 2);
    return (float)x;
}
// [Cin][9][Cout] fp32 -> fp16 hi/lo split [Cin/16][9][64][hi16 | lo16] (kernels_det_conv3h.hip); empty unless Cin is 64 or 16 and 16 <= Cout <= 64
std::vector<uint16_t> pack_conv3_split(const std::vector<float> &w, int cin, int cout) {
    if ((cin != 64 && cin != 16) || cout > 64 || cout < 16) return {};
    const int nch = cin / 16;
    std::vector<uint16_t> o((size_t)nch * 9 * 64 * 32, 0);
    for (int c = 0; c < nch; ++c)
        for (int t = 0; t < 9; ++t)
            for (int co = 0; co < cout; ++co)
                for (int k = 0; k < 16; ++k) {
                    const float x = w[((size_t)(c * 16 + k) * 9 + t) * cout + co];
                    const uint16_t hi = frt::f32_to_f16(x);
                    const uint16_t lo = frt::f32_to_f16(x - f16_to_f32(hi));
                    const size_t row = (((size_t)c * 9 + t) * 64 + co) * 32;
                    o[row + k] = hi;
                    o[row + 16 + k] = lo;
                }
    return o;
}
// pointwise weights [Cin][Cout] fp32 -> fp16 hi/lo split [Cout][Cin/16][hi16 | lo16] (dwpw_mfma_kernel / pw_mfma_kernel); empty unless Cin % 16 == 0
std::vector<uint16_t> pack_pw_split(const std::vector<float> &w, int cin, int cout) {
    if (cin % 16) return {};
    std::vector<uint16_t> o((size_t)cout * cin * 2, 0);
    for (int co = 0; co < cout; ++co)
        for (int k = 0; k < cin; ++k) {
            const float x = w[(size_t)k * cout + co];
            const uint16_t hi = frt::f32_to_f16(x);
            const size_t row = ((size_t)co * (cin / 16) + k / 16) * 32;
            o[row + k % 16] = hi;
            o[row + 16 + k % 16] = frt::f32_to_f16(x - f16_to_f32(hi));
        }
    return o;
}
// ---- Slim / RFB (conversion/retina/models/net_slim.py, net_rfb.py): the tensors of the state_dict, shapes included
struct TensorSpec {
    std::string name;
    std::vector<uint32_t> dims;
};
constexpr int SLIM_DW[12][3] = {{16, 32, 1}, {32, 32, 2}, {32, 32, 1}, {32, 64, 2}, {64, 64, 1}, {64, 64, 1}, {64, 64, 1},
                                {64, 128, 2}, {128, 128, 1}, {128, 128, 1}, {128, 256, 2}, {256, 256, 1}};  // conv2 - conv13: cin, cout, stride
constexpr int SLIM_HEAD_C[3] = {64, 128, 256}, SLIM_NA[4] = {3, 2, 2, 3};
// RFB conv8 (BasicRFB(64, 64, scale=1.0), inter_planes 8): branch convs {branch, index, cout, cin, k, dilation}
constexpr int RFB_CONVS[10][6] = {{0, 0, 8, 64, 1, 1}, {0, 1, 16, 8, 3, 1}, {0, 2, 16, 16, 3, 2}, {1, 0, 8, 64, 1, 1}, {1, 1, 16, 8, 3, 1},
                                  {1, 2, 16, 16, 3, 3}, {2, 0, 8, 64, 1, 1}, {2, 1, 12, 8, 3, 1}, {2, 2, 16, 12, 3, 1}, {2, 3, 16, 16, 3, 5}};

std::vector<TensorSpec> slim_tensors(bool rfb, bool landmarks) {
    std::vector<TensorSpec> v;
    auto bn = [&](const std::string &p, uint32_t c) {
        for (const char *f : {".weight", ".bias", ".running_mean", ".running_var"}) v.push_back({p + f, {c}});
    };
    v.push_back({"conv1.0.weight", {16, 3, 3, 3}});
    bn("conv1.1", 16);
    for (int i = 0; i < 12; ++i) {
        const std::string p = "conv" + std::to_string(i + 2);
        const uint32_t cin = SLIM_DW[i][0], cout = SLIM_DW[i][1];
        if (rfb && i == 6) {
            for (const auto &c : RFB_CONVS) {
                const std::string q = "conv8.branch" + std::to_string(c[0]) + "." + std::to_string(c[1]);
                v.push_back({q + ".conv.weight", {(uint32_t)c[2], (uint32_t)c[3], (uint32_t)c[4], (uint32_t)c[4]}});
                bn(q + ".bn", c[2]);
            }
            v.push_back({"conv8.ConvLinear.conv.weight", {64, 48, 1, 1}});
            bn("conv8.ConvLinear.bn", 64);
            v.push_back({"conv8.shortcut.conv.weight", {64, 64, 1, 1}});
            bn("conv8.shortcut.bn", 64);
            continue;
        }
        v.push_back({p + ".0.weight", {cin, 1, 3, 3}});
        bn(p + ".1", cin);
        v.push_back({p + ".3.weight", {cout, cin, 1, 1}});
        bn(p + ".4", cout);
    }
    v.push_back({"conv14.0.weight", {64, 256, 1, 1}});
    v.push_back({"conv14.0.bias", {64}});
    v.push_back({"conv14.2.0.weight", {64, 1, 3, 3}});
    v.push_back({"conv14.2.0.bias", {64}});
    v.push_back({"conv14.2.2.weight", {256, 64, 1, 1}});
    v.push_back({"conv14.2.2.bias", {256}});
    const char *heads[3] = {"loc", "conf", "landm"};
    const uint32_t per[3] = {4, 2, 10};
    for (int h = 0; h < (landmarks ? 3 : 2); ++h) {
        for (int k = 0; k < 3; ++k) {
            const std::string p = std::string(heads[h]) + "." + std::to_string(k);
            const uint32_t c = SLIM_HEAD_C[k], co = per[h] * SLIM_NA[k];
            v.push_back({p + ".0.weight", {c, 1, 3, 3}});
            v.push_back({p + ".0.bias", {c}});
            v.push_back({p + ".2.weight", {co, c, 1, 1}});
            v.push_back({p + ".2.bias", {co}});
        }
        const std::string p = std::string(heads[h]) + ".3";
        v.push_back({p + ".weight", {per[h] * SLIM_NA[3], 256, 3, 3}});
        v.push_back({p + ".bias", {per[h] * SLIM_NA[3]}});
    }
    return v;
}

}  // namespace

// The network a detector blob holds; throws std::runtime_error naming the first missing, misshapen or unexpected tensor of a Slim / RFB blob
// (FRT_ERR_FORMAT at the C ABI).  Host only: frt_detector_describe runs it without a device.
DetLayout det_layout(const frt::Blob &b) {
    DetLayout L;
    L.family = (int)b.kind;
    if (b.kind == 1) {  // mnet0.25: validated tensor by tensor while frt_detector::build folds it
        L.levels = 3;
        L.has_landmarks = b.has("LandmarkHead.0.conv1x1.weight");
        return L;
    }
    if (b.kind != 4 && b.kind != 5) raise(FRT_ERR_FORMAT, "detector: weight blob is not a RetinaFace mobilenet0.25 / Slim / RFB blob");
    L.levels = 4;
    L.has_landmarks = b.has("landm.0.0.weight");
    const std::vector<TensorSpec> spec = slim_tensors(b.kind == 5, L.has_landmarks);
    std::map<std::string, int> want;
    for (const auto &t : spec) {
        want[t.name] = 1;
        auto it = b.t.find(t.name);
        if (it == b.t.end()) throw std::runtime_error("weight blob: missing tensor " + t.name);
        size_t n = 1;
        for (uint32_t d : t.dims) n *= d;
        if (it->second.numel != n || it->second.dims != t.dims)
            throw std::runtime_error("weight blob: wrong shape for " + t.name);
    }
    for (const auto &kv : b.t)
        if (!want.count(kv.first))
            throw std::runtime_error("weight blob: unexpected tensor " + kv.first + (b.kind == 4 ? " (not part of the Slim net)" : " (not part of the RFB net)"));
    return L;
}

// one conv_dw block (dw3x3 + bias -> ReLU -> 1x1 + bias -> ReLU, BN folded) with every weight layout its kernels may use; its scratch
// (tmp) is set once the whole op list is known (frt_detector_create: sized from the ops)
DwPwArgs frt_detector::dwpw_op(const float *in, float *out, const std::vector<float> &w, const std::vector<float> &bias,
                               const std::vector<float> &w2, const std::vector<float> &bias2, int cin, int cout, int h, int w_, int oh, int ow,
                               int stride) {
    const int B = max_batch;
    flops_per_frame += 2.0 * oh * ow * (9.0 * cin + (double)cin * cout);
    std::vector<float> w12((size_t)cin * 12, 0.f);
    for (int ci = 0; ci < cin; ++ci) {
        for (int t = 0; t < 9; ++t) w12[(size_t)ci * 12 + t] = w[(size_t)ci * 9 + t];
        w12[(size_t)ci * 12 + 9] = bias[ci];
    }
    DwPwArgs d{in, out, arena.upload(w), arena.upload(bias), arena.upload(w2), arena.upload(bias2), nullptr, 0, 0,
               B, cin, h, w_, cout, oh, ow, stride, 1, nullptr, arena.upload(w12), nullptr};
    {
        const std::vector<uint16_t> ph = pack_pw_split(w2, cin, cout);
        if (!ph.empty()) d.wph = reinterpret_cast<const half_t *>(arena.upload(ph));
        if (cin % 2 == 0) {  // depthwise weights of channel pairs (kernels_det_wave.hip, kernels_det_stem.hip)
            std::vector<float> wp2((size_t)cin * 10, 0.f);  // [Cin/2][10][2]: taps 0-8, bias; the channel pair interleaved
            for (int ci = 0; ci < cin; ++ci) {
                for (int t = 0; t < 9; ++t) wp2[(size_t)(ci / 2) * 20 + 2 * t + (ci & 1)] = w[(size_t)ci * 9 + t];
                wp2[(size_t)(ci / 2) * 20 + 18 + (ci & 1)] = bias[ci];
            }
            d.wdp = arena.upload(wp2);
            if (cin <= 16) {
                std::vector<float> wt((size_t)cin * 10, 0.f);
                for (int ci = 0; ci < cin; ++ci) {
                    for (int t = 0; t < 9; ++t) wt[((size_t)t * (cin / 2) + ci / 2) * 2 + (ci & 1)] = w[(size_t)ci * 9 + t];
                    wt[((size_t)9 * (cin / 2) + ci / 2) * 2 + (ci & 1)] = bias[ci];
                }
                d.wdt = arena.upload(wt);
            }
        }
        if (!ph.empty() && cout % 32 == 0) {  // the other operands of dwpw_wave_kernel
            std::vector<uint16_t> pf(ph.size());
            const int ng = cin / 16, ncb = cout / 32;
            for (int gq = 0; gq < ng; ++gq)
                for (int cb = 0; cb < ncb; ++cb)
                    for (int part = 0; part < 2; ++part)
                        for (int ln = 0; ln < 64; ++ln)
                            for (int j = 0; j < 8; ++j)
                                pf[((((size_t)gq * ncb + cb) * 2 + part) * 64 + ln) * 8 + j] =
                                    ph[((size_t)(cb * 32 + (ln & 31)) * ng + gq) * 32 + part * 16 + 8 * (ln >> 5) + j];
            if (!d_wave_zeros) {
                d_wave_zeros = arena.alloc<float>(dwpw_wave_zero_bytes() / 4);
                HIPCHK(hipMemset(d_wave_zeros, 0, dwpw_wave_zero_bytes()));
            }
            d.zeros = d_wave_zeros;
            d.wpf = reinterpret_cast<const half_t *>(arena.upload(pf));
        }
    }
    return d;
}

// a plain 1x1 conv + bias + ReLU (BN folded), optionally adding a nearest-upsampled [B][cout][add_h][add_w] tensor behind the ReLU
DwPwArgs frt_detector::pw_op(const float *in, float *out, const std::vector<float> &w2, const std::vector<float> &bias2, int cin, int cout, int h,
                             int w_, const float *add, int add_h, int add_w) {
    flops_per_frame += 2.0 * h * w_ * cin * cout;
    DwPwArgs d{in, out, nullptr, nullptr, arena.upload(w2), arena.upload(bias2), add, add_h, add_w, max_batch, cin, h, w_, cout, h, w_, 1, 1,
               nullptr, nullptr, nullptr};
    const std::vector<uint16_t> ph = pack_pw_split(w2, cin, cout);
    if (!ph.empty()) d.wph = reinterpret_cast<const half_t *>(arena.upload(ph));
    return d;
}

// a dense 3x3 conv + bias + ReLU (w, bias: fold_conv3 / fold_conv3_pair) writing channels [coff, coff + cout) of a ctotal-channel tensor; stride 1:
// with the split-fp16 layout where pack_conv3_split covers the shape
Conv3Args frt_detector::conv3_op(const float *in, float *out, const std::vector<float> &w, const std::vector<float> &bias, int cin, int cout, int h,
                                 int w_, int stride, int ctotal, int coff) {
    Conv3Args c{in, out, arena.upload(w), arena.upload(bias), max_batch, cin, h, w_, cout, conv_out(h, stride), conv_out(w_, stride), stride, 1, ctotal, coff};
    flops_per_frame += 2.0 * cin * 9 * cout * c.Ho * c.Wo;
    if (stride == 1) {
        const std::vector<uint16_t> ph = pack_conv3_split(w, cin, cout);
        if (!ph.empty()) c.wh = reinterpret_cast<const half_t *>(arena.upload(ph));
    }
    return c;
}

frt_detector::Stem frt_detector::stem() {
    Stem st;
    Conv3Op *c = ops.empty() ? nullptr : std::get_if<Conv3Op>(&ops[0]);
    if (!c || c->n != 1) return st;
    st.c = &c->p[0];
    DwPwArgs *d1 = ops.size() >= 3 ? std::get_if<DwPwArgs>(&ops[1]) : nullptr, *d2 = d1 ? std::get_if<DwPwArgs>(&ops[2]) : nullptr;
    if (d2) {
        st.d1 = d1;
        st.d2 = d2;
    }
    return st;
}

void frt_detector::build(const frt::Blob &b) {
    const int H = g.in_h, W = g.in_w;
    std::vector<float> w, bias, w2, bias2;
    auto act = [&](int c, int h, int w_) { return arena.alloc<float>((size_t)max_batch * c * h * w_); };
    const auto ssh = [](int k, const char *name) { return "ssh" + std::to_string(k + 1) + "." + name; };
    // ---- body (net.py:102-124); return layers stage1/2/3 (config.py:17)
    struct L {
        int cin, cout, stride;
    };
    const std::vector<std::pair<std::string, std::vector<L>>> stages = {
        {"stage1", {{3, 8, 2}, {8, 16, 1}, {16, 32, 2}, {32, 32, 1}, {32, 64, 2}, {64, 64, 1}}},
        {"stage2", {{64, 128, 2}, {128, 128, 1}, {128, 128, 1}, {128, 128, 1}, {128, 128, 1}, {128, 128, 1}}},
        {"stage3", {{128, 256, 2}, {256, 256, 1}}}};
    const float *cur = d_input;
    int ch = H, cw = W;
    const float *feat[3];
    int fh[3], fw[3];
    int si = 0;
    for (auto &st : stages) {
        for (size_t i = 0; i < st.second.size(); ++i) {
            const L l = st.second[i];
            const std::string p = "body." + st.first + "." + std::to_string(i);
            const int oh = conv_out(ch, l.stride), ow = conv_out(cw, l.stride);
            float *out = act(l.cout, oh, ow);
            if (l.cin == 3) {
                fold_conv3(b, p + ".0", p + ".1", l.cout, 3, w, bias);
                ops.push_back(Conv3Op{{conv3_op(cur, out, w, bias, 3, l.cout, ch, cw, l.stride, l.cout, 0)}, 1});
            } else {
                fold_dw(b, p + ".0", p + ".1", l.cin, w, bias);
                fold_pw(b, p + ".3", p + ".4", l.cout, l.cin, w2, bias2);
                ops.push_back(dwpw_op(cur, out, w, bias, w2, bias2, l.cin, l.cout, ch, cw, oh, ow, l.stride));
            }
            cur = out;
            ch = oh;
            cw = ow;
        }
        feat[si] = cur;
        fh[si] = ch;
        fw[si] = cw;
        ++si;
    }
    // the first three layers as one kernel (kernels_det_stem.hip): their weights gathered into one buffer
    if (const Stem st = stem(); st.d1 && st.d1->wdt && st.d2->wdt && st.d1->Cin == 8 && st.d1->Cout == 16 && st.d2->Cin == 16 && st.d2->Cout == 32) {
        float *buf = arena.alloc<float>(det_stem_weight_floats());
        det_stem_pack(*st.c, *st.d1, *st.d2, buf, nullptr);
        HIPCHK(hipStreamSynchronize(nullptr));
        st.d1->stem = buf;
    }
    for (int k = 0; k < 3; ++k)
        if (fh[k] != g.fh[k] || fw[k] != g.fw[k]) raise(FRT_ERR_INVALID, "detector: feature-map size mismatch");
    // ---- FPN (net.py:81-98): laterals 1x1+BN+ReLU, nearest-upsample-add top-down (fused), 3x3 merges
    const int cins[3] = {64, 128, 256};
    float *lat[3];
    auto add_lat = [&](int k, const float *addsrc, int ah, int aw) {
        const std::string p = "fpn.output" + std::to_string(k + 1);
        fold_pw(b, p + ".0", p + ".1", 64, cins[k], w2, bias2);
        lat[k] = act(64, fh[k], fw[k]);
        ops.push_back(pw_op(feat[k], lat[k], w2, bias2, cins[k], 64, fh[k], fw[k], addsrc, ah, aw));
    };
    auto add_merge = [&](int k, const float *in, float *out) {
        const std::string p = "fpn.merge" + std::to_string(k + 1);
        fold_conv3(b, p + ".0", p + ".1", 64, 64, w, bias);
        ops.push_back(Conv3Op{{conv3_op(in, out, w, bias, 64, 64, fh[k], fw[k], 1, 64, 0)}, 1});
    };
    add_lat(2, nullptr, 0, 0);
    add_lat(1, lat[2], fh[2], fw[2]);
    float *p4 = act(64, fh[1], fw[1]);
    add_merge(1, lat[1], p4);
    add_lat(0, p4, fh[1], fw[1]);
    float *p3 = act(64, fh[0], fw[0]);
    add_merge(0, lat[0], p3);
    const float *const pyr[3] = {p3, p4, lat[2]};
    // ---- SSH (net.py:55-66) + heads (retinaface_trim.py:14-35).  Every SSH conv ends in a ReLU: either its own or the
    //      ReLU applied to the concat it feeds exclusively.  The same conv on every pyramid level is ONE launch (blockIdx.z = level).
    float *cat[3], *t1[3], *t2[3];
    for (int k = 0; k < 3; ++k) {
        cat[k] = act(64, fh[k], fw[k]);
        t1[k] = act(16, fh[k], fw[k]);
        t2[k] = act(16, fh[k], fw[k]);
    }
    // two convs reading the same tensor on every level: one launch with the output channels concatenated and a split epilogue (a's couta
    // channels -> outa at coffa, c's coutc -> outc); same weights, same summation order as the two separate convs
    auto add_c3_pair_levels = [&](const float *const in[3], int cin, const char *na, int couta, float *const outa[3], int coffa, const char *nc,
                                  int coutc, float *const outc[3]) {
        Conv3Op o{{}, 3};
        for (int k = 0; k < 3; ++k) {
            fold_conv3_pair(b, ssh(k, na), couta, ssh(k, nc), coutc, cin, w, bias);
            o.p[k] = conv3_op(in[k], outa[k], w, bias, cin, couta + coutc, fh[k], fw[k], 1, 64, coffa);
            if (!o.p[k].wh) raise(FRT_ERR_INVALID, "detector: fused SSH conv shape not covered");
            o.p[k].out2 = outc[k];
            o.p[k].split = couta;
            o.p[k].out2_ctotal = 16;
            o.p[k].out2_coff = 0;
        }
        ops.push_back(o);
    };
    add_c3_pair_levels(pyr, 64, "conv3X3", 32, cat, 0, "conv5X5_1", 16, t1);  // -> cat[0:32], t1
    add_c3_pair_levels(t1, 16, "conv5X5_2", 16, cat, 32, "conv7X7_2", 16, t2);  // -> cat[32:48], t2
    {
        Conv3Op o{{}, 3};
        for (int k = 0; k < 3; ++k) {
            fold_conv3(b, ssh(k, "conv7x7_3") + ".0", ssh(k, "conv7x7_3") + ".1", 16, 16, w, bias);
            o.p[k] = conv3_op(t2[k], cat[k], w, bias, 16, 16, fh[k], fw[k], 1, 64, 48);
        }
        ops.push_back(o);
    }
    HeadsOp ho{{}, 3};
    for (int k = 0; k < 3; ++k) {
        std::vector<float> wc, bc;
        pw_bias(b, "BboxHead." + std::to_string(k) + ".conv1x1", 8, 64, w, bias);
        pw_bias(b, "ClassHead." + std::to_string(k) + ".conv1x1", 4, 64, wc, bc);
        ho.p[k] = HeadArgs{cat[k], arena.upload(w), arena.upload(bias), arena.upload(wc), arena.upload(bc), d_loc, d_conf, max_batch, 64, fh[k], fw[k], g.A,
                           g.base[k], nullptr, nullptr, nullptr};
        flops_per_frame += 2.0 * fh[k] * fw[k] * 64 * 12;
        if (has_landmarks) {
            pw_bias(b, "LandmarkHead." + std::to_string(k) + ".conv1x1", 20, 64, w, bias);
            ho.p[k].wl = arena.upload(w);
            ho.p[k].bl = arena.upload(bias);
            ho.p[k].ldm = d_ldm;
            flops_per_frame += 2.0 * fh[k] * fw[k] * 64 * 20;
        }
    }
    ops.push_back(ho);
}

// Slim (net_slim.py) and RFB (net_rfb.py): conv_bn + 12 conv_dw blocks (RFB: conv8 is a BasicRFB), conv14, and the loc / conf / landm heads
// of four levels (x8, x11, x13, x14).  Blob validated by det_layout.
void frt_detector::build_slim(const frt::Blob &b, bool rfb) {
    const int B = max_batch, H = g.in_h, W = g.in_w;
    std::vector<float> w, bias, w2, bias2;
    auto act = [&](int c, int h, int w_) { return arena.alloc<float>((size_t)B * c * h * w_); };
    int ch = conv_out(H, 2), cw = conv_out(W, 2);
    float *cur = act(16, ch, cw);
    {  // conv1 = conv_bn(3, 16, 2): preprocess + the generic first conv (the fused u8 first conv covers mnet's Cout = 8 only)
        fold_conv3(b, "conv1.0", "conv1.1", 16, 3, w, bias);
        ops.push_back(Conv3Op{{conv3_op(d_input, cur, w, bias, 3, 16, H, W, 2, 16, 0)}, 1});
    }
    const float *feat[4];
    int fh[4], fw[4];
    for (int i = 0; i < 12; ++i) {
        const int cin = SLIM_DW[i][0], cout = SLIM_DW[i][1], stride = SLIM_DW[i][2];
        const int oh = conv_out(ch, stride), ow = conv_out(cw, stride);
        float *out = act(cout, oh, ow);
        if (rfb && i == 6) {  // conv8 = BasicRFB(64, 64, scale = 1.0): 5 launches (kernels_det_slim.hip)
            const int HW = ch * cw;
            float *red = act(24, ch, cw), *sc = act(64, ch, cw), *ta = act(44, ch, cw), *tb = act(16, ch, cw), *cat = act(48, ch, cw);
            std::vector<float> wp((size_t)64 * 88), bp(88);
            for (int j = 0; j < 3; ++j) {
                const std::string q = "conv8.branch" + std::to_string(j) + ".0";
                fold_pw(b, q + ".conv", q + ".bn", 8, 64, w2, bias2);
                for (int ci = 0; ci < 64; ++ci)
                    for (int co = 0; co < 8; ++co) wp[(size_t)ci * 88 + j * 8 + co] = w2[(size_t)ci * 8 + co];
                for (int co = 0; co < 8; ++co) bp[j * 8 + co] = bias2[co];
            }
            fold_pw(b, "conv8.shortcut.conv", "conv8.shortcut.bn", 64, 64, w2, bias2);
            for (int ci = 0; ci < 64; ++ci)
                for (int co = 0; co < 64; ++co) wp[(size_t)ci * 88 + 24 + co] = w2[(size_t)ci * 64 + co];
            for (int co = 0; co < 64; ++co) bp[24 + co] = bias2[co];
            ops.push_back(RfbProjArgs{cur, arena.upload(wp), arena.upload(bp), red, sc, B, ch, cw});
            flops_per_frame += 2.0 * HW * 64 * 88;
            // 3x3 convs: {branch.index, cin, cout, dilation, relu, in, in_ctotal, in_coff, out, out_ctotal, out_coff}
            struct C3 {
                const char *name;
                int cin, cout, dil, relu;
                const float *in;
                int ict, ico;
                float *out;
                int oct, oco;
            };
            const C3 stages[3][3] = {{{"branch0.1", 8, 16, 1, 1, red, 24, 0, ta, 44, 0}, {"branch1.1", 8, 16, 1, 1, red, 24, 8, ta, 44, 16},
                                      {"branch2.1", 8, 12, 1, 1, red, 24, 16, ta, 44, 32}},
                                     {{"branch2.2", 12, 16, 1, 1, ta, 44, 32, tb, 16, 0}, {}, {}},
                                     {{"branch0.2", 16, 16, 2, 0, ta, 44, 0, cat, 48, 0}, {"branch1.2", 16, 16, 3, 0, ta, 44, 16, cat, 48, 16},
                                      {"branch2.3", 16, 16, 5, 0, tb, 16, 0, cat, 48, 32}}};
            for (int st = 0; st < 3; ++st) {
                RfbConvOp c{{}, st == 1 ? 1 : 3};
                c.a.B = B;
                c.a.H = ch;
                c.a.W = cw;
                for (int k = 0; k < c.n; ++k) {
                    const C3 &d = stages[st][k];
                    const std::string q = std::string("conv8.") + d.name;
                    if (d.cin > 16 || d.cout > 16) raise(FRT_ERR_INVALID, "detector: RFB conv shape not covered");
                    fold_conv3(b, q + ".conv", q + ".bn", d.cout, d.cin, w, bias);
                    std::vector<float> wpad((size_t)d.cin * 9 * 16, 0.f), bpad(16, 0.f);
                    for (size_t r = 0; r < (size_t)d.cin * 9; ++r)
                        for (int co = 0; co < d.cout; ++co) wpad[r * 16 + co] = w[r * d.cout + co];
                    for (int co = 0; co < d.cout; ++co) bpad[co] = bias[co];
                    c.a.p[k] = RfbConvArgs{d.in, d.out, arena.upload(wpad), arena.upload(bpad), d.cin, d.cout, d.dil, d.relu, d.ict, d.ico, d.oct, d.oco};
                    flops_per_frame += 2.0 * HW * d.cin * 9 * d.cout;
                }
                for (int k = c.n; k < 3; ++k) c.a.p[k] = c.a.p[0];
                ops.push_back(c);
            }
            fold_pw(b, "conv8.ConvLinear.conv", "conv8.ConvLinear.bn", 64, 48, w2, bias2);
            ops.push_back(RfbTailArgs{cat, arena.upload(w2), arena.upload(bias2), sc, out, 1.0f, B, ch, cw});
            flops_per_frame += 2.0 * HW * 48 * 64;
        } else {
            const std::string p = "conv" + std::to_string(i + 2);
            fold_dw(b, p + ".0", p + ".1", cin, w, bias);
            fold_pw(b, p + ".3", p + ".4", cout, cin, w2, bias2);
            ops.push_back(dwpw_op(cur, out, w, bias, w2, bias2, cin, cout, ch, cw, oh, ow, stride));
        }
        cur = out;
        ch = oh;
        cw = ow;
        const int lv = i == 6 ? 0 : (i == 9 ? 1 : (i == 11 ? 2 : -1));
        if (lv >= 0) {
            feat[lv] = cur;
            fh[lv] = ch;
            fw[lv] = cw;
        }
    }
    {  // conv14: 1x1 256 -> 64 + bias + ReLU, then depth_conv2d(64, 256, 3, stride 2) + ReLU (a conv_dw block with biases for BN)
        float *mid = act(64, ch, cw);
        pw_bias(b, "conv14.0", 64, 256, w2, bias2);
        ops.push_back(pw_op(cur, mid, w2, bias2, 256, 64, ch, cw, nullptr, 0, 0));
        const int oh = conv_out(ch, 2), ow = conv_out(cw, 2);
        float *out = act(256, oh, ow);
        dw_bias(b, "conv14.2.0", 64, w, bias);
        pw_bias(b, "conv14.2.2", 256, 64, w2, bias2);
        ops.push_back(dwpw_op(mid, out, w, bias, w2, bias2, 64, 256, ch, cw, oh, ow, 2));
        feat[3] = out;
        fh[3] = oh;
        fw[3] = ow;
    }
    for (int k = 0; k < 4; ++k)
        if (fh[k] != g.fh[k] || fw[k] != g.fw[k]) raise(FRT_ERR_INVALID, "detector: feature-map size mismatch");
    const char *heads[3] = {"loc", "conf", "landm"};
    const int per[3] = {4, 2, 10}, chan0[3] = {0, 12, 18};  // channel offsets of the three heads in the kernels' 48-channel layout
    const int nh = has_landmarks ? 3 : 2;
    SlimHeadsOp ho{{}, 3};
    ho.a.loc = d_loc;
    ho.a.conf = d_conf;
    ho.a.ldm = has_landmarks ? d_ldm : nullptr;
    ho.a.B = B;
    ho.a.A = g.A;
    for (int k = 0; k < 3; ++k) {
        const int C = SLIM_HEAD_C[k], na = SLIM_NA[k];
        std::vector<float> wd((size_t)C * 30, 0.f), wp((size_t)C * 48, 0.f), bp(48, 0.f);
        for (int h = 0; h < nh; ++h) {
            const std::string p = std::string(heads[h]) + "." + std::to_string(k);
            dw_bias(b, p + ".0", C, w, bias);
            for (int ci = 0; ci < C; ++ci) {
                for (int t = 0; t < 9; ++t) wd[(size_t)ci * 30 + h * 10 + t] = w[(size_t)ci * 9 + t];
                wd[(size_t)ci * 30 + h * 10 + 9] = bias[ci];
            }
            const int co_n = per[h] * na;
            pw_bias(b, p + ".2", co_n, C, w2, bias2);
            for (int ci = 0; ci < C; ++ci)
                for (int co = 0; co < co_n; ++co) wp[(size_t)ci * 48 + chan0[h] + co] = w2[(size_t)ci * co_n + co];
            for (int co = 0; co < co_n; ++co) bp[chan0[h] + co] = bias2[co];
            flops_per_frame += 2.0 * fh[k] * fw[k] * C * (9.0 + co_n);
        }
        ho.a.lv[k] = SlimHeadArgs{feat[k], arena.upload(wd), arena.upload(wp), arena.upload(bp), C, fh[k], fw[k], na, g.base[k]};
    }
    ops.push_back(ho);
    {  // level 3: loc / conf / landm = dense 3x3 convs 256 -> 12 / 6 / 30 (+ bias), one launch with the channels concatenated
        const int na = SLIM_NA[3], cout = na * (has_landmarks ? 16 : 6), cpad = (cout + 15) / 16 * 16;
        std::vector<float> wc((size_t)256 * 9 * cpad, 0.f), bc(cpad, 0.f);
        int off = 0;
        for (int h = 0; h < nh; ++h) {
            const std::string p = std::string(heads[h]) + ".3";
            const int co_n = per[h] * na;
            const float *src = b.get(p + ".weight", (size_t)co_n * 256 * 9).data, *bs = b.get(p + ".bias", co_n).data;
            for (int co = 0; co < co_n; ++co) {
                for (int ci = 0; ci < 256; ++ci)
                    for (int t = 0; t < 9; ++t) wc[((size_t)ci * 9 + t) * cpad + off + co] = src[((size_t)co * 256 + ci) * 9 + t];
                bc[off + co] = bs[co];
            }
            off += co_n;
        }
        ops.push_back(DenseHeadArgs{feat[3], arena.upload(wc), arena.upload(bc), d_loc, d_conf, has_landmarks ? d_ldm : nullptr, B, 256, fh[3], fw[3], na, cout,
                                    cpad, g.A, g.base[3]});
        flops_per_frame += 2.0 * fh[3] * fw[3] * 256 * 9 * cout;
    }
}

void frt_detector::preprocess(const uint8_t *frames_dev, int n, size_t row_stride, size_t frame_stride, hipStream_t s) {
    ProfScope ps(2, "det_preprocess", (double)n * g.frame_h * g.frame_w * 3, s);
    launch_det_preprocess(frames_dev, n, g.frame_h, g.frame_w, row_stride, frame_stride, g.in_h, g.in_w, d_input, s);
}

void frt_detector::forward_frames(const uint8_t *frames_dev, int n, size_t row_stride, size_t frame_stride, hipStream_t s) {
    // the one place that knows how many leading ops a fused kernel stood in for: the stem kernel for ops 0 - 2, the u8 first conv for op 0
    int done = 0;
    if (const Stem st = stem(); st.c && g.frame_h == g.in_h && g.frame_w == g.in_w) {
        Conv3Args c = *st.c;
        c.B = n;
        if (st.d1) {  // first conv + the first two conv_dw blocks in one kernel
            ProfScope ps(2, "det_stem", (double)n * g.frame_h * g.frame_w * 3, s);
            if (launch_det_stem(frames_dev, row_stride, frame_stride, c, *st.d1, *st.d2, s)) done = 3;
        }
        if (!done) {
            ProfScope ps(2, "det_preprocess", (double)n * g.frame_h * g.frame_w * 3, s);  // fused into the first conv
            if (launch_det_conv1_u8(frames_dev, row_stride, frame_stride, c, s)) done = 1;
        }
    }
    if (!done) preprocess(frames_dev, n, row_stride, frame_stride, s);
    forward(n, s, done);
}

void frt_detector::forward(int n, hipStream_t s, int first_op) {
    ProfScope ps(2, "det_network", flops_per_frame * n, s);
    for (size_t i = first_op; i < ops.size(); ++i) run_op(i, n, s);
    HIPCHK(hipGetLastError());  // a failed launch (e.g. the dynamic-LDS opt-in missing on this device) must not pass silently
}

void frt_detector::postprocess(int n, hipStream_t s, frt_bbox *boxes_out, int *nout_out, float *landmarks_out) {
    ProfScope ps(2, "det_postprocess", (double)n * g.A, s);
    frt_bbox *bo = boxes_out ? boxes_out : d_boxes;  // the pipeline passes its slot buffers: no device-to-device copies afterwards
    int *no = nout_out ? nout_out : d_nout;
    launch_decode(d_loc, d_conf, n, g, d_cand, d_cand_count, s);
    launch_nms(d_cand, d_loc, d_cand_count, n, g, d_dead, bo, no, d_kept_anchor, s);
    if (has_landmarks) launch_landmark_decode(d_ldm, d_kept_anchor, no, n, g, landmarks_out ? landmarks_out : d_landmarks, s);
    HIPCHK(hipGetLastError());
}

namespace {

// frt_detector_find_faces_batch, and with landmarks_out frt_detector_find_faces_landmarks
void find_faces(frt_detector *d, const uint8_t *bgr, int n_frames, int rows, int cols, size_t row_stride, size_t frame_stride, frt_bbox *out,
                float *landmarks_out, int *n_out) {
    if (!d || !bgr || !out || !n_out) raise(FRT_ERR_INVALID, "null argument");
    if (landmarks_out && !d->has_landmarks) raise(FRT_ERR_FORMAT, "findFaceLandmarks: the detector blob has no LandmarkHead (trimmed export)");
    if (rows != d->g.frame_h || cols != d->g.frame_w) raise(FRT_ERR_INVALID, "findFace: frame must be frameWidth x frameHeight");
    if (n_frames < 1 || n_frames > d->max_batch) raise(FRT_ERR_CAPACITY, "findFace: more frames than det_maxBatchSize");
    std::lock_guard<std::mutex> lk(d->mu);
    use_device(d->device);
    hipStream_t s = d->stream;
    d->wait_idle(s);
    const size_t tight = (size_t)cols * 3;
    for (int f = 0; f < n_frames; ++f)
        HIPCHK(hipMemcpy2DAsync(d->d_frames + (size_t)f * rows * tight, tight, bgr + (size_t)f * frame_stride, row_stride, tight, rows,
                                hipMemcpyHostToDevice, s));
    d->forward_frames(d->d_frames, n_frames, tight, (size_t)rows * tight, s);
    d->postprocess(n_frames, s);
    HIPCHK(hipMemcpyAsync(out, d->d_boxes, sizeof(frt_bbox) * n_frames * d->g.max_faces, hipMemcpyDeviceToHost, s));
    if (landmarks_out) HIPCHK(hipMemcpyAsync(landmarks_out, d->d_landmarks, sizeof(float) * 10 * n_frames * d->g.max_faces, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(n_out, d->d_nout, sizeof(int) * n_frames, hipMemcpyDeviceToHost, s));
    sync_stream_spinning(s);
}

// frt_detector_infer, and with ldm_out frt_detector_infer_landmarks
void infer(frt_detector *d, const float *chw, int batch, float *loc_out, float *conf_out, float *ldm_out) {
    if (!d || !chw || !loc_out || !conf_out) raise(FRT_ERR_INVALID, "null argument");
    if (ldm_out && !d->has_landmarks) raise(FRT_ERR_FORMAT, "doInference: the detector blob has no LandmarkHead (trimmed export)");
    if (batch < 1 || batch > d->max_batch) raise(FRT_ERR_CAPACITY, "doInference: batch exceeds det_maxBatchSize");
    std::lock_guard<std::mutex> lk(d->mu);
    use_device(d->device);
    hipStream_t s = d->stream;
    d->wait_idle(s);
    const size_t in_elems = (size_t)3 * d->g.in_h * d->g.in_w;
    HIPCHK(hipMemcpyAsync(d->d_input, chw, sizeof(float) * in_elems * batch, hipMemcpyHostToDevice, s));
    d->forward(batch, s);
    HIPCHK(hipMemcpyAsync(loc_out, d->d_loc, sizeof(float) * (size_t)batch * d->g.A * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(conf_out, d->d_conf, sizeof(float) * (size_t)batch * d->g.A * 2, hipMemcpyDeviceToHost, s));
    if (ldm_out) HIPCHK(hipMemcpyAsync(ldm_out, d->d_ldm, sizeof(float) * (size_t)batch * d->g.A * 10, hipMemcpyDeviceToHost, s));
    sync_stream_spinning(s);
}

}  // namespace

DetGeom det_geometry(int family, int levels, int in_w, int in_h, int frame_w, int frame_h, float nms_threshold, float bbox_threshold, int max_faces) {
    DetGeom g{};
    g.in_w = in_w; g.in_h = in_h; g.frame_w = frame_w; g.frame_h = frame_h;
    // the anchor table of the network's own training config: cfg_mnet, or cfg_slim / cfg_rfb (conversion/retina/config.py)
    static const int mnet_sizes[3][DET_MAX_SIZES] = {{10, 20}, {32, 64}, {128, 256}}, mnet_n[3] = {2, 2, 2};
    static const int slim_sizes[4][DET_MAX_SIZES] = {{10, 16, 24}, {32, 48}, {64, 96}, {128, 192, 256}}, slim_n[4] = {3, 2, 2, 3};
    const bool mnet = family == 1;
    g.levels = levels;
    int base = 0;
    for (int k = 0; k < g.levels; ++k) {
        g.step[k] = (float)(8 << k);
        g.nsz[k] = mnet ? mnet_n[k] : slim_n[k];
        for (int l = 0; l < DET_MAX_SIZES; ++l) g.min_size[k][l] = mnet ? mnet_sizes[k][l] : slim_sizes[k][l];
        g.fh[k] = (int)std::ceil(in_h / g.step[k]);
        g.fw[k] = (int)std::ceil(in_w / g.step[k]);
        g.base[k] = base;
        base += g.fh[k] * g.fw[k] * g.nsz[k];
    }
    g.A = base;
    g.scale_h = (float)in_h / frame_h;  // retinaface.cpp:21-22
    g.scale_w = (float)in_w / frame_w;
    g.nms_thr = nms_threshold;
    g.bbox_thr = bbox_threshold;
    g.max_faces = max_faces;
    return g;
}

extern "C" {

int frt_detector_create(const char *weights_path, int frame_w, int frame_h, int in_c, int in_h, int in_w, int max_batch, int max_faces,
                        float nms_threshold, float bbox_threshold, int device, frt_detector **out) {
    return guarded([&] {
        if (!out || !weights_path) raise(FRT_ERR_INVALID, "null argument");
        *out = nullptr;
        if (in_c != 3 || in_h < 32 || in_w < 32 || frame_w < 1 || frame_h < 1 || max_batch < 1 || max_faces < 1)
            raise(FRT_ERR_INVALID, "detector: invalid shape arguments");
        frt::Blob blob;
        std::string err;
        const int rc = blob.load(weights_path, err);
        if (rc) raise(rc, err);
        const DetLayout layout = det_layout(blob);  // (host only: a malformed blob fails before any HIP call)
        use_device(device);
        std::unique_ptr<frt_detector> d(new frt_detector);
        d->device = device;
        d->max_batch = max_batch;
        d->family = layout.family;
        d->g = det_geometry(layout.family, layout.levels, in_w, in_h, frame_w, frame_h, nms_threshold, bbox_threshold, max_faces);
        const DetGeom &g = d->g;
        const bool mnet = layout.family == 1;
        HIPCHK(hipStreamCreate(&d->stream));
        HIPCHK(hipEventCreateWithFlags(&d->ev_busy, hipEventDisableTiming));
        const size_t B = (size_t)max_batch;
        d->d_frames = d->arena.alloc<uint8_t>(B * frame_h * frame_w * 3);
        d->d_input = d->arena.alloc<float>(B * 3 * in_h * in_w);
        d->d_loc = d->arena.alloc<float>(B * g.A * 4);
        d->d_conf = d->arena.alloc<float>(B * g.A * 2);
        d->d_cand = d->arena.alloc<Candidate>(B * g.A);
        d->d_cand_count = d->arena.alloc<int>((size_t)B * 32);  // one 128-byte line per frame (kernels_post.hip: CC_STRIDE)
        HIPCHK(hipMemset(d->d_cand_count, 0, sizeof(int) * B * 32));  // kept at zero between calls by nms_kernel
        d->d_nout = d->arena.alloc<int>(B);
        d->d_dead = d->arena.alloc<uint8_t>(B * g.A);
        d->d_boxes = d->arena.alloc<frt_bbox>(B * max_faces);
        d->has_landmarks = layout.has_landmarks;
        if (d->has_landmarks) {
            d->d_ldm = d->arena.alloc<float>(B * g.A * 10);
            d->d_kept_anchor = d->arena.alloc<int>(B * max_faces);
            d->d_landmarks = d->arena.alloc<float>(B * max_faces * 10);
        }
        if (mnet) d->build(blob);
        else d->build_slim(blob, layout.family == 5);
        // scratch of the split depthwise -> pointwise path: the largest depthwise intermediate of the built conv_dw ops
        size_t tmp = B * 64 * (size_t)g.fh[0] * g.fw[0];
        for (const auto &o : d->ops)
            if (const DwPwArgs *dw = std::get_if<DwPwArgs>(&o); dw && dw->wd) tmp = std::max(tmp, B * dw->Cin * (size_t)dw->Ho * dw->Wo);
        d->d_tmp = d->arena.alloc<float>(tmp);
        for (auto &o : d->ops)
            if (DwPwArgs *dw = std::get_if<DwPwArgs>(&o); dw && dw->wd) dw->tmp = d->d_tmp;
        HIPCHK(hipDeviceSynchronize());
        *out = d.release();
    });
}

void frt_detector_destroy(frt_detector *d) {
    if (!d) return;
    (void)hipSetDevice(d->device);
    if (d->stream) {
        (void)hipStreamSynchronize(d->stream);
        (void)hipStreamDestroy(d->stream);
    }
    if (d->ev_busy) (void)hipEventDestroy(d->ev_busy);
    d->arena.release();
    delete d;
}

int frt_detector_describe(const char *weights_path, int *family, int *levels, int *has_landmarks) {
    return guarded([&] {
        if (!weights_path) raise(FRT_ERR_INVALID, "null argument");
        frt::Blob blob;
        std::string err;
        const int rc = blob.load(weights_path, err);
        if (rc) raise(rc, err);
        const DetLayout layout = det_layout(blob);
        if (family) *family = layout.family;
        if (levels) *levels = layout.levels;
        if (has_landmarks) *has_landmarks = layout.has_landmarks ? 1 : 0;
    });
}

int frt_detector_num_anchors(const frt_detector *d) { return d ? d->g.A : 0; }
int frt_detector_geometry(const frt_detector *d, int *frame_w, int *frame_h, int *max_batch, int *max_faces, int *device) {
    if (!d) return FRT_ERR_INVALID;
    if (frame_w) *frame_w = d->g.frame_w;
    if (frame_h) *frame_h = d->g.frame_h;
    if (max_batch) *max_batch = d->max_batch;
    if (max_faces) *max_faces = d->g.max_faces;
    if (device) *device = d->device;
    return FRT_OK;
}

int frt_detector_find_faces_batch(frt_detector *d, const uint8_t *bgr, int n_frames, int rows, int cols, size_t row_stride,
                                  size_t frame_stride, frt_bbox *out, int *n_out) {
    return guarded([&] { find_faces(d, bgr, n_frames, rows, cols, row_stride, frame_stride, out, nullptr, n_out); });
}

int frt_detector_find_faces(frt_detector *d, const uint8_t *bgr, int rows, int cols, size_t row_stride, frt_bbox *out, int *n_out) {
    return frt_detector_find_faces_batch(d, bgr, 1, rows, cols, row_stride, row_stride * (size_t)rows, out, n_out);
}

int frt_detector_has_landmarks(const frt_detector *d) { return d && d->has_landmarks ? 1 : 0; }

int frt_detector_find_faces_landmarks(frt_detector *d, const uint8_t *bgr, int rows, int cols, size_t row_stride, frt_bbox *out,
                                      float *landmarks_out, int *n_out) {
    return guarded([&] {
        if (!landmarks_out) raise(FRT_ERR_INVALID, "null argument");
        find_faces(d, bgr, 1, rows, cols, row_stride, row_stride * (size_t)rows, out, landmarks_out, n_out);
    });
}

int frt_detector_preprocess(frt_detector *d, const uint8_t *bgr, int rows, int cols, size_t row_stride, float *chw_out) {
    return guarded([&] {
        if (!d || !bgr || !chw_out) raise(FRT_ERR_INVALID, "null argument");
        if (rows != d->g.frame_h || cols != d->g.frame_w) raise(FRT_ERR_INVALID, "preprocess: frame must be frameWidth x frameHeight");
        std::lock_guard<std::mutex> lk(d->mu);
        use_device(d->device);
        hipStream_t s = d->stream;
        d->wait_idle(s);
        const size_t tight = (size_t)cols * 3;
        HIPCHK(hipMemcpy2DAsync(d->d_frames, tight, bgr, row_stride, tight, rows, hipMemcpyHostToDevice, s));
        d->preprocess(d->d_frames, 1, tight, (size_t)rows * tight, s);
        HIPCHK(hipMemcpyAsync(chw_out, d->d_input, sizeof(float) * 3 * d->g.in_h * d->g.in_w, hipMemcpyDeviceToHost, s));
        sync_stream_spinning(s);
    });
}

int frt_detector_infer(frt_detector *d, const float *chw, int batch, float *loc_out, float *conf_out) {
    return guarded([&] { infer(d, chw, batch, loc_out, conf_out, nullptr); });
}

int frt_detector_infer_landmarks(frt_detector *d, const float *chw, int batch, float *loc_out, float *conf_out, float *ldm_out) {
    return guarded([&] {
        if (!ldm_out) raise(FRT_ERR_INVALID, "null argument");
        infer(d, chw, batch, loc_out, conf_out, ldm_out);
    });
}

int frt_detector_postprocess(frt_detector *d, const float *loc, const float *conf, frt_bbox *out, int *n_out) {
    return guarded([&] {
        if (!d || !loc || !conf || !out || !n_out) raise(FRT_ERR_INVALID, "null argument");
        std::lock_guard<std::mutex> lk(d->mu);
        use_device(d->device);
        hipStream_t s = d->stream;
        d->wait_idle(s);
        HIPCHK(hipMemcpyAsync(d->d_loc, loc, sizeof(float) * (size_t)d->g.A * 4, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(d->d_conf, conf, sizeof(float) * (size_t)d->g.A * 2, hipMemcpyHostToDevice, s));
        d->postprocess(1, s);
        HIPCHK(hipMemcpyAsync(out, d->d_boxes, sizeof(frt_bbox) * d->g.max_faces, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(n_out, d->d_nout, sizeof(int), hipMemcpyDeviceToHost, s));
        sync_stream_spinning(s);
    });
}

// -------------------------------------------------------------------------------------------------------- frame ingest
int frt_resize_frame(const uint8_t *bgr, int rows, int cols, size_t row_stride, uint8_t *out, int out_rows, int out_cols, int device) {
    return guarded([&] {
        if (!bgr || !out || rows < 1 || cols < 1 || out_rows < 1 || out_cols < 1) raise(FRT_ERR_INVALID, "resize: bad argument");
        if (device >= 0) use_device(device);
        Arena a;
        struct Guard {
            Arena &a;
            ~Guard() { a.release(); }
        } guard{a};
        const size_t tight = (size_t)cols * 3, otight = (size_t)out_cols * 3;
        uint8_t *d_src = a.alloc<uint8_t>((size_t)rows * tight);
        uint8_t *d_dst = a.alloc<uint8_t>((size_t)out_rows * otight);
        HIPCHK(hipMemcpy2D(d_src, tight, bgr, row_stride, tight, rows, hipMemcpyHostToDevice));
        launch_resize_linear(d_src, 1, rows, cols, tight, 0, d_dst, out_rows, out_cols, otight, 0, nullptr);
        HIPCHK(hipMemcpy(out, d_dst, (size_t)out_rows * otight, hipMemcpyDeviceToHost));
    });
}

int frt_resize_frames_dev(const void *src_dev, int n, int rows, int cols, size_t row_stride, size_t frame_stride, void *dst_dev, int out_rows,
                          int out_cols, void *hip_stream) {
    return guarded([&] {
        if (!src_dev || !dst_dev || n < 0 || rows < 1 || cols < 1 || out_rows < 1 || out_cols < 1) raise(FRT_ERR_INVALID, "resize: bad argument");
        launch_resize_linear(reinterpret_cast<const uint8_t *>(src_dev), n, rows, cols, row_stride, frame_stride, reinterpret_cast<uint8_t *>(dst_dev),
                             out_rows, out_cols, (size_t)out_cols * 3, (size_t)out_rows * out_cols * 3, reinterpret_cast<hipStream_t>(hip_stream));
        HIPCHK(hipGetLastError());
    });
}


}  // extern "C"
