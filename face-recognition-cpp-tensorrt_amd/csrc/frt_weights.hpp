// FRTW weight-blob reader + host-side folding helpers (see weights_io.py for the format).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <stdexcept>
#include <string>
#include <vector>

namespace frt {

struct Tensor {
    const float *data = nullptr;
    std::vector<uint32_t> dims;
    size_t numel = 0;
};

class Blob {
  public:
    uint32_t kind = 0;
    std::map<std::string, Tensor> t;
    std::vector<char> buf;

    // returns 0 ok, 2 not found, 3 malformed
    int load(const char *path, std::string &err) {
        FILE *f = std::fopen(path, "rb");
        if (!f) {
            err = "Cant find engine file";  // the reference's message (src/retinaface.cpp:53, src/arcface.cpp:67)
            return 2;
        }
        std::fseek(f, 0, SEEK_END);
        long sz = std::ftell(f);
        std::fseek(f, 0, SEEK_SET);
        if (sz < 0) {  // not seekable (directory, pipe): ftell failed
            std::fclose(f);
            err = "weight blob: bad magic / truncated file";
            return 3;
        }
        buf.resize((size_t)sz);
        size_t rd = std::fread(buf.data(), 1, (size_t)sz, f);
        std::fclose(f);
        if ((long)rd != sz || sz < 16 || std::memcmp(buf.data(), "FRTW0001", 8) != 0) {
            err = "weight blob: bad magic / truncated file";
            return 3;
        }
        uint32_t n;
        std::memcpy(&kind, buf.data() + 8, 4);
        std::memcpy(&n, buf.data() + 12, 4);
        size_t p = 16;
        for (uint32_t i = 0; i < n; ++i) {
            if (p + 2 > buf.size()) return bad(err);
            uint16_t ln;
            std::memcpy(&ln, buf.data() + p, 2);
            p += 2;
            if (p + ln + 1 > buf.size()) return bad(err);
            std::string name(buf.data() + p, ln);
            p += ln;
            uint8_t nd = (uint8_t)buf[p++];
            Tensor x;
            if (p + 4u * nd + 16 > buf.size()) return bad(err);
            for (int d = 0; d < nd; ++d) {
                uint32_t v;
                std::memcpy(&v, buf.data() + p, 4);
                p += 4;
                x.dims.push_back(v);
            }
            uint64_t off, ne;
            std::memcpy(&off, buf.data() + p, 8);
            std::memcpy(&ne, buf.data() + p + 8, 8);
            p += 16;
            if ((off & 3) || off > buf.size() || ne > (buf.size() - off) / 4) return bad(err);  // (no uint64 wrap: ne is checked against the room left)
            x.data = reinterpret_cast<const float *>(buf.data() + off);
            x.numel = (size_t)ne;
            t[name] = x;
        }
        return 0;
    }
    bool has(const std::string &n) const { return t.count(n) != 0; }
    const Tensor &get(const std::string &n, size_t expect_numel) const {
        auto it = t.find(n);
        if (it == t.end()) throw std::runtime_error("weight blob: missing tensor " + n);
        if (expect_numel && it->second.numel != expect_numel) throw std::runtime_error("weight blob: wrong size for " + n);
        return it->second;
    }

  private:
    static int bad(std::string &err) {
        err = "weight blob: malformed header";
        return 3;
    }
};

// BatchNorm (eval) as y = x*scale + bias; eps = 1e-5 (PyTorch default, never overridden by the reference).
inline void bn_fold(const Blob &b, const std::string &p, int c, std::vector<float> &scale, std::vector<float> &bias) {
    const float *g = b.get(p + ".weight", c).data, *be = b.get(p + ".bias", c).data;
    const float *mu = b.get(p + ".running_mean", c).data, *var = b.get(p + ".running_var", c).data;
    scale.resize(c);
    bias.resize(c);
    for (int i = 0; i < c; ++i) {
        const double s = (double)g[i] / std::sqrt((double)var[i] + 1e-5);
        scale[i] = (float)s;
        bias[i] = (float)((double)be[i] - (double)mu[i] * s);
    }
}

// ArcFace IR / IR-SE backbone layout, read from the tensors of a kind-2 (IR) or kind-3 (IR-SE) blob (model_irse.py:97-125, get_blocks(50 |
// 100 | 152)).  The units are body.0 .. body.N-1 in order; a unit opens a stage where its conv1 changes width or it carries a shortcut conv
// (body.0 opens stage 1: 64 -> 64, stride 2, MaxPool shortcut).  Accepted: the three stage tables of model_irse.py with widths 64 / 128 / 256 /
// 512, every unit SE iff the blob is IR-SE.  Anything else - a missing or mis-sized tensor, a body.* tensor no unit owns, a shortcut where the
// width does not change, SE mixed with plain units, another stage table - throws std::runtime_error naming the tensor (FRT_ERR_FORMAT at the
// C ABI).  Host only: no HIP call (frt_embedder_describe runs it without a device).
struct ArcUnitShape {
    int cin, depth, stride, h_in;  // h_in: input spatial size (square)
};
struct ArcLayout {
    int num_layers = 0;               // 50, 100 or 152
    bool se = false;
    int stage_units[4] = {0, 0, 0, 0};
    std::vector<ArcUnitShape> units;
};

inline ArcLayout arc_layout(const Blob &b, bool se) {
    auto fail = [](const std::string &m) { throw std::runtime_error("weight blob: " + m); };
    auto bn = [&](const std::string &p, int c) {
        for (const char *f : {".weight", ".bias", ".running_mean", ".running_var"}) b.get(p + f, c);
    };
    static const int width[4] = {64, 128, 256, 512};
    static const struct {
        int layers, units[4];
    } tables[3] = {{50, {3, 4, 14, 3}}, {100, {3, 13, 30, 3}}, {152, {3, 8, 36, 3}}};
    ArcLayout L;
    L.se = se;
    b.get("input_layer.0.weight", 64 * 27);
    bn("input_layer.1", 64);
    b.get("input_layer.2.weight", 64);
    int n = 0;
    while (b.has("body." + std::to_string(n) + ".res_layer.1.weight")) ++n;
    if (n == 0) fail("missing tensor body.0.res_layer.1.weight");
    std::map<std::string, int> owned;  // body.* tensors of units 0 .. n-1
    int st = -1, h = 112, prev = 64;
    for (int i = 0; i < n; ++i) {
        const std::string p = "body." + std::to_string(i);
        const Tensor &w1 = b.get(p + ".res_layer.1.weight", 0);
        if (w1.dims.size() != 4 || w1.dims[2] != 3 || w1.dims[3] != 3) fail("wrong shape for " + p + ".res_layer.1.weight");
        const int depth = (int)w1.dims[0], cin = (int)w1.dims[1];
        const bool sc = b.has(p + ".shortcut_layer.0.weight");
        const bool start = i == 0 || sc || depth != prev;
        if (start && (++st >= 4 || depth != width[st]))
            fail(p + ".res_layer.1.weight: a unit " + std::to_string(depth) + " channels wide cannot open stage " + std::to_string(st + 1) +
                 " (IR stages are 64 / 128 / 256 / 512 wide)");
        if (cin != prev) fail("wrong size for " + p + ".res_layer.1.weight (" + std::to_string(cin) + " input channels, the stream has " + std::to_string(prev) + ")");
        if (sc != (cin != depth)) fail(std::string(sc ? "unexpected tensor " : "missing tensor ") + p + ".shortcut_layer.0.weight");
        const bool has_se = b.has(p + ".res_layer.5.fc1.weight") || b.has(p + ".res_layer.5.fc2.weight");
        if (has_se != se)
            fail(se ? "missing tensor " + p + ".res_layer.5.fc1.weight (IR-SE blob: every unit has an SE module)"
                    : "unexpected tensor " + p + ".res_layer.5.fc1.weight (IR blob: SE units mixed with plain ones)");
        std::vector<std::pair<std::string, size_t>> need = {{".res_layer.1.weight", (size_t)depth * cin * 9},
                                                            {".res_layer.2.weight", (size_t)depth},
                                                            {".res_layer.3.weight", (size_t)depth * depth * 9}};
        for (const char *f : {".weight", ".bias", ".running_mean", ".running_var"}) {
            need.push_back({std::string(".res_layer.0") + f, (size_t)cin});
            need.push_back({std::string(".res_layer.4") + f, (size_t)depth});
            if (sc) need.push_back({std::string(".shortcut_layer.1") + f, (size_t)depth});
        }
        if (sc) need.push_back({".shortcut_layer.0.weight", (size_t)depth * cin});
        if (se) {
            need.push_back({".res_layer.5.fc1.weight", (size_t)depth / 16 * depth});
            need.push_back({".res_layer.5.fc2.weight", (size_t)depth * (depth / 16)});
        }
        for (const auto &t : need) {
            b.get(p + t.first, t.second);
            owned[p + t.first] = i;
        }
        const int stride = start ? 2 : 1;
        L.units.push_back({cin, depth, stride, h});
        ++L.stage_units[st];
        h /= stride;
        prev = depth;
    }
    for (const auto &kv : b.t)
        if (kv.first.compare(0, 5, "body.") == 0 && !owned.count(kv.first))
            fail("unexpected tensor " + kv.first + " (the units are body.0 - body." + std::to_string(n - 1) + "; missing tensor body." +
                 std::to_string(n) + ".res_layer.1.weight?)");
    for (const auto &t : tables)
        if (st == 3 && std::equal(t.units, t.units + 4, L.stage_units)) L.num_layers = t.layers;
    if (!L.num_layers) {
        std::string got;
        for (int s = 0; s <= st && s < 4; ++s) got += (s ? "," : "") + std::to_string(L.stage_units[s]);
        fail("units body.0 - body." + std::to_string(n - 1) + " form the stage table {" + got +
             "}: not IR-50 {3,4,14,3}, IR-100 {3,13,30,3} or IR-152 {3,8,36,3}");
    }
    bn("output_layer.0", 512);
    b.get("output_layer.3.weight", (size_t)512 * 25088);
    b.get("output_layer.3.bias", 512);
    bn("output_layer.4", 512);
    return L;
}

// IEEE fp32 -> fp16, round-to-nearest-even (clang's native _Float16 conversion; this file is compiled by hipcc only).
inline uint16_t f32_to_f16(float f) {
    const _Float16 h = (_Float16)f;
    uint16_t u;
    std::memcpy(&u, &h, 2);
    return u;
}

}  // namespace frt
