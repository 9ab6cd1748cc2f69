"""The Slim and RFB detectors op by op in float64, in the product's op order (frt_detector::build_slim), with the bounds of tests/det_op_ref.py.
The network is tests/slim_ref.py's restatement (net_slim.py / net_rfb.py in phase 'test'); weights are folded to fp32 as the product folds them.

Ops.  0: conv1 3 -> 16 / 2 (dense, 27 terms in any order).  1 - 12: conv2 - conv13, conv_dw blocks (known-order bound; the split kernels' terms where
det_op_ref.runs_split says one runs).  RFB replaces conv8 (op 7) by five launches: the four 1x1 convs of x in one pass (64
terms on top of the bias, ascending channels, no ReLU) -> red [24] | sc [64]; three rounds of <= 3 dense 3x3 convs with dilation 1 / 1 / 2, 3, 5
on channel slices (<= 144 terms, any order); ConvLinear 48 -> 64, then (acc + b) * scale + shortcut and the ReLU (three more roundings).  Then
conv14's 1x1 (256 -> 64 + bias) and its conv_dw block (64 -> 256 / 2, biases for BN), the heads of levels 0 - 2 (per head a depthwise 3x3 +
bias + ReLU and a 1x1 + bias, ascending channels: the conv_dw bound without split terms; conf through the 2-class softmax) and the dense
3x3 head of level 3 (channel outer, tap inner: groups of 16 channels x 9 taps, 144 roundings per group)."""
import numpy as np

import det_op_ref as R
from det_op_ref import U, WIDE, Op, Prob, _f32, _fold, _plain

SLIM_DW = [(16, 32, 1), (32, 32, 2), (32, 32, 1), (32, 64, 2), (64, 64, 1), (64, 64, 1), (64, 64, 1), (64, 128, 2), (128, 128, 1), (128, 128, 1), (128, 256, 2), (256, 256, 1)]
SLIM_NA = (3, 2, 2, 3)
# RFB conv8: the three rounds of 3x3 convs: (name, dilation, relu, input tensor, its channel slice, output tensor, its channel offset)
RFB_ROUNDS = [[("branch0.1", 1, True, "red", (0, 8), "ta", 0), ("branch1.1", 1, True, "red", (8, 16), "ta", 16), ("branch2.1", 1, True, "red", (16, 24), "ta", 32)],
              [("branch2.2", 1, True, "ta", (32, 44), "tb", 0)],
              [("branch0.2", 2, False, "ta", (0, 16), "cat", 0), ("branch1.2", 3, False, "ta", (16, 32), "cat", 16), ("branch2.3", 5, False, "tb", (0, 16), "cat", 32)]]


def _taps_dil(x, dil):
    B, C, H, W = x.shape
    xp = np.zeros((B, C, H + 2 * dil, W + 2 * dil), x.dtype)
    xp[:, :, dil:dil + H, dil:dil + W] = x
    return [xp[:, :, kh * dil:kh * dil + H, kw * dil:kw * dil + W] for kh in range(3) for kw in range(3)]


def dense3_any(x, w, b, dil, relu):
    """3x3, stride 1, dilation = padding = dil, K = 9 Cin terms in any order."""
    B, Cin, H, W = x.shape
    w = w.astype(np.float64)
    acc = mag = 0.0
    for t, tap in enumerate(_taps_dil(x, dil)):
        a = np.ascontiguousarray(tap).reshape(B, Cin, H * W)
        acc = acc + w[:, :, t // 3, t % 3] @ a
        mag = mag + np.abs(w[:, :, t // 3, t % 3]) @ np.abs(a)
    e = 9 * Cin * U * WIDE * mag
    return R._epilogue(acc.reshape(B, -1, H, W), e.reshape(B, -1, H, W), b, relu=relu)


def pointwise_plain(x, w, b, relu):
    """1x1 in ascending channel order without split terms; -> acc-level (value, bound) through det_op_ref's epilogue."""
    B, Cin, H, W = x.shape
    w = w.astype(np.float64).reshape(w.shape[0], Cin)
    xx = x.reshape(B, Cin, H * W)
    acc, e = R._grouped([(w[:, c:c + 16], xx[:, c:c + 16]) for c in range(0, Cin, 16)], None, False)
    return R._epilogue(acc.reshape(B, -1, H, W), e.reshape(B, -1, H, W), b, relu=relu)


def _anchors(v, na):
    """[B][na per][H][W] -> [B][H W na][per]"""
    B, C, H, W = v.shape
    return v.transpose(0, 2, 3, 1).reshape(B, H * W * na, C // na)


def _softmax_bound(v, e):
    m = v.max(-1, keepdims=True)
    ex = np.exp(v - m)
    p = ex / ex.sum(-1, keepdims=True)
    return p, WIDE * (p * p[..., ::-1] * e.sum(-1, keepdims=True) + 4 * U * p) + R.SOFTMAX_ALLOW


class SlimNet:
    def __init__(self, sd, rfb):
        self.sd, self.rfb = sd, rfb
        self.landmarks = "landm.0.0.weight" in sd
        self.heads = ["loc", "conf"] + (["landm"] if self.landmarks else [])
        self.n_ops = 21 if rfb else 17

    def forward(self, x):
        """list of Op in the product's order; every input is the producing reference output rounded to fp32."""
        sd, ops = self.sd, []
        self.outs = {}  # (op, problem) -> [(tensor name, channel offset) of out (and out2)]; Prob.src: the same of `in`, Prob.add_src: of `in1`
        t = {"x": _f32(x)}  # tensors by name, fp32

        self._n_emitted = lambda: len(ops)

        def emit(kind, probs):
            ops.append(Op(len(ops), kind, "op%d" % len(ops), probs))

        def one(kind, src, res, dst, add=None, split=False):
            out, bound, out2, bound2, rng = res
            self.outs[(len(ops), 0)] = [(d, 0) for d in dst]
            emit(kind, [Prob(t[src], add, (src, 0), None, out, bound, out2, bound2, t[src].shape[1:], rng, split)])

        def dwpw(src, dst, fd, fp, stride):
            x64 = t[src].astype(np.float64)
            d, e_d = R.depthwise(x64, None, fd[0], fd[1], stride)
            split = R.runs_split(x64.shape[1], fp[0].shape[0], x64.shape[2], x64.shape[3], stride)
            out, e = R.pointwise(d, e_d, fp[0], fp[1], split)
            one("dwpw", src, (out, e, None, None, R._rng_stats(d)), [dst], split=split)
            t[dst] = _f32(out)

        w, b = _fold(sd, "conv1.0", "conv1.1")
        out, e = R.conv3(t["x"].astype(np.float64), None, w, b, 2, False)
        one("conv3", "x", (out, e, None, None, None), ["c1"])
        t["c1"] = _f32(out)
        cur = "c1"
        feats = []
        for i, (cin, cout, stride) in enumerate(SLIM_DW):
            n = "c%d" % (i + 2)
            if self.rfb and i == 6:
                self._rfb(t, cur, n, one, emit)
            else:
                p = "conv%d" % (i + 2)
                dwpw(cur, n, _fold(sd, p + ".0", p + ".1"), _fold(sd, p + ".3", p + ".4"), stride)
            cur = n
            if i in (6, 9, 11):
                feats.append(cur)
        w, b = _plain(sd, "conv14.0")
        out, e = R.pointwise(t[cur].astype(np.float64), None, w, b, True)
        one("dwpw", cur, (out, e, None, None, R._rng_stats(t[cur])), ["c14a"], split=True)
        t["c14a"] = _f32(out)
        dwpw("c14a", "c14", _plain(sd, "conv14.2.0"), _plain(sd, "conv14.2.2"), 2)
        feats.append("c14")
        # heads of levels 0 - 2: one op
        probs = []
        for k in range(3):
            x64 = t[feats[k]].astype(np.float64)
            outs, bounds = [], []
            for h in self.heads:
                wd, bd = _plain(sd, "%s.%d.0" % (h, k))
                wp, bp = _plain(sd, "%s.%d.2" % (h, k))
                d, e_d = R.depthwise(x64, None, wd, bd, 1)
                B, C, H, W = d.shape
                ww = wp.astype(np.float64).reshape(wp.shape[0], C)
                dd, ee = d.reshape(B, C, H * W), e_d.reshape(B, C, H * W)
                g = list(range(0, C, 16))
                acc, e = R._grouped([(ww[:, c:c + 16], dd[:, c:c + 16]) for c in g], [ee[:, c:c + 16] for c in g], False)
                v, e = R._epilogue(acc.reshape(B, -1, H, W), e.reshape(B, -1, H, W), bp, relu=False)
                v, e = _anchors(v, SLIM_NA[k]), _anchors(e, SLIM_NA[k])
                if h == "conf":
                    v, e = _softmax_bound(v, e)
                outs.append(v)
                bounds.append(e)
            probs.append(Prob(t[feats[k]], None, (feats[k], 0), None, tuple(outs), tuple(bounds), None, None, t[feats[k]].shape[1:], None))
        emit("slim_heads", probs)
        # level 3: the dense head, channels loc | conf | ldm
        x64 = t["c14"].astype(np.float64)
        B, C, H, W = x64.shape
        taps = [np.ascontiguousarray(tp).reshape(B, C, H * W) for tp in R._taps(x64, 1)]
        outs, bounds = [], []
        for h in self.heads:
            w, b = _plain(sd, "%s.3" % h)
            w = w.astype(np.float64)
            groups = [(np.concatenate([w[:, c:c + 16, tt // 3, tt % 3] for tt in range(9)], 1), np.concatenate([tp[:, c:c + 16] for tp in taps], 1)) for c in range(0, C, 16)]
            acc, e = R._grouped(groups, None, False)
            v, e = R._epilogue(acc.reshape(B, -1, H, W), e.reshape(B, -1, H, W), b, relu=False)
            v, e = _anchors(v, SLIM_NA[3]), _anchors(e, SLIM_NA[3])
            if h == "conf":
                v, e = _softmax_bound(v, e)
            outs.append(v)
            bounds.append(e)
        emit("dense_head", [Prob(t["c14"], None, ("c14", 0), None, tuple(outs), tuple(bounds), None, None, t["c14"].shape[1:], None)])
        assert len(ops) == self.n_ops
        return ops

    def _rfb(self, t, src, dst, one, emit):
        sd = self.sd
        x64 = t[src].astype(np.float64)
        folds = [_fold(sd, "conv8.branch%d.0.conv" % j, "conv8.branch%d.0.bn" % j) for j in range(3)] + [_fold(sd, "conv8.shortcut.conv", "conv8.shortcut.bn")]
        w = np.concatenate([f[0] for f in folds])
        b = np.concatenate([f[1] for f in folds])
        out, e = pointwise_plain(x64, w, b, relu=False)
        one("rfb_proj", src, (out[:, :24], e[:, :24], out[:, 24:], e[:, 24:], None), ["red", "sc"])
        t["red"], t["sc"] = _f32(out[:, :24]), _f32(out[:, 24:])
        width = {"ta": 44, "tb": 16, "cat": 48}
        for rnd in RFB_ROUNDS:
            probs, new = [], {}
            for name, dil, relu, tin, (c0, c1), tout, coff in rnd:
                w, b = _fold(sd, "conv8.%s.conv" % name, "conv8.%s.bn" % name)
                xin = np.ascontiguousarray(t[tin][:, c0:c1])
                out, e = dense3_any(xin.astype(np.float64), w, b, dil, relu)
                self.outs[(self._n_emitted(), len(probs))] = [(tout, coff)]
                probs.append(Prob(xin, None, (tin, c0), None, out, e, None, None, xin.shape[1:], None))
                buf = new.setdefault(tout, np.zeros((xin.shape[0], width[tout]) + xin.shape[2:], np.float32))
                buf[:, coff:coff + out.shape[1]] = out
            t.update(new)
            emit("rfb_conv", probs)
        w, b = _fold(sd, "conv8.ConvLinear.conv", "conv8.ConvLinear.bn")
        acc, e = pointwise_plain(t["cat"].astype(np.float64), w, b, relu=False)
        sc = t["sc"].astype(np.float64)
        y = acc * 1.0 + sc  # scale = 1.0: the product still multiplies
        e = e + 2 * U * WIDE * (np.abs(acc) + np.abs(sc) + e)
        self.outs[(self._n_emitted(), 0)] = [(dst, 0)]
        ops_prob = Prob(t["cat"], t["sc"], ("cat", 0), ("sc", 0), np.maximum(y, 0), e, None, None, t["cat"].shape[1:], None)
        emit("rfb_tail", [ops_prob])
        t[dst] = _f32(np.maximum(y, 0))


def final_outputs(ops, heads):
    """(loc, conf[, ldm]) [B][A][.]: levels 0 - 2 of the heads op, level 3 of the dense head."""
    lv = [p.out for p in ops[-2].probs] + [ops[-1].probs[0].out]
    return tuple(np.concatenate([o[h] for o in lv], 1) for h in range(len(heads)))
