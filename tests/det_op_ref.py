"""float64 reference and error bounds for the detector's ops run one at a time (tests/cpp/det_op_check.cpp).  A reference, not a test:
tests/test_det_op_ref.py (no GPU) and tests/test_gpu_det_ops.py use it.

Reference.  RetinaFace mobilenet0.25 as oracle/nets.py states it in fp32, restated in float64 on NumPy, in the product's op order
(frt_detector::build): op 0 the 3 -> 8 first conv, ops 1 - 13 the conv_dw blocks, 14 / 15 / 17 the FPN laterals (15 and 17 add the
nearest-upsampled coarser level behind their ReLU), 16 / 18 the merges, 19 the fused SSH 64 -> 32 + 16 pair (out2 = the 16 channels of
conv5X5_1), 20 the 16 -> 16 + 16 pair, 21 conv7x7_3, 22 the heads of the three levels with the 2-class softmax (and the landmark head where
the blob has it).  BN is folded in float64 and rounded to fp32 exactly as the product folds it (frt::bn_fold: scale = fp32(g / sqrt(var +
eps)), weight = fp32 product of the fp32 weight and that scale, bias = fp32(beta - mean * scale64)): the split kernels' host packers split
these fp32 values, so the reference must start from them.  Every op's input is the reference output of its predecessor ROUNDED TO FP32 -
what the harness can put into the op's `in` pointer - and the op's reference output is computed in float64 from that rounded input, so
that the comparison sees one op's arithmetic alone.

Bound.  Per output element, u = 2^-24 (fp32 unit roundoff), first order in u and widened by 1 + 2^-10 for the higher orders.  None of the
constants is fitted to a kernel.
  * depthwise 3x3: nine FMAs on top of the bias, ten roundings, each at most u times an intermediate no larger than sum|w||x| + |b|:
        e_d = 10 u (sum|w||x| + |b|) + sum|w| e_x        (e_x: the error of the input, zero for an op run alone);   ReLU is 1-Lipschitz.
  * a sum of K products in fp32 (pointwise conv, dense conv, head).  Two forms:
      - any order:   e_acc = K u sum|w||x|                                      (first conv: K = 27; heads: K = 64)
      - known order: the products are added to ONE accumulator in groups of 16 input channels, the groups in ascending order (dense 3x3:
        chunk of 16 channels, then tap - kernels_det_conv3h.hip "(chunk, tap, hi*hi, hi*lo, lo*hi)").  With S_g the exact sum after group g
        and T_g = sum over the group of |w||x|, no intermediate inside group g exceeds |S_(g-1)| + T_g, and the group costs at most R
        roundings:   e_acc = R u sum_g (|S_(g-1)| + T_g).   R is the group's own number of products for the fp32 kernels of the conv_dw / 1x1
        family (16, or 8 for the 8-channel block: they all walk the input channels in ascending order with one FMA, or one k-step of an fp32
        MFMA, per channel) and three times that, 48, for the split kernels (three MFMAs of 16 products each, a rounding per product whatever
        the order inside the instruction).
    The any-order form is what an FMA chain of unknown order allows; for K = 576 it is ~ 20 x the second form and would let a dropped `lo`
    term pass (tests/test_det_op_ref.py), which is why the ops whose order is documented use the second.
  * split kernels (conv3x3_split_kernel, dwpw_mfma_kernel<SPLIT>, pw_mfma_kernel<_, true>, dwpw_wave_kernel; which launches those are:
    runs_split() below): each operand is hi = fp16(x), lo = fp16(x - hi), and a b ~ a_hi b_hi + a_hi b_lo + a_lo b_hi.  With r(x) = |x - hi - lo|
    and l(x) = |lo| the product misses   r(a)|b| + |a| r(b) + l(a) l(b).
        weights:     r and l are computed exactly from the fp32 folded weights (the packer's own rounding, NumPy's astype(float16));
        activations: r(a) <= max(2^-22 |a|, 2^-25): 2^-11 relative per rounding while lo is a normal fp16 number, and half a subnormal
                     spacing (2^-24) once |a - hi| < 2^-14, i.e. |a| below about 2^-3;  l(a) <= (1 + 2^-11) max(2^-11 |a|, 2^-25).
                     |a| is taken as |reference| + its error, so the bound holds for the value the device split.
    The 2^-25 term is absolute: per element it is 2^-25 times the other operand's magnitude, whatever the scale of the activations.
    Above 65504 hi is inf and the product NaN: Prob.rng holds the largest and the smallest non-zero magnitude entering each split
    (asserted below 65504 on the CPU, tests/test_det_op_ref.py).
  * epilogue: + bias, one rounding u (|acc| + |b| + e_acc); ReLU; the upsample-add one more, u (|v| + |add|).
  * heads: loc / ldm = 64-term sums + bias.  conf = softmax of two such logits c0, c1: p0 = 1 / (1 + exp(c1 - c0)) has slope p0 p1 <= 1/4 in
    c1 - c0, so the logits' errors enter as p0 p1 (e_c0 + e_c1); the subtraction, the sum and the division add 4 u p.  The device expf is not
    derived: SOFTMAX_ALLOW = 4 x the largest |conf - float64| seen on an MI355X (SOFTMAX_SEEN, see tests/test_gpu_det_ops.py).
The GPU test fails on err > bound, on a NaN and on any changed canary word, and prints max(err / bound) per (op, batch)."""
import collections
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24
WIDE = 1 + 2.0 ** -10
SOFTMAX_SEEN = 4.19e-7  # largest |conf - float64 reference| seen on an MI355X: 640x640, frame 0, at every batch (tests/test_gpu_det_ops.py)
SOFTMAX_ALLOW = 4 * SOFTMAX_SEEN
MEAN = np.array([104, 117, 123], np.float64)
N_OPS = 23
# one op per split family for the mutation checks and the range-edge cases: merge1 (dense 3x3 64 -> 64), the 64 -> 64 conv_dw block (op 5; 80x80 at
# 640x640: dwpw_wave_kernel from 3 frames, dwpw_mfma_kernel below), the 64 -> 64 lateral with the upsample-add
FAMILY_OPS = {"conv3": 18, "dwpw": 5, "pw": 17}

Prob = collections.namedtuple("Prob", "inp add src add_src out bound out2 bound2 dims rng split", defaults=(None,))  # split: bound of a split kernel
Op = collections.namedtuple("Op", "index kind name probs")


# ------------------------------------------------------------------------------------------------ weights, folded as the product folds them
def _bn_fold(sd, p):
    g, be, mu, var = (np.asarray(sd[p + k], np.float32).astype(np.float64) for k in (".weight", ".bias", ".running_mean", ".running_var"))
    s = g / np.sqrt(var + 1e-5)
    return s.astype(np.float32), (be - mu * s).astype(np.float32)


def _fold(sd, conv, bn):
    """fp32 folded weight [Cout][Cin/groups][k][k] and bias, as fold_conv3 / fold_dw / fold_pw compute them."""
    w = np.asarray(sd[conv + ".weight"], np.float32)
    sc, bi = _bn_fold(sd, bn)
    return (w * sc[:, None, None, None]).astype(np.float32), bi


def _plain(sd, conv):
    return np.asarray(sd[conv + ".weight"], np.float32), np.asarray(sd[conv + ".bias"], np.float32)


STAGES = [("stage1", [(3, 8, 2), (8, 16, 1), (16, 32, 2), (32, 32, 1), (32, 64, 2), (64, 64, 1)]),
          ("stage2", [(64, 128, 2)] + [(128, 128, 1)] * 5), ("stage3", [(128, 256, 2), (256, 256, 1)])]


# ------------------------------------------------------------------------------------------------ arithmetic with bounds
def _taps(x, stride, fill=False):
    """The nine shifted views [B][C][Ho][Wo] of x [B][C][H][W] with zero padding 1 (fill: the border mutation - tap 0 reads the nearest pixel where it should read padding)."""
    B, C, H, W = x.shape
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    xp = np.zeros((B, C, H + 2, W + 2), x.dtype)
    xp[:, :, 1:-1, 1:-1] = x
    out = []
    for kh in range(3):
        for kw in range(3):
            src = xp
            if fill and kh == 0 and kw == 0:  # tap 0 reads the nearest pixel instead of the zero padding
                src = np.pad(x, ((0, 0), (0, 0), (1, 1), (1, 1)), mode="edge")
            out.append(src[:, :, kh:kh + (Ho - 1) * stride + 1:stride, kw:kw + (Wo - 1) * stride + 1:stride])
    return out


def depthwise(x, e_x, w, b, stride, mut=None):
    """x float64 [B][C][H][W], w fp32 [C][1][3][3], b [C] -> relu(d), e_d."""
    w = w.astype(np.float64).reshape(-1, 9)
    b = b.astype(np.float64)
    taps = _taps(x, stride, fill=mut == "border")
    d = sum(t * w[None, :, k, None, None] for k, t in enumerate(taps)) + b[None, :, None, None]
    mag = sum(np.abs(t) * np.abs(w[None, :, k, None, None]) for k, t in enumerate(taps)) + np.abs(b)[None, :, None, None]
    e = 10 * U * WIDE * mag
    if e_x is not None:
        e = e + sum(t * np.abs(w[None, :, k, None, None]) for k, t in enumerate(_taps(e_x, stride)))
    return np.maximum(d, 0), e


def _split16(w):
    """hi, lo of the host packers (pack_conv3_split / pack_pw_split), as float64."""
    w = np.asarray(w, np.float32)
    hi = w.astype(np.float16).astype(np.float32)
    lo = (w - hi).astype(np.float16).astype(np.float32)
    return hi.astype(np.float64), lo.astype(np.float64)


def _grouped(groups, e_a_groups, split):
    """groups: (W [Cout][k] fp32-valued float64, A [B][k][N] float64) in the kernel's order -> acc, e_acc (module docstring).  e_a_groups: the
    error of A per group or None.  split: three roundings per product and the hi / lo terms, otherwise one; mutations change W before it gets here."""
    S = chain = prop = extra = 0.0
    for gi, (W, A) in enumerate(groups):
        aW, aA = np.abs(W), np.abs(A)
        e_a = None if e_a_groups is None else e_a_groups[gi]
        if e_a is not None:
            prop = prop + aW @ e_a
            aA = aA + e_a
        T = aW @ aA
        chain = chain + (3 if split else 1) * W.shape[1] * (np.abs(S) + T)
        S = S + W @ A
        if split:
            hi, lo = _split16(W)
            r_w, l_w = np.abs(W - hi - lo), np.abs(lo)
            r_a = np.maximum(2.0 ** -22 * aA, 2.0 ** -25)
            l_a = (1 + 2.0 ** -11) * np.maximum(2.0 ** -11 * aA, 2.0 ** -25)
            extra = extra + aW @ r_a + r_w @ aA + l_w @ l_a
    return S, WIDE * (U * chain + extra) + prop


def _epilogue(acc, e_acc, b, relu=True, add=None):
    b = b.astype(np.float64)[None, :, None, None]
    v = acc + b
    e = e_acc + U * WIDE * (np.abs(acc) + np.abs(b) + e_acc)
    if relu:
        v = np.maximum(v, 0)
    if add is not None:
        e = e + U * WIDE * (np.abs(v) + np.abs(add) + e)
        v = v + add
    return v, e


def _mutate_w(w, mut):
    if mut == "fp16":  # the weights as one fp16 number: the lo part dropped
        return w.astype(np.float16).astype(np.float32)
    return w


def _mutate_b(b, mut):
    if mut == "bias":  # the bias of channel c ^ 1
        return b[np.arange(len(b)) ^ 1]
    return b


def pointwise(d, e_d, w, b, split, add=None, mut=None):
    """d float64 [B][Cin][H][W] (+ its error), w fp32 [Cout][Cin][1][1] -> relu(w d + b) (+ add), bound; the channels in ascending groups of 16."""
    B, Cin, H, W_ = d.shape
    w = _mutate_w(w, mut).astype(np.float64).reshape(w.shape[0], Cin)
    dd = d.reshape(B, Cin, H * W_)
    ee = None if e_d is None else e_d.reshape(B, Cin, H * W_)
    g = list(range(0, Cin, 16))
    acc, e_acc = _grouped([(w[:, c:c + 16], dd[:, c:c + 16]) for c in g], None if ee is None else [ee[:, c:c + 16] for c in g], split)
    return _epilogue(acc.reshape(B, -1, H, W_), e_acc.reshape(B, -1, H, W_), _mutate_b(b, mut), add=add)


def conv3(x, e_x, w, b, stride, split, mut=None):
    """Dense 3x3, pad 1: x float64 [B][Cin][H][W], w fp32 [Cout][Cin][3][3].  split: the (chunk, tap) order of conv3x3_split_kernel with the
    known-order bound; otherwise the any-order bound with K = 9 Cin."""
    B, Cin, H, W_ = x.shape
    Cout = w.shape[0]
    w = _mutate_w(w, mut).astype(np.float64)
    taps = _taps(x, stride, fill=mut == "border")
    Ho, Wo = taps[0].shape[2:]
    e_taps = None if e_x is None else _taps(e_x, stride)
    step = 16 if split else Cin
    groups, egroups = [], []
    for c in range(0, Cin, step):
        for t in range(9):
            groups.append((w[:, c:c + step, t // 3, t % 3], np.ascontiguousarray(taps[t][:, c:c + step]).reshape(B, -1, Ho * Wo)))
            egroups.append(None if e_taps is None else np.ascontiguousarray(e_taps[t][:, c:c + step]).reshape(B, -1, Ho * Wo))
    if split:
        acc, e_acc = _grouped(groups, egroups, True)
    else:
        acc = sum(W @ A for W, A in groups)
        mag = sum(np.abs(W) @ (np.abs(A) + (0 if E is None else E)) for (W, A), E in zip(groups, egroups))
        e_acc = 9 * Cin * U * WIDE * mag + (0 if e_taps is None else sum(np.abs(W) @ E for (W, A), E in zip(groups, egroups)))
    return _epilogue(acc.reshape(B, Cout, Ho, Wo), np.broadcast_to(e_acc, acc.shape).reshape(B, Cout, Ho, Wo), _mutate_b(b, mut))


def runs_split(cin, cout, h, w, stride, depthwise_stage=True):
    """Whether a conv_dw block (or, depthwise_stage = False, a plain 1x1 conv) of the detectors runs on a split kernel.  This restates what
    kernels_det_mfma.hip: launch_dwpw_mfma accepts - the one piece of the dispatch the bound depends on - and tests/test_det_op_ref.py holds it
    against the kernels recorded in profiles/det_ops/, so it cannot drift from the product unnoticed.  1x1 convs: always (every one carries wph).
    conv_dw blocks: the matrix-core kernels take maps of 4-pixel segments (Wo % 4 == 0, W == stride Wo, H W % 4 == 0, H == stride Ho for
    stride 2 up to an odd last row), leave the stride-1 blocks with at most 32 channels to the scalar kernels, and run split where the input
    channels come in chunks of 32 (8 and 16 channels: fp32 MFMA).  dwpw_wave_kernel covers a subset of these shapes.  Independent of the batch."""
    if not depthwise_stage:
        return cin % 16 == 0 and cout >= 16
    ho, wo = (h - 1) // stride + 1, (w - 1) // stride + 1
    if cin % 2 or cout < 16 or wo % 4 or w != stride * wo or (h * w) % 4 or (h != ho if stride == 1 else (h + 1) // 2 != ho):
        return False
    if cout <= 32 and cin <= 32 and stride == 1:
        return False
    return cin % 32 == 0 and (cout <= 32 or cout in (64, 128, 256))


def upsample_nearest(x, oh, ow):
    """F.interpolate(mode='nearest') to (oh, ow): src = min(floor(dst * fp32(in / out)), in - 1), the index in fp32 as PyTorch and the kernels compute it."""
    ih, iw = x.shape[2:]
    iy = np.minimum(np.floor(np.arange(oh, dtype=np.float32) * (np.float32(ih) / np.float32(oh))).astype(np.int64), ih - 1)
    ix = np.minimum(np.floor(np.arange(ow, dtype=np.float32) * (np.float32(iw) / np.float32(ow))).astype(np.int64), iw - 1)
    return x[:, :, iy][:, :, :, ix]


def _rng_stats(a):
    a = np.abs(a)
    nz = a[a > 0]
    return float(a.max()), float(nz.min()) if nz.size else 0.0


def _f32(a):
    return np.ascontiguousarray(a, np.float32)


# ------------------------------------------------------------------------------------------------ the ops
class Net:
    """The ops' weights (folded as the product folds them) and run(i, inputs): the float64 reference of op i alone."""

    def __init__(self, sd):
        self.sd = sd
        self.landmarks = "LandmarkHead.0.conv1x1.weight" in sd
        self.body = []
        for st, layers in STAGES:
            for i, (cin, cout, stride) in enumerate(layers):
                p = "body.%s.%d" % (st, i)
                if cin == 3:
                    self.body.append(("conv", _fold(sd, p + ".0", p + ".1"), stride))
                else:
                    self.body.append(("dw", _fold(sd, p + ".0", p + ".1"), _fold(sd, p + ".3", p + ".4"), stride, cin))
        self.lat = [_fold(sd, "fpn.output%d.0" % (k + 1), "fpn.output%d.1" % (k + 1)) for k in range(3)]
        self.merge = [_fold(sd, "fpn.merge%d.0" % (k + 1), "fpn.merge%d.1" % (k + 1)) for k in range(2)]
        ssh = lambda k, n: _fold(sd, "ssh%d.%s.0" % (k + 1, n), "ssh%d.%s.1" % (k + 1, n))
        cat2 = lambda a, b: (np.concatenate([a[0], b[0]]), np.concatenate([a[1], b[1]]))
        self.ssh_a = [cat2(ssh(k, "conv3X3"), ssh(k, "conv5X5_1")) for k in range(3)]    # 64 -> 32 | 16
        self.ssh_b = [cat2(ssh(k, "conv5X5_2"), ssh(k, "conv7X7_2")) for k in range(3)]  # 16 -> 16 | 16
        self.ssh_c = [ssh(k, "conv7x7_3") for k in range(3)]
        heads = ["BboxHead", "ClassHead"] + (["LandmarkHead"] if self.landmarks else [])
        self.heads = [[_plain(sd, "%s.%d.conv1x1" % (h, k)) for h in heads] for k in range(3)]

    # every function: (list of fp32 inputs per problem, list of fp32 adds) -> list of (out, bound, out2, bound2, rng)
    def run(self, i, inps, adds=None, mut=None, split=None):
        """split: for a conv_dw block, whether to give the bound of its split kernel (None: runs_split of the shape)."""
        x = [np.asarray(a, np.float64) for a in inps]
        if i == 0:
            (w, b), stride = self.body[0][1], self.body[0][2]
            return [conv3(x[0], None, w, b, stride, False) + (None, None, None)]
        if i <= 13:
            _, (wd, bd), (wp, bp), stride, cin = self.body[i]
            d, e_d = depthwise(x[0], None, wd, bd, stride, mut if mut == "border" else None)
            if split is None:
                split = runs_split(cin, wp.shape[0], x[0].shape[2], x[0].shape[3], stride)
            out, e = pointwise(d, e_d, wp, bp, split, mut=None if mut == "border" else mut)
            return [(out, e, None, None, _rng_stats(d), split)]
        if i in (14, 15, 17):
            k = {14: 2, 15: 1, 17: 0}[i]
            add = None
            if adds and adds[0] is not None:
                add = upsample_nearest(np.asarray(adds[0], np.float64), *x[0].shape[2:])
            out, e = pointwise(x[0], None, self.lat[k][0], self.lat[k][1], True, add=add, mut=mut)
            return [(out, e, None, None, _rng_stats(x[0]), True)]
        if i in (16, 18):
            w, b = self.merge[1 if i == 16 else 0]
            return [conv3(x[0], None, w, b, 1, True, mut) + (None, None, _rng_stats(x[0]), True)]
        if i in (19, 20, 21):
            res = []
            for k in range(3):
                w, b = (self.ssh_a, self.ssh_b, self.ssh_c)[i - 19][k]
                out, e = conv3(x[k], None, w, b, 1, True, mut)
                s = {19: 32, 20: 16, 21: 16}[i]
                res.append((out[:, :s], e[:, :s], out[:, s:] if i < 21 else None, e[:, s:] if i < 21 else None, _rng_stats(x[k]), True))
            return res
        assert i == 22
        return [self._heads(k, x[k]) for k in range(3)]

    def _heads(self, k, x):
        """-> ((loc, conf[, ldm]) as [B][H W 2][4 | 2 | 10], their bounds, None, None, None)"""
        B, C, H, W_ = x.shape
        xx = x.reshape(B, C, H * W_)
        outs, bounds = [], []
        for hi, (w, b) in enumerate(self.heads[k]):
            w = w.astype(np.float64).reshape(w.shape[0], C)
            b = b.astype(np.float64)[None, :, None]
            v = w @ xx + b
            e = (C + 1) * U * WIDE * (np.abs(w) @ np.abs(xx) + np.abs(b))
            per = w.shape[0] // 2
            v = v.transpose(0, 2, 1).reshape(B, H * W_ * 2, per)  # anchor = (pixel, l), channels per l .. per l + per - 1
            e = e.transpose(0, 2, 1).reshape(B, H * W_ * 2, per)
            if hi == 1:
                m = v.max(-1, keepdims=True)
                ex = np.exp(v - m)
                p = ex / ex.sum(-1, keepdims=True)
                e = WIDE * (p * p[..., ::-1] * e.sum(-1, keepdims=True) + 4 * U * p) + SOFTMAX_ALLOW
                v = p
            outs.append(v)
            bounds.append(e)
        return tuple(outs), tuple(bounds), None, None, None


def op_sources():
    """op -> per problem (producer op, 'out' | 'out2', problem) of `in`, and of `add`; producer -1: the network input."""
    src = {0: [(-1, "out", 0)]}
    for i in range(1, 14):
        src[i] = [(i - 1, "out", 0)]
    src[14], src[15], src[17] = [(13, "out", 0)], [(11, "out", 0)], [(5, "out", 0)]
    src[16], src[18] = [(15, "out", 0)], [(17, "out", 0)]
    src[19] = [(18, "out", 0), (16, "out", 0), (14, "out", 0)]
    src[20] = [(19, "out2", k) for k in range(3)]
    src[21] = [(20, "out2", k) for k in range(3)]
    src[22] = [(21, "out", k) for k in range(3)]  # the concat target: channels 0-31 from op 19, 32-47 from op 20, 48-63 from op 21
    return src, {15: (14, "out", 0), 17: (16, "out", 0)}


def preprocess(frames):
    """u8 BGR [B][H][W][3] -> the network input, planar, mean-subtracted (exact in fp32)."""
    return _f32((frames.astype(np.float64) - MEAN).transpose(0, 3, 1, 2))


def forward(sd, x):
    """Every op of the network on x fp32 [B][3][H][W]: list of Op in the product's order (inputs: the predecessor's reference output rounded to fp32)."""
    net = Net(sd)
    src, add_src = op_sources()
    ops, outs = [], {(-1, "out", 0): _f32(x)}
    for i in range(N_OPS):
        if i == 22:  # the concat of the SSH outputs
            inps = [_f32(np.concatenate([outs[(19, "out", k)], outs[(20, "out", k)], outs[(21, "out", k)]], 1)) for k in range(3)]
        else:
            inps = [outs[s] for s in src[i]]
        adds = [outs[add_src[i]]] if i in add_src else [None]
        res = net.run(i, inps, adds)
        probs = []
        for k, r in enumerate(res):
            out, bound, out2, bound2, rng = r[:5]
            if i < 22:
                outs[(i, "out", k)] = _f32(out)
                if out2 is not None:
                    outs[(i, "out2", k)] = _f32(out2)
            dims = inps[k].shape[1:]
            probs.append(Prob(inps[k], adds[0] if k == 0 else None, None if i == 22 else src[i][k], add_src.get(i) if k == 0 else None, out, bound, out2, bound2, dims, rng, r[5] if len(r) > 5 else False))
        kind = "conv3" if i in (0, 16, 18, 19, 20, 21) else ("heads" if i == 22 else "dwpw")
        ops.append(Op(i, kind, "op%d" % i, probs))
    return net, ops


def final_outputs(ops):
    """(loc, conf[, ldm]) [B][A][4 | 2 | 10] of the whole reference, the levels concatenated."""
    per_level = [p.out for p in ops[22].probs]
    return tuple(np.concatenate([lv[h] for lv in per_level], 1) for h in range(len(per_level[0])))


def split_ops(ops):
    """Indices of the ops whose arguments carry split weights (wh / wph): every stride-1 dense conv with 16 or 64 input channels, every
    conv_dw block and 1x1 conv whose input channels are a multiple of 16."""
    return [o.index for o in ops if (o.kind == "conv3" and o.index > 0) or (o.kind == "dwpw" and o.probs[0].dims[0] % 16 == 0)]


def stem_chain(net, x):
    """Ops 0 - 2 with the error carried from layer to layer (launch_det_stem writes op 2's output only): out, bound."""
    x = np.asarray(x, np.float64)
    (w, b), stride = net.body[0][1], net.body[0][2]
    y, e = conv3(x, None, w, b, stride, False)
    for i in (1, 2):
        _, (wd, bd), (wp, bp), stride, cin = net.body[i]
        d, e_d = depthwise(y, e, wd, bd, stride)
        y, e = pointwise(d, e_d, wp, bp, runs_split(cin, wp.shape[0], y.shape[2], y.shape[3], stride))
    return y, e
