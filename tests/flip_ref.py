"""Float64 references for the recogniser's flip-augmented embeddings (frt_embedder_set_flip, csrc/kernels_arc_flip.hip; DESIGN "Flip-augmented
embeddings"): the two kernels launched alone (tests/test_gpu_flip_launches.py, tests/cpp/flip_launch_check.cpp) and the mode end to end
(tests/test_gpu_flip.py).  What needs no device is checked in tests/test_flip_ref.py.

Pair-up (launch_arc_flip_pair / launch_arc_flip_mirror): pure data movement, compared bit for bit.

Pair finalize (launch_fc_finalize_pair): partials in {-1, 0, 1} make both slice sums integers of magnitude <= 49, exact in fp32 whatever the order,
as the `fc` cases of arc_launch_ref do.  What remains is fp32, u = 2^-24.  For each of the two sums the steps of launch_fc_finalize,
    t = pre + bias, m = t s, v = m + b        e_va, e_vb = u (2 |t s| + |v|)                    (arc_launch_ref.fc_finalize_reference's e_v)
then one fp32 addition                        v = va + vb:  e_v = e_va + e_vb + u |v|
and the tail of launch_fc_finalize unchanged: tot = sum v^2 (a rounding per square, a tree of depth <= 16), nrm = sqrt(tot), out = v / nrm:
    e_tot = sum(2 |v| e_v + e_v^2) + 17 u tot,     e_out = e_v / nrm + |out| (e_tot / (2 tot) + 4 u).
The factor WIDE of arc_launch_ref covers the second-order terms, as there.  A row with valid == 0 must be zeros."""
import collections

import numpy as np

import arc_launch_ref as R

FACE = 3 * 112 * 112

FinalizeCase = collections.namedtuple("FinalizeCase", "id n splits")
FINALIZE_CASES = [FinalizeCase("fin_n%d_k%d" % (n, k), n, k) for n, k in ((1, 49), (2, 49), (33, 49), (64, 49), (1, 1), (2, 1))]
PAIR_UP_N = (1, 2, 3)


def pair_up_reference(x):
    """[n][3][112][112] -> [2n][3][112][112]: the faces, then the same faces with the W axis reversed."""
    return np.concatenate([x, x[..., ::-1]])


def pair_up_input(n):
    """Every float its own bit pattern: a misplaced value cannot pass for the right one."""
    assert n * FACE < 1 << 23
    return (np.arange(n * FACE, dtype=np.uint32) | np.uint32(0x3f000000)).view(np.float32).reshape(n, 3, 112, 112)  # (its index in the mantissa)


def finalize_inputs(c):
    """partial [splits][2n][512] in {-1, 0, 1}; p = bias, s, b [3][512]; valid [n] (the last row of n > 1 is invalid)."""
    r = lambda what: R._rng(c.id, what)
    p = np.zeros((3, 512), np.float32)
    p[0] = 0.05 * r("bias").standard_normal(512)
    p[1], p[2] = R._bn_like(r, "bn", 512)
    valid = np.ones(c.n, np.int32)
    if c.n > 1:
        valid[c.n - 1] = 0
    return {"partial": R._ternary(r("partial"), (c.splits, 2 * c.n, 512)).astype(np.float32), "p": p, "valid": valid}


def pair_finalize_reference(pre_a, pre_b, p, valid):
    """launch_fc_finalize_pair on exact sums pre_a, pre_b [n][512] with p = bias, s, b: (float64 embeddings, bound), see the module comment."""
    def bn(pre):
        t = pre + p[0]
        v = t * p[1] + p[2]
        return v, R.WIDE * R.U * (2 * np.abs(t * p[1]) + np.abs(v))
    va, e_va = bn(pre_a)
    vb, e_vb = bn(pre_b)
    v = va + vb
    e_v = e_va + e_vb + R.WIDE * R.U * np.abs(v)
    tot = (v * v).sum(1, keepdims=True)
    e_tot = (2 * np.abs(v) * e_v + e_v * e_v).sum(1, keepdims=True) + 17 * R.U * tot
    out = v / np.sqrt(tot)
    e_out = R.WIDE * (e_v / np.sqrt(tot) + np.abs(out) * (e_tot / (2 * tot) + 4 * R.U))
    out[valid == 0] = 0
    e_out[valid == 0] = 0
    return out, e_out


def finalize_case_reference(c, d):
    sums = d["partial"].astype(np.float64).sum(0)
    return pair_finalize_reference(sums[:c.n], sums[c.n:], d["p"].astype(np.float64), d["valid"])


def pre_vectors(sd, x):
    """The oracle's pre-normalisation vectors of x and of its mirror image, float64 [n][512] each."""
    from oracle import nets
    x = np.array(x, np.float32)  # (a writable copy: torch wraps it)
    pre = nets.arcface_forward(sd, x, return_blocks=True)[2].astype(np.float64)
    pre_m = nets.arcface_forward(sd, np.ascontiguousarray(x[..., ::-1]), return_blocks=True)[2].astype(np.float64)
    return pre, pre_m


def normalize(v):
    return v / np.maximum(np.sqrt((v * v).sum(1, keepdims=True)), 1e-12)


def flip_reference(sd, x):
    """normalize(pre(x) + pre(mirror x)), float64 [n][512]."""
    pre, pre_m = pre_vectors(sd, x)
    return normalize(pre + pre_m)


def sum_ratio(pre, pre_m):
    """|pre + pre_m| / max(|pre|, |pre_m|) per face: how much of the longer vector the sum keeps (small: a cancellation, which would
    magnify the relative error of the sum)."""
    nrm = lambda v: np.sqrt((v * v).sum(1))
    return nrm(pre + pre_m) / np.maximum(nrm(pre), nrm(pre_m))
