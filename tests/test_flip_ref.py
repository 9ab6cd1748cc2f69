"""The references of the flip-augmented embeddings (tests/flip_ref.py), the part that needs no device: the two kernels' float64 restatements
against their definitions and against arc_launch_ref's bound for the plain finalize launch, the end-to-end reference's symmetry, and the
condition the GPU tests' tolerances rest on - on the faces they use, the sum pre(x) + pre(mirror x) is no cancellation."""
import numpy as np
import pytest

import arc_launch_ref as R
import flip_ref as FR
from conftest import face_input


def test_pair_up_reference_is_the_faces_then_their_mirror_images():
    x = FR.pair_up_input(3)
    assert len(np.unique(x.view(np.uint32))) == x.size
    y = FR.pair_up_reference(x)
    assert y.shape == (6, 3, 112, 112) and y.dtype == np.float32
    assert np.array_equal(y[:3], x)
    for f, c, r, col in ((0, 0, 0, 0), (1, 2, 111, 111), (2, 1, 57, 3)):
        assert y[3 + f, c, r, col] == x[f, c, r, 111 - col]
    assert np.array_equal(FR.pair_up_reference(y[3:])[3:], x)  # mirrored twice


@pytest.mark.parametrize("c", FR.FINALIZE_CASES, ids=[c.id for c in FR.FINALIZE_CASES])
def test_pair_finalize_reference_and_its_bound(c):
    d = FR.finalize_inputs(c)
    assert set(np.unique(d["partial"])) <= {-1.0, 0.0, 1.0} and d["partial"].shape == (c.splits, 2 * c.n, 512)
    out, bound = FR.finalize_case_reference(c, d)
    ok = d["valid"] != 0
    assert np.allclose((out[ok] ** 2).sum(1), 1, atol=1e-12) and not out[~ok].any() and not bound[~ok].any()
    assert (c.n == 1) == bool(ok.all())
    # a face paired with itself: the plain launch's embedding, under a bound no tighter than the plain launch's
    p = d["p"].astype(np.float64)
    sums = d["partial"].astype(np.float64).sum(0)[:c.n]
    twice, e_twice = FR.pair_finalize_reference(sums, sums, p, d["valid"])
    plain, e_plain = R.fc_finalize_reference(sums, p, d["valid"])
    assert np.abs(twice - plain).max() < 1e-14 and (e_twice >= e_plain).all()
    # the kernel's arithmetic in numpy fp32, with and without the multiply-add contracted, stays inside the bound (and the bound is no
    # blanket: below 1e-5 of a unit vector's length everywhere)
    pf = d["p"]
    sa, sb = d["partial"][:, :c.n].sum(0, dtype=np.float32), d["partial"][:, c.n:].sum(0, dtype=np.float32)
    for fused in (False, True):
        def bn(s):
            t = s + pf[0]
            return (t.astype(np.float64) * pf[1] + pf[2]).astype(np.float32) if fused else t * pf[1] + pf[2]
        v = bn(sa) + bn(sb)
        got = v / np.sqrt((v * v).sum(1, keepdims=True, dtype=np.float32))
        got[~ok] = 0
        assert (np.abs(got - out) <= bound).all()
    assert bound.max() < 1e-5


@pytest.mark.parametrize("mode", ["ir", "ir_se"])
def test_flip_reference_is_symmetric_and_the_sum_is_no_cancellation(synth, blobs, mode):
    """normalize(pre(x) + pre(mirror x)) of a face and of its mirror image are the same vector.  And the condition behind the GPU tests'
    tolerances (tests/test_gpu_flip.py): on their faces the sum keeps at least 1.3 times the longer of the two vectors' length - measured 1.36
    (ir) and 1.35 (ir_se) -, so two relative errors of the plain path's class grow by at most (2 / 1.3)^2 ~ 2.4 in 1 - cos."""
    _, sd = blobs(mode)
    x = face_input(synth.make_faces(9))
    pre, pre_m = FR.pre_vectors(sd, x)
    ratio = FR.sum_ratio(pre, pre_m)
    print("%s: |pre + pre_m| / max(|pre|, |pre_m|) = %.3f .. %.3f" % (mode, ratio.min(), ratio.max()))
    assert ratio.min() >= 1.3
    ref = FR.normalize(pre + pre_m)
    assert np.array_equal(ref, FR.normalize(pre_m + pre))
    # (all nine mirror images in one batch, as above: the oracle is torch's fp32 on the CPU, and on some hosts its sums differ in their last
    #  bits - 6e-7 of a unit vector - from one batch size to another, which is no asymmetry of the reference)
    again = FR.flip_reference(sd, x[:, :, :, ::-1])
    assert np.abs(again - ref).max() < 1e-12
    # and the mode is no near no-op: the flip embedding is far from the plain one
    cos_plain = (ref * FR.normalize(pre)).sum(1)
    assert cos_plain.max() < 0.9
