"""The detector's op-by-op reference (tests/det_op_ref.py) checked without a GPU: it is the network the oracle states, its bounds can
fail, and the synthetic blobs keep the split kernels' inputs far below the fp16 range."""
import numpy as np
import pytest

import det_op_ref as R

LOC_TOL = 2e-4   # tests/test_gpu_detector.py
CONF_TOL = 2e-5
GEOMETRIES = {"100x172": (100, 172), "640x640": (640, 640)}
_cache = {}


def _reference(synth, geom, landmarks=False):
    key = (geom, landmarks)
    if key not in _cache:
        h, w = GEOMETRIES[geom]
        sd = synth.retinaface_state(1, landmarks=landmarks)
        x = R.preprocess(synth.make_frames(2, h, w))
        _cache[key] = (sd, x) + R.forward(sd, x)
    return _cache[key]


@pytest.mark.parametrize("landmarks", [False, True], ids=["det", "det_ldm"])
def test_reference_is_the_oracles_network(synth, landmarks):
    """The last outputs of the float64 restatement against oracle.nets.retinaface_forward (fp32), within the tolerances the GPU network is held to."""
    from oracle import nets
    sd, x, _, ops = _reference(synth, "100x172", landmarks)
    want = nets.retinaface_forward(sd, x)
    got = R.final_outputs(ops)
    assert len(got) == len(want) == (3 if landmarks else 2)
    for g, w, tol in zip(got, want, (LOC_TOL, CONF_TOL, LOC_TOL)):
        assert g.shape == w.shape and np.abs(g - w).max() < tol, np.abs(g - w).max()


def test_op_sources_cover_the_network():
    src, add_src = R.op_sources()
    assert sorted(src) == list(range(R.N_OPS)) and sorted(add_src) == [15, 17]
    assert all(p < i for i in src for p, _, _ in src[i])


# a 1x1 conv has no taps and no padding: the border mutation does not exist for the pw family
MUTATIONS = [(f, m) for f in ("conv3", "dwpw", "pw") for m in ("fp16", "border", "bias") if (f, m) != ("pw", "border")]


@pytest.mark.parametrize("family,mutation", MUTATIONS, ids=["%s-%s" % fm for fm in MUTATIONS])
def test_bound_rejects_a_mutated_op(synth, family, mutation):
    """The bound must be able to fail: one split op per family (R.FAMILY_OPS) with its reference mutated - weights rounded to fp16 (lo dropped),
    one border tap not zero-padded, the bias of channel c ^ 1 - lands outside the bound of the unmutated op."""
    _, _, net, ops = _reference(synth, "100x172")
    op = ops[R.FAMILY_OPS[family]]
    assert op.index in R.split_ops(ops)
    p = op.probs[0]
    # (with the bound of the family's split kernel, whichever kernel this small geometry would get)
    ref_out, bound = net.run(op.index, [p.inp], [p.add], split=True)[0][:2]
    out = net.run(op.index, [p.inp], [p.add], mut=mutation, split=True)[0][0]
    err = np.abs(out - ref_out)
    outside = err > bound
    print("%s %s: max(err / bound) = %.1f, %d of %d elements outside" % (family, mutation, (err / bound).max(), outside.sum(), outside.size))
    assert outside.any()
    assert np.array_equal(ref_out, p.out)  # (the unmutated run is the reference itself)


@pytest.mark.parametrize("geom", sorted(GEOMETRIES))
def test_split_inputs_stay_inside_the_fp16_range(synth, geom):
    """Per split op, the largest magnitude entering the hi / lo split (the op's input; for a conv_dw block its depthwise output) and the smallest
    non-zero one.  Above 65504 hi is inf and the op's output NaN: the GPU comparison would mean nothing."""
    _, _, _, ops = _reference(synth, geom)
    for i in R.split_ops(ops):
        for k, p in enumerate(ops[i].probs):
            hi, lo = p.rng
            print("op %2d p%d %-14s largest %8.3f (headroom %7.0fx)  smallest non-zero %.3g" % (i, k, "x".join(str(v) for v in p.dims), hi, 65504 / hi, lo))
            assert 0 < hi < 65504


@pytest.mark.parametrize("rfb", [False, True], ids=["slim", "rfb"])
def test_slim_rfb_reference_is_the_restated_network(synth, rfb):
    """tests/det_slim_op_ref.py's op-by-op float64 network against tests/slim_ref.py's torch restatement, and its split inputs inside the fp16 range."""
    import det_slim_op_ref as S
    import slim_ref
    sd = synth.slim_state(5, rfb=rfb)
    x = R.preprocess(synth.make_frames(2, 100, 172))
    net = S.SlimNet(sd, rfb)
    ops = net.forward(x)
    got, want = S.final_outputs(ops, net.heads), slim_ref.forward(sd, x, rfb)
    assert len(got) == 3
    for g, w, tol in zip(got, want, (LOC_TOL, CONF_TOL, LOC_TOL)):
        assert g.shape == w.shape and np.abs(g - w).max() < tol, np.abs(g - w).max()
    for op in ops:
        if op.kind == "dwpw":
            hi, lo = op.probs[0].rng
            print("%s op %2d %-12s largest %8.3f (headroom %7.0fx)  smallest non-zero %.3g" % ("rfb" if rfb else "slim", op.index, "x".join(str(v) for v in op.probs[0].dims), hi, 65504 / hi, lo))
            assert 0 < hi < 65504


def _recorded_cases():
    import glob
    import os
    return sorted(os.path.basename(f)[:-4] for f in glob.glob(os.path.join(R.ROOT, "profiles", "det_ops", "*-B*.txt")))


@pytest.mark.parametrize("case", _recorded_cases())
def test_runs_split_is_what_the_recorded_kernels_say(synth, case):
    """det_op_ref.runs_split decides which bound an op is held to.  It restates a piece of the product's dispatch, so it is held against the
    kernels that tools/det_ops_coverage.py recorded on an MI355X (profiles/det_ops/): an op's bound is a split kernel's exactly where a
    split kernel ran (dwpw_wave_kernel, dwpw_mfma_kernel<.., SPLIT = true, PRE>, pw_mfma_kernel<_, true>, conv3x3_split_kernel)."""
    import os
    import re
    import det_slim_op_ref as S
    blob, geom, _ = case.split("-")
    h, w = (int(v) for v in geom.split("x"))
    x = R.preprocess(synth.make_frames(1, h, w))
    if blob in ("slim", "rfb"):
        ops = S.SlimNet(synth.slim_state(5, rfb=blob == "rfb"), blob == "rfb").forward(x)
    else:
        ops = R.forward(synth.retinaface_state(1, landmarks=blob == "det_ldm"), x)[1]
    ran = dict(ln.rstrip("\n").split("\t") for ln in open(os.path.join(R.ROOT, "profiles", "det_ops", case + ".txt")) if not ln.startswith("#"))
    checked = 0
    for op in ops:
        if op.kind not in ("dwpw", "conv3"):
            continue
        k = ran["op%d" % op.index]
        was_split = bool(re.search(r"dwpw_wave_kernel|conv3x3_split_kernel|pw_mfma_kernel<\d, true>|dwpw_mfma_kernel<(\d+, ){5}\w+, true, \d>", k))
        assert all(bool(p.split) == was_split for p in op.probs), (case, op.index, k, [p.split for p in op.probs])
        checked += 1
    assert checked >= 13
