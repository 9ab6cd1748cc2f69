"""ArcFace IR-50 / IR-SE-50 HIP forward (fp16 MFMA convs, fp32 accumulate) vs the fp32 oracle and the reference goldens.

Tolerance from BASELINE.json north_star: embeddings cosine-equal within 1e-4."""
import os

import numpy as np
import pytest

from conftest import GOLDEN, face_input

pytestmark = pytest.mark.gpu
COS_TOL = 1e-4


@pytest.mark.parametrize("mode", ["ir", "ir_se"])
def test_embeddings_match_oracle_and_goldens(frt, synth, blobs, mode):
    from oracle import nets
    path, sd = blobs(mode)
    g = np.load(os.path.join(GOLDEN, "arcface_%s.npz" % mode))
    nf = int(g["n_faces"])
    rec = frt.ArcFaceIR50(path, maxBatchSize=8)
    x = face_input(synth.make_faces(nf))
    emb = rec.doInference(x)
    assert emb.shape == (nf, 512)
    assert np.allclose((emb.astype(np.float64) ** 2).sum(1), 1, atol=1e-5)
    cos_gold = (emb * g["embeddings"]).sum(1)
    assert cos_gold.min() > 1 - COS_TOL, cos_gold
    oemb = nets.arcface_forward(sd, x)
    assert (emb * oemb).sum(1).min() > 1 - COS_TOL
    assert np.abs(emb - oemb).max() < 2e-3
    # the pairwise cosine structure (what matching consumes) is preserved
    assert np.abs(emb @ emb.T - g["cos"]).max() < 2e-3
    rec.close()


def test_batch_chunking_and_batch1_agree(frt, synth, blobs):
    path, _ = blobs("ir")
    x = face_input(synth.make_faces(5))
    rec1 = frt.ArcFaceIR50(path, maxBatchSize=1)   # the reference default (config.json:18): one face per launch
    rec4 = frt.ArcFaceIR50(path, maxBatchSize=4)   # 5 faces -> chunks of 4 + 1
    e1, e4 = rec1.doInference(x), rec4.doInference(x)
    # 1 face and 4 faces take different kernels for the large layers (kernels_arc_small.hip's K split over four waves sums in another
    # order than the strip kernels): fp16 roundings of activations flip here and there - the two agree as closely as either agrees
    # with the fp32 oracle (1 - cos ~ 3e-6, tools/small_batch_parity.py), not bit for bit
    assert (e1 * e4).sum(1).min() > 1 - 1e-5
    assert np.abs(e1 - e4).max() < 1e-3
    # the same batch twice: bit-identical (the K split is summed in a fixed order)
    assert np.array_equal(rec4.doInference(x), e4) and np.array_equal(rec1.doInference(x), e1)
    rec1.close()
    rec4.close()


def test_forward_crops_and_embeds_like_the_oracle(frt, orc, synth, blobs):
    from oracle import nets
    path, sd = blobs("ir")
    rec = frt.ArcFaceIR50(path, maxBatchSize=4)
    fr = synth.make_frame(3, 480, 640)
    boxes = np.zeros(3, frt.BBOX_DTYPE)
    boxes[0] = (30, 40, 200, 180, 0.9)
    boxes[1] = (100, 300, 212, 412, 0.8)
    boxes[2] = (250, 10, 479, 300, 0.7)
    emb = rec.forward(fr, boxes)
    ocrops = orc.crop_faces(fr, boxes)
    assert np.array_equal(np.stack([c["face"] for c in rec.croppedFaces]), ocrops)  # CroppedFace.face (app.cpp:329)
    assert [c["x1"] for c in rec.croppedFaces] == [30, 100, 250]
    oemb = nets.arcface_forward(sd, orc.face_normalize(ocrops))
    assert (emb * oemb).sum(1).min() > 1 - COS_TOL
    # featureMatching / getOutputs vs the fused device path
    gal = synth.make_gallery(777)
    gal[[5, 700]] = oemb[[1, 2]]
    rec.initKnownEmbeds(len(gal))
    for i, e in enumerate(gal):
        rec.addEmbedding("u%d" % i, e)
    rec.initMatMul()
    names, sims = rec.getOutputs(rec.featureMatching())
    n2, s2 = rec.matchTop1()
    assert names == n2 and names[1:] == ["u5", "u700"] and np.allclose(sims, s2, atol=1e-6) and min(sims[1:]) > 0.999
    rec.resetEmbeddings()
    with pytest.raises(frt.FrtError):
        rec.featureMatching()
    rec.close()


def test_batch_of_128_equals_small_batches(frt, synth, blobs):
    """Benchmark batch (128 faces) vs the same faces in batches of 64: identical embeddings (strip walks of the persistent conv
    kernels, grid-dependent tile variants and the split-K linear must be batch-size independent per face).  Batches of 32 take the
    medium-batch kernel (kernels_arc_ks.hip) and batches of 8 the small-batch kernel (kernels_arc_small.hip) for most layers - K split
    over the waves, another fp32 summation order, so fp16 roundings of activations flip: as close to the 128-face result as either is
    to the fp32 oracle."""
    path, _ = blobs("ir")
    big = frt.ArcFaceIR50(path, maxBatchSize=128)
    mid = frt.ArcFaceIR50(path, maxBatchSize=64)
    med = frt.ArcFaceIR50(path, maxBatchSize=32)
    small = frt.ArcFaceIR50(path, maxBatchSize=8)
    x = np.random.default_rng(11).standard_normal((128, 3, 112, 112)).astype(np.float32) * 0.5
    e = big.doInference(x)
    for f0 in (0, 64):
        em = mid.doInference(x[f0:f0 + 64])
        assert np.abs(e[f0:f0 + 64] - em).max() < 2e-6, (f0, np.abs(e[f0:f0 + 64] - em).max())
    for f0 in (0, 96):
        em = med.doInference(x[f0:f0 + 32])
        assert (e[f0:f0 + 32] * em).sum(1).min() > 1 - 1e-5 and np.abs(e[f0:f0 + 32] - em).max() < 1e-3, f0
        assert np.array_equal(med.doInference(x[f0 + 5:f0 + 32])[:20], em[5:25])  # position / batch size inside the class: bit for bit
    med.close()
    for f0 in (0, 40, 120):
        es = small.doInference(x[f0:f0 + 8])
        assert (e[f0:f0 + 8] * es).sum(1).min() > 1 - 1e-5 and np.abs(e[f0:f0 + 8] - es).max() < 1e-3, f0
        # position in the batch does not matter: the same faces alone, bit for bit
        assert np.array_equal(small.doInference(x[f0 + 2:f0 + 8])[:3], es[2:5])
    big.close()
    mid.close()
    small.close()


@pytest.mark.parametrize("mode", ["ir", "ir_se"])
def test_small_batches_match_the_oracle(frt, synth, blobs, mode):
    """1, 2 and 7 faces per pass: the small-batch convolution kernel (kernels_arc_small.hip: ragged last pixel tiles at every
    resolution - 196 x F is never a multiple of 32 for these F -, tiles that span two faces, the fused 1x1 shortcut convs of IR-50, the
    stand-alone SE tail of IR-SE-50 behind it) against the fp32 oracle (model_irse.py:48-66, 139-156)."""
    from oracle import nets
    path, sd = blobs(mode)
    x = np.random.default_rng(23).standard_normal((7, 3, 112, 112)).astype(np.float32) * 0.5
    want = nets.arcface_forward(sd, x)
    for F in (1, 2, 7):
        rec = frt.ArcFaceIR50(path, maxBatchSize=F)
        e = rec.doInference(x[:F])
        rec.close()
        assert (e * want[:F]).sum(1).min() > 1 - COS_TOL, (mode, F)
        assert np.abs(e - want[:F]).max() < 2e-3, (mode, F)


@pytest.mark.parametrize("mode", ["ir", "ir_se"])
def test_medium_batches_match_the_oracle(frt, synth, blobs, mode):
    """16, 24 and 40 faces per pass take the medium-batch kernel (kernels_arc_ks.hip: one 32-cout block x a strip per workgroup, K split
    over the four waves; half-image strips up to 20 faces, whole-image strips above, 7x7 images whole), 9 / 10 sit on the boundary to the
    small-batch kernel, 41 / 48 on the boundary back to the strip kernels: against the fp32 oracle (model_irse.py:48-66, 139-156), and the
    same face must embed bit for bit wherever it sits in a batch of its class."""
    from oracle import nets
    path, sd = blobs(mode)
    x = np.random.default_rng(29).standard_normal((48, 3, 112, 112)).astype(np.float32) * 0.5
    want = nets.arcface_forward(sd, x[:10])
    for F in (9, 10, 16, 24, 40, 41, 48):
        rec = frt.ArcFaceIR50(path, maxBatchSize=F)
        e = rec.doInference(x[:F])
        e2 = rec.doInference(np.concatenate([x[F - 4:F], x[:F - 4]]))
        rec.close()
        assert np.isfinite(e).all()
        n = min(F, 10)
        assert (e[:n] * want[:n]).sum(1).min() > 1 - COS_TOL, (mode, F)
        assert np.abs(e[:n] - want[:n]).max() < 2e-3, (mode, F)
        assert np.array_equal(e2[4:], e[:F - 4]) and np.array_equal(e2[:4], e[F - 4:]), (mode, F)


@pytest.mark.parametrize("mode", ["ir", "ir_se"])
def test_every_batch_size_class_embeds_alike(frt, synth, blobs, mode):
    """The strip heights, images per strip and (IR-SE) which units run the SE tail inside conv2's epilogue all follow the batch size;
    odd batch sizes leave a last strip with a single image.  The same faces must embed alike (fp16 rounding flips only) whatever
    batch they travel in."""
    path, _ = blobs(mode)
    x = np.random.default_rng(17).standard_normal((100, 3, 112, 112)).astype(np.float32) * 0.5
    ref = frt.ArcFaceIR50(path, maxBatchSize=8)
    want = np.concatenate([ref.doInference(x[i:i + 8]) for i in (0, 24, 92)])  # faces 0-7, 24-31, 92-99
    ref.close()
    for F in (1, 3, 12, 16, 21, 33, 40, 64, 100):
        rec = frt.ArcFaceIR50(path, maxBatchSize=F)
        e = rec.doInference(x[:F])
        rec.close()
        assert np.isfinite(e).all() and np.allclose((e.astype(np.float64) ** 2).sum(1), 1, atol=1e-5), F
        for lo, k in ((0, 0), (24, 8), (92, 16)):
            n = min(8, F - lo)
            if n > 0:
                assert (e[lo:lo + n] * want[k:k + n]).sum(1).min() > 1 - 1e-5, (F, lo)


@pytest.mark.parametrize("which,scale", [("stream", 1e-3), ("stream", 1e3), ("branch", 1e-3), ("branch", 1e3)])
def test_dynamic_range_of_the_fp16_activation_storage(frt, synth, tmp_path, which, scale):
    """Round-2 VERDICT robustness item 7a.  All other parity evidence sits on weights that keep activations O(1).  tools/dynamic_range_sweep.py
    rescales the network WITHOUT changing the function it computes so that the residual stream (tensors Y / Z / SC, fp16) or the
    conv1 -> conv2 activation (tensor T, fp16, plus the fp16 weights around it) sits 10^-3 ... 10^3 away from that; measured
    (profiles/r03/r03a_dynamic_range.json): 1 - cos stays at 3e-6 ... 1.5e-5 over that whole range for IR-50 and IR-SE-50, degrades silently
    below (branch scale 1e-4: 4.8e-4) and turns non-finite - visibly - at 1e4.  The tolerance is north_star's 1e-4."""
    import importlib.util

    from conftest import ROOT, face_input
    from oracle import nets
    spec = importlib.util.spec_from_file_location("drs", os.path.join(ROOT, "tools", "dynamic_range_sweep.py"))
    drs = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(drs)
    base = synth.arcface_state(2, "ir", calib=synth.load_calibration("ir"))
    sd = drs.rescale(base, s=scale if which == "stream" else 1.0, t=scale if which == "branch" else 1.0)
    x = face_input(synth.make_faces(4))
    want = nets.arcface_forward(sd, x)
    assert ((want * nets.arcface_forward(base, x)).sum(1) > 1 - 1e-6).all()  # the rescaling preserved the function
    path = frt.write_weights(str(tmp_path / "w.frtw"), sd, frt.weights_io.KIND_ARCFACE_IR50)
    rec = frt.ArcFaceIR50(path, maxBatchSize=4)
    got = rec.doInference(x)
    rec.close()
    assert np.isfinite(got).all()
    assert ((got * want).sum(1) > 1 - 1e-4).all(), (got * want).sum(1)


@pytest.mark.parametrize("scale", [1e-6, 1e-4, 1e-2, 1e2, 1e3, 1e5])
def test_branch_conditioning_at_load_removes_the_silent_range_failure(frt, synth, tmp_path, scale):
    """Round-4 review item 6.  The one SILENT failure of the sweep above was a conv1 -> PReLU -> conv2 branch 1e-4 times smaller than the
    synthetic weights keep it (1 - cos 4.8e-4, five times north_star's tolerance): T and conv1's fp16 weights in the subnormals, conv2's near
    overflow.  libfrt now conditions every unit at load (frt_embedder.cpp: conv1 rows, conv2 columns / rows and the closing BatchNorm's scale by
    powers of two - the same function, exactly); the embeddings of a branch rescaled by 1e-6 ... 1e5 match the fp32 oracle as well as the
    well-scaled network does (1 - cos <= 1e-5)."""
    import importlib.util

    from conftest import ROOT, face_input
    from oracle import nets
    spec = importlib.util.spec_from_file_location("drs", os.path.join(ROOT, "tools", "dynamic_range_sweep.py"))
    drs = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(drs)
    for mode, kind in (("ir", frt.weights_io.KIND_ARCFACE_IR50),):
        base = synth.arcface_state(2, mode, calib=synth.load_calibration(mode))
        sd = drs.rescale(base, t=scale, mode=mode)
        x = face_input(synth.make_faces(4))
        want = nets.arcface_forward(base, x)   # (the fp32 oracle of the rescaled weights is the same function; at 1e-6 / 1e5 its own fp32 products still hold)
        path = frt.write_weights(str(tmp_path / ("w_%s.frtw" % mode)), sd, kind)
        rec = frt.ArcFaceIR50(path, maxBatchSize=4)
        got = rec.doInference(x)
        rec.close()
        assert np.isfinite(got).all()
        assert ((got * want).sum(1) > 1 - 1e-5).all(), (scale, 1 - (got * want).sum(1))


@pytest.mark.parametrize("mode", ["ir", "ir_se"])
def test_fp32_precision_mode_matches_the_fp32_oracle(frt, synth, tmp_path, mode):
    """BASELINE configs[1] says "fp32".  frt_embedder_set_precision(e, 1) runs the recogniser with fp32 activations, fp32 weights and exact
    fp32 products (kernels_arc_f32.hip): against the fp32 oracle (torch-CPU, another summation order) the embeddings agree to 1 - cos <= 1e-6
    and element-wise to 2e-5 - two orders of magnitude tighter than north_star's tolerance, which the default fp16-MFMA path meets at ~ 3e-6.
    Nine faces exercise the chunking (eight per pass); switching back restores the default path."""
    from conftest import face_input
    from oracle import nets
    sd = synth.arcface_state(2, mode, calib=synth.load_calibration(mode))
    kind = frt.weights_io.KIND_ARCFACE_IR50 if mode == "ir" else frt.weights_io.KIND_ARCFACE_IR_SE50
    path = frt.write_weights(str(tmp_path / "w.frtw"), sd, kind)
    x = face_input(synth.make_faces(9))
    want = nets.arcface_forward(sd, x)
    rec = frt.ArcFaceIR50(path, maxBatchSize=9)
    fast = rec.doInference(x)
    rec.setPrecision(True)
    got = rec.doInference(x)
    one = rec.doInference(x[4:5])
    rec.setPrecision(False)
    again = rec.doInference(x)
    rec.close()
    assert np.isfinite(got).all()
    cos = (got.astype(np.float64) * want).sum(1)
    assert (cos > 1 - 1e-6).all(), 1 - cos
    assert np.abs(got - want).max() < 2e-5, np.abs(got - want).max()
    assert np.array_equal(one[0], got[4])                      # a face's embedding does not depend on its position in the batch
    assert np.array_equal(again, fast)                         # back on the default path
    assert 1 - (fast * want).sum(1).min() > 1 - (cos.min())    # ... which is the less accurate of the two


def test_fp16_overflow_is_not_silent(frt, synth, tmp_path):
    """... and at a stream scale of 1e4 the fp16 tensors overflow: the embeddings come back non-finite, never as plausible numbers."""
    import importlib.util

    from conftest import ROOT, face_input
    spec = importlib.util.spec_from_file_location("drs", os.path.join(ROOT, "tools", "dynamic_range_sweep.py"))
    drs = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(drs)
    sd = drs.rescale(synth.arcface_state(2, "ir", calib=synth.load_calibration("ir")), s=1e4)
    path = frt.write_weights(str(tmp_path / "w.frtw"), sd, frt.weights_io.KIND_ARCFACE_IR50)
    rec = frt.ArcFaceIR50(path, maxBatchSize=2)
    got = rec.doInference(face_input(synth.make_faces(2)))
    rec.close()
    assert not np.isfinite(got).all()


@pytest.mark.parametrize("mode", ["ir", "ir_se"])
def test_compact_strips_at_ragged_batches(frt, synth, blobs, mode):
    """Round 6: from 112 faces per pass the 14x14 and 7x7 body convs run on compact strips (conv_patchc_kernel: 8 images of 14x14 per 7 strips,
    128 images of 7x7 per 49 strips; a strip crosses image boundaries, and the LAST strips of a pass whose face count is not a multiple of 8
    hold pixels of images that do not exist).  Batches of 112, 113, 119, 121 and 127 faces must embed every face like the 128-face pass does -
    bit for bit: a face's outputs depend on nothing but its own pixels and the kernel class (IR-SE's fused tail: up to the parity of its slot,
    see below) - and like the fp32 oracle to north_star's 1e-4
    (the first, a middle and the last face of each batch).  IR-SE takes the compact kernel for conv1 and the padded one, SE tail fused, for conv2."""
    from oracle import nets
    path, sd = blobs(mode)
    x = np.random.default_rng(23).standard_normal((128, 3, 112, 112)).astype(np.float32) * 0.5
    full = frt.ArcFaceIR50(path, maxBatchSize=128)
    want = full.doInference(x)
    again = full.doInference(x)
    full.close()
    assert np.array_equal(want, again)
    probe = [0, 63, 111, 112, 118, 126, 127]
    ref = nets.arcface_forward(sd, x[probe])
    assert ((want[probe].astype(np.float64) * ref).sum(1) > 1 - 1e-4).all()
    for F in (112, 113, 119, 121, 127):
        rec = frt.ArcFaceIR50(path, maxBatchSize=F)
        e = rec.doInference(x[:F])
        shifted = rec.doInference(np.concatenate([x[1:F], x[:1]]))  # the same faces one slot earlier: other strips, other image boundaries
        rec.close()
        assert np.isfinite(e).all(), F
        assert np.array_equal(e, want[:F]), (mode, F, int((e != want[:F]).any(1).sum()))
        back = np.concatenate([shifted[F - 1:], shifted[:F - 1]])  # undo the shift
        if mode == "ir":
            assert np.array_equal(back, e), (mode, F)
        else:
            # IR-SE with the SE tail fused into conv2 (the padded strips, unchanged this round): at 7x7 a strip holds TWO images and the second
            # one's channel sums are accumulated in another lane / tile order than the first one's (it starts in the middle of a pixel tile) - an
            # image's pooled mean can differ in its last fp32 bit with the parity of its slot, and once in ~ 100 faces that flips an fp16 rounding
            # downstream (measured: 1 face of 128, 6e-6 in one element; with the stand-alone SE tail: none)
            diff = (back != e).any(1)
            assert diff.sum() <= 3 and np.abs(back - e).max() < 5e-5 and ((back * e).sum(1) > 1 - 1e-6).all(), (mode, F, int(diff.sum()))


def conv_label_sequence(frt, path, fused, F):
    """Profiling labels of the conv launches of ONE doInference pass of F faces on a fresh embedder (public Python surface only)."""
    rec = frt.ArcFaceIR50(path, maxBatchSize=F)
    if fused is not None:
        rec.setSeFused(fused)
    x = np.random.default_rng(F).standard_normal((F, 3, 112, 112)).astype(np.float32) * 0.5
    frt.profile_enable(1)
    try:
        rec.doInference(x)
        labels, _, _ = frt.profile_collect()
    finally:
        frt.profile_enable(0)
        rec.close()
    return labels


CONV_LABEL_CASES = [("ir", None), ("ir_se", True), ("ir_se", False)]
CONV_LABEL_BATCHES = (1, 12, 33, 64, 128)


def conv_label_key(mode, fused, F):
    return "%s%s F=%d" % (mode, "" if fused is None else (" fused" if fused else " standalone"), F)


@pytest.mark.parametrize("F", CONV_LABEL_BATCHES)
@pytest.mark.parametrize("mode,fused", CONV_LABEL_CASES)
def test_conv_launch_labels_are_the_recorded_ones(frt, blobs, mode, fused, F):
    """The kernels one pass really launches - per-device SE gate included - are the ones tests/golden/arc_conv_labels.json holds: the label
    sequence this same code recorded on an MI355X with the library of the commit before the dispatch became conv_plan (two launches per
    unit: conv1, conv2).  IR-50, and IR-SE-50 with the SE tail in conv2's epilogue and as launches of its own; one batch per size class."""
    import json
    path, _ = blobs(mode)
    want = json.load(open(os.path.join(GOLDEN, "arc_conv_labels.json")))[conv_label_key(mode, fused, F)]
    got = conv_label_sequence(frt, path, fused, F)
    assert len(want) == 48
    assert got == want
