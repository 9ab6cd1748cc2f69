"""IR-100 / IR-152 / IR-SE-100 / IR-SE-152 on the HIP recogniser (the six backbones of model_irse.py:193-240): every execution path runs
the deeper stacks - the fp16 strip / small-batch kernels, fp32 mode, the fused and stand-alone SE tails, the pipeline with graphs and merging -
against the reference goldens (tests/golden/make_golden_deep.py) and the fp32 oracle.  Tolerance from BASELINE.json north_star: embeddings
cosine-equal within 1e-4."""
import importlib.util
import os

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, face_input

pytestmark = pytest.mark.gpu
COS_TOL = 1e-4
DEEP = ["ir100", "ir152", "ir_se100", "ir_se152"]


def split(tag):
    return ("ir_se", int(tag[5:])) if tag.startswith("ir_se") else ("ir", int(tag[2:]))


@pytest.fixture(scope="module")
def deep(frt, synth, tmp_path_factory):
    """tag -> (blob path, state dict, golden); the state dict is regenerated from the golden's seed and calibration."""
    d = tmp_path_factory.mktemp("deep_weights")
    cache = {}

    def get(tag):
        if tag not in cache:
            mode, layers = split(tag)
            g = np.load(os.path.join(GOLDEN, "arcface_%s.npz" % tag))
            sd = synth.arcface_state(int(g["seed"]), mode, num_layers=layers, calib=(g["calib_mean"], g["calib_var"]))
            kind = frt.weights_io.KIND_ARCFACE_IR_SE if mode == "ir_se" else frt.weights_io.KIND_ARCFACE_IR
            cache[tag] = (frt.write_weights(str(d / ("%s.frtw" % tag)), sd, kind), sd, g)
        return cache[tag]

    return get


def drs():
    spec = importlib.util.spec_from_file_location("drs", os.path.join(ROOT, "tools", "dynamic_range_sweep.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.mark.parametrize("tag", DEEP)
def test_deep_embeddings_match_golden_and_oracle(frt, synth, deep, tag):
    from oracle import nets
    path, sd, g = deep(tag)
    mode, layers = split(tag)
    nf = int(g["n_faces"])
    assert nf == 8
    rec = frt.ArcFaceIR50(path, maxBatchSize=nf)
    assert rec.numLayers == layers and rec.se == (mode == "ir_se")
    x = face_input(synth.make_faces(nf))
    emb = rec.doInference(x)
    rec.close()
    assert np.isfinite(emb).all() and np.allclose((emb.astype(np.float64) ** 2).sum(1), 1, atol=1e-5)
    cos_gold = (emb.astype(np.float64) * g["embeddings"]).sum(1)
    assert cos_gold.min() > 1 - COS_TOL, 1 - cos_gold
    oemb = nets.arcface_forward(sd, x)
    assert (emb.astype(np.float64) * oemb).sum(1).min() > 1 - COS_TOL
    assert np.abs(emb @ emb.T - g["cos"]).max() < 2e-3


@pytest.mark.parametrize("tag", DEEP)
def test_deep_batch1_and_batch4_agree_and_repeat_bit_identically(frt, synth, deep, tag):
    """1 face per pass takes the small-batch kernel (kernels_arc_small.hip), 4 faces the strip kernels: not bit-equal (the K split sums in
    another order, fp16 roundings of activations flip here and there), the same call twice is bit-identical.  Twice IR-50's units give those
    flips twice the room: measured 1 - cos 1.1e-5 ... 1.5e-5 for IR-100 / IR-152 (IR-50: ~ 3e-6), below 1e-5 for the SE stacks - held to
    3e-5 here, a third of north_star's tolerance, which each path meets against the fp32 oracle on its own."""
    path, _, _ = deep(tag)
    x = face_input(synth.make_faces(4))
    rec1 = frt.ArcFaceIR50(path, maxBatchSize=1)
    rec4 = frt.ArcFaceIR50(path, maxBatchSize=4)
    e1, e4 = rec1.doInference(x), rec4.doInference(x)
    assert np.isfinite(e1).all() and np.isfinite(e4).all()
    assert 1 - (e1.astype(np.float64) * e4).sum(1).min() <= (1e-5 if tag.startswith("ir_se") else 3e-5), 1 - (e1 * e4).sum(1)
    assert np.array_equal(rec4.doInference(x), e4) and np.array_equal(rec1.doInference(x), e1)
    rec1.close()
    rec4.close()


@pytest.mark.parametrize("tag", DEEP)
def test_deep_fp32_mode_matches_the_fp32_oracle(frt, synth, deep, tag):
    from oracle import nets
    path, sd, _ = deep(tag)
    x = face_input(synth.make_faces(3))
    want = nets.arcface_forward(sd, x)
    rec = frt.ArcFaceIR50(path, maxBatchSize=3)
    rec.setPrecision(True)
    got = rec.doInference(x)
    rec.close()
    assert np.isfinite(got).all()
    cos = (got.astype(np.float64) * want).sum(1)
    assert (1 - cos <= 1e-6).all(), 1 - cos


@pytest.mark.parametrize("tag", ["ir_se100", "ir_se152"])
def test_deep_se_fused_equals_stand_alone_tail(frt, synth, deep, tag):
    """24 faces: the smallest batches whose IR-SE pass has fused launches (tests/golden/arc_conv_plan.txt: conv2_se ... se=1 from F = 23; at 8 faces
    both settings plan the same launches).  The profiling labels show that the first pass ran twins with the SE tail and the second none."""
    import arc_launch_ref
    twins = {t.label for t in arc_launch_ref.FUSED.values()}
    path, _, _ = deep(tag)
    x = face_input(synth.make_faces(24))
    rec = frt.ArcFaceIR50(path, maxBatchSize=24)

    def profiled():
        frt.profile_enable(1)
        try:
            emb = rec.doInference(x)
            labels, _, _ = frt.profile_collect()
        finally:
            frt.profile_enable(0)
        return emb, set(labels)

    fused, fused_labels = profiled()
    rec.setSeFused(False)
    alone, alone_labels = profiled()
    rec.close()
    assert fused_labels & twins and not alone_labels & twins, (sorted(fused_labels & twins), sorted(alone_labels & twins))
    assert np.isfinite(fused).all() and np.isfinite(alone).all()
    assert ((fused.astype(np.float64) * alone).sum(1) >= 1 - 1e-5).all()
    assert np.abs(fused - alone).max() < 1e-3


@pytest.mark.parametrize("tag", ["ir100", "ir152", "ir_se152"])
def test_deep_stream_holds_where_ir50_holds(frt, synth, tmp_path, tag):
    """Stream scale 1e3 (tools/dynamic_range_sweep.py): IR-50 holds it (peak 48 -> 4.8e4 < 65504); the deep IR stacks peak 545 / 783 and
    would overflow, so libfrt conditions their stream at load (frt_embedder.cpp build()).  The embeddings match the oracle."""
    from oracle import nets
    mode, layers = split(tag)
    base = synth.arcface_state(2, mode, num_layers=layers)
    sd = drs().rescale(base, s=1e3, mode=mode)
    x = face_input(synth.make_faces(4))
    want = nets.arcface_forward(base, x)
    kind = frt.weights_io.KIND_ARCFACE_IR_SE if mode == "ir_se" else frt.weights_io.KIND_ARCFACE_IR
    rec = frt.ArcFaceIR50(frt.write_weights(str(tmp_path / "w.frtw"), sd, kind), maxBatchSize=4)
    got = rec.doInference(x)
    rec.close()
    assert np.isfinite(got).all()
    assert ((got.astype(np.float64) * want).sum(1) > 1 - COS_TOL).all(), 1 - (got * want).sum(1)


@pytest.mark.parametrize("tag", ["ir100", "ir_se152"])
def test_deep_fp16_overflow_is_not_silent(frt, synth, tmp_path, tag):
    """At stream scale 1e4 (where IR-50 overflows too) the result is non-finite or an error, never a plausible embedding."""
    mode, layers = split(tag)
    sd = drs().rescale(synth.arcface_state(2, mode, num_layers=layers), s=1e4, mode=mode)
    kind = frt.weights_io.KIND_ARCFACE_IR_SE if mode == "ir_se" else frt.weights_io.KIND_ARCFACE_IR
    rec = frt.ArcFaceIR50(frt.write_weights(str(tmp_path / "w.frtw"), sd, kind), maxBatchSize=2)
    try:
        got = rec.doInference(face_input(synth.make_faces(2)))
    except frt.FrtError:
        got = None
    rec.close()
    assert got is None or not np.isfinite(got).all(), got


def test_ir100_pipeline_against_the_oracle(frt, orc, synth, blobs, deep):
    """IR-100 behind the detector in the default pipeline mode: 640x640, K = 4, graphs on, 12 back-to-back 4-frame submits into an 8-frame
    pipeline (several tickets in flight, later ones merged into one call), then repeated run_dev calls that graph replay serves.  Every record: box within one pixel of the oracle's, the planted
    top-1 row, cosine to the oracle's embedding > 1 - 1e-4 (test_gpu_headline.check_faces)."""
    import torch
    from test_gpu_headline import check_faces, oracle_frame
    dpath, dsd = blobs("det")
    rpath, rsd, _ = deep("ir100")
    M, K, H, W, N = 8, 4, 640, 640, 50_000
    pool = [synth.make_frame(i, H, W) for i in (0, 9, 18, 31)]
    gal = synth.make_gallery(N)
    want = []
    for p, frame in enumerate(pool):
        boxes, emb = oracle_frame(orc, dsd, rsd, frame, H, W, K)
        assert len(boxes) == K
        slots = 777 + 12011 * p + 2003 * np.arange(K)
        gal[slots] = emb
        want.append((boxes, emb, slots))
    det = frt.RetinaFace(dpath, W, H, (3, H, W), M, K, 0.4, 0.6)
    rec = frt.ArcFaceIR50(rpath, W, H, maxBatchSize=M * K, maxFacesPerScene=K)
    assert rec.numLayers == 100
    rec.setGallery(gal)
    rec.initMatMul()
    pipe = frt.Pipeline(det, rec, M)
    pipe.set_graph(True)
    own_cache = {}
    m0 = pipe.merge_stats()
    for rnd in range(2):  # (the second round finds every staging set, slot and activation set holding the first round's data)
        tks = []
        for t in range(12):
            fl = [(t + k) % len(pool) for k in range(4)]
            tks.append(dict(fl=fl, frames=torch.from_numpy(np.stack([pool[i] for i in fl])).pin_memory(),
                            res=torch.zeros(len(fl) * K * frt.RESULT_DTYPE.itemsize, dtype=torch.uint8).pin_memory(),
                            emb=torch.zeros(len(fl) * K, 512).pin_memory()))
        tickets = [pipe.submit(tk["frames"].numpy(), tk["res"].numpy().view(frt.RESULT_DTYPE), tk["emb"].numpy()) for tk in tks]
        for t in tickets:
            pipe.wait(t)
        for tk in tks:
            res, emb = tk["res"].numpy().view(frt.RESULT_DTYPE), tk["emb"].numpy()
            assert np.isfinite(emb).all()
            for f, p in enumerate(tk["fl"]):
                oboxes, oemb, slots = want[p]
                check_faces(res, emb, f, K, oboxes, oemb, slots, orc, rsd, pool[p], own_cache)
    m1 = pipe.merge_stats()
    assert m1[0] > m0[0], (m0, m1)
    # run_dev on the same device buffers: the call's (slot, activation set) keys recur every NSLOT calls, so the stage graphs - the deep
    # network's ~100 launches among them - are captured at their second occurrence and replayed from the third, bit-identical to the eager calls
    d_frames = torch.from_numpy(np.stack(pool)).cuda()
    d_res = torch.zeros(len(pool) * K * frt.RESULT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    d_emb = torch.zeros(len(pool) * K, 512, device="cuda")
    torch.cuda.synchronize()
    g0 = pipe.graph_stats()
    runs = []
    for _ in range(30):
        pipe.run_dev(d_frames.data_ptr(), len(pool), d_res.data_ptr(), d_emb.data_ptr())
        pipe.sync()
        runs.append((d_res.cpu().numpy().view(frt.RESULT_DTYPE).copy(), d_emb.cpu().numpy().copy()))
    g1 = pipe.graph_stats()
    assert g1[0] > g0[0] and g1[1] > g0[1], (g0, g1)
    for res, emb in runs[1:]:
        assert np.array_equal(res, runs[0][0]) and np.array_equal(emb, runs[0][1])
    for f, p in enumerate(range(len(pool))):
        oboxes, oemb, slots = want[p]
        check_faces(runs[-1][0], runs[-1][1], f, K, oboxes, oemb, slots, orc, rsd, pool[p], own_cache)
    pipe.close()
    det.close()
    rec.close()


@pytest.mark.parametrize("tag", ["ir100", "ir_se152"])
def test_deep_coalescer_embeds_like_the_direct_call(frt, synth, blobs, deep, tag):
    """frt_coalescer_* (several threads' frames into one pipeline call) on a deep backbone: every face's embedding equals the pipeline's
    synchronous run of the same frame to float rounding."""
    import threading
    dpath, _ = blobs("det")
    rpath, _, _ = deep(tag)
    K, H, W = 4, 640, 640
    frames = [synth.make_frame(i, H, W) for i in (0, 9, 18, 31)]
    det = frt.RetinaFace(dpath, W, H, (3, H, W), 4, K, 0.4, 0.6)
    rec = frt.ArcFaceIR50(rpath, W, H, maxBatchSize=4 * K, maxFacesPerScene=K)
    rec.setGallery(synth.make_gallery(1000))
    rec.initMatMul()
    pipe = frt.Pipeline(det, rec, 4)
    res, emb = pipe.run(np.stack(frames))
    pipe.close()
    co = frt.Coalescer(det, rec, 4, window_us=2000)
    out = [None] * len(frames)

    def worker(i):
        out[i] = co.infer(frames[i])

    th = [threading.Thread(target=worker, args=(i,)) for i in range(len(frames))]
    for t in th:
        t.start()
    for t in th:
        t.join()
    co.close()
    det.close()
    rec.close()
    for i, (r, e) in enumerate(out):
        n = len(r)
        assert n == int(res[i * K:(i + 1) * K]["valid"].sum()) and n > 0
        assert np.isfinite(e).all()
        assert ((e.astype(np.float64) * emb[i * K:i * K + n]).sum(1) > 1 - 1e-5).all(), i
