"""Slim / RFB detectors on the MI355X: the HIP forward against the CPU restatement and the reference-module goldens, the 4-level
post-processing against the restatement, findFace / findFaceBatch end to end, the pipeline on top of them, and alignment mode."""
import os

import numpy as np
import pytest

import slim_ref
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

LOC_TOL = 2e-4   # mnet's tolerances (test_gpu_detector.py)
CONF_TOL = 2e-5
FAMILIES = [("slim", False), ("rfb", True)]
_BLOBS = {}


def _blob(frt, synth, tmp_path_factory, name, landmarks=True):
    key = (name, landmarks)
    if key not in _BLOBS:
        rfb = name == "rfb"
        sd = synth.slim_state(5, rfb=rfb, landmarks=landmarks)
        kind = frt.weights_io.KIND_RETINAFACE_RFB if rfb else frt.weights_io.KIND_RETINAFACE_SLIM
        path = frt.write_weights(str(tmp_path_factory.mktemp("slim") / ("%s_%d.frtw" % key)), sd, kind)
        _BLOBS[key] = (path, sd)
    return _BLOBS[key]


def _input(synth, n, h, w, start=0):
    fr = synth.make_frames(n, h, w, start=start)
    return np.ascontiguousarray((fr.astype(np.float32) - np.array([104, 117, 123], np.float32)).transpose(0, 3, 1, 2))


@pytest.mark.parametrize("name,rfb", FAMILIES)
@pytest.mark.parametrize("tag,hw", [("96x160", (96, 160)), ("288x320", (288, 320)), ("640", (640, 640)), (None, (100, 172))])
def test_network_matches_restatement_and_goldens(frt, synth, tmp_path_factory, name, rfb, tag, hw):
    h, w = hw
    path, sd = _blob(frt, synth, tmp_path_factory, name)
    det = frt.RetinaFace(path, w, h, (3, h, w), 2, 4)
    assert det.family == name and det.hasLandmarks and det.numAnchors == slim_ref.anchor_count(w, h)
    x = _input(synth, 2, h, w)
    loc, conf, ldm = det.doInferenceLandmarks(x)
    loc2, conf2 = det.doInference(x)
    assert np.array_equal(loc, loc2) and np.array_equal(conf, conf2)
    rloc, rconf, rldm = slim_ref.forward(sd, x, rfb)
    assert np.abs(loc - rloc).max() < LOC_TOL, np.abs(loc - rloc).max()
    assert np.abs(ldm - rldm).max() < LOC_TOL, np.abs(ldm - rldm).max()
    assert np.abs(conf - rconf).max() < CONF_TOL, np.abs(conf - rconf).max()
    if tag:
        g = np.load(os.path.join(GOLDEN, "retinaface_%s.npz" % name))
        s = int(g["step_" + tag])
        assert np.abs(loc[:, ::s] - g["loc_" + tag]).max() < LOC_TOL
        assert np.abs(ldm[:, ::s] - g["ldm_" + tag]).max() < LOC_TOL
        assert np.abs(conf[:, ::s] - g["conf_" + tag]).max() < CONF_TOL
    det.close()


def test_trimmed_slim_blob_without_landmark_heads(frt, synth, tmp_path_factory):
    path, sd = _blob(frt, synth, tmp_path_factory, "slim", landmarks=False)
    det = frt.RetinaFace(path, 160, 96, (3, 96, 160), 1, 4)
    assert not det.hasLandmarks
    x = _input(synth, 1, 96, 160)
    loc, conf = det.doInference(x)
    rloc, rconf, _ = slim_ref.forward(sd, x)
    assert np.abs(loc - rloc).max() < LOC_TOL and np.abs(conf - rconf).max() < CONF_TOL
    det.close()


@pytest.mark.parametrize("geom", [(640, 640, 640, 640), (320, 288, 640, 480), (320, 288, 480, 640), (160, 96, 161, 97), (172, 100, 172, 100)])
def test_postprocessing_on_injected_heads(frt, synth, tmp_path_factory, geom):
    in_w, in_h, fw, fh = geom
    path, _ = _blob(frt, synth, tmp_path_factory, "slim")
    for k in (4, 64):
        det = frt.RetinaFace(path, fw, fh, (3, in_h, in_w), 1, k, 0.4, 0.6)
        A = det.numAnchors
        assert A == slim_ref.anchor_count(in_w, in_h)
        for seed in range(3):
            r = np.random.default_rng(100 + seed)
            loc = (r.standard_normal((A, 4)) * 1.5).astype(np.float32)
            conf = np.zeros((A, 2), np.float32)
            conf[:, 1] = r.random(A).astype(np.float32) ** 8
            conf[r.integers(0, A, 40), 1] = np.float32(0.75)  # ties: lower anchor index first
            conf[r.integers(0, A, 5), 1] = np.nan             # NaN never passes the strict '>'
            conf[:, 0] = 1 - conf[:, 1]
            got = det.postprocessing(loc, conf)
            want = slim_ref.postprocess(loc, conf, in_w, in_h, fw, fh, 0.4, 0.6, k)
            assert len(got) == len(want) > 0, (geom, k, seed)
            for f in ("x1", "y1", "x2", "y2", "score"):
                assert np.array_equal(got[f], want[f]), (geom, k, seed, f)
        det.close()


@pytest.mark.parametrize("name,rfb", FAMILIES)
@pytest.mark.parametrize("geom", [(640, 640, 640, 640), (320, 288, 640, 480)])
def test_find_face_boxes_match_restatement(frt, orc, synth, tmp_path_factory, name, rfb, geom):
    in_w, in_h, fw, fh = geom
    path, sd = _blob(frt, synth, tmp_path_factory, name)
    det = frt.RetinaFace(path, fw, fh, (3, in_h, in_w), 4, 4, 0.4, 0.6)
    frames = synth.make_frames(4, fh, fw)
    got = det.findFaceBatch(frames)
    exact = total = 0
    for f in range(4):
        x = orc.det_preprocess(frames[f], in_h, in_w)
        rloc, rconf, _ = slim_ref.forward(sd, x[None], rfb)
        want = slim_ref.postprocess(rloc[0], rconf[0], in_w, in_h, fw, fh, 0.4, 0.6, 4)
        assert len(got[f]) == len(want) == 4
        single = det.findFace(frames[f])
        for k in ("x1", "y1", "x2", "y2", "score"):
            assert np.array_equal(single[k], got[f][k])
        for k in ("x1", "y1", "x2", "y2"):
            d = np.abs(got[f][k] - want[k])
            assert d.max() <= 1, (f, k, got[f], want)
            exact += int((d == 0).sum())
            total += d.size
        assert np.abs(got[f]["score"] - want["score"]).max() < CONF_TOL
    assert exact >= total - 2, (exact, total)
    det.close()


@pytest.mark.parametrize("name,rfb", FAMILIES)
def test_batch_of_32_equals_frame_by_frame(frt, synth, tmp_path_factory, name, rfb):
    path, _ = _blob(frt, synth, tmp_path_factory, name)
    det32 = frt.RetinaFace(path, 640, 640, (3, 640, 640), 32, 4)
    det1 = frt.RetinaFace(path, 640, 640, (3, 640, 640), 1, 4)
    frames = synth.make_frames(32, 640, 640)
    batch = det32.findFaceBatch(frames)
    for i in range(32):
        assert np.array_equal(batch[i], det1.findFace(frames[i])), i
    x = _input(synth, 32, 640, 640)
    loc32, conf32, ldm32 = det32.doInferenceLandmarks(x)
    for i in (0, 17, 31):
        loc1, conf1, ldm1 = det1.doInferenceLandmarks(x[i:i + 1])
        assert np.array_equal(loc32[i], loc1[0]) and np.array_equal(conf32[i], conf1[0]) and np.array_equal(ldm32[i], ldm1[0]), i
    det32.close()
    det1.close()


@pytest.mark.parametrize("name,rfb", FAMILIES)
@pytest.mark.parametrize("graph", [False, True])
def test_pipeline_submit_wait_equals_stage_by_stage(frt, synth, blobs, tmp_path_factory, name, rfb, graph):
    path, _ = _blob(frt, synth, tmp_path_factory, name)
    rpath, _ = blobs("ir")
    H = W = 320
    det = frt.RetinaFace(path, W, H, (3, H, W), 4, 4)
    rec = frt.ArcFaceIR50(rpath, W, H, maxBatchSize=64, maxFacesPerScene=4)
    gal = synth.make_gallery(2000)
    rec.setGallery(gal)
    rec.initMatMul()
    pipe = frt.Pipeline(det, rec, 4)
    pipe.set_graph(graph)
    calls = [synth.make_frames(1 + c % 2, H, W, start=3 * c) for c in range(8)]
    res = [np.zeros(len(f) * 4, frt.RESULT_DTYPE) for f in calls]
    emb = [np.zeros((len(f) * 4, 512), np.float32) for f in calls]
    crops = [np.zeros((len(f) * 4, 112, 112, 3), np.uint8) for f in calls]
    tickets = [pipe.submit(f, r, e, c) for f, r, e, c in zip(calls, res, emb, crops)]  # >= 6 in flight: merging may engage
    for t in tickets:
        pipe.wait(t)
    for f, r, e, c in zip(calls, res, emb, crops):
        boxes = det.findFaceBatch(f)
        for i in range(len(f)):
            rr = r[i * 4:(i + 1) * 4]
            n = len(boxes[i])
            assert n > 0
            for k in ("x1", "y1", "x2", "y2", "score"):
                assert np.array_equal(rr[k][:n], boxes[i][k]), (name, graph, k)
            assert np.all(rr["frame"] == i)
            assert np.all(rr["valid"][:n] == 1) and np.all(rr["valid"][n:] == 0)
            emb1 = rec.forward(f[i], boxes[i])  # stage by stage: the recogniser on the detector's boxes
            for j in range(n):
                assert np.array_equal(c[i * 4 + j], rec.croppedFaces[j]["face"]), (name, graph, j)
                assert float((e[i * 4 + j].astype(np.float64) * emb1[j]).sum()) > 1 - 1e-5
            idx, sim = rec.matmul.top1(e[i * 4:i * 4 + n])
            assert np.array_equal(rr["match_idx"][:n], idx) and np.array_equal(rr["match_sim"][:n], sim)
    pipe.close()
    rec.close()
    det.close()


def test_alignment_mode_on_slim_landmarks(frt, synth, tmp_path_factory):
    path, sd = _blob(frt, synth, tmp_path_factory, "slim")
    det = frt.RetinaFace(path, 320, 288, (3, 288, 320), 1, 4)
    frame = synth.make_frames(1, 288, 320)[0]
    boxes, ldm = det.findFaceLandmarks(frame)
    assert len(boxes) > 0 and ldm.shape == (len(boxes), 5, 2)
    for k in ("x1", "y1", "x2", "y2", "score"):
        assert np.array_equal(boxes[k], det.findFace(frame)[k])
    # landmarks = anchor centre + pre * 0.1 * anchor size with the kept anchors of the 4-level table
    x = _input(synth, 1, 288, 320)
    rloc, rconf, rldm = slim_ref.forward(sd, x)
    _, kept = slim_ref.postprocess(rloc[0], rconf[0], 320, 288, 320, 288, 0.4, 0.6, 4, return_kept=True)
    anc = slim_ref.anchors(320, 288)[kept]
    pre = rldm[0][kept].reshape(-1, 5, 2)
    want = np.stack([(anc[:, None, 0] + pre[..., 0] * 0.1 * anc[:, None, 2]) * 320, (anc[:, None, 1] + pre[..., 1] * 0.1 * anc[:, None, 3]) * 288], -1)
    assert np.abs(ldm - want).max() < 0.05, np.abs(ldm - want).max()
    det.close()
