"""Flip-augmented embeddings (frt_embedder_set_flip; DESIGN "Flip-augmented embeddings"): normalize(pre(x) + pre(mirror x)) on every path that
goes through the recogniser, against the float64 reference of tests/flip_ref.py built on the fp32 oracle.

Tolerances.  Against the reference: cos > 1 - 1e-4, test_gpu_embedder.py's COS_TOL.  It holds here by derivation, not by luck: each of the two
pre-normalisation vectors carries the plain path's error (1 - cos of 6e-6 class), and their sum is at least 1.3 times as long as the longer of
them on these faces (tests/test_flip_ref.py asserts it from the oracle alone), so 1 - cos grows by at most (2 / 1.3)^2 ~ 2.4.  fp32 mode: the
plain mode's 1e-6 times that, 3e-6.  One function over different kernel paths (batch position, batch size class): cos > 1 - 1e-5 and
max |d| < 1e-3, as everywhere in this suite.  Nine faces at maxBatchSize 8 run as sub-passes of 4 + 4 + 1."""
import numpy as np
import pytest

import flip_ref as FR
from conftest import face_input

pytestmark = pytest.mark.gpu
COS_TOL = 1e-4
MODES = ["ir", "ir_se"]


@pytest.fixture(scope="module")
def nine(synth, blobs):
    """mode -> (blob path, state dict, x [9][3][112][112], reference [9][512]); computed once per mode, never modified."""
    x = face_input(synth.make_faces(9))
    x.flags.writeable = False
    cache = {}

    def get(mode):
        if mode not in cache:
            path, sd = blobs(mode)
            ref = FR.flip_reference(sd, x)
            ref.flags.writeable = False
            cache[mode] = (path, sd, x, ref)
        return cache[mode]

    return get


def cos64(a, b):
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64)).sum(1)


def alike(a, b):
    """one function over different kernel paths"""
    return cos64(a, b).min() > 1 - 1e-5 and np.abs(a - b).max() < 1e-3


@pytest.mark.parametrize("mode", MODES)
def test_flip_embeddings_match_the_reference_and_off_restores_the_plain_bytes(frt, nine, mode):
    path, _, x, ref = nine(mode)
    rec = frt.ArcFaceIR50(path, maxBatchSize=8)
    assert rec.flip is False
    plain = rec.doInference(x)
    rec.setFlip(True)
    assert rec.flip is True
    emb = rec.doInference(x)
    rec.setFlip(False)
    assert rec.flip is False
    back = rec.doInference(x)
    rec.close()
    cos = cos64(emb, ref)
    print("%s: 1 - cos to the reference %.3g .. %.3g, cos to the plain embeddings %.3f .. %.3f" % (mode, 1 - cos.max(), 1 - cos.min(), cos64(emb, plain).min(), cos64(emb, plain).max()))
    assert np.isfinite(emb).all() and cos.min() > 1 - COS_TOL
    assert np.allclose((emb.astype(np.float64) ** 2).sum(1), 1, atol=1e-5)
    assert cos64(emb, plain).max() < 0.9                # another vector altogether: a missing mirror image would not pass
    assert np.array_equal(back, plain)                  # off again: the bytes from before the mode was ever set


@pytest.mark.parametrize("mode", MODES)
def test_a_face_and_its_mirror_image_embed_alike(frt, nine, mode):
    path, _, x, _ = nine(mode)
    rec = frt.ArcFaceIR50(path, maxBatchSize=8)
    rec.setFlip(True)
    a = rec.doInference(x)
    b = rec.doInference(np.ascontiguousarray(x[..., ::-1]))
    rec.close()
    print("%s: 1 - cos %.3g, max |d| %.3g" % (mode, 1 - cos64(a, b).min(), np.abs(a - b).max()))
    assert alike(a, b)


@pytest.mark.parametrize("mode", MODES)
def test_every_batch_size_embeds_alike_and_repeats_bit_for_bit(frt, nine, mode):
    """maxBatchSize 1: the face and its mirror image as two one-face passes; 5: sub-passes of 2 + 2 faces of every 5; 8: 4 + 4 + 1."""
    path, _, x, ref = nine(mode)
    got = {}
    for mb in (8, 1, 5):
        rec = frt.ArcFaceIR50(path, maxBatchSize=mb)
        rec.setFlip(True)
        got[mb] = rec.doInference(x)
        assert np.array_equal(rec.doInference(x), got[mb]), mb
        rec.close()
        assert cos64(got[mb], ref).min() > 1 - COS_TOL, mb
    for mb in (1, 5):
        print("%s: maxBatchSize %d against 8: 1 - cos %.3g, max |d| %.3g" % (mode, mb, 1 - cos64(got[mb], got[8]).min(), np.abs(got[mb] - got[8]).max()))
        assert alike(got[mb], got[8]), mb


@pytest.mark.parametrize("mode", MODES)
def test_flip_in_fp32_mode(frt, nine, mode):
    path, _, x, ref = nine(mode)
    rec = frt.ArcFaceIR50(path, maxBatchSize=8)
    rec.setPrecision(True)
    rec.setFlip(True)
    got = rec.doInference(x)
    rec.close()
    cos = cos64(got, ref)
    print("%s fp32: 1 - cos to the reference %.3g .. %.3g" % (mode, 1 - cos.max(), 1 - cos.min()))
    assert np.isfinite(got).all() and (1 - cos).max() <= 3e-6


def test_frame_and_face_image_routes_and_enrolment(frt, orc, synth, blobs):
    """forward (boxes on a frame), forwardFaces (images of any sizes) and enrolFaces with flip on: the reference on the oracle's crops; the
    enrolled rows are the probes' own (gallery and probes in one mode)."""
    path, sd = blobs("ir")
    rec = frt.ArcFaceIR50(path, maxBatchSize=4)
    rec.setFlip(True)
    fr = synth.make_frame(3, 480, 640)
    boxes = np.zeros(3, frt.BBOX_DTYPE)
    boxes[0] = (30, 40, 200, 180, 0.9)
    boxes[1] = (100, 300, 212, 412, 0.8)
    boxes[2] = (250, 10, 479, 300, 0.7)
    emb = rec.forward(fr, boxes).copy()
    ocrops = orc.crop_faces(fr, boxes)
    assert np.array_equal(np.stack([c["face"] for c in rec.croppedFaces]), ocrops)
    pre, pre_m = FR.pre_vectors(sd, orc.face_normalize(ocrops))
    assert FR.sum_ratio(pre, pre_m).min() >= 1.3
    assert cos64(emb, FR.normalize(pre + pre_m)).min() > 1 - COS_TOL
    # face images: five sizes, chunks of 4 + 1
    imgs = [synth.make_frame(100 + i, r, c) for i, (r, c) in enumerate([(56, 56), (112, 112), (113, 111), (224, 224), (37, 201)])]
    icrops = np.stack([orc.resize_linear(im, 112, 112) for im in imgs])
    femb = rec.forwardFaces(imgs).copy()
    assert np.array_equal(np.stack([c["face"] for c in rec.croppedFaces]), icrops)
    pre, pre_m = FR.pre_vectors(sd, orc.face_normalize(icrops))
    assert FR.sum_ratio(pre, pre_m).min() >= 1.3
    assert cos64(femb, FR.normalize(pre + pre_m)).min() > 1 - COS_TOL
    assert np.array_equal(femb, rec.doInference(face_input(icrops)))
    # enrol them behind a random gallery, then look the same faces up
    gal = synth.make_gallery(300)
    rec.setGallery(gal, ["u%d" % i for i in range(300)])
    rec.initMatMul()
    names = ["new%d" % i for i in range(5)]
    first, eemb = rec.enrolFaces(names, imgs)
    assert first == 300 and np.array_equal(eemb, femb)
    rec.forwardFaces(imgs)
    got_names, sims = rec.matchTop1()
    assert got_names == names and min(sims) > 0.9999
    # a plain probe against the flip rows: no match of that quality (the header's contract, seen from the other side)
    rec.setFlip(False)
    rec.forwardFaces(imgs)
    _, sims_plain = rec.matchTop1()
    assert max(sims_plain) < 0.9
    rec.close()


def test_pipeline_with_flip_and_graph_replay(frt, synth, blobs):
    """The pipeline route: two 160x224 frames (test_gpu_pipeline.py's smallest) of four faces, recogniser maxBatchSize 8: one call is two
    sub-passes of four faces.  make_frames(start=26) is the first seed at which the oracle's detector finds four faces in both frames and the
    oracle's recogniser a sum ratio >= 1.3 on all eight crops (1.309 .. 1.945; seeds 10 - 12 also give eight faces, with ratios down to 1.22).
    Then hipGraph replay.  A part-1 key carries the call's box slot, which recurs every NSLOT = 10 calls, so "three sightings of the same
    buffers" are three rounds of ten calls: the first round runs eagerly, the second is captured, the third replays.  Flip off: graph_stats
    shows replays and every call equals the run without graphs.  Flip on: a captured plain graph must not replay - part 1 is captured anew
    (10 more graphs) and all three rounds return the flip embeddings."""
    import torch
    dpath, _ = blobs("det")
    rpath, rsd = blobs("ir")
    B, K, H, W = 2, 4, 160, 224
    det = frt.RetinaFace(dpath, W, H, (3, H, W), B, K, 0.4, 0.6)
    rec = frt.ArcFaceIR50(rpath, W, H, maxBatchSize=B * K, maxFacesPerScene=K)
    rec.setGallery(synth.make_gallery(512))
    rec.initMatMul()
    pipe = frt.Pipeline(det, rec, B)
    frames = synth.make_frames(B, H, W, start=26)

    def with_crops():
        res, emb, crops = np.zeros(B * K, frt.RESULT_DTYPE), np.zeros((B * K, 512), np.float32), np.zeros((B * K, 112, 112, 3), np.uint8)
        pipe.wait(pipe.submit(frames, res, emb, crops))
        return res, emb, crops

    res0, plain, crops = with_crops()
    assert res0["valid"].all()
    rec.setFlip(True)
    res1, emb, crops1 = with_crops()
    assert all(np.array_equal(res1[c], res0[c]) for c in ("x1", "y1", "x2", "y2", "valid")) and np.array_equal(crops1, crops)
    x = face_input(crops)
    direct = rec.doInference(x)
    assert cos64(emb, direct).min() > 1 - 1e-5
    pre, pre_m = FR.pre_vectors(rsd, x)
    ratio = FR.sum_ratio(pre, pre_m)
    print("|pre + pre_m| / max(|pre|, |pre_m|) on the call's crops: %.3f .. %.3f" % (ratio.min(), ratio.max()))
    # (these crops are the device's own, a pixel of a box may differ from the oracle's: the condition is asked with that margin - (2 / 1.2)^2 ~ 2.8
    #  times the plain path's 6e-6 class is still far inside 1e-4)
    assert ratio.min() >= 1.2
    assert cos64(emb, FR.normalize(pre + pre_m)).min() > 1 - COS_TOL
    assert cos64(emb, plain).min() < 0.9
    rec.setFlip(False)

    # ---- graphs: device-resident calls on the same buffers
    d_f = torch.from_numpy(frames).cuda()
    d_r = torch.zeros(B * K * frt.RESULT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    d_e = torch.zeros((B * K, 512), dtype=torch.float32, device="cuda")
    st = torch.cuda.Stream()
    pipe.set_stream(st.cuda_stream)

    def call():
        d_e.zero_()
        torch.cuda.synchronize()
        pipe.run_dev(d_f.data_ptr(), B, d_r.data_ptr(), d_e.data_ptr())
        pipe.sync()
        st.synchronize()
        return d_e.cpu().numpy().copy()

    want_plain = call()
    rec.setFlip(True)
    want_flip = call()
    rec.setFlip(False)
    assert alike(want_plain, plain) and alike(want_flip, emb) and cos64(want_flip, want_plain).min() < 0.9
    pipe.set_graph(True)
    c0, r0 = pipe.graph_stats()
    for i in range(30):
        assert np.array_equal(call(), want_plain), i
    c1, r1 = pipe.graph_stats()
    assert c1 - c0 == 30 and r1 - r0 == 30, (c1 - c0, r1 - r0)   # 3 parts x 10 slots captured in the second round, replayed in the third
    rec.setFlip(True)
    for i in range(30):
        assert np.array_equal(call(), want_flip), i
    c2, r2 = pipe.graph_stats()
    # parts 0 and 2 go on replaying (3 x 20); part 1 is seen anew: eager, captured (10 more graphs), replayed (10)
    assert c2 - c1 == 10 and r2 - r1 == 70, (c2 - c1, r2 - r1)
    pipe.set_graph(False)
    pipe.close()
    det.close()
    rec.close()
