"""Whole photos of any sizes: frt_resize_images, frt_enrol_select_dev, frt_pipeline_run_images / _enrol_images and their shells (resizeImages,
Pipeline.runImages / enrolImages, ArcFaceIR50::enrolImages) - the head of /inference (src/app.cpp:296-301) and /insert/face without
api_imgIsCropped (:163-187) for ragged batches."""
import os
import subprocess
import threading
import time

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

PKG = os.path.join(ROOT, "face-recognition-cpp-tensorrt_amd")
SIZES = [(1, 1), (1, 7), (9, 1), (56, 56), (112, 112), (224, 224), (448, 448), (113, 111), (37, 201), (333, 500)]
# the ten photos of the end-to-end rule: synth.make_frame(300 + i, rows, cols)
PHOTOS = [(0, (160, 160)), (1, (97, 131)), (2, (240, 320)), (3, (333, 500)), (4, (64, 48)), (5, (480, 360)), (7, (123, 457)), (8, (320, 240)),
          (9, (50, 61)), (11, (161, 159))]
H = W = 160
B, K = 4, 4  # pipeline max_frames (chunks 4 + 4 + 2), maxFacesPerScene
OK, MANY, NONE, EMPTY_ROI = 1, 2, 3, 4


def rule(counts, valid0=None):
    """the "exactly one face" rule of app.cpp:172-177 on box counts"""
    counts = np.asarray(counts)
    one = np.where(np.ones(len(counts), bool) if valid0 is None else np.asarray(valid0) != 0, OK, EMPTY_ROI)
    return np.where(counts == 0, NONE, np.where(counts > 1, MANY, one)).astype(np.int32)


def intern(names):
    table = {}
    return np.array([table.setdefault(n, len(table)) for n in names], np.int32)


@pytest.fixture(scope="module")
def ragged(synth):
    """The eleven images of tests/test_gpu_faces.py: ten sizes and one 50x61 view of a 50x80 array (padded stride)."""
    rng = np.random.default_rng(20240611)
    imgs = [synth.make_frame(100 + i, r, c) if min(r, c) >= 32 else rng.integers(0, 256, (r, c, 3), dtype=np.uint8) for i, (r, c) in enumerate(SIZES)]
    imgs.append(synth.make_frame(77, 50, 80)[:, :61])
    assert imgs[-1].strides[0] == 240 and not imgs[-1].flags.c_contiguous
    for a in imgs:
        a.flags.writeable = False
    return imgs


@pytest.fixture(scope="module")
def photos(synth, orc, blobs):
    """The ten photos, their oracle frames (cv::resize to 160 x 160), the oracle's boxes with maxFacesPerScene 4 and 1, and the distance of
    the nearest anchor score to the 0.6 threshold.  Shared, never modified."""
    from oracle import nets
    _, dsd = blobs("det")
    imgs = [synth.make_frame(300 + i, r, c) for i, (r, c) in PHOTOS]
    frames = np.stack([orc.resize_linear(im, H, W) for im in imgs])
    boxes, boxes1, margin = [], [], []
    for f in frames:
        loc, conf = nets.retinaface_forward(dsd, orc.det_preprocess(f, H, W)[None])
        boxes.append(orc.postprocess(loc[0], conf[0], W, H, W, H, 0.4, 0.6, K))
        boxes1.append(orc.postprocess(loc[0], conf[0], W, H, W, H, 0.4, 0.6, 1))
        margin.append(float(np.abs(conf[0][:, 1] - 0.6).min()))
    status = rule([len(b) for b in boxes])
    # preconditions: a changed generator fails here, loudly, instead of testing nothing
    print("oracle box counts %s, nearest score to the threshold %.4f" % ([len(b) for b in boxes], min(margin)))
    assert min(margin) >= 0.004, margin
    assert {OK, MANY, NONE} <= set(status.tolist()), status
    for a in imgs + [frames]:
        a.flags.writeable = False
    return dict(imgs=imgs, frames=frames, boxes=boxes, boxes1=boxes1, status=status)


def make_pipeline(frt, blobs, max_faces=K, gallery=None, names=None):
    dpath, _ = blobs("det")
    rpath, _ = blobs("ir")
    det = frt.RetinaFace(dpath, W, H, (3, H, W), B, max_faces, 0.4, 0.6)
    rec = frt.ArcFaceIR50(rpath, W, H, maxBatchSize=B * max_faces, maxFacesPerScene=max_faces)
    if gallery is not None:
        rec.setGallery(gallery, list(names) if names is not None else None)
        rec.initMatMul()
    return det, rec, frt.Pipeline(det, rec, B)


def close(*objs):
    for o in objs:
        o.close()


# ------------------------------------------------------------------------------------------------------------ 1. the resize kernel
def test_resize_kernel_is_the_oracle_bit_for_bit(frt, orc, synth, ragged):
    """resizeImages == oracle.resize_linear == resizeFrame per image, at 160 x 160, 96 rows x 160 cols (a rows / cols swap shows), 37 x 53 and,
    for three of them, 640 x 640; a same-size source is a copy; 320 x 320 at 160 x 160 is the 2 x 2 rounded mean."""
    for rows, cols, pick in ((160, 160, range(11)), (96, 160, range(11)), (37, 53, range(11)), (640, 640, (3, 9, 10))):
        imgs = [ragged[i] for i in pick]
        got = frt.resizeImages(imgs, cols, rows)
        assert got.shape == (len(imgs), rows, cols, 3)
        for j, im in enumerate(imgs):
            assert np.array_equal(got[j], orc.resize_linear(im, rows, cols)), (rows, cols, im.shape)
            assert np.array_equal(got[j], frt.resizeFrame(im, cols, rows)), (rows, cols, im.shape)
    same = frt.resizeImages([ragged[8], ragged[4], ragged[10]], 201, 37)  # 37 x 201 among others
    assert np.array_equal(same[0], ragged[8])
    assert np.array_equal(frt.resizeImages([ragged[10]], 61, 50)[0], ragged[10])  # the strided view, copied tight
    big = synth.make_frame(120, 320, 320)
    q = big.astype(np.int32)
    mean = ((q[0::2, 0::2] + q[0::2, 1::2] + q[1::2, 0::2] + q[1::2, 1::2] + 2) >> 2).astype(np.uint8)
    assert np.array_equal(frt.resizeImages([ragged[0], big], 160, 160)[1], mean)
    assert frt.resizeImages([], 160, 160).shape == (0, 160, 160, 3)


# ------------------------------------------------------------------------------------------------------------ 2. the selection kernel
def injected(frt, rng, n, max_faces):
    """records [n][max_faces] as the pipeline packs them (boxes from slot 0 on, unused slots zero with score 0) covering every status, and
    what the kernel must make of them, in NumPy"""
    rec = np.zeros((n, max_faces), frt.RESULT_DTYPE)
    rec["frame"] = np.arange(n, dtype=np.int32)[:, None] % 7  # (chunk-local in real use: any value must be kept)
    rec["match_idx"] = -1
    kind = rng.integers(0, 4 if max_faces > 1 else 3, n)  # 0 none, 1 one valid box, 2 one box with an empty ROI, 3 several boxes
    for f in range(n):
        nb = (0, 1, 1, 0)[kind[f]] or (int(rng.integers(2, max_faces + 1)) if kind[f] == 3 else 0)
        for j in range(nb):
            for c in ("x1", "y1", "x2", "y2"):
                rec[c][f, j] = rng.integers(0, 80)
            rec["score"][f, j] = 0.6 + 0.4 * rng.random()
            rec["valid"][f, j] = 0 if kind[f] == 2 else (1 if kind[f] == 1 else rng.integers(0, 2))
            if rec["valid"][f, j]:
                rec["match_idx"][f, j], rec["match_sim"][f, j] = rng.integers(0, 1000), rng.random()
    emb = rng.standard_normal((n, max_faces, 512)).astype(np.float32)
    status = rule((rec["score"] > 0).sum(1), rec["valid"][:, 0]) if n else np.zeros(0, np.int32)
    face = rec[:, 0].copy()
    gone = (status == MANY) | (status == NONE)
    keep = face["frame"][gone].copy()
    face[gone] = np.zeros((), frt.RESULT_DTYPE)
    face["frame"][gone] = keep
    return rec, emb, status, face, emb[status == OK, 0]


@pytest.mark.parametrize("max_faces", [1, 4])
def test_selection_kernel_on_injected_records(frt, max_faces):
    import torch
    rng = np.random.default_rng(77 + max_faces)
    dev = torch.device("cuda:0")
    side = torch.cuda.Stream(device=dev)
    seen = set()
    for n in (0, 1, 5, 33, 257):
        a, b = injected(frt, rng, n, max_faces), injected(frt, rng, n, max_faces)
        seen |= set(a[2].tolist()) | set(b[2].tolist())
        for stream in (None, side):
            cap = 2 * n + 3
            rows = torch.full((cap, 512), -7.0, device=dev)
            count = torch.tensor([0], dtype=torch.int32, device=dev)
            outs = []
            up = []
            for rec, emb, _, _, _ in (a, b):
                up.append((torch.from_numpy(rec.view(np.uint8).reshape(-1).copy()).to(dev), torch.from_numpy(emb).to(dev)))
                outs.append((torch.full((max(n, 1),), -1, dtype=torch.int32, device=dev),
                             torch.zeros(max(n, 1) * frt.RESULT_DTYPE.itemsize, dtype=torch.uint8, device=dev)))
            torch.cuda.synchronize()
            for (d_rec, d_emb), (d_status, d_face) in zip(up, outs):  # two calls in a row on one stream with the same count append
                frt.enrol_select_dev(d_rec.data_ptr(), d_emb.data_ptr(), n, max_faces, d_status.data_ptr(), d_face.data_ptr(), rows.data_ptr(),
                                     count.data_ptr(), stream.cuda_stream if stream else None)
            torch.cuda.synchronize()
            want_rows = np.concatenate([a[4], b[4]])
            assert int(count.item()) == len(want_rows), (n, max_faces)
            got_rows = rows.cpu().numpy()
            assert np.array_equal(got_rows[:len(want_rows)], want_rows) and (got_rows[len(want_rows):] == -7.0).all(), (n, max_faces)
            for (_, _, status, face, _), (d_status, d_face) in zip((a, b), outs):
                assert np.array_equal(d_status.cpu().numpy()[:n], status), (n, max_faces)
                assert np.array_equal(d_face.cpu().numpy()[:n * frt.RESULT_DTYPE.itemsize].view(frt.RESULT_DTYPE), face), (n, max_faces)
            if n:  # face_dev may be NULL; a non-zero base is kept
                count.fill_(2)
                frt.enrol_select_dev(up[0][0].data_ptr(), up[0][1].data_ptr(), n, max_faces, outs[0][0].data_ptr(), None, rows.data_ptr(), count.data_ptr(),
                                     stream.cuda_stream if stream else None)
                torch.cuda.synchronize()
                assert int(count.item()) == 2 + len(a[4]) and np.array_equal(rows.cpu().numpy()[2:2 + len(a[4])], a[4])
            else:  # n_frames == 0 leaves count alone
                count.fill_(5)
                frt.enrol_select_dev(None, None, 0, max_faces, None, None, None, count.data_ptr(), None)
                torch.cuda.synchronize()
                assert int(count.item()) == 5
    assert seen == ({OK, MANY, NONE, EMPTY_ROI} if max_faces > 1 else {OK, NONE, EMPTY_ROI}), seen


# ------------------------------------------------------------------------------------------------------------ 3. the rule end to end
def run_in_chunks(frt, pipe, frames):
    """Pipeline.run's path (submit + wait, with crops) over chunks of B frames, `frame` rebased to the index in the call"""
    res, emb, crops = [], [], []
    for f0 in range(0, len(frames), B):
        part = np.ascontiguousarray(frames[f0:f0 + B])
        r = np.zeros(len(part) * K, frt.RESULT_DTYPE)
        e = np.zeros((len(part) * K, 512), np.float32)
        c = np.zeros((len(part) * K, 112, 112, 3), np.uint8)
        pipe.wait(pipe.submit(part, r, e, c))
        r["frame"] += f0
        res.append(r)
        emb.append(e)
        crops.append(c)
    return np.concatenate(res), np.concatenate(emb), np.concatenate(crops)


def test_the_rule_end_to_end(frt, orc, synth, blobs, photos):
    from oracle import nets
    _, rsd = blobs("ir")
    imgs, frames, ostatus = photos["imgs"], photos["frames"], photos["status"]
    gal = synth.make_gallery(400)
    det, rec, pipe = make_pipeline(frt, blobs, gallery=gal)
    # /inference for the ten photos == Pipeline.run on the oracle's resized frames, fed in the same chunks, bit for bit
    res, emb, crops = pipe.runImages(imgs, want_crops=True)
    wres, wemb, wcrops = run_in_chunks(frt, pipe, frames)
    assert np.array_equal(res, wres) and np.array_equal(res["frame"], np.repeat(np.arange(10), K))
    assert np.array_equal(emb, wemb)
    used = res["valid"] != 0
    assert np.array_equal(crops[used], wcrops[used])
    res2, emb2 = pipe.runImages(imgs)  # without crops, second call on the same staging
    assert np.array_equal(res2, res) and np.array_equal(emb2, emb)
    res3, none = pipe.runImages(imgs[:5], want_embeds=False)
    assert none is None and np.array_equal(res3, res[:5 * K])
    assert pipe.runImages([])[0].shape == (0,)
    # the rule: the oracle's, and the one applied to the detector's own boxes on the resized frames
    status, first, enrolled, faces = pipe.enrolImages(["p%d" % i for i in range(10)], imgs)
    found = []
    for f0 in range(0, 10, B):
        found += det.findFaceBatch(frames[f0:f0 + B])
    print("status %s" % status.tolist())
    assert np.array_equal(status, ostatus)
    assert np.array_equal(status, rule([len(b) for b in found]))
    assert np.array_equal(status, rule((res["score"].reshape(10, K) > 0).sum(1), res["valid"].reshape(10, K)[:, 0]))
    assert first == 400 and len(enrolled) == int((ostatus == OK).sum()) and rec.classNames[400:] == ["p%d" % i for i in np.flatnonzero(ostatus == OK)]
    # the accepted photos against the oracle chain, when the box is the oracle's (tests/test_gpu_pipeline.py's tolerance)
    compared = 0
    for row, i in enumerate(np.flatnonzero(ostatus == OK)):
        ob = photos["boxes"][i]
        oemb = nets.arcface_forward(rsd, orc.face_normalize(orc.crop_faces(frames[i], ob)))[0]
        r = res[i * K]
        assert all(abs(int(r[c]) - int(ob[0][c])) <= 1 for c in ("x1", "y1", "x2", "y2")), (i, r, ob)
        cos = float((enrolled[row] * oemb).sum())
        print("photo %d: cosine vs the oracle chain %.8f" % (i, cos))
        if all(r[c] == ob[0][c] for c in ("x1", "y1", "x2", "y2")):
            assert cos >= 1 - 1e-4, (i, cos)
            compared += 1
    assert compared >= 1
    close(pipe, det, rec)
    # maxFacesPerScene 1: the cap behind NMS leaves one box, so "more than one" cannot occur (the reference's behaviour too)
    det1, rec1, pipe1 = make_pipeline(frt, blobs, max_faces=1)
    status1 = pipe1.enrolImages(["p%d" % i for i in range(10)], imgs)[0]
    assert np.array_equal(status1, rule([len(b) for b in photos["boxes1"]]))
    assert np.array_equal(status1, np.where(ostatus == MANY, OK, ostatus))
    close(pipe1, det1, rec1)


# ------------------------------------------------------------------------------------------------------------ 4. enrolment is one edit
@pytest.mark.parametrize("labelled", [False, True], ids=["unlabelled", "labelled"])
def test_enrol_images_is_one_gallery_edit(frt, synth, blobs, photos, labelled):
    imgs, ostatus = photos["imgs"], photos["status"]
    accepted = np.flatnonzero(ostatus == OK)
    N = 400
    gal = synth.make_gallery(N)
    names = ["u%d" % (i % 100) for i in range(N)]
    new_names = ["u3", "new", "new", "u7", "zed", "new", "u9", "amy", "bob", "zed"]
    all_labels = intern(names + new_names)
    det, rec, pipe = make_pipeline(frt, blobs, gallery=gal, names=names)
    mm = rec.matmul
    if labelled:
        mm.set_labels(all_labels[:N])
    res, emb = pipe.runImages(imgs)
    want_emb = emb.reshape(10, K, 512)[accepted, 0]
    old = frt.MatMul(0)
    old.init(gal)
    # room for the new rows: an add that has to move the gallery of a matcher with a pipeline also moves its scratch, which is a generation
    # step of its own (frt_matcher_generation); inside the capacity one edit is exactly one step
    mm.galleryReserve(N + 16)
    gen = mm.generation()
    uploaded = mm.editStats()["rows_uploaded"]

    def unchanged():
        return frt.lib.frt_matcher_num_rows(mm._h) == N and mm.generation() == gen and rec.classCount == N

    # refused before any device work: a negative label, the wrong form for the gallery
    bad = all_labels[N:].copy()
    bad[6] = -1
    for labels, word in ((bad, "image 6"), (None if labelled else all_labels[N:], "labelled" if labelled else "no labels")):
        with pytest.raises(frt.FrtError) as err:
            pipe.enrolImages(new_names, imgs, labels=labels)
        assert err.value.code == frt.FRT_ERR_INVALID and word in str(err.value) and unchanged()
    # a batch with no acceptable photo: no edit
    nobody = [i for i in range(10) if ostatus[i] != OK]
    st, first, e, _ = pipe.enrolImages([new_names[i] for i in nobody], [imgs[i] for i in nobody], labels=all_labels[N:][nobody] if labelled else None)
    assert np.array_equal(st, ostatus[nobody]) and first == N and e.shape == (0, 512) and unchanged()

    def enrol():
        return pipe.enrolImages(new_names, imgs, labels=all_labels[N:] if labelled else None)

    def check(got):
        status, first, e, faces = got
        assert np.array_equal(status, ostatus) and first == N and len(e) == 2 == len(accepted)
        assert frt.lib.frt_matcher_num_rows(mm._h) == N + 2 == mm.m and mm.generation() == gen + 1  # ONE edit
        assert mm.editStats()["rows_uploaded"] == uploaded + 2
        assert rec.classNames[N:] == [new_names[i] for i in accepted] and rec.classCount == N + 2
        assert np.array_equal(e, want_emb)
        # the faces: slot 0's record of the accepted photos, matched against the gallery as it was before the call
        assert np.array_equal(faces["frame"], np.arange(10))
        oidx, osim = old.top1(e)
        assert np.array_equal(faces["match_idx"][accepted], oidx) and np.array_equal(faces["match_sim"][accepted], osim)
        assert (faces["match_idx"][accepted] < N).all() and (faces["valid"][accepted] == 1).all()
        for c in ("x1", "y1", "x2", "y2", "score", "match_idx", "match_sim", "valid"):
            assert np.array_equal(faces[c][accepted], res[c].reshape(10, K)[accepted, 0]), c
            assert (faces[c][nobody] == 0).all(), c
        # the gallery answers as a fresh one initialised with the old rows + those embeddings (+ labels)
        fresh = frt.MatMul(0)
        fresh.init(np.concatenate([gal, e]))
        q = np.concatenate([e, synth.make_queries(gal, [5, 250], noise=0.02, seed=9)])
        assert np.array_equal(mm.calculate(q), fresh.calculate(q))
        idx, sim = mm.top1(e)
        assert idx.tolist() == [N, N + 1] and sim.min() > 0.999
        if labelled:
            fresh.set_labels(np.concatenate([all_labels[:N], all_labels[N:][accepted]]))
            for x, y in zip(mm.topk_labels(q, 3), fresh.topk_labels(q, 3)):
                assert np.array_equal(x, y)
        fresh.close()

    check(enrol())
    # the same call while another thread keeps submits in flight on the same pipeline: the same answers on both sides
    batches = [synth.make_frames(B, H, W, start=40 + 4 * i) for i in range(4)]
    want = [tuple(a.copy() for a in pipe.run(b)) for b in batches]
    mm.galleryRemove([N, N + 1])
    rec.classNames = rec.classNames[:N]
    rec.classCount = N
    gen = mm.generation()
    uploaded = mm.editStats()["rows_uploaded"]
    got, stamps, errors = [], [], []
    started, stop = threading.Event(), threading.Event()

    def worker():  # keeps one submit after the other in flight until the main thread says that its call has returned
        try:
            while not stop.is_set() and len(got) < 4000:
                b = batches[len(got) % len(batches)]
                r = np.zeros(B * K, frt.RESULT_DTYPE)
                e = np.zeros((B * K, 512), np.float32)
                stamps.append(time.perf_counter())
                pipe.wait(pipe.submit(b, r, e))
                got.append((r, e))
                started.set()
        except Exception as ex:  # noqa: BLE001
            errors.append(ex)
        started.set()

    t = threading.Thread(target=worker)
    t.start()
    assert started.wait(60)
    t0 = time.perf_counter()
    beside = enrol()
    t1 = time.perf_counter()
    stop.set()
    t.join()
    during = sum(t0 <= x <= t1 for x in stamps)
    print("submits of the other thread: %d in all, %d made while enrolImages ran (%.1f ms)" % (len(stamps), during, (t1 - t0) * 1e3))
    assert during >= 1, (len(stamps), t0, t1)
    assert not errors, errors
    check(beside)
    for i, (r, e) in enumerate(got):  # (the match fields may see the gallery before or after the edit)
        w = want[i % len(batches)]
        for c in ("x1", "y1", "x2", "y2", "score", "frame", "valid"):
            assert np.array_equal(r[c], w[0][c]), (i, c)
        assert np.array_equal(e, w[1]), i
    # too many images for one call: refused before anything runs
    arr, keep = frt._face_images([imgs[0]])
    many = (frt.FaceImage * 65537)(*([arr[0]] * 65537))
    status = np.zeros(65537, np.int32)
    assert frt.lib.frt_pipeline_enrol_images(pipe._h, many, 65537, None, status.ctypes.data, None, None, None, None) == frt.FRT_ERR_CAPACITY
    assert frt.lib.frt_matcher_num_rows(mm._h) == N + 2
    # a pipeline without a matcher cannot enrol
    bare = frt.Pipeline(det, rec, B, match=False)
    assert frt.lib.frt_pipeline_enrol_images(bare._h, arr, 1, None, status.ctypes.data, None, None, None, None) == frt.FRT_ERR_INVALID
    with pytest.raises(frt.FrtError) as err:
        bare.enrolImages(["x"], [imgs[0]])
    assert err.value.code == frt.FRT_ERR_INVALID and frt.lib.frt_matcher_num_rows(mm._h) == N + 2
    close(bare, old, pipe, det, rec)


@pytest.mark.parametrize("mode", [2, -2])
def test_pairing_modes_that_hold_run_dev_calls_change_nothing(frt, synth, blobs, photos, mode):
    """frt_pipeline_set_pairing 2 (always pairs) and -2 (adaptive for run_dev calls too) park a chunk of at most half of max_frames photos
    until a partner comes; the image route flushes behind every chunk, so 10 photos (chunks 4 + 4 + 2) and 2 photos give the answers of
    pairing off, bit for bit, and leave nothing pending that points into the staging of the next call."""
    imgs = photos["imgs"]
    N = 400
    det, rec, pipe = make_pipeline(frt, blobs, gallery=synth.make_gallery(N))
    mm = rec.matmul
    mm.galleryReserve(N + 16)
    calls = [imgs, [imgs[2], imgs[3]], [imgs[5], imgs[0]], imgs[:6]]  # (consecutive calls land in the same staging sets with other photos)

    def answers():
        out = []
        for batch in calls:
            out.append(pipe.runImages(batch, want_crops=True))
            status, first, emb, faces = pipe.enrolImages(["n%d" % i for i in range(len(batch))], batch)
            out.append((status, np.int32(first), emb, faces))
            rows = int(frt.lib.frt_matcher_num_rows(mm._h))
            assert rows == N + int((status == OK).sum()) == rec.classCount
            if rows > N:
                mm.galleryRemove(list(range(N, rows)))
            rec.classNames = list(rec.classNames)[:N]
            rec.classCount = N
        return out

    want = answers()
    assert want[1][0].tolist() == photos["status"].tolist() and want[3][0].tolist() == [OK, MANY]
    pipe.set_pairing(mode)
    for rounds in range(2):
        got = answers()
        for ci, (g, w) in enumerate(zip(got, want)):
            for x, y in zip(g, w):
                assert np.array_equal(x, y), (mode, rounds, ci)
    pipe.sync()
    close(pipe, det, rec)


def test_cpp_shell_agrees_with_the_python_binding(frt, synth, blobs, photos, tmp_path):
    """tests/cpp/photos_demo.cpp: ArcFaceIR50::enrolImages on the same bytes as Pipeline.enrolImages (one photo as a row-strided cv::Mat)."""
    imgs, ostatus = list(photos["imgs"]), photos["status"]
    wide = np.zeros((240, 330, 3), np.uint8)
    wide[:, :320] = imgs[2]
    imgs[2] = wide[:, :320]  # the same pixels behind a padded stride
    dpath, _ = blobs("det")
    rpath, _ = blobs("ir")
    exe = str(tmp_path / "photos_demo")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "photos_demo.cpp"), "-o", exe, os.path.join(PKG, "libfrt.so"), "-Wl,-rpath," + PKG,
                           "-Wl,-rpath,/opt/rocm/lib"])
    N = 400
    gal = synth.make_gallery(N)
    names = ["u%d" % (i % 100) for i in range(N)]
    new_names = ["p%d" % i for i in range(10)]
    det, rec, pipe = make_pipeline(frt, blobs, gallery=gal, names=names)
    status, first, emb, _ = pipe.enrolImages(new_names, imgs)
    close(pipe, det, rec)
    assert np.array_equal(status, ostatus) and first == N
    blob = [np.int32(len(imgs)).tobytes()]
    for f in imgs:  # rows, cols, row stride, then the rows with their padding
        padded = np.zeros((f.shape[0], f.strides[0]), np.uint8)
        padded[:, :f.shape[1] * 3] = f.reshape(f.shape[0], -1)
        blob.append(np.array([f.shape[0], f.shape[1], f.strides[0]], np.int32).tobytes())
        blob.append(padded.tobytes())
    (tmp_path / "photos.bin").write_bytes(b"".join(blob))
    (tmp_path / "gal.bin").write_bytes(gal.tobytes())
    (tmp_path / "names.txt").write_text("".join(n + "\n" for n in names))
    (tmp_path / "enrol.txt").write_text("".join(n + "\n" for n in new_names))
    out = subprocess.run([exe, dpath, rpath, str(tmp_path / "photos.bin"), str(tmp_path / "gal.bin"), str(N), str(tmp_path / "names.txt"),
                          str(tmp_path / "enrol.txt"), str(W), str(H), str(B), str(K), str(tmp_path / "embeds.bin")], capture_output=True, text=True,
                         timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = [l.split() for l in out.stdout.splitlines()]
    assert [int(l[2]) for l in lines if l[0] == "status"] == status.tolist()
    assert [l[1:] for l in lines if l[0] == "enrolled"] == [[str(len(emb)), str(N + len(emb))]]
    rows = [l for l in lines if l[0] == "row"]
    assert [int(l[2]) for l in rows] == list(range(N, N + len(emb))) and all(float(l[3]) > 0.999 for l in rows)
    got = np.fromfile(str(tmp_path / "embeds.bin"), np.float32).reshape(-1, 512)
    assert np.array_equal(got, emb)
