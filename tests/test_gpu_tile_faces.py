"""Recognising a large photo by tiles on the GPU (frt_select_faces, frt_pipeline_run_photo_tiled and their shells): everything is compared
for exact equality - ints, score bits, crop bytes, embedding bits, match indices and similarity bits.  The reference is never the code under
test: it is tests/tile_faces_ref.py (numpy) around the EXISTING findFaceTiled / forward / forwardAligned / MatMul.top1.

Detector: the synthetic `det` / `det_ldm` blob, frame = input = 96 x 160, max_batch 4, max_faces 8, nms 0.4, bbox threshold 0.02; recogniser:
the synthetic `ir` blob, maxBatchSize 4."""
import ctypes
import os
import subprocess
import threading

import numpy as np
import pytest

import tile_faces_ref as tf
from conftest import ROOT

pytestmark = pytest.mark.gpu
T_R, T_C, BATCH, SLOTS, NMS, BBOX, REC_BATCH = 96, 160, 4, 8, 0.4, 0.02, 4
PKG = os.path.join(ROOT, "face-recognition-cpp-tensorrt_amd")
KEEP_ALL = dict(overlap=32, overview=True, metric=0, drop_cut=False, threshold=0.99)  # test_landmarks_follow_their_boxes' settings
GALLERY_ROWS, ROW_A, ROW_B = 777, 100, 500


# ------------------------------------------------------------------------------------------------------------------- 1. select alone
BOXES = {}


def random_list(n):
    """n boxes with sides 1 .. 60 (extents 0 .. 59), sources and landmarks; shared by the cases of one size"""
    if n not in BOXES:
        rng = np.random.Generator(np.random.PCG64(1000 + n))
        b = np.zeros(n, tf.BBOX_DTYPE)
        b["x1"], b["y1"] = rng.integers(0, 2000, n), rng.integers(0, 3000, n)
        b["x2"] = b["x1"] + rng.integers(1, 61, n)
        b["y2"] = b["y1"] + rng.integers(1, 61, n)
        b["score"] = np.sort(rng.random(n, np.float32))[::-1]
        BOXES[n] = (b, rng.permutation(16384)[:n].astype(np.int32), rng.standard_normal((n, 5, 2)).astype(np.float32) * 100)
    return BOXES[n]


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 1025, 16384])
def test_select_alone(frt, n):
    """below, at and above a wave and a step of the workgroup, several steps, the most there may be: whole arrays, everything behind the count"""
    b, src, ldm = random_list(n)
    kept = set()
    for min_face in (0, 1, 20, 61):
        for max_batch in (1, 4, 128):
            for with_extras in (True, False):
                want = tf.select(b, src if with_extras else None, ldm if with_extras else None, min_face, max_batch)
                got = frt.selectFaces(b, src if with_extras else None, ldm if with_extras else None, min_face, max_batch)
                tf.same_selection(got, want)
                kept.add((min_face, want["n_kept"]))
    if n >= 63:
        counts = dict(kept)
        assert counts[0] == n and 0 < counts[20] < counts[1] <= n and counts[61] == 0, counts


def test_select_keeps_a_zero_extent_box_at_min_face_zero_and_leaves_nothing_stale(frt):
    b = np.array([(5, 5, 5, 40, .9), (5, 5, 25, 5, .8), (7, 7, 7, 7, .7), (1, 1, 30, 30, .6)], tf.BBOX_DTYPE)
    got = frt.selectFaces(b, min_face=0, max_batch=4)
    tf.same_selection(got, tf.select(b, min_face=0, max_batch=4))
    assert got["n_kept"] == 4 and got["boxes"].tobytes() == b.tobytes()
    assert frt.selectFaces(b, min_face=1, max_batch=4)["keep_pos"].tolist() == [3, -1, -1, -1]
    # a small call after the largest one
    big, bsrc, bldm = random_list(16384)
    tf.same_selection(frt.selectFaces(big, bsrc, bldm, 20, 128), tf.select(big, bsrc, bldm, 20, 128))
    small, ssrc, sldm = random_list(65)
    for min_face in (20, 61):
        tf.same_selection(frt.selectFaces(small, ssrc, sldm, min_face, 4), tf.select(small, ssrc, sldm, min_face, 4))


# ------------------------------------------------------------------------------------------------------------------- objects
def make_det(frt, blobs, kind="det"):
    path, _ = blobs(kind)
    return frt.RetinaFace(path, T_C, T_R, (3, T_R, T_C), BATCH, SLOTS, NMS, BBOX)


def make_rec(frt, blobs, gallery=None, names=None):
    path, _ = blobs("ir")
    rec = frt.ArcFaceIR50(path, T_C, T_R, maxBatchSize=REC_BATCH, maxFacesPerScene=SLOTS)
    if gallery is not None:
        rec.setGallery(gallery, names)
        rec.initMatMul()
    return rec


def close(*objs):
    for o in objs:
        o.close()


@pytest.fixture(scope="module")
def photos(synth):
    return {shape: synth.make_frames(1, *shape)[0] for shape in ((200, 410), (60, 300), (50, 70))}


@pytest.fixture(scope="module")
def gallery(frt, synth, blobs, photos):
    """777 synthetic rows, two of them replaced by two of the reference's own embeddings of the 200 x 410 photo (faces 0 and 5)"""
    det, rec = make_det(frt, blobs), make_rec(frt, blobs)
    ref = tf.loop(frt, det, rec, photos[(200, 410)], 0, 96, **KEEP_ALL)
    close(det, rec)
    assert ref["n"] >= 9 and ref["results"]["valid"][:ref["n"]].all()
    g = synth.make_gallery(GALLERY_ROWS)
    g[ROW_A], g[ROW_B] = ref["embeds"][0], ref["embeds"][5]
    return g


@pytest.fixture(scope="module")
def objs(frt, blobs, gallery):
    det, rec = make_det(frt, blobs), make_rec(frt, blobs, gallery)
    pipe = frt.Pipeline(det, rec, BATCH)
    yield det, rec, pipe
    close(pipe, det, rec)


@pytest.fixture(scope="module")
def objs_ldm(frt, blobs, gallery):
    det, rec = make_det(frt, blobs, "det_ldm"), make_rec(frt, blobs, gallery)
    pipe = frt.Pipeline(det, rec, BATCH)
    pipe.set_align(True)
    yield det, rec, pipe
    close(pipe, det, rec)


def run_full(frt, pipe, photo, min_face=0, max_out=256, landmarks=False, overlap=None, overview=True, metric=1, drop_cut=True, threshold=None,
             defaults=False):
    """frt_pipeline_run_photo_tiled with every output asked for -> the WHOLE arrays, as tile_faces_ref.loop returns them"""
    photo = np.ascontiguousarray(photo, np.uint8)
    opt = frt.tileOptions(T_R, T_C, overlap, overview, metric, drop_cut, threshold)
    res = np.full(max_out, 7, frt.RESULT_DTYPE)
    src = np.full(max_out, 7, np.int32)
    ldm = np.full((max_out, 5, 2), 7, np.float32) if landmarks else None
    emb = np.zeros((max_out, 512), np.float32)
    crops = np.zeros((max_out, 112, 112, 3), np.uint8)
    n = ctypes.c_int(-1)
    p = lambda a: ctypes.c_void_p(a.ctypes.data) if a is not None else None
    rc = frt.lib.frt_pipeline_run_photo_tiled(pipe._h, p(photo), photo.shape[0], photo.shape[1], photo.strides[0],
                                              None if defaults else ctypes.addressof(opt), min_face, max_out, p(res), p(ldm), p(emb), p(crops), p(src),
                                              ctypes.byref(n))
    assert rc == frt.FRT_OK, frt.lib.frt_last_error()
    return dict(results=res, src=src, landmarks=ldm, embeds=emb[:n.value], crops=crops[:n.value], n=n.value)


def same(got, want, what=""):
    assert got["n"] == want["n"], (what, got["n"], want["n"])
    assert got["src"].tobytes() == want["src"].tobytes(), what
    for c in tf.RESULT_DTYPE.names:
        assert got["results"][c].tobytes() == want["results"][c].tobytes(), (what, c, got["results"][c][:got["n"]], want["results"][c][:want["n"]])
    assert got["crops"].tobytes() == want["crops"].tobytes(), what
    assert got["embeds"].tobytes() == want["embeds"].tobytes(), what
    if want["landmarks"] is not None and got["landmarks"] is not None:
        assert got["landmarks"].tobytes() == want["landmarks"].tobytes(), what


# ------------------------------------------------------------------------------------------------------------------- 2. end to end
def test_end_to_end_equals_the_loop(frt, objs, photos):
    det, rec, pipe = objs
    photo = photos[(200, 410)]
    want = tf.loop(frt, det, rec, photo, 0, 96, **KEEP_ALL)
    max_out = 96
    if want["n"] % REC_BATCH == 0:  # the last pass must be a partial one
        max_out = want["n"] - 1
        want = tf.loop(frt, det, rec, photo, 0, max_out, **KEEP_ALL)
    n = want["n"]
    kinds = want["src"][:n] // SLOTS == 10 - 1  # the plan has 10 tiles, the overview last
    print("reference: kept %d of %d (passes of %d), from the overview %d, from grid tiles %d" % (n, len(want["merged"]), REC_BATCH, kinds.sum(), (~kinds).sum()))
    assert n >= 9 and n % REC_BATCH != 0 and kinds.any() and (~kinds).any()  # asserted ON THE REFERENCE
    r = want["results"]
    assert r["match_idx"][0] == ROW_A and r["match_idx"][5] == ROW_B and r["match_sim"][0] > 0.999 and r["match_sim"][5] > 0.999
    assert r["valid"][:n].all() and (r["match_idx"][:n] >= 0).all() and (r["frame"] == 0).all()
    got = run_full(frt, pipe, photo, 0, max_out, **KEEP_ALL)
    same(got, want, "min_face 0")
    # the Python surface: trimmed to the count
    res, emb, crops, src = pipe.runTiled(photo, min_face=0, max_out=max_out, want_crops=True, sources=True, **KEEP_ALL)
    assert res.tobytes() == r[:n].tobytes() and emb.tobytes() == want["embeds"].tobytes() and crops.tobytes() == want["crops"].tobytes()
    assert np.array_equal(src, want["src"][:n])
    res, emb = pipe.runTiled(photo, min_face=0, max_out=max_out, want_embeds=False, **KEEP_ALL)
    assert emb is None and res.tobytes() == r[:n].tobytes()

    # the gate at the median kept side
    side = np.minimum(r["x2"][:n] - r["x1"][:n], r["y2"][:n] - r["y1"][:n])
    min_face = int(np.median(side))
    gated = tf.loop(frt, det, rec, photo, min_face, max_out, **KEEP_ALL)
    print("reference: min_face %d keeps %d of %d" % (min_face, gated["n"], n))
    assert 1 <= gated["n"] < n  # on the reference: the gate drops at least one face and keeps at least one
    same(run_full(frt, pipe, photo, min_face, max_out, **KEEP_ALL), gated, "min_face %d" % min_face)

    # the defaults (options NULL)
    dflt = tf.loop(frt, det, rec, photo, 0, 96)
    assert dflt["n"] >= 1
    same(run_full(frt, pipe, photo, 0, 96, defaults=True), dflt, "defaults")
    res, emb = pipe.runTiled(photo, max_out=96)
    assert res.tobytes() == dflt["results"][:dflt["n"]].tobytes() and emb.tobytes() == dflt["embeds"].tobytes()


def test_end_to_end_without_a_gallery(frt, blobs, photos, objs):
    det, rec, _ = objs
    photo = photos[(200, 410)]
    want = tf.loop(frt, det, rec, photo, 0, 96, match=False, **KEEP_ALL)
    assert want["n"] >= 9 and (want["results"]["match_idx"] == -1).all() and (want["results"]["match_sim"] == 0).all()
    bare = frt.Pipeline(det, rec, BATCH, match=False)
    same(run_full(frt, bare, photo, 0, 96, **KEEP_ALL), want, "no matcher")
    bare.close()
    # a matcher without rows
    rec2 = make_rec(frt, blobs)
    pipe2 = frt.Pipeline(det, rec2, BATCH)
    same(run_full(frt, pipe2, photo, 0, 96, **KEEP_ALL), want, "empty gallery")
    close(pipe2, rec2)


# ------------------------------------------------------------------------------------------------------------------- 3. padded photo, one tile
def test_padded_photo_and_one_tile(frt, synth, objs, photos):
    det, rec, pipe = objs
    photo = photos[(60, 300)]
    for kw in (dict(overlap=32, overview=True, metric=1, drop_cut=True), dict(overlap=32, overview=False, metric=0, drop_cut=False, threshold=0.25)):
        want = tf.loop(frt, det, rec, photo, 0, 64, **kw)
        assert want["n"] >= 1
        same(run_full(frt, pipe, photo, 0, 64, **kw), want, str(kw))
    # max_out caps the merged list BEFORE the gate
    full = tf.loop(frt, det, rec, photo, 0, 64, overlap=32, overview=True, metric=0, drop_cut=False)
    assert full["n"] > 3
    capped = tf.loop(frt, det, rec, photo, 0, 3, overlap=32, overview=True, metric=0, drop_cut=False)
    assert capped["n"] == 3
    same(run_full(frt, pipe, photo, 0, 3, overlap=32, overview=True, metric=0, drop_cut=False), capped, "max_out 3")
    # one tile: the records of Pipeline.run on that frame
    frame = synth.make_frames(2, T_R, T_C)[1]
    res, emb = pipe.run(frame[None])
    used = res["score"] > 0
    k = int(used.sum())
    assert k >= 1 and used[:k].all()
    got, gemb = pipe.runTiled(frame, overlap=32, overview=False, metric=0, drop_cut=False, min_face=0, max_out=SLOTS)
    assert len(got) == k
    for c in ("x1", "y1", "x2", "y2", "score", "frame", "valid", "match_idx", "match_sim"):
        assert got[c].tobytes() == res[c][:k].tobytes(), c
    assert gemb.tobytes() == emb[:k].tobytes()


# ------------------------------------------------------------------------------------------------------------------- 4. modes
def test_align_mode(frt, objs, objs_ldm, photos):
    det, rec, pipe = objs_ldm
    photo = photos[(200, 410)]
    want = tf.loop(frt, det, rec, photo, 0, 96, align=True, **KEEP_ALL)
    assert want["n"] >= 9 and want["results"]["valid"][:want["n"]].all()
    got = run_full(frt, pipe, photo, 0, 96, landmarks=True, **KEEP_ALL)
    same(got, want, "align")  # crops: forwardAligned's; landmarks: findFaceTiled(landmarks=True)'s, zeros behind the count
    plain = tf.loop(frt, det, rec, photo, 0, 96, align=False, **KEEP_ALL)
    assert plain["crops"].tobytes() != want["crops"].tobytes()
    # landmarks without the align switch: the boxes' crops, the same landmarks
    pipe.set_align(False)
    got = run_full(frt, pipe, photo, 0, 96, landmarks=True, **KEEP_ALL)
    same(got, plain, "landmarks only")
    assert got["landmarks"].tobytes() == want["landmarks"].tobytes()
    pipe.set_align(True)
    # the trimmed blob has no LandmarkHead
    tdet, trec, tpipe = objs
    with pytest.raises(frt.FrtError) as e:
        tpipe.runTiled(photo, landmarks=True)
    assert e.value.code == frt.FRT_ERR_FORMAT
    with pytest.raises(frt.FrtError) as e:
        tpipe.set_align(True)
    assert e.value.code == frt.FRT_ERR_FORMAT


@pytest.mark.parametrize("mode", ["flip", "fp32"])
def test_recogniser_modes(frt, objs, photos, mode):
    det, rec, pipe = objs
    photo = photos[(200, 410)]
    plain = tf.loop(frt, det, rec, photo, 0, 96, match=False, **KEEP_ALL)
    switch = rec.setFlip if mode == "flip" else rec.setPrecision
    switch(True)
    try:
        want = tf.loop(frt, det, rec, photo, 0, 96, **KEEP_ALL)
        assert want["n"] == plain["n"] and want["embeds"].tobytes() != plain["embeds"].tobytes()
        same(run_full(frt, pipe, photo, 0, 96, **KEEP_ALL), want, mode)
    finally:
        switch(False)
    same(run_full(frt, pipe, photo, 0, 96, **KEEP_ALL), tf.loop(frt, det, rec, photo, 0, 96, **KEEP_ALL), "back")


# ------------------------------------------------------------------------------------------------------------------- 5. state
def test_state_across_calls(frt, synth, blobs, gallery, objs, photos):
    det, rec, pipe = objs
    first = run_full(frt, pipe, photos[(200, 410)], 0, 96, **KEEP_ALL)
    same(first, tf.loop(frt, det, rec, photos[(200, 410)], 0, 96, **KEEP_ALL), "first")
    assert run_full(frt, pipe, photos[(50, 70)], 0, 96, **KEEP_ALL)["n"] >= 0
    same(run_full(frt, pipe, photos[(60, 300)], 10, 16, overlap=32), tf.loop(frt, det, rec, photos[(60, 300)], 10, 16, overlap=32), "60 x 300")
    same(run_full(frt, pipe, photos[(200, 410)], 0, 96, **KEEP_ALL), first, "again")
    # a capacity error between calls changes nothing: overlap T - 1 on this photo is far more than 4096 tiles
    res = np.full(4, 7, frt.RESULT_DTYPE)
    n = ctypes.c_int(-1)
    opt = frt.TileOptions(T_R - 1, T_C - 1, 1, 1, 1, -1.0)
    big = photos[(200, 410)]
    assert frt.lib.frt_pipeline_run_photo_tiled(pipe._h, big.ctypes.data, 200, 410, 1230, ctypes.addressof(opt), 0, 4, res.ctypes.data, None, None, None,
                                                None, ctypes.byref(n)) == frt.FRT_ERR_CAPACITY
    opt = frt.TileOptions(T_R, 0, 1, 1, 1, -1.0)
    assert frt.lib.frt_pipeline_run_photo_tiled(pipe._h, big.ctypes.data, 200, 410, 1230, ctypes.addressof(opt), 0, 4, res.ctypes.data, None, None, None,
                                                None, ctypes.byref(n)) == frt.FRT_ERR_INVALID
    assert n.value == -1 and res.tobytes() == np.full(4, 7, frt.RESULT_DTYPE).tobytes()
    # afterwards the plain routes answer as a fresh set of objects
    frames = synth.make_frames(BATCH, T_R, T_C)
    fdet, frec = make_det(frt, blobs), make_rec(frt, blobs, gallery)
    fpipe = frt.Pipeline(fdet, frec, BATCH)
    want_run = fpipe.run(frames)
    want_tiled = fdet.findFaceTiled(photos[(200, 410)], sources=True)
    want_one = fdet.findFace(frames[0])
    close(fpipe, fdet, frec)
    got_run = pipe.run(frames)
    assert got_run[0].tobytes() == want_run[0].tobytes() and got_run[1].tobytes() == want_run[1].tobytes()
    got_tiled = det.findFaceTiled(photos[(200, 410)], sources=True)
    assert got_tiled[0].tobytes() == want_tiled[0].tobytes() and np.array_equal(got_tiled[1], want_tiled[1])
    assert det.findFace(frames[0]).tobytes() == want_one.tobytes()


# ------------------------------------------------------------------------------------------------------------------- 6. beside other callers
def test_beside_submits_of_another_thread(frt, synth, objs, photos):
    det, rec, pipe = objs
    frames = synth.make_frames(BATCH, T_R, T_C, start=20)
    want_frames = tuple(a.copy() for a in pipe.run(frames))
    calls = [(photos[(200, 410)], 0, 96, KEEP_ALL), (photos[(60, 300)], 0, 32, dict(overlap=32)), (photos[(200, 410)], 12, 96, KEEP_ALL)]
    want = [run_full(frt, pipe, ph, mf, mo, **kw) for ph, mf, mo, kw in calls]
    got_frames, errors = [], []
    started = threading.Event()
    CALLS = 200  # the helper is bound by a call count, not by time

    def worker():
        try:
            for _ in range(CALLS):
                r = np.zeros(BATCH * SLOTS, frt.RESULT_DTYPE)
                e = np.zeros((BATCH * SLOTS, 512), np.float32)
                pipe.wait(pipe.submit(frames, r, e))
                got_frames.append((r, e))
                started.set()
        except Exception as ex:  # noqa: BLE001
            errors.append(ex)
        started.set()

    t = threading.Thread(target=worker)
    t.start()
    assert started.wait(60)
    got = [run_full(frt, pipe, ph, mf, mo, **kw) for ph, mf, mo, kw in calls]
    t.join()
    assert not errors, errors
    assert len(got_frames) == CALLS
    for g, w in zip(got, want):
        same(g, w, "beside submits")
    for r, e in got_frames:
        assert r.tobytes() == want_frames[0].tobytes() and e.tobytes() == want_frames[1].tobytes()


# ------------------------------------------------------------------------------------------------------------------- 7. the C++ shell
def test_cpp_shell_agrees_with_the_python_binding(frt, synth, blobs, gallery, objs, photos, tmp_path):
    """tests/cpp/tiled_faces_demo.cpp: ArcFaceIR50::recognizeTiled on the same bytes (behind a padded row stride) as Pipeline.runTiled"""
    det, rec, pipe = objs
    dpath, _ = blobs("det")
    rpath, _ = blobs("ir")
    exe = str(tmp_path / "tiled_faces_demo")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "tiled_faces_demo.cpp"), "-o", exe, os.path.join(PKG, "libfrt.so"), "-Wl,-rpath," + PKG,
                           "-Wl,-rpath,/opt/rocm/lib"])
    photo = photos[(200, 410)]
    wide = np.zeros((200, 410 * 3 + 7), np.uint8)
    wide[:, :410 * 3] = photo.reshape(200, -1)
    (tmp_path / "photo.bin").write_bytes(wide.tobytes())
    (tmp_path / "gal.bin").write_bytes(gallery.tobytes())
    names = ["u%d" % i for i in range(GALLERY_ROWS)]
    (tmp_path / "names.txt").write_text("".join(n + "\n" for n in names))
    min_face, max_out = 12, 64
    res, _, src = pipe.runTiled(photo, min_face=min_face, max_out=max_out, sources=True, **KEEP_ALL)
    n_default = len(pipe.runTiled(photo)[0])
    assert len(res) > 3
    out = subprocess.run([exe, dpath, rpath, str(tmp_path / "photo.bin"), "200", "410", str(wide.shape[1]), str(T_C), str(T_R), str(BATCH), str(SLOTS),
                          str(REC_BATCH), str(tmp_path / "gal.bin"), str(GALLERY_ROWS), str(tmp_path / "names.txt"), "32", "1", "0", "0", "0.99",
                          str(min_face), str(max_out)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = [l.split() for l in out.stdout.splitlines()]
    got = [l[1:] for l in lines if l[0] == "face"]
    want = [[str(int(r["x1"])), str(int(r["y1"])), str(int(r["x2"])), str(int(r["y2"])), str(int(np.float32(r["score"]).view(np.uint32))), str(int(s)),
             str(int(r["valid"])), names[r["match_idx"]] if r["match_idx"] >= 0 else "-", str(int(np.float32(r["match_sim"]).view(np.uint32)))]
            for r, s in zip(res, src)]
    assert got == want
    assert [l[1] for l in lines if l[0] == "default"] == [str(n_default)]
