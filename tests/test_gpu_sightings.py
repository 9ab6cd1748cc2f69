"""The sighting book on the device (kernels_sightings.hip behind frt_sightings_* and frt_pipeline_run_sighted) against its numpy restatement
(tests/sightings_ref.py): after every step the open entries of every stream, and every drained record and payload row, are compared by
bytes.  The tracker under the book is fed through its host form; its integer answers are compared with track_ref's on the way, its float32
templates are handed to both books."""
import numpy as np
import pytest

import sightings_cases as sc
import sightings_ref as sr
import track_ref as tk

pytestmark = pytest.mark.gpu


def same(a, b, what):
    if a is None or b is None:
        assert a is None and b is None, what
        return
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), what


def same_open(dev, ref, streams, what):
    for s in streams:
        got, want = dev.open(s), ref.open(s)
        for g, w, part in zip(got, want, ("records", "best embeddings", "templates", "crops")):
            same(g, w, "%s: open entries of stream %d, %s" % (what, s, part))


def same_drain(dev, ref, max_out, what):
    got, want = dev.drain(max_out), ref.drain(max_out)
    for g, w, part in zip(got[:4], want[:4], ("records", "best embeddings", "templates", "crops")):
        same(g, w, "%s: drained %s" % (what, part))
    assert got[4] == want[4], (what, got[4], want[4])
    return got


class Rig:
    """the library's tracker and book beside the restated pair"""

    def __init__(self, frt, capacity, rank=0, min_hits=1, keep_crops=True, max_missed=1, track_min_hits=2, shape=sc.SHAPE):
        self.shape = shape
        self.ref = sc.RefRig(capacity, rank, min_hits, keep_crops, max_missed, track_min_hits, shape)
        self.tracker = frt.Tracker(shape["n_streams"], shape["max_tracks"], shape["max_faces"], shape["dim"], 0.3, max_missed, track_min_hits)
        self.book = frt.Sightings(self.tracker, capacity, rank, min_hits, keep_crops)
        self.streams = range(shape["n_streams"])

    def update(self, res, emb, qual, crops, ids, templates=True, what=""):
        trk, tpl = self.tracker.update(res, emb, ids)
        if not templates:
            tpl = None
        want = self.ref.update(res, emb, qual, crops, ids, templates=tpl)
        same(trk, want, what + ": the tracker's records")
        self.book.update(res, trk, emb, qual, tpl, crops, ids)
        same_open(self.book, self.ref.book, self.streams, what)

    def close(self):
        self.tracker.close()      # (takes the book with it)


def play(frt, script, rig_kw, seed=0):
    rig = Rig(frt, **rig_kw)
    rng = np.random.default_rng(seed)
    for i, step in enumerate(script):
        what = "step %d %s" % (i, step[0])
        if step[0] == "update":
            ids = list(step[1])
            rig.update(*sc.arrays([step[1][s] for s in ids], rig.shape["max_faces"], rig.shape["dim"], rig.ref.book.keep_crops, rng), ids, what=what)
        elif step[0] == "close":
            rig.book.close(step[1])
            rig.ref.book.close(step[1])
            same_open(rig.book, rig.ref.book, rig.streams, what)
        elif step[0] == "drain":
            same_drain(rig.book, rig.ref.book, step[1], what)
        elif step[0] == "reset":
            rig.tracker.reset(step[1])
            rig.ref.tracker.reset(step[1])
    same_drain(rig.book, rig.ref.book, 64, "what is left")
    rig.close()


@pytest.mark.parametrize("name", sorted(sc.SCENES))
def test_scripted_scenes(frt, name):
    """the scenes of tests/test_sightings_ref.py - birth to expiry, REPLACED and reopened in one update, min_hits, overflow, the three ranks,
    flagged against unflagged, a tie, a NaN, close and go on - plus the sparse calls and close with and without the tracker's reset"""
    script, rig = sc.SCENES[name]
    play(frt, script, rig)


def random_call(rng, n_streams, max_faces, dim, keep_crops):
    """a random subset of the streams in random order; faces at five anchors that jitter, so that tracks live, coast, die and are replaced;
    random validity and quality records, the metrics from few values (ties) with a NaN now and then"""
    ids = list(rng.permutation(n_streams)[:rng.integers(1, n_streams + 1)])
    n = len(ids)
    res = np.zeros((n, max_faces), tk.RESULT_DTYPE)
    res["match_idx"] = -1
    qual = np.zeros((n, max_faces), sr.QUALITY_DTYPE)
    anchors = [(10, 10), (100, 100), (200, 10), (10, 200), (200, 200)]
    for f in range(n):
        for d, a in enumerate(rng.permutation(5)[:rng.integers(0, max_faces + 1)]):
            x, y = anchors[a][0] + rng.integers(-6, 7), anchors[a][1] + rng.integers(-6, 7)
            res[f, d] = (x, y, x + 40, y + 40, rng.choice([0.5, 0.75, 0.9]), f, -1, 0.0, rng.random() < 0.8)
            if rng.random() < 0.85:
                nan = np.float32("nan")
                qual[f, d] = (rng.integers(0, 1 << 20), rng.integers(0, 1 << 20), rng.integers(-99, 99), rng.integers(0, 99), rng.integers(0, 99),
                              rng.integers(38, 42), rng.integers(0, 1 << 40), rng.random() * 255, rng.random() * 100,
                              nan if rng.random() < 0.05 else rng.integers(0, 4), nan if rng.random() < 0.1 else rng.choice([0.25, 0.5, 0.75]),
                              rng.choice([0, 0, 2, 8]), 1)
    emb = rng.standard_normal((n, max_faces, dim)).astype(np.float32)
    crops = rng.integers(0, 256, (n, max_faces) + sr.CROP, dtype=np.uint8) if keep_crops else None
    return (res.reshape(-1), emb.reshape(-1, dim), qual.reshape(-1), crops.reshape((-1,) + sr.CROP) if keep_crops else None), ids


@pytest.mark.parametrize("keep_crops,templates,rank,min_hits", [(True, True, 0, 1), (False, False, 2, 2), (True, True, 1, 1)])
def test_random_soak(frt, keep_crops, templates, rank, min_hits):
    """40 random updates at capacity 5 with two sightings drained every third update: the ring wraps, overflows and discards many times"""
    rig = Rig(frt, capacity=5, rank=rank, min_hits=min_hits, keep_crops=keep_crops)
    rng = np.random.default_rng(100 + rank)
    n_drained = 0
    for i in range(40):
        args, ids = random_call(rng, keep_crops=keep_crops, **{k: sc.SHAPE[k] for k in ("n_streams", "max_faces", "dim")})
        rig.update(*args, ids, templates=templates, what="update %d" % i)
        if i % 3 == 2:
            n_drained += len(same_drain(rig.book, rig.ref.book, 2, "after update %d" % i)[0])
    rig.book.close(-1)
    rig.ref.book.close(-1)
    counters = same_drain(rig.book, rig.ref.book, 64, "the end")[4]
    assert n_drained > 10 and counters["overflowed"] > 0 and counters["closed"] > 20 and (min_hits == 1 or counters["discarded"] > 0), counters
    rig.close()


def test_queue_order_across_256_frames(frt):
    """256 streams x 64 tracks, every slot filled, then one empty update with max_missed 0 whose frames come in reversed stream order: 16 384
    tracks end in one launch, the first 16 000 of them - frames in call order, slots ascending - fill the queue and 384 are lost.  (The
    tracker's state is read back from the library here: 16 384 tracks are too many for the restated tracker.)"""
    S, T, D, CAP = 256, 64, 4, 16000
    tracker = frt.Tracker(S, T, T, D, 0.3, 0, 1)
    book = frt.Sightings(tracker, CAP, keep_crops=False)
    ref = sr.Book(S, T, T, D, CAP, keep_crops=False)
    rng = np.random.default_rng(5)
    res = np.zeros((S, T), tk.RESULT_DTYPE)
    gx, gy = np.meshgrid(np.arange(8) * 30, np.arange(8) * 30)
    res["x1"], res["y1"] = gx.reshape(-1), gy.reshape(-1)
    res["x2"], res["y2"], res["score"], res["match_idx"], res["valid"] = res["x1"] + 20, res["y1"] + 20, 0.9, -1, 1
    qual = np.zeros((S, T), sr.QUALITY_DTYPE)
    qual["present"], qual["sharpness"] = 1, rng.random((S, T))
    emb = rng.standard_normal((S * T, D)).astype(np.float32)
    empty = np.zeros(S * T, tk.RESULT_DTYPE)
    for call, (r, ids) in enumerate(((res.reshape(-1), list(range(S))), (empty, list(range(S))[::-1]))):
        trk, tpl = tracker.update(r, emb, ids)
        book.update(r, trk, emb, qual, tpl, None, ids)
        slots = np.stack([tracker.tracks(s)[0] for s in ids])
        assert (slots["live"] != 0).all() if call == 0 else not slots["live"].any()
        ref.update(slots, np.full(S, call), r, trk, emb, qual, tpl, None, ids)
    got = same_drain(book, ref, 20000, "16 384 closes")
    assert len(got[0]) == CAP and got[4] == dict(queued=CAP, overflowed=S * T - CAP, discarded=0, closed=S * T)
    assert got[0]["stream"][0] == S - 1 and (np.diff(got[0]["stream"]) <= 0).all()
    same_open(book, ref, (0, 100, S - 1), "after the closes")
    tracker.close()


@pytest.mark.parametrize("dim", [2048, 12])
def test_wide_and_odd_dimensions(frt, dim):
    """the payload copies reach the last float of a row and not one past it: two streams of one track each, whose rows are neighbours both
    among the open entries and in the queue"""
    shape = dict(n_streams=2, max_tracks=1, max_faces=1, dim=dim)
    rig = Rig(frt, capacity=2, max_missed=0, shape=shape)
    rng = np.random.default_rng(dim)
    frames = ([[sc.det(sc.A, 1.0)], [sc.det(sc.B, 5.0)]], [[sc.det(sc.A, 2.0)], [sc.det(sc.B, 4.0)]], [[], []])
    for i, f in enumerate(frames):
        rig.update(*sc.arrays(f, 1, dim, True, rng), [0, 1], what="update %d" % i)
    got = same_drain(rig.book, rig.ref.book, 1, "first")
    assert got[0]["best_tick"][0] == 1 and got[1][0, -1] != 0 and got[2][0, -1] != 0
    got = same_drain(rig.book, rig.ref.book, 1, "second")
    assert got[0]["best_tick"][0] == 0 and got[1][0, -1] != 0
    rig.close()


def test_update_dev_on_a_stream_of_its_own(frt):
    """the device form behind Tracker.updateDev, both queued on one side stream, from buffers in HBM: the sparse scene.  The open entries
    are read back before the test synchronises that stream: open (on the tracker's own stream) has to wait for what was queued"""
    import torch

    script, kw = sc.SCENES["sparse"]
    rig = Rig(frt, **kw)
    rng = np.random.default_rng(0)
    st = torch.cuda.Stream()
    MF, D = sc.SHAPE["max_faces"], sc.SHAPE["dim"]
    keep = []                                            # the buffers of every queued update stay alive until the end

    def dev(arr):
        keep.append(torch.from_numpy(np.ascontiguousarray(arr).view(np.uint8).reshape(-1).copy()).cuda())
        return keep[-1]

    for i, step in enumerate(script):
        what = "step %d %s" % (i, step[0])
        if step[0] == "update":
            ids = list(step[1])
            res, emb, qual, crops = sc.arrays([step[1][s] for s in ids], MF, D, True, rng)
            d_res, d_emb, d_qual, d_crops = dev(res), dev(emb), dev(qual), dev(crops)
            d_trk, d_tpl = dev(np.zeros(len(ids) * MF, frt.TRACK_DTYPE)), dev(np.zeros((len(ids) * MF, D), np.float32))
            torch.cuda.synchronize()                     # (the uploads ran on torch's stream)
            rig.tracker.updateDev(d_res.data_ptr(), d_emb.data_ptr(), len(ids), d_trk.data_ptr(), d_tpl.data_ptr(), ids, None, st.cuda_stream)
            rig.book.updateDev(d_res.data_ptr(), d_trk.data_ptr(), d_emb.data_ptr(), d_qual.data_ptr(), len(ids), d_tpl.data_ptr(), d_crops.data_ptr(), ids,
                               st.cuda_stream)
            got = [rig.book.open(s) for s in rig.streams]    # not synchronised by the test: open has to wait for the queued update itself
            st.synchronize()
            tpl = d_tpl.cpu().numpy().view(np.float32).reshape(-1, D)
            rig.ref.update(res, emb, qual, crops, ids, templates=tpl)
            for s, g in zip(rig.streams, got):
                for x, y, part in zip(g, rig.ref.book.open(s), ("records", "best embeddings", "templates", "crops")):
                    same(x, y, "%s: open entries of stream %d read while the update was queued, %s" % (what, s, part))
        elif step[0] == "close":
            rig.book.close(step[1])
            rig.ref.book.close(step[1])
        elif step[0] == "drain":
            same_drain(rig.book, rig.ref.book, step[1], what)
        elif step[0] == "reset":
            rig.tracker.reset(step[1])
            rig.ref.tracker.reset(step[1])
        same_open(rig.book, rig.ref.book, rig.streams, what)
    rig.close()


def test_pipeline_run_sighted(frt, synth, blobs):
    """Pipeline.runSighted over six calls of two streams - four of a drifting scene, two of blank frames in which the tracks expire - on the
    96 x 160 det + ir fixtures: the records and tracks are runTracked's of a second tracker, the quality records runQuality's, and the open
    entries and the drained sightings, crops included, are the restatement's run on those outputs"""
    H, W, MF, PER = 96, 160, 8, 2
    dpath, _ = blobs("det")
    rpath, _ = blobs("ir")
    det = frt.RetinaFace(dpath, W, H, (3, H, W), 4, MF, 0.4, 0.02)
    rec = frt.ArcFaceIR50(rpath, W, H, maxBatchSize=4, maxFacesPerScene=MF)
    first = synth.make_frames(PER, H, W)
    res0, emb0 = frt.Pipeline(det, rec, 4, match=False).run(first)
    rng = np.random.default_rng(31)
    g = rng.standard_normal((300, 512)).astype(np.float32)
    g /= np.linalg.norm(g, axis=1, keepdims=True)
    g[100], g[200] = emb0[0], emb0[MF]
    rec.setGallery(g)
    rec.initMatMul()
    pipe = frt.Pipeline(det, rec, 4)
    _, _, q0 = pipe.runQuality(first)
    opt = frt.QualityOptions(min_sharpness=float(np.median(q0["sharpness"][q0["present"] != 0])))   # flags about half the faces of call 0
    sighted, alone = frt.Tracker(PER, 16, MF, max_missed=1), frt.Tracker(PER, 16, MF, max_missed=1)
    book = frt.Sightings(sighted, 64)
    ref = sr.Book(PER, 16, MF, 512, 64)
    ids = [1, 0]
    for c in range(6):
        frames = np.roll(first, 2 * c, axis=2) if c < 4 else np.zeros_like(first)
        res, emb, trk, qual = pipe.runSighted(sighted, book, frames, opt, ids)
        want_res, want_emb, want_trk, want_tpl = pipe.runTracked(alone, frames, ids)
        same(res, want_res, "call %d records" % c), same(emb, want_emb, "call %d embeddings" % c), same(trk, want_trk, "call %d tracks" % c)
        q_res, _, want_qual, crops = pipe.runQuality(frames, opt, want_crops=True)
        same(res, q_res, "call %d records (runQuality)" % c), same(qual, want_qual, "call %d quality" % c)
        state = [sighted.tracks(s) for s in ids]
        ref.update(np.stack([s[0] for s in state]), [s[1]["tick"] - 1 for s in state], res, trk, emb, qual, want_tpl, crops, ids)
        same_open(book, ref, range(PER), "call %d" % c)
        if c == 0:
            assert (qual["flags"] != 0).any() and (qual["present"] != 0).sum() >= 4
    got = same_drain(book, ref, 64, "the tracks that ended")
    book.close(-1)
    ref.close(-1)
    rest = same_drain(book, ref, 64, "the tracks that were closed")
    ended = np.concatenate([got[0], rest[0]])
    assert len(ended) >= 4 and (ended["best_tick"] >= 0).any() and (ended["match_idx"] >= 0).any() and (got[3].any() or rest[3].any())
    assert (rest[0]["reason"] == sr.CLOSED).all() and (got[0]["reason"] != sr.CLOSED).all()
    with pytest.raises(frt.FrtError) as ei:
        pipe.runSighted(alone, book, first, opt, ids)            # the book belongs to `sighted`
    assert ei.value.code == frt.FRT_ERR_INVALID
    for o in (sighted, alone, pipe, rec, det):
        o.close()
