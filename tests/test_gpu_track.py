"""The face tracker on the GPU (frt_tracker_*, frt_pipeline_run_tracked and their Python shells) against tests/track_ref.py, the numpy
restatement: every update's records, the slots and the counters are compared for equality, the fp32 sums by their bits, the templates within
the bound derived below, the identities by bits against MatMul.top1 of the very template rows the update returned.  The reference is never
the code under test.  The tracker alone needs no detector or recogniser: its inputs are synthetic records and embeddings.

Template bound (check_templates).  The sums are exact (bit-equal to numpy's), so a template differs from the float64 sum / ||sum|| only by
the norm's reduction and the division.  With u = 2^-24: the squared norm is, per lane, a chain of m = 4 * ceil(dim / 256) fmas (one rounding
each) followed by the 6 additions of the wave's xor butterfly; all terms are >= 0, so n2' = n2 (1 + a), |a| <= (m + 6) u + O(u^2).
sqrtf and the fp32 division are correctly rounded: nrm' = sqrt(n2') (1 + b), t' = (s / nrm') (1 + c), |b|, |c| <= u.  Hence
|t' - t| <= ((m + 6) / 2 + 2) u |t| + O(u^2); the test allows 1.001 times the first-order term (the second-order ones are below 1e-5 of it)
plus 2^-149 for a component that is subnormal.  dim 512: 9 u; dim 1024: 13 u."""
import ctypes

import numpy as np
import pytest

import track_ref as tk

pytestmark = pytest.mark.gpu
U = 2.0 ** -24


def template_bound(dim):
    return 1.001 * ((4 * -(-dim // 256) + 6) / 2 + 2) * U


def frame(max_faces, *dets):
    """dets: (x1, y1, x2, y2[, score[, valid]]) -> RESULT_DTYPE [max_faces] as the pipeline writes them: unused slots zero but match_idx -1"""
    r = np.zeros(max_faces, tk.RESULT_DTYPE)
    r["match_idx"] = -1
    for i, d in enumerate(dets):
        d = tuple(d) + (0.9, 1)[len(d) - 4:]
        r[i] = (d[0], d[1], d[2], d[3], d[4], 0, -1, 0.0, d[5])
    return r


class Pair:
    """a device tracker and its restatement, fed the same calls"""

    def __init__(self, frt, n_streams, max_tracks, max_faces, dim, matcher=None, seed=0, **opt):
        self.frt, self.mm = frt, matcher
        self.dev = frt.Tracker(n_streams, max_tracks, max_faces, dim, **opt)
        self.ref = tk.Tracker(n_streams, max_tracks, max_faces, dim, **opt)
        self.rng = np.random.default_rng(seed)
        self.max_faces, self.dim, self.n_streams = max_faces, dim, n_streams

    def embeds(self, n_frames):
        e = self.rng.standard_normal((n_frames * self.max_faces, self.dim)).astype(np.float32)
        return e / np.linalg.norm(e, axis=1, keepdims=True).astype(np.float32)

    def update(self, results, embeds=None, ids=None):
        """one update on both; the records must be equal, the templates within the bound -> (records, templates) of the device"""
        results = np.concatenate(results) if isinstance(results, (list, tuple)) else results
        n = len(results) // self.max_faces
        embeds = self.embeds(n) if embeds is None else embeds
        got, tpl = self.dev.update(results, embeds, ids, self.mm)
        want, want_tpl = self.ref.update(results, embeds, ids)
        if self.mm is not None and self.mm.m > 0:
            idx, sim = self.mm.top1(tpl.reshape(-1, self.dim))   # the matcher's own answer for the rows the update searched
            self.ref.apply_identity(want, ids, idx, sim)
        assert got.shape == want.shape and got.tobytes() == want.tobytes(), (got, want)
        check_templates(tpl, want_tpl, self.dim)
        return got, tpl

    def check_state(self):
        for s in range(self.n_streams):
            slots, cnt, sums = self.dev.tracks(s, want_sums=True)
            assert slots.tobytes() == self.ref.slots[s].tobytes(), (s, slots, self.ref.slots[s])
            assert [cnt["next_id"], cnt["tick"], cnt["dropped"]] == self.ref.counters(s).tolist(), s
            assert sums.tobytes() == self.ref.sums[s].tobytes(), s      # fl(fl(decay * sum) + e): the bits of numpy float32

    def close(self):
        self.dev.close()


def check_templates(got, want64, dim):
    assert got.dtype == np.float32 and got.shape == want64.shape
    err = np.abs(got.astype(np.float64) - want64)
    assert (err <= template_bound(dim) * np.abs(want64) + 2.0 ** -149).all(), float((err / np.maximum(np.abs(want64), 1e-300)).max() / U)
    assert not got[want64 == 0].any()


A, B, C = (10, 10, 50, 50), (100, 100, 140, 140), (200, 200, 240, 240)
SCRIPT = dict(n_streams=3, max_tracks=4, max_faces=3, dim=512)


@pytest.mark.parametrize("decay", [1.0, 0.75])
def test_scripted_sequences(frt, decay):
    """steady motion, a tie of two tracks, detection-order priority, coasts of max_missed and max_missed + 1 updates, more detections than
    slots, an empty-ROI detection, a stream left out, a permuted batch, reset of one stream and of all"""
    def fr(*d):
        return frame(3, *d)

    # ---- steady motion in stream 0, two faces; stream 1 has one face; stream 2 stays out of every call but one
    p = Pair(frt, seed=1, decay=decay, max_missed=2, **SCRIPT)
    for k in range(5):
        got, _ = p.update([fr((10 + 2 * k, 10 + k, 50 + 2 * k, 50 + k), (100, 100 - 3 * k, 140, 140 - 3 * k)), fr(B)], ids=[0, 1])
        assert got[0]["track_id"].tolist() == [0, 1, -1] and got[1]["track_id"].tolist() == [0, -1, -1] and got[0, 0]["hits"] == k + 1
    assert got[0, 0]["confirmed"] == 1 and got[0, 0]["n_embeds"] == 5
    p.check_state()
    assert p.dev.tracks(2)[1] == dict(next_id=0, tick=0, dropped=0)                        # the stream left out of every call: untouched
    # ---- an empty-ROI detection: the box follows, n_embeds does not
    got, _ = p.update([fr((20, 15, 60, 55, 0.9, 0))], ids=[0])
    assert got[0, 0]["track_id"] == 0 and got[0, 0]["hits"] == 6 and got[0, 0]["n_embeds"] == 5
    # ---- a coast of exactly max_missed updates keeps the id; stream 1 is left out meanwhile and does not age
    for _ in range(2):
        p.update([fr()], ids=[0])
    got, _ = p.update([fr((20, 15, 60, 55)), fr(B)], ids=[0, 1])
    assert got[0, 0]["track_id"] == 0 and got[0, 0]["age"] == 9 and got[1, 0]["track_id"] == 0 and got[1, 0]["age"] == 6
    # ---- a coast of max_missed + 1: a new id, born into the slot freed in the same update (track 1 of stream 0 went earlier)
    for _ in range(3):
        p.update([fr()], ids=[0])
    got, _ = p.update([fr((20, 15, 60, 55))], ids=[0])
    assert got[0, 0]["track_id"] == 2 and got[0, 0]["slot"] == 0 and got[0, 0]["age"] == 1
    p.check_state()
    # ---- the same frames in permuted batch order: the same per-stream state
    q = Pair(frt, seed=2, decay=decay, **SCRIPT)
    r = Pair(frt, seed=2, decay=decay, **SCRIPT)
    for k in range(3):
        frames = [fr((10 + k, 10, 50 + k, 50)), fr(B, A), fr(C)]
        e = q.embeds(3).reshape(3, 3, 512)
        q.update(frames, e.reshape(-1, 512), ids=[0, 1, 2])
        order = [2, 0, 1]
        r.update([frames[i] for i in order], e[order].reshape(-1, 512), ids=order)
    q.check_state(), r.check_state()
    for s in range(3):
        assert [a.tobytes() for a in q.dev.tracks(s, True)[::2]] == [a.tobytes() for a in r.dev.tracks(s, True)[::2]]
    # ---- reset of one stream (ids go on, tick and dropped start over), then of all
    q.dev.reset(1), q.ref.reset(1)
    q.check_state()
    got, _ = q.update([fr(B)], ids=[1])
    assert got[0, 0]["track_id"] == 2 and got[0, 0]["age"] == 1
    q.dev.reset(), q.ref.reset()
    q.check_state()
    assert q.dev.tracks(0)[1] == dict(next_id=1, tick=0, dropped=0)
    for x in (p, q, r):
        x.close()


def test_ties_priority_overflow_and_the_exact_threshold(frt):
    def fr(*d):
        return frame(3, *d)

    # ---- two tracks tie on one detection: the lowest slot takes it.  Tracks 0 and 1 are born apart, walk onto the same box, then one detection
    p = Pair(frt, seed=3, iou_threshold=0.1, **SCRIPT)
    p.update([fr((0, 0, 9, 9), (0, 12, 9, 21))], ids=[0])
    got, _ = p.update([fr((0, 0, 9, 9), (0, 6, 9, 15))], ids=[0])
    assert got[0]["slot"][:2].tolist() == [0, 1]
    got, _ = p.update([fr((0, 3, 9, 12, 0.9), (0, 3, 9, 12, 0.8))], ids=[0])          # symmetric between the tracks (0,0,9,9) and (0,6,9,15)
    assert got[0]["slot"][:2].tolist() == [0, 1]
    # ---- detection-order priority: the first detection takes the track although the second overlaps it more
    got, _ = p.update([fr((0, 1, 9, 10, 0.9), (0, 3, 9, 12, 0.8))], ids=[0])
    assert got[0]["slot"][:2].tolist() == [0, 1] and got[0]["hits"][:2].tolist() == [4, 4]
    p.check_state()
    # ---- more detections than free slots: the overflow is untracked and counted
    p2 = Pair(frt, 1, 2, 3, 512, seed=4)
    got, tpl = p2.update([fr(A, B, C)])
    assert got[0]["track_id"].tolist() == [0, 1, -1] and got[0]["slot"].tolist() == [0, 1, -1] and not tpl[0, 2].any()
    got, _ = p2.update([fr(C, A, B)])
    assert got[0]["track_id"].tolist() == [-1, 0, 1] and p2.dev.tracks(0)[1] == dict(next_id=2, tick=2, dropped=2)
    p2.check_state()
    # ---- the pair whose overlap is exactly 0.5
    for thr, same in ((0.5, True), (float(np.nextafter(np.float32(0.5), np.float32(1))), False)):
        p3 = Pair(frt, seed=5, iou_threshold=thr, **SCRIPT)
        p3.update([fr((0, 0, 9, 9))], ids=[2])
        got, _ = p3.update([fr((0, 0, 9, 4))], ids=[2])
        assert (got[0, 0]["track_id"] == 0) == same and (got[0, 0]["hits"] == 2) == same
        p3.check_state()
        p3.close()
    p.close(), p2.close()


def walk_frames(rng, n_streams, max_faces, updates, faces=5):
    """a seeded random walk: `faces` faces per stream on a 240 x 320 frame with their own velocities (they cross), each seen with probability 0.8
    -> per update a list of per-stream RESULT_DTYPE [max_faces] (score-descending, at most max_faces boxes; one in ten with an empty ROI)"""
    pos = rng.uniform(20, 200, (n_streams, faces, 2))
    vel = rng.uniform(-6, 6, (n_streams, faces, 2))
    size = rng.integers(20, 60, (n_streams, faces))
    out = []
    for _ in range(updates):
        pos += vel
        vel[(pos < 10) | (pos > 260)] *= -1
        per_stream = []
        for s in range(n_streams):
            dets = []
            for f in range(faces):
                if rng.random() < 0.8:
                    x, y = int(pos[s, f, 0]) + int(rng.integers(-2, 3)), int(pos[s, f, 1]) + int(rng.integers(-2, 3))
                    dets.append((x, y, x + int(size[s, f]), y + int(size[s, f]), float(np.float32(rng.uniform(0.1, 1.0))), int(rng.random() >= 0.1)))
            dets.sort(key=lambda d: -d[4])
            per_stream.append(frame(max_faces, *dets[:max_faces]))
        out.append(per_stream)
    return out


@pytest.mark.parametrize("n_streams,max_tracks,max_faces,dim,decay", [(8, 1, 1, 4, 1.0), (8, 8, 5, 64, 1.0), (8, 33, 5, 512, 0.75), (2, 64, 64, 1024, 1.0),
                                                                        (8, 4, 5, 512, 1.0)])
def test_random_walk(frt, n_streams, max_tracks, max_faces, dim, decay):
    """8 streams (2 at the caps), 5 faces each with dropouts and crossings, 40 updates; a random subset of the streams per call, in random order;
    max_tracks 1 / 8 / 33 / 64 and max_faces 1 / 5 / 64: one lane, part of a wave, an odd count, the whole wave; 4 slots for 5 faces: drops"""
    rng = np.random.default_rng(100 + max_tracks)
    p = Pair(frt, n_streams, max_tracks, max_faces, dim, seed=200 + max_tracks, decay=decay, max_missed=2, iou_threshold=0.25)
    ids_seen = set()
    for k, per_stream in enumerate(walk_frames(rng, n_streams, max_faces, 40)):
        ids = [int(s) for s in rng.permutation(n_streams)[:rng.integers(1, n_streams + 1)]]
        got, _ = p.update([per_stream[s] for s in ids], ids=ids)
        ids_seen.update(int(i) for i in got["track_id"].reshape(-1) if i >= 0)
        if k % 13 == 12:
            p.check_state()
    p.check_state()
    assert len(ids_seen) > 3 and p.ref.tick.sum() > 40
    if max_tracks < 5:
        assert p.ref.dropped.sum() > 0
    if max_tracks >= 8:
        assert (p.ref.slots["hits"] >= 3).any() and p.ref.next_id.max() > 5    # long tracks, and expiries with rebirths
    p.close()


def test_a_full_wave_of_detections_and_tracks(frt):
    """64 detections on 64 slots: every lane of the wave takes part in the reductions, the ballot and the births"""
    rng = np.random.default_rng(7)
    p = Pair(frt, 1, 64, 64, 256, seed=8, iou_threshold=0.2)
    grid = [(16 * (i // 8), 16 * (i % 8), 16 * (i // 8) + 12, 16 * (i % 8) + 12, 1.0 - i / 100.0) for i in range(64)]
    got, _ = p.update([frame(64, *grid)])
    assert got[0]["slot"].tolist() == list(range(64))
    perm = rng.permutation(64)
    moved = [(grid[j][0] + 1, grid[j][1] + 1, grid[j][2] + 1, grid[j][3] + 1, 1.0 - i / 100.0) for i, j in enumerate(perm)]
    got, _ = p.update([frame(64, *moved)])
    assert got[0]["slot"].tolist() == perm.tolist() and (got[0]["hits"] == 2).all()
    got, _ = p.update([frame(64, *moved[:40])])
    p.check_state()
    p.close()


def planted_gallery(rows=777):
    rng = np.random.default_rng(31)
    g = rng.standard_normal((rows, 512)).astype(np.float32)
    return g / np.linalg.norm(g, axis=1, keepdims=True).astype(np.float32)


def test_identity(frt):
    """777 rows, two planted: a track whose embeddings are a planted row (plus noise) is identified as that row, by the bits of MatMul.top1 of
    the update's template rows; -1 / 0 without a matcher, with an empty gallery and for n_embeds == 0; a coasting track keeps its identity"""
    g = planted_gallery()
    mm = frt.MatMul()
    mm.init(g)
    p = Pair(frt, matcher=mm, seed=9, **SCRIPT)
    rng = np.random.default_rng(10)

    def emb(*rows):
        e = p.embeds(1)
        for i, r in enumerate(rows):
            if r is not None:
                v = g[r] + 0.02 * rng.standard_normal(512).astype(np.float32)
                e[i] = v / np.float32(np.linalg.norm(v))
        return e

    for k in range(3):
        got, _ = p.update([frame(3, A, B, (200, 200, 240, 240, 0.5, 0))], emb(100, 500, 7), ids=[1])
        assert got[0]["match_idx"].tolist() == [100, 500, -1] and got[0, 2]["match_sim"] == 0 and got[0, 2]["n_embeds"] == 0
        assert got[0, 0]["match_sim"] > 0.9 and got[0, 0]["n_embeds"] == k + 1
    # track of A coasts: B alone is seen, A's slot keeps 100
    p.update([frame(3, B)], emb(500), ids=[1])
    slots, _ = p.dev.tracks(1)
    assert slots["match_idx"][:3].tolist() == [100, 500, -1] and slots["missed"][:3].tolist() == [1, 0, 1]
    p.check_state()
    # the same tracker without a matcher, and with an empty gallery: the records say -1 / 0, the tracks keep what they had
    empty = frt.MatMul()
    empty.galleryBegin(0, 512)
    empty.galleryCommit()
    for m in (None, empty):
        p.mm = m
        got, _ = p.update([frame(3, A, B)], emb(100, 500), ids=[1])
        assert got[0]["match_idx"].tolist() == [-1, -1, -1] and not got[0]["match_sim"].any()
    p.check_state()
    assert p.dev.tracks(1)[0]["match_idx"][:2].tolist() == [100, 500]
    # a matcher of another width is refused, nothing changes
    narrow = frt.MatMul()
    narrow.init(np.ones((3, 64), np.float32))
    with pytest.raises(frt.FrtError) as ei:
        p.dev.update(frame(3, A), p.embeds(1), [1], narrow)
    assert ei.value.code == frt.FRT_ERR_INVALID
    p.check_state()
    p.close()
    for m in (mm, empty, narrow):
        m.close()


def test_update_dev_on_a_stream_of_its_own_gives_the_bits_of_update(frt):
    import torch

    g = planted_gallery()
    mm = frt.MatMul()
    mm.init(g)
    opt = dict(n_streams=3, max_tracks=4, max_faces=3, dim=512)
    a, b = frt.Tracker(**opt), frt.Tracker(**opt)
    rng = np.random.default_rng(12)
    st = torch.cuda.Stream()
    for k, per_stream in enumerate(walk_frames(rng, 3, 3, 6)):
        ids = [2, 0] if k % 2 else [0, 1, 2]
        res = np.concatenate([per_stream[s] for s in ids])
        e = rng.standard_normal((len(res), 512)).astype(np.float32)
        want, want_tpl = a.update(res, e, ids, mm)
        with torch.cuda.stream(st):
            d_res = torch.from_numpy(res.view(np.uint8).copy()).cuda()
            d_e = torch.from_numpy(e).cuda()
            d_trk = torch.zeros(len(res) * 32, dtype=torch.uint8, device="cuda")
            d_tpl = torch.zeros((len(res), 512), dtype=torch.float32, device="cuda")
            st.synchronize()
            b.updateDev(d_res.data_ptr(), d_e.data_ptr(), len(ids), d_trk.data_ptr(), d_tpl.data_ptr() if k != 3 else None, ids, mm, st.cuda_stream)
            st.synchronize()
        assert d_trk.cpu().numpy().view(frt.TRACK_DTYPE).tobytes() == want.tobytes()
        if k != 3:
            assert d_tpl.cpu().numpy().tobytes() == want_tpl.tobytes()
    for s in range(3):
        assert [x.tobytes() for x in a.tracks(s, True)[::2]] == [x.tobytes() for x in b.tracks(s, True)[::2]] and a.tracks(s)[1] == b.tracks(s)[1]
    a.close(), b.close(), mm.close()


def test_pipeline_run_tracked(frt, synth, blobs):
    """three consecutive calls of two frames, the later ones rolled copies of the first, on the 96 x 160 det + ir fixtures: the records and
    embeddings are Pipeline.run's bits, the tracks and templates are Tracker.update's for those records, a track id lives through all three"""
    H, W, MF, PER = 96, 160, 8, 2
    dpath, _ = blobs("det")
    rpath, _ = blobs("ir")
    det = frt.RetinaFace(dpath, W, H, (3, H, W), 4, MF, 0.4, 0.02)
    rec = frt.ArcFaceIR50(rpath, W, H, maxBatchSize=4, maxFacesPerScene=MF)
    first = synth.make_frames(PER, H, W)
    res0, emb0 = frt.Pipeline(det, rec, 4, match=False).run(first)
    assert (res0["valid"] != 0).sum() >= 4
    g = planted_gallery()
    g[100], g[500] = emb0[0], emb0[MF]
    rec.setGallery(g)
    rec.initMatMul()
    pipe = frt.Pipeline(det, rec, 4)
    tracked, alone = frt.Tracker(PER, 16, MF), frt.Tracker(PER, 16, MF)
    alive = None
    for c in range(3):
        frames = np.roll(first, 2 * c, axis=2)
        want_res, want_emb = pipe.run(frames)
        res, emb, trk, tpl = pipe.runTracked(tracked, frames)
        assert res.tobytes() == want_res.tobytes() and emb.tobytes() == want_emb.tobytes()
        want_trk, want_tpl = alone.update(want_res, want_emb, None, rec.matmul)
        assert trk.tobytes() == want_trk.tobytes() and tpl.tobytes() == want_tpl.tobytes()
        ids = set(int(i) for i in trk[0]["track_id"] if i >= 0)
        alive = ids if alive is None else alive & ids
        if c == 0:
            assert trk[0, 0]["match_idx"] == 100 and trk[1, 0]["match_idx"] == 500
    assert alive, "no track id lived through the three calls"
    for s in range(PER):
        assert [x.tobytes() for x in tracked.tracks(s, True)[::2]] == [x.tobytes() for x in alone.tracks(s, True)[::2]]
    # the tracker must be the pipeline's shape: refused before any device work, nothing written
    other = frt.Tracker(PER, 16, MF - 1)
    with pytest.raises(frt.FrtError) as ei:
        pipe.runTracked(other, first)
    assert ei.value.code == frt.FRT_ERR_INVALID
    with pytest.raises(frt.FrtError) as ei:
        pipe.runTracked(tracked, np.concatenate([first] * 3)[:5], stream_ids=None)   # 5 frames on a pipeline (and a tracker) for fewer
    assert ei.value.code == frt.FRT_ERR_INVALID
    for o in (other, tracked, alone, pipe, rec, det):
        o.close()
