"""The tracker's gate on the GPU (frt_tracker_gate, frt_pipeline_run_tracked_gated and their Python shells) against tests/track_gate_ref.py,
the numpy restatement of include/frt.h "Gate".  The reference is never the code under test.

The gate alone: the state is built by Tracker.update on scripted and seeded random-walk sequences (the device tracker and track_ref's, fed
the same calls as in tests/test_gpu_track.py), then Tracker.gate is compared with the restatement run on track_ref's slots: the records by
their bytes, the list, the count and the pass counts for equality.  Behind every gate the tracker's state is compared with what it was.

End to end, the reference composition is made of routes that existed before the gate: the boxes, flags and crops of every slot from
Pipeline.submit with crops; the numpy gate on the slots of a TWIN tracker; ArcFaceIR50.doInference over the listed crops' CHW in passes of
maxBatchSize (rows of invalid crops zeroed, as the recogniser's last kernel zeroes them); MatMul.top1 of the compact rows; the records and
embeddings assembled in numpy and handed to the twin's Tracker.update.  Records, gate records, embeddings, crops, tracks and templates are
compared by their bytes on every call, the slots and the sums at the end.  Nothing here compares with Pipeline.run's embeddings: the pass
sizes differ, and with them the recogniser's launch plan."""
import threading

import numpy as np
import pytest

import track_gate_ref as gr
from test_gpu_track import SCRIPT, A, B, C, Pair, frame, planted_gallery, walk_frames

pytestmark = pytest.mark.gpu
BOX = ("x1", "y1", "x2", "y2", "score")


def to_boxes(res):
    """RESULT_DTYPE records -> BBOX_DTYPE, same shape"""
    res = np.asarray(res)
    b = np.zeros(res.shape, gr.BBOX_DTYPE)
    for k in BOX:
        b[k] = res[k]
    return b


def state_bytes(trk, streams):
    return [[x.tobytes() for x in trk.tracks(s, True)[::2]] + [trk.tracks(s)[1]] for s in streams]


def check_gate(p, results, ids, refresh, min_embeds, skip_iou, max_batch, n_boxes=None):
    """Tracker.gate of the pair's device tracker against the restatement on the pair's ref slots -> the reference's (records, list, n, passes)"""
    res = np.concatenate(results).reshape(len(results), p.max_faces)
    boxes = to_boxes(res)
    streams = range(p.n_streams)
    before = state_bytes(p.dev, streams)
    got = p.dev.gate(boxes, refresh, min_embeds, skip_iou, ids, n_boxes, max_batch)
    assert state_bytes(p.dev, streams) == before                                     # the gate writes no state
    order = list(range(len(results))) if ids is None else list(ids)
    want = gr.gate(p.ref.slots[order], boxes, n_boxes, p.ref.thr, p.ref.min_hits, refresh, min_embeds, skip_iou, max_batch)
    assert got[0].dtype == gr.GATE_DTYPE and got[0].shape == want[0].shape and got[0].tobytes() == want[0].tobytes(), (got[0], want[0])
    assert got[1].dtype == np.int32 and got[1].tolist() == want[1].tolist()
    assert got[2] == want[2] and got[3].dtype == np.int32 and got[3].tolist() == want[3].tolist()
    return want


def update_and_check_prediction(p, results, ids, gate_rec):
    """the update that follows (appearance off): every present detection's peek is the slot of an overlap match, -1 otherwise"""
    res = np.concatenate(results)
    e = p.embeds(len(results))
    got, _, assoc = p.dev.update(res, e, ids, None, want_templates=False, want_assoc=True)
    want, _ = p.ref.update(res, e, ids)
    assert got.tobytes() == want.tobytes()
    if gate_rec is not None:
        present = gate_rec["decision"] != gr.ABSENT
        by_overlap = assoc["how"] == p.frt.TRACK_ASSOC_IOU
        assert (present == (assoc["how"] != p.frt.TRACK_ASSOC_ABSENT)).all()
        assert (gate_rec["slot"][present & by_overlap] == got["slot"][present & by_overlap]).all()
        assert (gate_rec["slot"][present & ~by_overlap] == -1).all()
        assert (gate_rec["ovr"][present & by_overlap].view(np.uint32) == assoc["ovr"][present & by_overlap].view(np.uint32)).all()


def test_scripted_all_embed_all_follow_and_the_reasons(frt):
    def fr(*d):
        return frame(3, *d)

    p = Pair(frt, seed=1, **SCRIPT)                                                   # min_hits 3
    calls = [[fr(A, B), fr(C)]] * 4
    seen = set()
    for k, c in enumerate(calls):
        for refresh, min_embeds in ((1, 1), (4, 2), (100, 1)):
            g, lst, n, pc = check_gate(p, c, [0, 2], refresh, min_embeds, 0.5, 2)
            seen.update(int(w) for w in g["why"].reshape(-1))
            if refresh == 1 or k == 0:                                                # an all-EMBED call: refresh 1, or no track yet
                assert n == 3 and lst.tolist() == [0, 1, 3, -1, -1, -1] and pc.tolist() == [2, 1, 0]
            if refresh == 100 and k == 3:                                             # an all-FOLLOW call: hits 3, embeddings 3
                assert n == 0 and (lst == -1).all() and not pc.any() and (g["decision"].reshape(-1)[[0, 1, 3]] == gr.FOLLOW).all()
        g = check_gate(p, c, [0, 2], 4, 2, 0.5, 2)[0]
        update_and_check_prediction(p, c, [0, 2], g)
    assert {gr.NO_TRACK, gr.REFRESH | gr.UNCONFIRMED, gr.UNCONFIRMED | gr.FEW_EMBEDS, gr.UNCONFIRMED, gr.REFRESH, 0} <= seen
    # n_boxes hides a stale box; a stream that was never updated has no track
    g = check_gate(p, [fr(A, B), fr(A)], [0, 1], 100, 1, 0.5, 4, n_boxes=[1, 1])[0]
    assert g["decision"].tolist() == [[gr.FOLLOW, gr.ABSENT, gr.ABSENT], [gr.EMBED, gr.ABSENT, gr.ABSENT]] and g[1, 0]["why"] == gr.NO_TRACK
    # the pair whose overlap is exactly 0.5, at skip_iou 0.5 and one ulp above
    q = Pair(frt, seed=2, iou_threshold=0.5, min_hits=1, **SCRIPT)
    q.update([fr((0, 0, 9, 9))], ids=[1])
    nxt = float(np.nextafter(np.float32(0.5), np.float32(1)))
    assert check_gate(q, [fr((0, 0, 9, 4))], [1], 9, 1, 0.5, 4)[0][0, 0].tolist() == (gr.FOLLOW, 0, 0.5, 0)
    assert check_gate(q, [fr((0, 0, 9, 4))], [1], 9, 1, nxt, 4)[0][0, 0].tolist() == (gr.EMBED, 0, 0.5, gr.LOW_OVERLAP)
    # two detections compete for one track, and two tracks tie on one detection (test_track_gate_ref.py has the expected records)
    check_gate(q, [fr((0, 1, 9, 10, 0.9), (0, 0, 9, 9, 0.8))], [1], 9, 1, 0.5, 4)
    p.close(), q.close()


@pytest.mark.parametrize("n_streams,max_tracks,max_faces,dim", [(8, 1, 1, 4), (8, 8, 5, 64), (8, 33, 5, 512), (2, 64, 64, 1024), (8, 4, 5, 512)])
def test_random_walk(frt, n_streams, max_tracks, max_faces, dim):
    """the walk of tests/test_gpu_track.py: a random subset of the streams per call in random order, n_frames 1 .. n_streams (3 among them);
    max_tracks 1 / 8 / 33 / 64 and max_faces 1 / 5 / 64; the options and max_batch change from call to call; every third call hides the last
    box of every frame behind n_boxes"""
    rng = np.random.default_rng(300 + max_tracks)
    p = Pair(frt, n_streams, max_tracks, max_faces, dim, seed=400 + max_tracks, max_missed=2, iou_threshold=0.25, min_hits=2)
    decisions, whys, sizes = set(), set(), set()
    for k, per_stream in enumerate(walk_frames(rng, n_streams, max_faces, 30)):
        n = 3 if k % 7 == 3 and n_streams >= 3 else int(rng.integers(1, n_streams + 1))
        ids = [int(s) for s in rng.permutation(n_streams)[:n]]
        results = [per_stream[s] for s in ids]
        refresh, min_embeds = int(rng.integers(1, 6)), int(rng.integers(1, 4))
        skip_iou = float(np.float32(rng.uniform(0.25, 0.9)))
        max_batch = int(rng.integers(1, 2 * max_faces + 2))
        counts = np.array([(r["score"] > 0).sum() for r in results], np.int32)
        n_boxes = None if k % 3 else np.maximum(counts - 1, 0)
        g, _, ne, _ = check_gate(p, results, ids, refresh, min_embeds, skip_iou, max_batch, n_boxes)
        if n_boxes is not None:                                                       # the prediction is for the boxes the update sees
            g = check_gate(p, results, ids, refresh, min_embeds, skip_iou, max_batch, counts)[0]
        update_and_check_prediction(p, results, ids, g)
        decisions.update(g["decision"].reshape(-1).tolist())
        whys.update(g["why"].reshape(-1).tolist())
        sizes.add(n)
    p.check_state()
    assert gr.EMBED in decisions and gr.NO_TRACK in whys and (3 in sizes or n_streams < 3)
    if max_tracks >= 8:                                                               # room for every face: tracks last, and are followed
        assert gr.FOLLOW in decisions and len(whys) >= 4
    p.close()


def test_the_full_list_of_256_frames_of_64_faces(frt):
    """16 384 slots, all of them embedded (no track yet): every LDS entry of the prefix, every lane of every wave, the whole list; then, with
    two tracks per stream, 512 followed faces spread over the list.  max_batch 128 (full passes) and 100 (a partial last pass)"""
    p = Pair(frt, 256, 2, 64, 4, seed=5, min_hits=1, iou_threshold=0.2)
    grid = [(16 * (i // 8), 16 * (i % 8), 16 * (i // 8) + 12, 16 * (i % 8) + 12, 1.0 - i / 100.0) for i in range(64)]
    rng = np.random.default_rng(6)
    ids = [int(s) for s in rng.permutation(256)]
    frames = [frame(64, *[grid[j] for j in rng.permutation(64)]) for _ in range(256)]
    for mb in (128, 100):
        g, lst, n, pc = check_gate(p, frames, ids, 7, 1, 0.5, mb)
        assert n == 16384 and lst.tolist() == list(range(16384)) and pc.sum() == 16384 and pc[-1] == (128 if mb == 128 else 84)
    update_and_check_prediction(p, frames, ids, g)
    g, lst, n, pc = check_gate(p, frames, ids, 7, 1, 0.5, 100)
    assert n == 16384 - 512 and (g["decision"] == gr.FOLLOW).sum() == 512 and (lst[n:] == -1).all()
    p.close()


# ----------------------------------------------------------------------------------------------------------------- the pipeline
H, W, MF, PER, REC_BATCH = 96, 160, 8, 2, 4
OPTS = dict(refresh=3, min_embeds=1, skip_iou=0.5)


def make(frt, blobs, kind="det", gallery=None):
    dpath, _ = blobs(kind)
    rpath, _ = blobs("ir")
    det = frt.RetinaFace(dpath, W, H, (3, H, W), 4, MF, 0.4, 0.02)
    rec = frt.ArcFaceIR50(rpath, W, H, maxBatchSize=REC_BATCH, maxFacesPerScene=MF)
    if gallery is not None:
        rec.setGallery(gallery)
        rec.initMatMul()
    return det, rec, frt.Pipeline(det, rec, 4, match=gallery is not None)


def close(*objs):
    for o in objs:
        o.close()


def every_slot(frt, pipe, frames):
    """the records (boxes, flags) and the u8 crops of every face slot, by the route that was there before the gate"""
    n = len(frames) * MF
    res, emb, crops = np.zeros(n, frt.RESULT_DTYPE), np.zeros((n, 512), np.float32), np.zeros((n, 112, 112, 3), np.uint8)
    pipe.wait(pipe.submit(np.ascontiguousarray(frames), res, emb, crops))
    return res, crops


def chw_of(crops, valid):
    """preprocessFace of u8 BGR crops: RGB planes, (x - 127.5) / 128, exact in float32; zeros for an invalid crop"""
    x = (crops[..., ::-1].astype(np.float32) - np.float32(127.5)) * np.float32(0.0078125)
    x = np.ascontiguousarray(x.transpose(0, 3, 1, 2))
    x[valid == 0] = 0
    return x


def compose(frt, pipe, rec, twin, frames, ids, tracker_opts, opts, gallery):
    """the reference composition of one call -> dict of what frt_pipeline_run_tracked_gated must return, and what the gate decided"""
    res_all, crops_all = every_slot(frt, pipe, frames)
    n = len(frames)
    boxes = to_boxes(res_all).reshape(n, MF)
    n_boxes = (boxes["score"] > 0).sum(1).astype(np.int32)
    order = list(range(n)) if ids is None else list(ids)
    slots = np.stack([twin.tracks(s)[0] for s in order])
    gate, lst, ne, pc = gr.gate(slots, boxes, n_boxes, tracker_opts["iou_threshold"], tracker_opts["min_hits"], opts["refresh"], opts["min_embeds"],
                                opts["skip_iou"], REC_BATCH)
    sel = lst[:ne]
    crops, valid_c = crops_all[sel], res_all["valid"][sel]
    emb_c = np.zeros((ne, 512), np.float32)
    chw = chw_of(crops, valid_c)
    for f0 in range(0, ne, REC_BATCH):
        emb_c[f0:f0 + REC_BATCH] = rec.doInference(chw[f0:f0 + REC_BATCH])
    emb_c[valid_c == 0] = 0
    res = res_all.copy()
    res["valid"], res["match_idx"], res["match_sim"] = 0, -1, 0
    res["valid"][sel] = valid_c
    if gallery and ne:
        idx, sim = rec.matmul.top1(emb_c)
        ok = valid_c != 0
        res["match_idx"][sel[ok]], res["match_sim"][sel[ok]] = idx[ok], sim[ok]
    emb = np.zeros((n * MF, 512), np.float32)
    emb[sel] = emb_c
    trk, tpl = twin.update(res, emb, ids, rec.matmul if gallery else None)
    return dict(res=res, emb=emb, trk=trk, tpl=tpl, gate=gate, crops=crops, ne=ne, pc=pc)


def run_and_compare(frt, pipe, rec, tracked, twin, frames, ids, tracker_opts, opts, gallery, what=""):
    want = compose(frt, pipe, rec, twin, frames, ids, tracker_opts, opts, gallery)
    res, emb, trk, tpl, ne, gate, crops = pipe.runTrackedGated(tracked, frames, stream_ids=ids, want_gate=True, want_crops=True, **opts)
    assert ne == want["ne"], (what, ne, want["ne"])
    for name, got in (("res", res), ("gate", gate), ("emb", emb), ("crops", crops), ("trk", trk), ("tpl", tpl)):
        assert got.shape == want[name].shape and got.tobytes() == want[name].tobytes(), (what, name)
    return want


def same_state(tracked, twin, streams):
    for s in streams:
        a, b = tracked.tracks(s, True), twin.tracks(s, True)
        assert a[0].tobytes() == b[0].tobytes() and a[2].tobytes() == b[2].tobytes() and a[1] == b[1], s   # slots, sums by their bits, counters


@pytest.fixture(scope="module")
def first(synth):
    return synth.make_frames(PER, H, W)


@pytest.fixture(scope="module")
def gallery(frt, blobs, first):
    det, rec, pipe = make(frt, blobs)
    _, emb0 = pipe.run(first)
    close(pipe, rec, det)
    g = planted_gallery()
    g[100], g[500] = emb0[0], emb0[MF]
    return g


@pytest.fixture(scope="module")
def objs(frt, blobs, gallery):
    det, rec, pipe = make(frt, blobs, gallery=gallery)
    yield det, rec, pipe
    close(pipe, rec, det)


TRACKER = dict(iou_threshold=0.3, max_missed=5, min_hits=2, decay=1.0)


def test_end_to_end_equals_the_composition(frt, objs, first):
    """2 streams, maxBatchSize 4, max_faces 8, min_hits 2, refresh 3, the frames rolled 2 px per call; what the sequence must show is asserted
    on the reference's gate"""
    det, rec, pipe = objs
    tracked, twin = frt.Tracker(PER, 16, MF, **TRACKER), frt.Tracker(PER, 16, MF, **TRACKER)
    decisions, whys, partial, counts = [], [], False, []
    for c in range(7):
        frames = np.roll(first, 2 * c, axis=2)
        want = run_and_compare(frt, pipe, rec, tracked, twin, frames, None, TRACKER, OPTS, True, "call %d" % c)
        present = want["gate"]["decision"] != gr.ABSENT
        decisions += want["gate"]["decision"][present].tolist()
        whys += want["gate"]["why"][present].tolist()
        partial = partial or want["ne"] % REC_BATCH != 0
        counts.append(want["ne"])
        # a followed face: no frame-level match, its box kept, its identity the track's
        fol = (want["gate"]["decision"] == gr.FOLLOW).reshape(-1)
        assert not want["res"]["valid"][fol].any() and (want["res"]["match_idx"][fol] == -1).all() and (want["res"]["score"][fol] > 0).all()
        assert not want["emb"][fol].any() and (want["trk"].reshape(-1)["track_id"][fol] >= 0).all()
    print("n_embed per call:", counts)
    assert gr.FOLLOW in decisions and any(w & gr.REFRESH for w in whys) and any(w & gr.NO_TRACK for w in whys) and partial, (counts, set(whys))
    same_state(tracked, twin, range(PER))
    # the streams in the other order, one stream alone
    run_and_compare(frt, pipe, rec, tracked, twin, first[::-1], [1, 0], TRACKER, OPTS, True, "swapped")
    run_and_compare(frt, pipe, rec, tracked, twin, first[1:], [1], TRACKER, OPTS, True, "one frame")
    same_state(tracked, twin, range(PER))
    close(tracked, twin)


def test_refresh_one_embeds_everything_and_a_still_scene_is_followed_whole(frt, objs, first):
    det, rec, pipe = objs
    tracked, twin = frt.Tracker(PER, 16, MF, **TRACKER), frt.Tracker(PER, 16, MF, **TRACKER)
    every = dict(refresh=1, min_embeds=1, skip_iou=0.5)
    for c in range(3):
        want = run_and_compare(frt, pipe, rec, tracked, twin, first, None, TRACKER, every, True, "refresh 1, call %d" % c)
        present = want["gate"]["decision"] != gr.ABSENT
        assert (want["gate"]["decision"][present] == gr.EMBED).all() and want["ne"] == present.sum()
    # the same frames again under a long refresh: every face sits on a confirmed track with embeddings - nothing for the recogniser, no
    # match call; a face whose ROI is empty never gathers an embedding and is embedded (in vain) every time, so min_embeds counts from 1
    still = dict(refresh=1000, min_embeds=1, skip_iou=0.5)
    want = run_and_compare(frt, pipe, rec, tracked, twin, first, None, TRACKER, still, True, "still")
    present = want["gate"]["decision"] != gr.ABSENT
    few = (want["gate"]["why"] & gr.FEW_EMBEDS) != 0
    assert (want["gate"]["decision"][present & ~few] == gr.FOLLOW).all()
    if not few.any():
        assert want["ne"] == 0 and want["crops"].shape[0] == 0 and not want["emb"].any()
        assert (want["trk"]["match_idx"].reshape(-1)[[0, MF]] == [100, 500]).all()      # the tracks' identities, from step 7
    print("still scene: n_embed", want["ne"], "of", int(present.sum()))
    same_state(tracked, twin, range(PER))
    close(tracked, twin)


def test_without_a_gallery(frt, blobs, first):
    det, rec, pipe = make(frt, blobs)
    tracked, twin = frt.Tracker(PER, 16, MF, **TRACKER), frt.Tracker(PER, 16, MF, **TRACKER)
    for c in range(4):
        want = run_and_compare(frt, pipe, rec, tracked, twin, np.roll(first, 2 * c, axis=2), None, TRACKER, OPTS, False, "no gallery, call %d" % c)
        assert (want["res"]["match_idx"] == -1).all() and (want["trk"]["match_idx"] == -1).all()
    same_state(tracked, twin, range(PER))
    close(tracked, twin, pipe, rec, det)


@pytest.mark.parametrize("mode", ["flip", "fp32"])
def test_recogniser_modes(frt, objs, first, mode):
    det, rec, pipe = objs
    switch = rec.setFlip if mode == "flip" else rec.setPrecision
    plain_t, plain_w = frt.Tracker(PER, 16, MF, **TRACKER), frt.Tracker(PER, 16, MF, **TRACKER)
    plain = run_and_compare(frt, pipe, rec, plain_t, plain_w, first, None, TRACKER, OPTS, True, "plain")
    close(plain_t, plain_w)
    tracked, twin = frt.Tracker(PER, 16, MF, **TRACKER), frt.Tracker(PER, 16, MF, **TRACKER)
    switch(True)
    try:
        for c in range(4):
            want = run_and_compare(frt, pipe, rec, tracked, twin, np.roll(first, 2 * c, axis=2), None, TRACKER, OPTS, True, "%s, call %d" % (mode, c))
            if c == 0:
                assert want["ne"] == plain["ne"] and want["emb"].tobytes() != plain["emb"].tobytes()
    finally:
        switch(False)
    run_and_compare(frt, pipe, rec, tracked, twin, first, None, TRACKER, OPTS, True, "back")
    same_state(tracked, twin, range(PER))
    close(tracked, twin)


def test_appearance_on_the_update_decides(frt, objs, first):
    """with appearance on the peek is a prediction: the twin runs the same settings, and its update - fed the followed faces with valid 0 -
    says what the tracks become"""
    det, rec, pipe = objs
    kw = dict(reid_threshold=0.5, iou_min_sim=0.2, **TRACKER)
    tracked, twin = frt.Tracker(PER, 16, MF, **kw), frt.Tracker(PER, 16, MF, **kw)
    for c in range(6):
        frames = np.roll(first, (2 * c) if c != 3 else 40, axis=2)                     # call 3 jumps: faces leave their boxes
        run_and_compare(frt, pipe, rec, tracked, twin, frames, None, TRACKER, OPTS, True, "appearance, call %d" % c)
    same_state(tracked, twin, range(PER))
    close(tracked, twin)


def test_gather_crops_are_the_bytes_of_the_slot_crops(frt, blobs, first, gallery):
    """the gather crop and the gather alignment against the kernels they share their arithmetic with: crop j of the call is row list[j] of
    the crops Pipeline.submit returns for every slot, on a list that mixes the frames (four frames in one call, the streams permuted, tracks
    on some of them only)"""
    frames4 = np.concatenate([first, np.roll(first, 6, axis=2)])
    for kind in ("det", "det_ldm"):
        det, rec, pipe = make(frt, blobs, kind, gallery)
        if kind == "det_ldm":
            pipe.set_align(True)
        tracked = frt.Tracker(4, 16, MF, **TRACKER)
        res_all, crops_all = every_slot(frt, pipe, frames4)
        ids = [2, 0, 3, 1]
        for c in range(4):
            use = frames4 if c != 1 else frames4[:2]                                    # call 1 feeds streams 2 and 0 only: they run ahead
            res, _, _, _, ne, gate, crops = pipe.runTrackedGated(tracked, use, stream_ids=ids[:len(use)], want_gate=True, want_crops=True, **OPTS)
            lst = np.nonzero(gate.reshape(-1)["decision"] == gr.EMBED)[0]
            assert ne == len(lst) and crops.shape[0] == ne
            assert crops.tobytes() == crops_all[lst].tobytes(), (kind, c)
            assert (res["valid"][lst] == res_all["valid"][lst]).all()
            if c == 3:
                assert 0 < ne < (gate["decision"] != gr.ABSENT).sum() and len(set(lst // MF)) > 1   # a list with gaps, from several frames
        close(tracked, pipe, rec, det)


def test_refusals_write_nothing(frt, objs, first):
    det, rec, pipe = objs
    tracked = frt.Tracker(PER, 16, MF, **TRACKER)
    before = state_bytes(tracked, range(PER))
    other = frt.Tracker(PER, 16, MF - 1)
    cases = [(other, first, None, OPTS, frt.FRT_ERR_INVALID),                                        # the tracker is not the pipeline's shape
             (tracked, np.concatenate([first] * 3)[:5], None, OPTS, frt.FRT_ERR_INVALID),             # 5 frames on a pipeline for 4
             (tracked, first, [0, 0], OPTS, frt.FRT_ERR_INVALID)]
    cases += [(tracked, first, None, dict(refresh=r, min_embeds=m, skip_iou=s), frt.FRT_ERR_INVALID)
              for r, m, s in ((0, 1, 0.5), (3, 0, 0.5), (3, 1, 0.0), (3, 1, 1.5), (3, 1, float("nan")))]
    for trk, frames, ids, opts, code in cases:
        with pytest.raises(frt.FrtError) as ei:
            pipe.runTrackedGated(trk, frames, stream_ids=ids, **opts)
        assert ei.value.code == code
    # the raw entry: sentinel bytes stay
    import ctypes
    res = np.full(PER * MF, 7, frt.RESULT_DTYPE)
    trk = np.full(PER * MF * 32, 0x55, np.uint8)
    ne = ctypes.c_int32(-7)
    bad = frt.TrackGateOptions(0, 1, 0.5)
    for o in (None, ctypes.addressof(bad)):
        assert frt.lib.frt_pipeline_run_tracked_gated(pipe._h, tracked._h, o, first.ctypes.data, PER, None, res.ctypes.data, trk.ctypes.data, None, None,
                                                      None, None, ctypes.addressof(ne)) == frt.FRT_ERR_INVALID
    assert res.tobytes() == np.full(PER * MF, 7, frt.RESULT_DTYPE).tobytes() and (trk == 0x55).all() and ne.value == -7
    assert state_bytes(tracked, range(PER)) == before
    close(other, tracked)


def test_beside_submits_of_another_thread(frt, synth, objs, first):
    det, rec, pipe = objs
    frames = synth.make_frames(4, H, W, start=20)
    want_frames = tuple(a.copy() for a in pipe.run(frames))
    seq = [np.roll(first, 2 * c, axis=2) for c in range(5)]

    def walk():
        t = frt.Tracker(PER, 16, MF, **TRACKER)
        out = [pipe.runTrackedGated(t, f, want_gate=True, want_crops=True, **OPTS) for f in seq]
        state = state_bytes(t, range(PER))
        t.close()
        return out, state

    want, want_state = walk()
    got_frames, errors = [], []
    started = threading.Event()
    CALLS = 200  # the helper is bound by a call count, not by time

    def worker():
        try:
            for _ in range(CALLS):
                r = np.zeros(4 * MF, frt.RESULT_DTYPE)
                e = np.zeros((4 * MF, 512), np.float32)
                pipe.wait(pipe.submit(frames, r, e))
                got_frames.append((r, e))
                started.set()
        except Exception as ex:  # noqa: BLE001
            errors.append(ex)
        started.set()

    th = threading.Thread(target=worker)
    th.start()
    assert started.wait(60)
    got, got_state = walk()
    th.join()
    assert not errors, errors
    assert len(got_frames) == CALLS and got_state == want_state
    for g, w in zip(got, want):
        assert g[4] == w[4] and all(a.tobytes() == b.tobytes() for a, b in zip(g[:4] + g[5:], w[:4] + w[5:]))
    for r, e in got_frames:
        assert r.tobytes() == want_frames[0].tobytes() and e.tobytes() == want_frames[1].tobytes()
