"""The scripted scenarios of the tracker's appearance term, written once for the CPU test (the restatement alone) and the GPU test (a device
tracker and the restatement fed the same calls, compared byte for byte per update).  A scenario takes `mk`, which makes a tracker-like object:

    t = mk(n_streams, max_tracks, max_faces, dim, **options)       # options: track_ref's, plus reid_threshold / iou_min_sim (None: off)
    trk, assoc = t.update([frame, ...], embeds [n * max_faces, dim], ids)
    t.set_appearance(reid_threshold, iou_min_sim);  t.slots(stream) -> STATE_DTYPE [max_tracks];  t.sums(stream);  t.close()

and asserts the outcomes include/frt.h states.  Inputs are finite (but for the NaN case), and every product is normal or zero."""
import numpy as np

import track_reid_ref as rr
from track_reid_ref import HOW_APPEARANCE, HOW_BIRTH, HOW_IOU, frame, noisy

A, B, C, D4 = (10, 10, 50, 50), (100, 100, 140, 140), (200, 200, 240, 240), (300, 10, 340, 50)   # pairwise disjoint: IoU 0


def unit_rows(dim, n=3, seed=0):
    return rr.identities(np.random.default_rng(seed), n, dim)


def emb(max_faces, dim, *rows):
    e = np.zeros((max_faces, dim), np.float32)
    for i, r in enumerate(rows):
        e[i] = r
    return e


def mixed(*parts):
    """normalised fp32 sum of (weight, vector) parts"""
    v = sum(np.float32(w) * x for w, x in parts).astype(np.float32)
    return (v / np.float32(np.linalg.norm(v))).astype(np.float32)


def reattach_after_a_jump(mk, dim, max_tracks, max_faces, on):
    """a track with embedding a coasts two updates and returns at a box of IoU 0 with a + small noise"""
    a = unit_rows(dim)[0]
    rng = np.random.default_rng(1)
    t = mk(2, max_tracks, max_faces, dim, max_missed=3, reid_threshold=0.5 if on else None)
    fr = lambda *d: frame(max_faces, *d)
    trk, _ = t.update([fr(A)], emb(max_faces, dim, a), [1])
    assert trk[0, 0]["track_id"] == 0
    for _ in range(2):
        t.update([fr()], emb(max_faces, dim), [1])
    assert t.slots(1)[0]["missed"] == 2
    trk, assoc = t.update([fr(B)], emb(max_faces, dim, noisy(rng, a, 0.1)), [1])
    if on:
        assert trk[0, 0]["track_id"] == 0 and trk[0, 0]["slot"] == 0 and trk[0, 0]["hits"] == 2 and trk[0, 0]["n_embeds"] == 2 and trk[0, 0]["age"] == 4
        assert assoc[0, 0]["how"] == HOW_APPEARANCE and assoc[0, 0]["gap"] == 2 and assoc[0, 0]["ovr"] == 0 and assoc[0, 0]["sim"] > 0.9
        assert t.slots(1)[0]["x1"] == B[0] and t.slots(1)[0]["missed"] == 0
    else:
        assert trk[0, 0]["track_id"] == 1 and trk[0, 0]["slot"] == 1 and trk[0, 0]["hits"] == 1
        assert assoc[0, 0]["how"] == HOW_BIRTH and assoc[0, 0]["gap"] == 0 and assoc[0, 0]["sim"] == 0
    t.close()


def coast_past_max_missed_then_return(mk, dim, max_tracks, max_faces, on):
    """expiry is unchanged: after max_missed + 1 unseen updates the track is gone, and the face comes back as a new id in either mode"""
    a = unit_rows(dim)[0]
    t = mk(1, max_tracks, max_faces, dim, max_missed=2, reid_threshold=0.5 if on else None, iou_min_sim=0.2 if on else None)
    fr = lambda *d: frame(max_faces, *d)
    t.update([fr(A)], emb(max_faces, dim, a))
    for _ in range(3):
        t.update([fr()], emb(max_faces, dim))
    assert t.slots(0)[0]["live"] == 0 and not t.sums(0)[0].any()
    trk, assoc = t.update([fr(B)], emb(max_faces, dim, a))
    assert trk[0, 0]["track_id"] == 1 and trk[0, 0]["slot"] == 0 and trk[0, 0]["age"] == 1 and assoc[0, 0]["how"] == HOW_BIRTH
    t.close()


def tie_goes_to_the_lowest_slot(mk, dim, max_tracks, max_faces):
    """two tracks with bit-identical sums"""
    a = unit_rows(dim)[0]
    rng = np.random.default_rng(2)
    t = mk(1, max_tracks, max_faces, dim, reid_threshold=0.5)
    fr = lambda *d: frame(max_faces, *d)
    t.update([fr(A, B)], emb(max_faces, dim, a, a))
    assert t.sums(0)[0].tobytes() == t.sums(0)[1].tobytes() and t.sums(0)[0].any()
    t.update([fr()], emb(max_faces, dim))
    trk, assoc = t.update([fr(C)], emb(max_faces, dim, noisy(rng, a, 0.1)))
    assert trk[0, 0]["slot"] == 0 and assoc[0, 0]["how"] == HOW_APPEARANCE and assoc[0, 0]["gap"] == 1
    assert t.slots(0)[1]["missed"] == 2
    t.close()


def detections_go_in_slot_order(mk, dim, max_tracks, max_faces):
    """two returning detections and two lost tracks: the first detection takes the track both like best, the second the other one"""
    a, b = unit_rows(dim)[:2]
    t = mk(1, max_tracks, max_faces, dim, reid_threshold=0.5)
    fr = lambda *d: frame(max_faces, *d)
    t.update([fr(A, B)], emb(max_faces, dim, a, b))                       # track 0: a, track 1: b
    t.update([fr()], emb(max_faces, dim))
    d0, d1 = mixed((1.0, b), (0.6, a)), mixed((1.0, b), (0.8, a))          # cosines with (a, b): (0.51, 0.86) and (0.62, 0.78)
    trk, assoc = t.update([fr(C, D4)], emb(max_faces, dim, d0, d1))
    assert trk[0]["slot"][:2].tolist() == [1, 0] and assoc[0]["how"][:2].tolist() == [HOW_APPEARANCE] * 2
    assert 0.85 < assoc[0, 0]["sim"] < 0.87 and 0.61 < assoc[0, 1]["sim"] < 0.64     # the second one's best track (0.78) was taken
    t.close()


def veto(mk, dim, max_tracks, max_faces, reid):
    """a detection sits on track 0's box and carries track 1's embedding, iou_min_sim 0.5"""
    a, b = unit_rows(dim)[:2]
    rng = np.random.default_rng(3)
    t = mk(1, max_tracks, max_faces, dim, iou_min_sim=0.5, reid_threshold=0.5 if reid else None)
    fr = lambda *d: frame(max_faces, *d)
    t.update([fr(A, B)], emb(max_faces, dim, a, b))
    trk, assoc = t.update([fr(A)], emb(max_faces, dim, noisy(rng, b, 0.1)))
    if reid:
        assert trk[0, 0]["track_id"] == 1 and trk[0, 0]["slot"] == 1 and assoc[0, 0]["how"] == HOW_APPEARANCE
        assert assoc[0, 0]["gap"] == 0 and assoc[0, 0]["ovr"] == 0 and assoc[0, 0]["sim"] > 0.9
        assert t.slots(0)[1]["x1"] == A[0] and t.slots(0)[1]["missed"] == 0
    else:
        assert trk[0, 0]["track_id"] == 2 and trk[0, 0]["slot"] == 2 and assoc[0, 0]["how"] == HOW_BIRTH
        assert t.slots(0)[1]["missed"] == 1
    assert t.slots(0)[0]["missed"] == 1 and t.slots(0)[0]["hits"] == 1 and t.slots(0)[0]["x1"] == A[0]       # track 0 coasts
    t.close()


def undefined_pairs_neither_veto_nor_match(mk, dim, max_tracks, max_faces):
    a, b = unit_rows(dim)[:2]
    fr = lambda *d: frame(max_faces, *d)
    # ---- a valid == 0 detection: ungated in 2a (it sits on track 0's box with the opposite embedding), never in 2b (far away with a itself)
    t = mk(1, max_tracks, max_faces, dim, iou_min_sim=0.5, reid_threshold=0.5)
    t.update([fr(A)], emb(max_faces, dim, a))
    trk, assoc = t.update([fr(A + (0.9, 0))], emb(max_faces, dim, -a))
    assert trk[0, 0]["track_id"] == 0 and assoc[0, 0]["how"] == HOW_IOU and assoc[0, 0]["sim"] == 0 and assoc[0, 0]["ovr"] == 1
    t.update([fr()], emb(max_faces, dim))
    trk, assoc = t.update([fr(B + (0.9, 0))], emb(max_faces, dim, a))
    assert trk[0, 0]["track_id"] == 1 and assoc[0, 0]["how"] == HOW_BIRTH
    t.close()
    # ---- a track born from an empty-ROI detection (n_embeds == 0): no veto on its box, no match away from it
    t = mk(1, max_tracks, max_faces, dim, iou_min_sim=0.5, reid_threshold=0.5)
    t.update([fr(A + (0.9, 0))], emb(max_faces, dim, a))
    assert t.slots(0)[0]["n_embeds"] == 0
    trk, assoc = t.update([fr(B)], emb(max_faces, dim, a))
    assert trk[0, 0]["track_id"] == 1 and assoc[0, 0]["how"] == HOW_BIRTH
    trk, assoc = t.update([fr(A, B)], emb(max_faces, dim, b, a))
    assert trk[0]["track_id"][:2].tolist() == [0, 1] and assoc[0]["how"][:2].tolist() == [HOW_IOU] * 2 and assoc[0, 0]["sim"] == 0
    assert assoc[0, 0]["gap"] == 1 and assoc[0, 1]["sim"] == 1
    t.close()
    # ---- a sum that is exactly zero (e then -e at decay 1, built with appearance off: -e on e's track would be vetoed)
    t = mk(1, max_tracks, max_faces, dim)
    t.update([fr(A)], emb(max_faces, dim, a))
    t.update([fr(A)], emb(max_faces, dim, -a))
    assert not t.sums(0)[0].any() and t.slots(0)[0]["n_embeds"] == 2
    t.set_appearance(0.5, 0.5)
    trk, assoc = t.update([fr(B)], emb(max_faces, dim, a))
    assert trk[0, 0]["track_id"] == 1 and assoc[0, 0]["how"] == HOW_BIRTH
    trk, assoc = t.update([fr(A, B)], emb(max_faces, dim, b, a))
    assert trk[0]["track_id"][:2].tolist() == [0, 1] and assoc[0, 0]["how"] == HOW_IOU and assoc[0, 0]["sim"] == 0 and assoc[0, 0]["gap"] == 1
    t.close()
    # ---- a NaN embedding: S is DEFINED and NaN; it does not veto on the track's box and does not match away from it.  The sum it lands
    #      in is NaN from then on (n2 is NaN, so the pairs of that track are not DEFINED)
    t = mk(1, max_tracks, max_faces, dim, iou_min_sim=0.5, reid_threshold=0.5)
    bad = a.copy()
    bad[dim // 2] = np.nan
    t.update([fr(A, B)], emb(max_faces, dim, a, b))
    t.update([fr()], emb(max_faces, dim))
    trk, assoc = t.update([fr(A, C)], emb(max_faces, dim, bad, bad))
    assert trk[0]["track_id"][:2].tolist() == [0, 2] and assoc[0]["how"][:2].tolist() == [HOW_IOU, HOW_BIRTH]
    assert np.isnan(assoc[0, 0]["sim"]) and assoc[0, 0]["gap"] == 1 and assoc[0, 1]["sim"] == 0
    t.update([fr()], emb(max_faces, dim))
    trk, assoc = t.update([fr(D4)], emb(max_faces, dim, a))                # the track that was a's holds NaN now: no match, a birth
    assert assoc[0, 0]["how"] == HOW_BIRTH and trk[0, 0]["track_id"] == 3
    t.close()


def permuted_batch_and_a_stream_left_out(mk, dim, max_tracks, max_faces, calls):
    """the frames of every call in another order, on a second tracker: the same per-stream state after every call"""
    opt = dict(iou_threshold=0.3, max_missed=3, reid_threshold=0.5, iou_min_sim=0.2)
    n_streams = 1 + max(max(ids) for ids, _, _ in calls)
    q, r = mk(n_streams, max_tracks, max_faces, dim, **opt), mk(n_streams, max_tracks, max_faces, dim, **opt)
    rng = np.random.default_rng(4)
    left_out = 0
    for ids, res, e in calls:
        n = len(ids)
        left_out += n < n_streams
        tq, aq = q.update(res, e, ids)
        order = rng.permutation(n)
        tr, ar = r.update(res.reshape(n, max_faces)[order].reshape(-1), e.reshape(n, max_faces, dim)[order].reshape(-1, dim), [ids[i] for i in order])
        assert tr.tobytes() == tq[order].tobytes() and ar.tobytes() == aq[order].tobytes()
        for s in range(n_streams):
            assert q.slots(s).tobytes() == r.slots(s).tobytes() and q.sums(s).tobytes() == r.sums(s).tobytes(), s
    assert left_out > 0
    q.close(), r.close()
