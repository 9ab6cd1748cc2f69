"""tests/track_ref.py, the numpy restatement of the face tracker (include/frt.h "Face tracker"), on hand-written cases: one per step of an
update, and the pair of boxes whose overlap is exactly the threshold.  Nothing here needs the library."""
import numpy as np

import track_ref as tk

D = 8


def frame(*dets, max_faces=3):
    """dets: (x1, y1, x2, y2[, score[, valid]]) -> RESULT_DTYPE [max_faces], unused slots zero (score 0, valid 0)"""
    r = np.zeros(max_faces, tk.RESULT_DTYPE)
    r["match_idx"] = -1
    for i, d in enumerate(dets):
        d = tuple(d) + (0.9, 1)[len(d) - 4:]
        r[i] = (d[0], d[1], d[2], d[3], d[4], 0, -1, 0.0, d[5])
    return r


def emb(*rows, max_faces=3):
    e = np.zeros((max_faces, D), np.float32)
    for i, r in enumerate(rows):
        e[i] = r
    return e


def unit(k, scale=1.0):
    v = np.zeros(D, np.float32)
    v[k] = scale
    return v


A, B = (10, 10, 50, 50), (100, 100, 140, 140)


def test_step1_presence_is_the_score_and_absent_slots_are_minus_one():
    t = tk.Tracker(1, 4, 3, D)
    trk, tpl = t.update(frame(A, (0, 0, 5, 5, 0.0, 1), (60, 60, 90, 90, 0.5, 0)), emb(unit(0), unit(1), unit(2)))
    assert trk[0, 0]["track_id"] == 0 and trk[0, 2]["track_id"] == 1     # the empty-ROI slot (valid 0, score > 0) is present
    assert trk[0, 1].tobytes() == tk.ABSENT.tobytes() and not tpl[0, 1].any()
    assert t.slots[0]["live"].tolist() == [1, 1, 0, 0]
    nan = frame((0, 0, 5, 5, np.nan, 1))
    assert t.update(nan, emb(unit(0)))[0][0, 0].tobytes() == tk.ABSENT.tobytes()  # a NaN score is not > 0


def test_step2_largest_overlap_wins_ties_go_to_the_lowest_slot_and_detections_go_in_slot_order():
    t = tk.Tracker(1, 4, 3, D, iou_threshold=0.1)
    t.update(frame((0, 0, 9, 9), (0, 20, 9, 29)), emb(unit(0), unit(1)))          # tracks 0 and 1
    # a detection between them, shifted towards track 1: larger overlap with slot 1
    trk, _ = t.update(frame((0, 12, 9, 21)), emb(unit(2)))
    assert trk[0, 0]["slot"] == 1 and trk[0, 0]["hits"] == 2
    assert t.slots[0, 1]["y1"] == 12 and t.slots[0, 0]["missed"] == 1            # the box follows the detection, the other track coasts
    # two tracks with the same box tie on a detection: the lowest slot takes it, the second detection (slot order) gets the other
    t = tk.Tracker(1, 4, 3, D, iou_threshold=0.1)
    t.update(frame((0, 0, 9, 9), (0, 40, 9, 49)), emb(unit(0), unit(1)))
    t.slots[0, 1]["y1"], t.slots[0, 1]["y2"] = 0, 9                                # slot 1 now sits on slot 0's box
    trk, _ = t.update(frame((0, 0, 9, 9, 0.9), (0, 1, 9, 10, 0.8)), emb(unit(0), unit(1)))
    assert trk[0]["slot"][:2].tolist() == [0, 1]
    # detection-order priority: the first detection takes the track although the second overlaps it more
    t = tk.Tracker(1, 4, 3, D, iou_threshold=0.1)
    t.update(frame((0, 0, 9, 9)), emb(unit(0)))
    trk, _ = t.update(frame((0, 3, 9, 12, 0.9), (0, 0, 9, 9, 0.8)), emb(unit(0), unit(1)))
    assert trk[0]["track_id"][:2].tolist() == [0, 1] and trk[0]["hits"][:2].tolist() == [2, 1]


def test_the_exact_threshold_pair():
    a, b = (0, 0, 9, 9), (0, 0, 9, 4)
    assert tk.overlap((0,) + a, (0,) + b, 0) == np.float32(0.5)
    for thr, same in ((0.5, True), (np.nextafter(np.float32(0.5), np.float32(1)), False)):
        t = tk.Tracker(1, 4, 3, D, iou_threshold=thr)
        t.update(frame(a), emb(unit(0)))
        trk, _ = t.update(frame(b), emb(unit(0)))
        assert (trk[0, 0]["track_id"] == 0) == same and (trk[0, 0]["hits"] == 2) == same
    # a NaN overlap (two boxes of zero area) never matches
    z = (5, 5, 4, 4)
    assert np.isnan(tk.overlap((0,) + z, (0,) + z, 0))
    t = tk.Tracker(1, 4, 3, D)
    t.update(frame(z), emb(unit(0)))
    assert t.update(frame(z), emb(unit(0)))[0][0, 0]["track_id"] == 1


def test_step3_a_track_coasts_max_missed_updates_and_expires_on_the_next():
    for coast, same in ((2, True), (3, False)):
        t = tk.Tracker(1, 2, 3, D, max_missed=2)
        t.update(frame(A), emb(unit(0)))
        for i in range(coast):
            t.update(frame(), emb())
            assert t.slots[0, 0]["missed"] == i + 1 if i < 2 else t.slots[0, 0]["live"] == 0
        if not same:
            assert not t.slots[0, 0].tobytes().strip(b"\0") and not t.sums[0, 0].any()   # freed: state and sum zeroed
        trk, _ = t.update(frame(A), emb(unit(1)))
        assert trk[0, 0]["track_id"] == (0 if same else 1) and trk[0, 0]["slot"] == 0
        assert trk[0, 0]["age"] == (coast + 2 if same else 1) and trk[0, 0]["hits"] == (2 if same else 1)


def test_step4_births_take_the_lowest_free_slot_also_one_freed_in_this_update_and_overflow_is_dropped():
    t = tk.Tracker(1, 2, 3, D, max_missed=0)
    t.update(frame(A, B), emb(unit(0), unit(1)))
    # A's track is not seen: it expires (max_missed 0) and the new detection C is born into its slot in the same update
    C = (200, 200, 240, 240)
    trk, _ = t.update(frame(B, C), emb(unit(1), unit(2)))
    assert trk[0, 0]["track_id"] == 1 and trk[0, 1]["track_id"] == 2 and trk[0, 1]["slot"] == 0
    assert np.array_equal(t.sums[0, 0], unit(2)) and t.slots[0, 0]["match_idx"] == -1
    # three detections, two slots, none matching: the third is untracked and counted
    t = tk.Tracker(1, 2, 3, D)
    trk, tpl = t.update(frame(A, B, (200, 200, 240, 240)), emb(unit(0), unit(1), unit(2)))
    assert trk[0]["track_id"].tolist() == [0, 1, -1] and trk[0]["slot"].tolist() == [0, 1, -1] and t.dropped[0] == 1 and t.next_id[0] == 2
    assert not tpl[0, 2].any() and trk[0, 2]["age"] == 0


def test_step5_and_6_the_sum_takes_two_roundings_and_the_template_is_its_direction():
    dec = np.float32(0.75)
    t = tk.Tracker(1, 2, 3, D, decay=0.75)
    rng = np.random.default_rng(5)
    e1, e2 = rng.standard_normal((2, D)).astype(np.float32)
    t.update(frame(A), emb(e1))
    trk, tpl = t.update(frame(A), emb(e2))
    want = (dec * e1).astype(np.float32) + e2
    assert np.array_equal(t.sums[0, 0], want) and trk[0, 0]["n_embeds"] == 2
    fused = (np.float64(dec) * e1.astype(np.float64) + e2.astype(np.float64)).astype(np.float32)   # what an fma would give
    assert (want != fused).any()                                                 # the case tells the two apart
    assert np.allclose(tpl[0, 0], want.astype(np.float64) / np.linalg.norm(want.astype(np.float64)), rtol=0, atol=1e-15)
    # an empty-ROI detection: the box follows, the sum and n_embeds do not; its template is still the track's
    trk, tpl2 = t.update(frame((12, 12, 52, 52, 0.9, 0)), emb(unit(5)))
    assert trk[0, 0]["n_embeds"] == 2 and trk[0, 0]["hits"] == 3 and np.array_equal(t.sums[0, 0], want) and t.slots[0, 0]["x1"] == 12
    assert np.array_equal(tpl2[0, 0], tpl[0, 0])
    # a track that has no embedding yet has a zero template; opposite embeddings cancel to one as well
    t = tk.Tracker(1, 2, 3, D)
    trk, tpl = t.update(frame((10, 10, 50, 50, 0.9, 0)), emb(unit(0)))
    assert trk[0, 0]["n_embeds"] == 0 and not tpl[0, 0].any()
    t.update(frame(A), emb(unit(0)))
    trk, tpl = t.update(frame(A), emb(-unit(0)))
    assert trk[0, 0]["n_embeds"] == 2 and not tpl[0, 0].any()


def test_step7_identity_goes_to_tracks_with_embeddings_and_a_coasting_track_keeps_it():
    t = tk.Tracker(1, 4, 3, D)
    seen = []

    def top1(q):
        seen.append(q.copy())
        return np.arange(len(q)) + 100, np.full(len(q), 0.5, np.float32)

    trk, _ = t.update(frame(A, (100, 100, 140, 140, 0.9, 0)), emb(unit(0), unit(1)), top1=top1)
    assert seen[0].shape == (3, D) and seen[0].dtype == np.float32           # one search over every template row of the call
    assert trk[0]["match_idx"].tolist() == [100, -1, -1] and trk[0]["match_sim"].tolist() == [0.5, 0, 0]  # n_embeds 0 / absent: -1 / 0
    assert t.slots[0, 0]["match_idx"] == 100 and t.slots[0, 1]["match_idx"] == -1
    t.update(frame(B), emb(unit(1)), top1=lambda q: (np.full(len(q), 7), np.full(len(q), 0.25, np.float32)))
    assert t.slots[0, 0]["match_idx"] == 100 and t.slots[0, 0]["missed"] == 1 and t.slots[0, 1]["match_idx"] == 7
    trk, _ = t.update(frame(A), emb(unit(0)))                                  # no matcher: the record says -1 / 0, the track keeps its identity
    assert trk[0, 0]["match_idx"] == -1 and t.slots[0, 0]["match_idx"] == 100


def test_step8_streams_are_independent_and_an_absent_stream_is_untouched():
    t = tk.Tracker(3, 2, 3, D, min_hits=2)
    both = np.concatenate([frame(A), frame(B)])
    t.update(both, np.concatenate([emb(unit(0)), emb(unit(1))]), stream_ids=[2, 0])
    assert t.tick.tolist() == [1, 0, 1] and t.next_id.tolist() == [1, 0, 1] and t.slots[2, 0]["x1"] == 10 and t.slots[0, 0]["x1"] == 100
    before = t.slots[0].copy()
    trk, _ = t.update(frame(A), emb(unit(0)), stream_ids=[2])
    assert trk[0, 0]["confirmed"] == 1 and trk[0, 0]["age"] == 2 and t.tick.tolist() == [1, 0, 2]
    assert t.slots[0].tobytes() == before.tobytes()                             # stream 0: no tick, no missed
    assert t.check_ids(2, [1, 1]) is None and t.check_ids(1, [3]) is None and t.check_ids(1, [-1]) is None and t.check_ids(257, None) is None
    assert t.check_ids(4, None) is None and t.check_ids(3, None) == [0, 1, 2]
    t.reset(2)
    assert t.tick.tolist() == [1, 0, 0] and t.next_id.tolist() == [1, 0, 1] and not t.slots[2]["live"].any() and t.slots[0, 0]["live"] == 1
    trk, _ = t.update(frame(A), emb(unit(0)), stream_ids=[2])
    assert trk[0, 0]["track_id"] == 1 and trk[0, 0]["age"] == 1                 # ids are never reused
    t.reset()
    assert not t.slots["live"].any() and not t.tick.any() and t.next_id.tolist() == [1, 0, 2]
