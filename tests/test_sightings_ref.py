"""The numpy restatement of the sighting book (tests/sightings_ref.py) pinned by hand-written expectations for scripted scenes
(tests/sightings_cases.py), so that what the device code is compared with is itself checked by something other than itself.  No GPU."""
import numpy as np

import sightings_cases as sc
import sightings_ref as sr

FIELDS = ("stream", "track_id", "first_tick", "last_tick", "close_tick", "reason", "hits", "n_embeds", "confirmed", "match_idx", "n_shots",
          "best_tick")


def _play(name):
    script, rig = sc.SCENES[name]
    return sc.run_ref(script, **rig)


def _row(rec):
    return tuple(int(rec[k]) for k in FIELDS)


def test_record_layout():
    assert sr.SIGHTING_DTYPE.itemsize == 96
    assert [sr.SIGHTING_DTYPE.fields[n][1] for n in sr.SIGHTING_DTYPE.names] == list(range(0, 96, 4))


def test_one_track_from_birth_to_expiry():
    rig, (drain,), inputs = _play("birth_to_expiry")
    rec, emb, tpl, crops, counters = drain
    # born at tick 0, seen at ticks 0 1 2, coasts through tick 3 (max_missed 1), expires in the update of tick 4; the tracker's min_hits is 2
    assert [_row(r) for r in rec] == [(0, 0, 0, 2, 4, sr.EXPIRED, 3, 3, 1, -1, 3, 1)]
    r = rec[0]
    assert (r["x1"], r["y1"], r["x2"], r["y2"]) == sc.A and r["score"] == np.float32(0.9) and r["match_sim"] == 0
    assert r["best_sharpness"] == 9.0 and r["best_flags"] == 0 and r["best_size"] == 40 and r["reserved"] == 0
    q1 = inputs[1][2][0]                                   # the quality record of the best shot: tick 1, face slot 0
    assert r["best_luma_var"] == q1["luma_var"] and r["best_mean"] == q1["mean"]
    assert np.array_equal(emb[0], inputs[1][1][0]) and np.array_equal(crops[0], inputs[1][3][0])
    s = inputs[0][1][0] + inputs[1][1][0] + inputs[2][1][0]    # decay 1: the template is the normalised sum of the three embeddings
    assert np.allclose(tpl[0], s / np.linalg.norm(s), atol=1e-6)
    assert counters == dict(queued=1, overflowed=0, discarded=0, closed=1)
    assert not rig.book.rec.view(np.uint8).any() and not rig.book.emb.any() and not rig.book.tpl.any() and not rig.book.crops.any()
    assert rig.book.drain(8)[0].size == 0


def test_replaced_close_and_reopen_in_one_update():
    rig, (drain,), inputs = _play("replaced")
    rec, emb, tpl, crops, counters = drain
    # max_missed 0: track 0 misses tick 1 and is freed, the far-away face is born into the same slot in the same update
    assert [_row(r) for r in rec] == [(0, 0, 0, 0, 1, sr.REPLACED, 1, 1, 0, -1, 1, 0)]
    assert np.array_equal(emb[0], inputs[0][1][0]) and np.array_equal(crops[0], inputs[0][3][0])    # the OLD payload went to the queue
    o_rec, o_emb, o_tpl, o_crops = rig.book.open(0)
    assert _row(o_rec[0]) == (0, 1, 1, 1, -1, 0, 1, 1, 0, -1, 1, 1) and not o_rec[1:].view(np.uint8).any()
    assert np.array_equal(o_emb[0], inputs[1][1][0]) and np.array_equal(o_crops[0], inputs[1][3][0])
    assert (o_rec[0]["x1"], o_rec[0]["y1"], o_rec[0]["x2"], o_rec[0]["y2"]) == sc.B


def test_min_hits_discards_and_counts():
    rig, (drain,), _ = _play("discard")
    assert drain[0].size == 0 and drain[4] == dict(queued=0, overflowed=0, discarded=1, closed=1)
    assert not rig.book.rec.view(np.uint8).any()


def test_overflow_at_capacity_two():
    rig, (drain,), _ = _play("overflow")
    rec, _, _, _, counters = drain
    assert [(int(r["track_id"]), int(r["reason"])) for r in rec] == [(0, sr.EXPIRED), (1, sr.EXPIRED)]     # slots ascending; the third is lost
    assert counters == dict(queued=2, overflowed=1, discarded=0, closed=3)
    assert not rig.book.rec.view(np.uint8).any()


def test_three_ranks_pick_three_shots():
    best = {}
    for name in ("rank_sharpness", "rank_size", "rank_score"):
        _, (drain,), _ = _play(name)
        rec = drain[0]
        assert rec.size == 1 and rec[0]["reason"] == sr.CLOSED and rec[0]["close_tick"] == rec[0]["last_tick"] == 2 and rec[0]["n_shots"] == 3
        best[name] = (int(rec[0]["best_tick"]), float(rec[0]["best_sharpness"]), int(rec[0]["best_size"]))
    assert best == dict(rank_sharpness=(0, 9.0, 30), rank_size=(1, 5.0, 50), rank_score=(2, 7.0, 40))


def test_flagged_sharp_shot_loses_to_unflagged_soft_one():
    _, (drain,), _ = _play("flagged")
    r = drain[0][0]
    assert (r["best_tick"], r["best_sharpness"], r["best_flags"], r["n_shots"]) == (1, 1.0, 0, 3)


def test_tie_keeps_the_earlier_shot():
    _, (drain,), inputs = _play("tie")
    assert drain[0][0]["best_tick"] == 0 and np.array_equal(drain[1][0], inputs[0][1][0])


def test_nan_never_replaces_a_shot_that_exists():
    _, (drain,), _ = _play("nan_score")
    r = drain[0][0]
    assert r["best_tick"] == 0 and r["n_shots"] == 3         # 0.5, then NaN, then 0.25


def test_close_then_the_same_track_continues():
    _, (drain,), _ = _play("close_continues")
    rec = drain[0]
    # the first sighting ends at its last tick; the track goes on and opens a second one with the same id and the track's own birth
    assert [_row(r) for r in rec] == [(0, 0, 0, 1, 1, sr.CLOSED, 2, 2, 1, -1, 2, 0), (0, 0, 0, 2, 2, sr.CLOSED, 3, 3, 1, -1, 1, 2)]


def test_sparse_calls_queue_in_call_order_then_slot_order():
    rig, drains, _ = _play("sparse")
    order = [[(int(r["stream"]), int(r["track_id"]), int(r["reason"])) for r in d[0]] for d in drains]
    # stream 2: track 0 (face C) is last seen at tick 1 and freed at tick 3, where face B is born into its slot: REPLACED.  Stream 0's
    # track 0 (face A) is last seen at tick 1 and expires in the next update, at its tick 3.
    assert order[0] == [(2, 0, sr.REPLACED)] and drains[0][4] == dict(queued=2, overflowed=0, discarded=0, closed=2)
    # the update with frames (stream 2, stream 0, stream 1): stream 2's slot 0 (track 2, REPLACED by the birth of face C) and slot 1
    # (track 1) fill the queue of capacity 3; stream 0's track 1 is lost, then stream 1's track 0 an update later, then close(1)'s
    assert order[1] == [(0, 0, sr.EXPIRED), (2, 2, sr.REPLACED), (2, 1, sr.EXPIRED)]
    assert drains[1][4] == dict(queued=3, overflowed=3, discarded=0, closed=7)
    assert order[2] == [(2, 3, sr.CLOSED)] and drains[2][4] == dict(queued=1, overflowed=3, discarded=0, closed=8)
    assert not rig.book.rec.view(np.uint8).any()
