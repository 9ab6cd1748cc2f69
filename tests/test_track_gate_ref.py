"""tests/track_gate_ref.py against hand-written cases: the numpy restatement of the gate (include/frt.h "Gate") is itself checked here, so
that the GPU test compares the kernel with something that was compared with the rules.  No GPU, no library."""
import numpy as np
import pytest

import track_gate_ref as gr
import track_ref as tk

NEXT = float(np.nextafter(np.float32(0.5), np.float32(1)))
A, B, C = (10, 10, 50, 50), (100, 100, 140, 140), (200, 200, 240, 240)
OPT = dict(iou_threshold=0.3, min_hits=3, refresh=4, min_embeds=2, skip_iou=0.5)


def slots(T, *tracks):
    """tracks: (slot, box, hits, n_embeds) -> STATE_DTYPE [T], the named slots live"""
    s = np.zeros(T, tk.STATE_DTYPE)
    for k, (t, box, hits, ne) in enumerate(tracks):
        s[t] = (1, 10 + k, box[0], box[1], box[2], box[3], 0.9, 0, hits, 0, ne, -1, 0.0)
    return s


def boxes(MF, *dets):
    b = np.zeros(MF, gr.BBOX_DTYPE)
    for i, d in enumerate(dets):
        b[i] = tuple(d[:4]) + (d[4] if len(d) > 4 else 0.9,)
    return b


def one(s, b, n_boxes=None, **kw):
    return gr.gate_frame(s, b, n_boxes, **{**OPT, **kw})


def rec(g):
    return (int(g["decision"]), int(g["slot"]), float(g["ovr"]), int(g["why"]))


def test_layout_and_options():
    assert gr.GATE_DTYPE.itemsize == 16 and [gr.GATE_DTYPE.fields[n][1] for n in ("decision", "slot", "ovr", "why")] == [0, 4, 8, 12]
    assert (gr.ABSENT, gr.EMBED, gr.FOLLOW) == (0, 1, 2)
    assert (gr.NO_TRACK, gr.UNCONFIRMED, gr.FEW_EMBEDS, gr.LOW_OVERLAP, gr.REFRESH) == (1, 2, 4, 8, 16)
    nan = float("nan")
    for ok in ((1, 1, 1.0), (16, 3, 2.0 ** -20), (2 ** 31 - 1, 2 ** 31 - 1, 0.5)):
        assert gr.check_options(*ok), ok
    for bad in ((0, 1, 0.5), (-1, 1, 0.5), (1, 0, 0.5), (1, -3, 0.5), (1, 1, 0.0), (1, 1, -0.5), (1, 1, 1.5), (1, 1, nan)):
        assert not gr.check_options(*bad), bad


def test_follow_and_each_reason_alone():
    # a confirmed track with embeddings, a detection right on it, (hits + 1) % 4 != 0: followed, why 0
    g = one(slots(4, (1, A, 5, 2)), boxes(3, A))
    assert rec(g[0]) == (gr.FOLLOW, 1, 1.0, 0) and rec(g[1]) == rec(g[2]) == (gr.ABSENT, -1, 0.0, 0)
    # NO_TRACK: nothing overlaps
    assert rec(one(slots(4, (1, A, 5, 2)), boxes(3, B))[0]) == (gr.EMBED, -1, 0.0, gr.NO_TRACK)
    # UNCONFIRMED alone: hits 2 < 3 ((2 + 1) % 4 != 0)
    assert rec(one(slots(4, (1, A, 2, 2)), boxes(3, A))[0]) == (gr.EMBED, 1, 1.0, gr.UNCONFIRMED)
    # FEW_EMBEDS alone
    assert rec(one(slots(4, (1, A, 5, 1)), boxes(3, A))[0]) == (gr.EMBED, 1, 1.0, gr.FEW_EMBEDS)
    # LOW_OVERLAP alone: matched (>= 0.3) but under skip_iou
    g = one(slots(4, (1, (0, 0, 9, 9), 5, 2)), boxes(3, (0, 0, 9, 3)))
    assert rec(g[0]) == (gr.EMBED, 1, float(np.float32(0.4)), gr.LOW_OVERLAP)
    # REFRESH alone: hits 7, (7 + 1) % 4 == 0
    assert rec(one(slots(4, (1, A, 7, 2)), boxes(3, A))[0]) == (gr.EMBED, 1, 1.0, gr.REFRESH)
    # all four at once
    g = one(slots(4, (1, (0, 0, 9, 9), 1, 0)), boxes(3, (0, 0, 9, 3)), refresh=2)
    assert rec(g[0])[3] == gr.UNCONFIRMED | gr.FEW_EMBEDS | gr.LOW_OVERLAP | gr.REFRESH


def test_the_equal_to_threshold_cases():
    """hits == min_hits, n_embeds == min_embeds, ovr == skip_iou (and == iou_threshold)"""
    assert rec(one(slots(2, (0, A, 3, 2)), boxes(1, A), refresh=5)[0]) == (gr.FOLLOW, 0, 1.0, 0)   # hits == min_hits ((3 + 1) % 5 != 0)
    assert rec(one(slots(2, (0, A, 2, 2)), boxes(1, A), refresh=5)[0])[3] == gr.UNCONFIRMED
    assert rec(one(slots(2, (0, A, 5, 2)), boxes(1, A))[0])[0] == gr.FOLLOW                           # n_embeds == min_embeds
    assert rec(one(slots(2, (0, A, 5, 1)), boxes(1, A))[0])[3] == gr.FEW_EMBEDS
    # the pair whose overlap is exactly 0.5
    s, b = slots(2, (0, (0, 0, 9, 9), 5, 2)), boxes(1, (0, 0, 9, 4))
    assert rec(one(s, b, skip_iou=0.5)[0]) == (gr.FOLLOW, 0, 0.5, 0)
    assert rec(one(s, b, skip_iou=NEXT)[0]) == (gr.EMBED, 0, 0.5, gr.LOW_OVERLAP)
    assert rec(one(s, b, iou_threshold=0.5, skip_iou=0.5)[0]) == (gr.FOLLOW, 0, 0.5, 0)
    assert rec(one(s, b, iou_threshold=NEXT, skip_iou=0.5)[0]) == (gr.EMBED, -1, 0.0, gr.NO_TRACK)


def test_refresh_and_its_neighbours():
    for hits, want in ((6, 0), (7, gr.REFRESH), (8, 0), (3, gr.REFRESH), (11, gr.REFRESH)):
        g = rec(one(slots(2, (0, A, hits, 2)), boxes(1, A))[0])
        assert g == ((gr.EMBED if want else gr.FOLLOW), 0, 1.0, want), hits
    # refresh == 1 embeds everything: REFRESH on every matched detection, NO_TRACK alone on the others
    g = one(slots(4, (0, A, 5, 2), (2, B, 1, 0)), boxes(3, A, B, C), refresh=1)
    assert [rec(x)[0] for x in g] == [gr.EMBED] * 3
    assert [rec(x)[3] for x in g] == [gr.REFRESH, gr.REFRESH | gr.UNCONFIRMED | gr.FEW_EMBEDS, gr.NO_TRACK]


def test_competition_ties_and_empty_streams():
    # two detections compete for one track: the first in slot order takes it although the second overlaps more; the second is NO_TRACK
    g = one(slots(4, (2, (0, 3, 9, 12), 5, 2)), boxes(3, (0, 1, 9, 10, 0.9), (0, 3, 9, 12, 0.8)))
    assert rec(g[0])[:2] == (gr.FOLLOW, 2) and rec(g[1]) == (gr.EMBED, -1, 0.0, gr.NO_TRACK)
    # two tracks tie on one detection: the lowest slot wins; the other track is left for the next detection
    s = slots(4, (1, (0, 0, 9, 9), 5, 2), (3, (0, 6, 9, 15), 5, 2))
    g = one(s, boxes(3, (0, 3, 9, 12, 0.9), (0, 3, 9, 12, 0.8)), iou_threshold=0.1, skip_iou=0.1)
    assert [rec(x)[1] for x in g[:2]] == [1, 3] and rec(g[0])[2] == rec(g[1])[2]
    # a stream with no live track
    g = one(slots(4), boxes(3, A, B))
    assert [rec(x) for x in g] == [(gr.EMBED, -1, 0.0, gr.NO_TRACK)] * 2 + [(gr.ABSENT, -1, 0.0, 0)]
    # a slot that is not live is no candidate even where its stale box matches
    s = slots(4, (1, A, 5, 2))
    s[1]["live"] = 0
    assert rec(one(s, boxes(3, A))[0]) == (gr.EMBED, -1, 0.0, gr.NO_TRACK)


def test_n_boxes_hides_a_stale_box():
    s, b = slots(4, (0, A, 5, 2), (1, B, 5, 2)), boxes(3, A, B)
    assert [rec(x)[0] for x in one(s, b)] == [gr.FOLLOW, gr.FOLLOW, gr.ABSENT]
    g = one(s, b, n_boxes=1)
    assert [rec(x) for x in g[1:]] == [(gr.ABSENT, -1, 0.0, 0)] * 2 and rec(g[0])[0] == gr.FOLLOW
    assert [rec(x)[0] for x in one(s, b, n_boxes=0)] == [gr.ABSENT] * 3
    # a score of zero is absent whatever the count says
    b["score"][0] = 0
    assert [rec(x)[0] for x in one(s, b, n_boxes=3)] == [gr.ABSENT, gr.FOLLOW, gr.ABSENT]


@pytest.mark.parametrize("n_embed", [0, 3, 4, 5])
def test_the_list_and_the_pass_counts(n_embed):
    """B = 4: n_embed = 0, B - 1, B, B + 1 out of 2 frames x 5 slots"""
    g = np.empty((2, 5), gr.GATE_DTYPE)
    g[:] = gr.ABSENT_RECORD
    g[0, 1] = (gr.FOLLOW, 0, 1.0, 0)
    where = [(1, 4), (0, 2), (1, 0), (0, 0), (1, 1)][:n_embed]
    for f, d in where:
        g[f, d] = (gr.EMBED, -1, 0.0, gr.NO_TRACK)
    lst, n, pc = gr.work_list(g, 4)
    want = sorted(f * 5 + d for f, d in where)
    assert n == n_embed and lst.tolist() == want + [-1] * (10 - n_embed) and lst.dtype == np.int32
    assert pc.tolist() == {0: [0, 0, 0], 3: [3, 0, 0], 4: [4, 0, 0], 5: [4, 1, 0]}[n_embed] and pc.dtype == np.int32


def test_a_whole_call_follows_a_ref_tracker():
    """the state of track_ref.Tracker after three updates, gated: what was confirmed and embedded is followed, the newcomer is embedded"""
    t = tk.Tracker(2, 4, 3, 8, min_hits=2)
    res = np.zeros((2, 3), tk.RESULT_DTYPE)
    res[0, 0] = A + (0.9, 0, -1, 0.0, 1)
    res[1, 0] = B + (0.8, 0, -1, 0.0, 1)
    e = np.ones((6, 8), np.float32)
    for _ in range(3):
        t.update(res.reshape(-1), e)
    b = np.zeros((2, 3), gr.BBOX_DTYPE)
    b[0, 0], b[0, 1], b[1, 0] = A + (0.9,), C + (0.5,), B + (0.8,)
    before = t.slots.tobytes()
    g, lst, n, pc = gr.gate(t.slots[[1, 0]], b[[1, 0]], None, 0.3, 2, 5, 2, 0.5, 4)    # frames in the order of streams 1, 0
    assert t.slots.tobytes() == before
    assert [rec(x) for x in g[0]] == [(gr.FOLLOW, 0, 1.0, 0), (gr.ABSENT, -1, 0.0, 0), (gr.ABSENT, -1, 0.0, 0)]
    assert [rec(x) for x in g[1]] == [(gr.FOLLOW, 0, 1.0, 0), (gr.EMBED, -1, 0.0, gr.NO_TRACK), (gr.ABSENT, -1, 0.0, 0)]
    assert n == 1 and lst.tolist() == [4, -1, -1, -1, -1, -1] and pc.tolist() == [1, 0]
