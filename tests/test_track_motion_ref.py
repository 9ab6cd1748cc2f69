"""tests/track_motion_ref.py on hand-computed cases (no GPU, nothing calls the library): the restatement of include/frt.h "Motion" that the
device code is compared with in tests/test_gpu_track_motion.py.  The scripted scenes live in SCENES so that the GPU file can replay them.
Boxes are 48 x 48 (x .. x + 47), for which the NMS IoU with its +1 of a shift by 10 px is 1824 / 2784 and of one by 30 px 864 / 3744."""
import numpy as np
import pytest

import track_gate_ref as gr
import track_motion_ref as mr
import track_ref as tk
import track_reid_ref as rr


def box(x, y=0, size=48, score=0.9):
    return (x, y, x + size - 1, y + size - 1, score)


def run(trk, frames, want_assoc=False):
    """frames: per update a tuple of detections (empty: nobody seen) -> the records of every update"""
    out = []
    for dets in frames:
        out.append(trk.update(rr.frame(trk.max_faces, *dets), np.zeros((trk.max_faces, trk.dim), np.float32), want_assoc=want_assoc))
    return out


def ids(records):
    return [int(r[0][0, 0]["track_id"]) for r in records]


ACCELERATION = [(box(x),) for x in (0, 10, 30, 60, 100, 140)]                    # shifts 10, 20, 30, 40, 40
COASTING = [(box(0),), (box(8),), (box(16),), (), (), (), (), (box(56),)]         # 8 px per update, four absent updates, back 40 px on
CROSSING = [(box(12 * i, 0, score=0.9), box(156 - 12 * i, 8, score=0.8)) for i in range(14)]
TRUNCATION = [(box(100),), (), (), ((99, 0, 147, 47, 0.9),), (box(99),)]
EMA = [(box(100, 50),), (box(104, 48),), (box(112, 48),), (), (), ((109, 50, 157, 98, 0.9),), (box(109, 50),)]
HUGE = [((-2 ** 30, 0, 2 ** 30, 47, 0.9),), ((-2 ** 30 + 2 ** 23, 0, 2 ** 30 + 2 ** 23, 47, 0.9),)]
HUGE_BACK = [HUGE[0], ((-2 ** 30 - 2 ** 23, 0, 2 ** 30 - 2 ** 23, 47, 0.9),)]
FAR = HUGE + [()] * 600 + [((2 ** 23, 0, 2 ** 31 - 1, 47, 0.9),)]
# name -> (the tracker's options, the frames): what tests/test_gpu_track_motion.py replays on the device
SCENES = {"acceleration": (dict(motion_gain=256), ACCELERATION), "coasting": (dict(motion_gain=256), COASTING),
          "crossing": (dict(motion_gain=128), CROSSING), "truncation": (dict(motion_gain=256), TRUNCATION), "ema": (dict(motion_gain=64), EMA),
          "first match": (dict(motion_gain=1), [(box(0),), (box(10, 3),), (box(10, 3),)]),
          "dcx clamp": (dict(motion_gain=256, iou_threshold=1e-6), HUGE), "dcx clamp, negative": (dict(motion_gain=256, iou_threshold=1e-6), HUGE_BACK),
          "shift clamp": (dict(motion_gain=256, iou_threshold=1e-6, max_missed=2000), FAR),
          "expiry and rebirth": (dict(motion_gain=256, max_missed=0), [(box(0),), (box(10),), (box(200),), (box(210),), ()])}


def test_tdiv_truncates_toward_zero():
    assert mr.tdiv(-128, 3) == -42 and -128 // 3 == -43
    assert mr.tdiv(-42, 256) == 0 and -42 // 256 == -1
    assert mr.tdiv(7, 2) == 3 and mr.tdiv(-7, 2) == -3 and mr.tdiv(0, 5) == 0 and mr.tdiv(-256, 256) == -1


def test_overlaps_of_the_issue():
    f = np.float32
    assert tk.overlap((0,) + box(0)[:4], (0,) + box(30)[:4], 0) == f(f(864) / f(3744)) < f(0.3)
    assert tk.overlap((0,) + box(0)[:4], (0,) + box(10)[:4], 0) == f(f(1824) / f(2784))
    assert tk.overlap((0,) + box(0)[:4], (0,) + box(40)[:4], 0) == f(f(384) / f(4224))


def test_acceleration_keeps_the_track_with_motion_and_loses_it_without():
    on = mr.Tracker(1, 2, 1, 4, motion_gain=256)
    recs = run(on, ACCELERATION, want_assoc=True)
    assert ids(recs) == [0] * 6
    # the residual is 10 px at every step but the last, where the prediction is exact
    assert [float(r[2][0, 0]["ovr"]) for r in recs[1:]] == [float(np.float32(1824) / np.float32(2784))] * 4 + [1.0]
    vel, pred = on.motion(0)
    assert vel.tolist() == [[40 * 256, 0], [0, 0]]
    assert pred[0].tolist() == (180, 0, 227, 47, np.float32(0.9)) and pred[1].tolist() == (0, 0, 0, 0, 0.0)
    off = mr.Tracker(1, 4, 1, 4)
    assert ids(run(off, ACCELERATION)) == [0, 0, 0, 1, 2, 3]                       # lost at the 30-px step, and at every one after it
    assert off.vel is None                                                        # never switched on: nothing is allocated


def test_coasting_return_is_matched_at_the_predicted_place():
    on = mr.Tracker(1, 2, 1, 4, motion_gain=256)
    recs = run(on, COASTING, want_assoc=True)
    assert ids(recs) == [0, 0, 0, -1, -1, -1, -1, 0]
    a = recs[-1][2][0, 0]
    assert (int(a["how"]), int(a["gap"]), float(a["ovr"])) == (rr.HOW_IOU, 4, 1.0)
    assert on.motion(0)[0][0].tolist() == [8 * 256, 0]                            # raw = 80 * 128 / 5 = 2048 again
    off = mr.Tracker(1, 2, 1, 4)
    assert ids(run(off, COASTING)) == [0, 0, 0, -1, -1, -1, -1, 1]


def test_truncation_toward_zero_in_the_velocity_and_in_the_shift():
    t = mr.Tracker(1, 1, 1, 4, motion_gain=256)
    # case 1: dcx = -1 (x1 one to the left, x2 where it was) at g = 3 -> raw = tdiv(-128, 3) = -42; hits at entry is 1, so v = raw
    run(t, TRUNCATION[:4])
    vel, pred = t.motion(0)
    assert vel[0].tolist() == [-42, 0]
    # case 2: v = -42 at k = 1 -> shift tdiv(-42, 256) = 0, not -1
    assert pred[0].tolist()[:4] == (99, 0, 147, 47)
    assert mr.shift(-42, 0) == 0 and mr.shift(-256, 0) == -1 and mr.shift(-42, 6) == -1


def test_the_ema_at_gain_64_over_three_matches():
    t = mr.Tracker(1, 1, 1, 4, motion_gain=64)
    run(t, [(box(100, 50),), (box(104, 48),)])
    assert t.motion(0)[0][0].tolist() == [1024, -512]                             # the first match takes raw: 8 * 128, -4 * 128
    run(t, [(box(112, 48),)])
    assert t.motion(0)[0][0].tolist() == [1024 + (2048 - 1024) * 64 // 256, -512 + 512 * 64 // 256] == [1280, -384]
    # two absent updates, then g = 3: dcx = -5 (x1 - 3, x2 - 2), dcy = +5 -> raw = (tdiv(-640, 3), tdiv(640, 3)) = (-213, 213)
    run(t, [(), (), ((109, 50, 157, 98, 0.9),)])
    # vx = 1280 + tdiv((-213 - 1280) * 64, 256) = 1280 + tdiv(-95552, 256) = 1280 - 373 (a floor: - 374); vy = -384 + tdiv(597 * 64, 256) = -384 + 149
    assert t.motion(0)[0][0].tolist() == [907, -235]
    assert ids(run(t, [(box(109, 50),)])) == [0]


@pytest.mark.parametrize("gain", [1, 64, 256])
def test_the_first_match_takes_raw_whatever_the_gain(gain):
    t = mr.Tracker(1, 1, 1, 4, motion_gain=gain)
    run(t, [(box(0),), (box(10, 3),)])
    assert t.motion(0)[0][0].tolist() == [2560, 768]
    run(t, [(box(10, 3),)])                                                      # raw 0: v - tdiv(v * gain, 256)
    assert t.motion(0)[0][0].tolist() == [2560 - 2560 * gain // 256, 768 - 768 * gain // 256]


def test_the_clamp_of_the_displacement():
    for sign in (1, -1):
        frames = HUGE if sign > 0 else HUGE_BACK
        t = mr.Tracker(1, 1, 1, 4, iou_threshold=1e-6, motion_gain=256)
        assert ids(run(t, frames)) == [0, 0]
        assert t.motion(0)[0][0].tolist() == [sign * 2 ** 29, 0]                  # dcx = +-2^24 -> +-2^22, * 128
    assert mr.matched_velocity((0, 0), dict(x1=5, x2=2 ** 31 - 1, y1=-2 ** 31, y2=0), dict(x1=-2 ** 31, x2=0, y1=2 ** 31 - 1, y2=9, missed=0, hits=1),
                               256) == (2 ** 29, -2 ** 29)


def test_the_clamp_of_the_shift_and_of_the_coordinates():
    t = mr.Tracker(1, 1, 1, 4, iou_threshold=1e-6, max_missed=2000, motion_gain=256)
    run(t, FAR[:-1])                                                              # v = 2^29: 2^21 px per update, 2^30 after 512
    vel, pred = t.motion(0)
    assert vel[0].tolist() == [2 ** 29, 0] and int(t.slots[0, 0]["missed"]) == 600
    assert mr.shift(2 ** 29, 510) == 511 * 2 ** 21 and mr.shift(2 ** 29, 511) == 2 ** 30 == mr.shift(2 ** 29, 600) == -mr.shift(-2 ** 29, 600)
    assert pred[0].tolist()[:4] == (2 ** 23, 0, 2 ** 31 - 1, 47)                  # x2 = 2^30 + 2^23 + 2^30 meets the int32 clamp
    recs = run(t, FAR[-1:], want_assoc=True)
    assert ids(recs) == [0] and float(recs[0][2][0, 0]["ovr"]) == 1.0 and int(recs[0][2][0, 0]["gap"]) == 600


def test_a_track_live_at_the_switch_the_zeroing_and_reset():
    t = mr.Tracker(1, 2, 1, 4)
    run(t, [(box(0),), (box(10),)])
    t.set_motion(64)                                                              # live with hits 2 and no velocity: the EMA branch
    assert t.vel is None
    run(t, [(box(20),)])
    assert t.motion(0)[0][0].tolist() == [2560 * 64 // 256, 0] == [640, 0]
    t.set_motion(256)                                                             # on -> on keeps
    assert t.motion(0)[0][0].tolist() == [640, 0]
    t.set_motion(0)
    assert t.vel[0, 0].tolist() == [640, 0]                                       # on -> off leaves the array alone
    run(t, [(box(30),)])
    assert t.vel[0, 0].tolist() == [640, 0]                                       # ... and it is neither read nor written while off
    t.set_motion(256)                                                             # off -> on zeroes
    assert t.motion(0)[0].tolist() == [[0, 0], [0, 0]]
    run(t, [(box(40),)])
    assert t.motion(0)[0][0].tolist() == [2560, 0]
    t.reset(0)
    assert t.motion(0)[0].tolist() == [[0, 0], [0, 0]] and not t.slots["live"].any()
    assert ids(run(t, [(box(40),)])) == [1]
    with pytest.raises(AssertionError):
        t.set_motion(257)
    with pytest.raises(AssertionError):
        t.set_motion(-1)


def test_expiry_and_birth_zero_the_velocity():
    t = mr.Tracker(1, 1, 1, 4, max_missed=0, motion_gain=256)
    run(t, [(box(0),), (box(10),)])
    assert t.motion(0)[0][0].tolist() == [2560, 0]
    recs = run(t, [(box(200),)])                                                  # the track expires and the slot is born again in one update
    assert ids(recs) == [1] and t.motion(0)[0][0].tolist() == [0, 0]
    run(t, [(box(210),), ()])
    assert t.motion(0)[0][0].tolist() == [0, 0] and not t.slots["live"].any()


def test_two_faces_crossing_keep_their_ids_with_motion_on():
    for gain in (64, 128, 256):
        t = mr.Tracker(1, 2, 2, 4, motion_gain=gain)
        for rec in run(t, CROSSING):
            assert rec[0][0]["track_id"].tolist() == [0, 1]
    # what overlap alone does with the same scene, computed with track_ref: the two swap their ids at the eighth update and keep them swapped
    ref = tk.Tracker(1, 2, 2, 4)
    got = [ref.update(rr.frame(2, *dets), np.zeros((2, 4), np.float32))[0][0]["track_id"].tolist() for dets in CROSSING]
    assert got == [[0, 1]] * 7 + [[1, 0]] * 7


def test_gain_zero_is_track_reid_ref_answer_for_answer():
    for kw in (dict(), dict(reid_threshold=0.5, iou_min_sim=0.2)):
        a, b = mr.Tracker(3, 4, 3, 8, max_missed=1, **kw), rr.Tracker(3, 4, 3, 8, max_missed=1, **kw)
        for sid, res, emb in rr.soak(11, 3, 3, 8, 25):
            ra, rb = a.update(res, emb, sid, want_assoc=True), b.update(res, emb, sid, want_assoc=True)
            assert all(x.tobytes() == y.tobytes() for x, y in zip(ra, rb))
        assert a.slots.tobytes() == b.slots.tobytes() and a.sums.tobytes() == b.sums.tobytes() and a.vel is None and a.vetoes == b.vetoes


def test_appearance_and_motion_combine():
    """a face leaves its track's box for good: 2b re-attaches it by appearance, reports the PREDICTED box's overlap and updates the velocity"""
    e = np.zeros((1, 4), np.float32)
    e[0, 1] = 1
    t = mr.Tracker(1, 2, 1, 4, reid_threshold=0.5, motion_gain=256)
    for x in (0, 10, 20):
        t.update(rr.frame(1, box(x)), e)
    _, _, assoc = t.update(rr.frame(1, box(70)), e, want_assoc=True)              # predicted at 30: 8 columns of overlap, below 0.3
    a = assoc[0, 0]
    assert int(a["how"]) == rr.HOW_APPEARANCE and float(a["sim"]) == 1.0
    assert a["ovr"] == tk.overlap((0,) + box(70)[:4], (0,) + box(30)[:4], 0) > 0
    assert t.motion(0)[0][0].tolist() == [50 * 256, 0] and int(t.slots[0, 0]["id"]) == 0


def test_the_gate_follows_a_coasting_return_only_with_motion():
    boxes = np.zeros((1, 1), gr.BBOX_DTYPE)
    boxes[0, 0] = box(56)
    for gain, want in ((256, (gr.FOLLOW, 0, 1.0, 0)), (0, (gr.EMBED, -1, 0.0, gr.NO_TRACK))):
        t = mr.Tracker(1, 2, 1, 4, min_hits=2, motion_gain=gain)
        e = np.ones((1, 4), np.float32)
        for dets in COASTING[:-1]:
            t.update(rr.frame(1, *dets), e)
        before = (t.slots.tobytes(), None if t.vel is None else t.vel.tobytes())
        rec, lst, n, pc = mr.tracker_gate(t, boxes, None, None, refresh=1000, min_embeds=1, skip_iou=0.9, max_batch=4)
        assert rec[0, 0].tolist() == want and n == (0 if gain else 1) and lst.tolist() == [-1 if gain else 0] and pc.tolist() == [n]
        assert before == (t.slots.tobytes(), None if t.vel is None else t.vel.tobytes())
    # gain 0 is track_gate_ref's gate
    t = mr.Tracker(1, 2, 1, 4)
    run(t, COASTING[:3])
    assert mr.tracker_gate(t, boxes, None, None, 3, 1, 0.5, 4)[0].tobytes() == gr.gate(t.slots[[0]], boxes, None, 0.3, 3, 3, 1, 0.5, 4)[0].tobytes()
