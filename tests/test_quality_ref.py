"""tests/quality_ref.py - the numpy restatement of include/frt.h "Face quality" that the device code is compared with - against cases worked
out by hand."""
import numpy as np

import quality_ref as qr


def _rec(x1=10, y1=20, x2=70, y2=60, score=0.9, valid=1):
    r = np.zeros((), qr.RESULT_DTYPE)
    r["x1"], r["y1"], r["x2"], r["y2"], r["score"], r["valid"] = x1, y1, x2, y2, score, valid
    return r


def test_record_layout():
    assert qr.QUALITY_DTYPE.itemsize == 56
    assert {n: qr.QUALITY_DTYPE.fields[n][1] for n in qr.QUALITY_DTYPE.names} == qr.OFFSETS
    assert list(qr.QUALITY_DTYPE.names) == ["sum_y", "sum_y2", "sum_lap", "n_dark", "n_bright", "size", "sum_lap2", "mean", "luma_var", "sharpness",
                                            "score", "flags", "present"]
    assert qr.N == 12544 and qr.M == 12100 and qr.ENROL_LOW_QUALITY == 5


def test_constant_crops():
    q = qr.quality_one(qr.constant(255, 255, 255))
    assert (q["sum_y"], q["sum_y2"], q["sum_lap"], q["sum_lap2"]) == (12544 * 255, 815673600, 0, 0)
    assert (q["n_dark"], q["n_bright"]) == (0, 12544)
    assert q["mean"] == np.float32(255) and q["luma_var"] == 0 and q["sharpness"] == 0 and q["present"] == 1 and q["flags"] == 0
    z = qr.quality_one(qr.constant(0, 0, 0))
    assert (z["sum_y"], z["sum_y2"], z["sum_lap"], z["sum_lap2"], z["n_dark"], z["n_bright"]) == (0, 0, 0, 0, 12544, 0)
    assert z["mean"] == 0 and z["luma_var"] == 0 and z["sharpness"] == 0 and z["present"] == 1
    assert z.tobytes() != bytes(56)                      # present: not the absent slot's record


def test_checkerboard():
    q = qr.quality_one(qr.checkerboard())
    assert q["sum_y"] == 1599360 and q["sum_y2"] == 6272 * 255 * 255
    assert q["sum_lap"] == 0 and q["sum_lap2"] == 12588840000 and int(q["sum_lap2"]) > 2 ** 32
    assert q["luma_var"] == np.float32(16256.25) and q["sharpness"] == np.float32(1040400.0) and q["mean"] == np.float32(127.5)
    assert q["n_dark"] == 6272 and q["n_bright"] == 6272


def test_pure_colours():
    for bgr, y in (((255, 0, 0), 29), ((0, 255, 0), 149), ((0, 0, 255), 77)):
        assert (qr.luma(qr.constant(*bgr)) == y).all()
        assert qr.quality_one(qr.constant(*bgr))["sum_y"] == 12544 * y
    assert (qr.luma(qr.constant(255, 255, 255)) == 255).all()


def test_the_border_has_no_laplacian():
    assert qr.quality_one(qr.single_pixel(0, 0))["sum_lap2"] == 0
    assert qr.quality_one(qr.single_pixel(111, 111))["sum_lap2"] == 0
    inner = qr.quality_one(qr.single_pixel(1, 1))
    assert inner["sum_lap2"] == 1020 * 1020 + 2 * 255 * 255 and inner["sum_lap"] == 1020 - 2 * 255   # itself and its two interior neighbours
    edge = qr.quality_one(qr.single_pixel(0, 1))
    assert edge["sum_lap2"] == 255 * 255 and edge["sum_lap"] == -255                               # only through (1, 1) below it
    mid = qr.quality_one(qr.single_pixel(50, 60))
    assert mid["sum_lap2"] == 1020 * 1020 + 4 * 255 * 255 and mid["sum_lap"] == 0


def test_each_flag_alone_and_equality_passes():
    crop, rec = qr.noise(), _rec()
    base = qr.quality_one(crop, rec)
    assert base["flags"] == 0 and base["present"] == 1 and base["size"] == 40 and base["score"] == np.float32(0.9)
    clipped = int(base["n_dark"]) + int(base["n_bright"])
    assert clipped > 0
    up = lambda v: float(np.nextafter(np.float32(v), np.float32(np.inf)))    # noqa: E731
    down = lambda v: float(np.nextafter(np.float32(v), np.float32(-np.inf)))  # noqa: E731
    cases = [
        (qr.SMALL, dict(min_size=41), dict(min_size=40)),
        (qr.BLURRED, dict(min_sharpness=up(base["sharpness"])), dict(min_sharpness=float(base["sharpness"]))),
        (qr.FLAT, dict(min_luma_var=up(base["luma_var"])), dict(min_luma_var=float(base["luma_var"]))),
        (qr.DARK, dict(min_mean=up(base["mean"])), dict(min_mean=float(base["mean"]))),
        (qr.BRIGHT, dict(max_mean=down(base["mean"])), dict(max_mean=float(base["mean"]))),
        (qr.CLIPPED, dict(max_clipped=clipped - 1), dict(max_clipped=clipped)),
        (qr.LOW_SCORE, dict(min_score=up(np.float32(0.9))), dict(min_score=float(np.float32(0.9)))),
    ]
    for bit, raising, equal in cases:
        assert qr.quality_one(crop, rec, qr.options(**raising))["flags"] == bit, qr.FLAG_NAMES[bit]
        assert qr.quality_one(crop, rec, qr.options(**equal))["flags"] == 0, qr.FLAG_NAMES[bit]
        assert not qr.passes(qr.quality_one(crop, rec, qr.options(**raising))) and qr.passes(qr.quality_one(crop, rec, qr.options(**equal)))


def test_without_records_small_and_low_score_are_never_raised():
    q = qr.quality_one(qr.noise(), None, qr.options(min_size=1000, min_score=2.0))
    assert q["flags"] == 0 and q["size"] == 0 and q["score"] == 0 and q["present"] == 1
    q = qr.quality_one(qr.noise(), _rec(), qr.options(min_size=1000, min_score=2.0))
    assert q["flags"] == qr.SMALL | qr.LOW_SCORE


def test_an_absent_slot_is_56_zero_bytes():
    q = qr.quality_one(qr.noise(), _rec(valid=0), qr.options(min_size=1000, min_sharpness=1e9))
    assert q.tobytes() == bytes(56) and not qr.passes(q)
    both = qr.quality(np.stack([qr.noise(), qr.noise()]), np.array([_rec(valid=0), _rec()]))
    assert both[0].tobytes() == bytes(56) and both[1]["present"] == 1


def test_blur_lowers_the_sharpness():
    sharp, soft = qr.quality_one(qr.noise()), qr.quality_one(qr.box_blur5(qr.noise()))
    assert sharp["sharpness"] > 20000 and soft["sharpness"] < 1000       # (about 49 600 against about 200: any threshold between separates them)
    one = qr.quality_one(qr.one_channel_constant())
    assert one["present"] == 1 and 0 < one["sharpness"] < sharp["sharpness"]


def test_the_gate_looks_at_slot_0_only():
    res = np.zeros((4, 2), qr.RESULT_DTYPE)
    res[:, 0]["score"], res[:, 0]["valid"] = 0.8, 1            # four frames with one valid face each
    res[3, 0]["valid"] = 0                                     # ... the last one an empty ROI
    ql = np.zeros((4, 2), qr.QUALITY_DTYPE)
    ql[1, 0]["flags"] = qr.BLURRED
    ql[2, 1]["flags"] = qr.DARK                                # slot 1: not looked at
    ql[3, 0]["flags"] = qr.FLAT                                # not OK in the first place
    assert list(qr.enrol_select(res)) == [1, 1, 1, 4]
    assert list(qr.enrol_select(res, ql)) == [1, 5, 1, 4]
