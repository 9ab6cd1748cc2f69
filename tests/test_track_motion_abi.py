"""The tracker's motion entry points (frt_tracker_set_motion / _get_motion / frt_tracker_motion), the part that needs no GPU: the symbols and
their bindings, every refusal with sentinel bytes in the outputs, and the set / get round trip on a tracker that has never touched a device
- creation does no device work, switching motion on before the state exists does none either, and every check runs before any."""
import ctypes
import os

import numpy as np

import track_motion_ref as mr
from conftest import ROOT
from test_track_abi import _create

_vp, _i = ctypes.c_void_p, ctypes.c_int
SIGNATURES = {
    "frt_tracker_set_motion": (_i, [_vp, _i]),
    "frt_tracker_get_motion": (_i, [_vp, _vp]),
    "frt_tracker_motion": (_i, [_vp, _i, _vp, _vp]),
}


def test_entry_points_are_declared_exported_and_bound(frt):
    header = open(os.path.join(ROOT, "include", "frt.h")).read()
    for name, (res, args) in SIGNATURES.items():
        assert "int %s(" % name in header, name
        fn = getattr(frt.lib, name)
        assert frt.ABI[name] == (res, args) and fn.restype is res and list(fn.argtypes) == args, name
    for decl in ("int frt_tracker_set_motion(frt_tracker *t, int gain);", "int frt_tracker_get_motion(frt_tracker *t, int *gain_out);",
                 "int frt_tracker_motion(frt_tracker *t, int stream, int32_t *vel_out, frt_bbox *pred_out /* may be NULL */);",
                 "Motion (frt_tracker_set_motion; off by default", "Nobody has measured a gain on real video"):
        assert decl in header, decl
    assert callable(frt.Tracker.setMotion) and callable(frt.Tracker.getMotion) and callable(frt.Tracker.motion)


def _get(frt, h):
    g = _i(-7)
    assert frt.lib.frt_tracker_get_motion(h, ctypes.addressof(g)) == frt.FRT_OK
    return g.value


def test_the_setter_checks_its_range_and_a_refused_set_changes_nothing(frt):
    L, INV, OK = frt.lib, frt.FRT_ERR_INVALID, frt.FRT_OK
    rc, h = _create(frt)
    assert rc == OK and _get(frt, h) == 0                                # off by default
    assert L.frt_tracker_set_motion(h, 64) == OK and _get(frt, h) == 64
    for bad in (-1, 257, -256, 2 ** 31 - 1, -2 ** 31):
        assert not mr.check_gain(bad)
        assert L.frt_tracker_set_motion(h, bad) == INV and "tracker motion" in L.frt_last_error().decode(), bad
        assert _get(frt, h) == 64, bad
    for ok in (1, 256, 0, 255, 0, 0):                                    # on -> on, on -> off, off -> on, off -> off: none needs a device here
        assert mr.check_gain(ok)
        assert L.frt_tracker_set_motion(h, ok) == OK and _get(frt, h) == ok, ok
    assert L.frt_tracker_set_motion(None, 64) == INV
    g = _i(-7)
    assert L.frt_tracker_get_motion(None, ctypes.addressof(g)) == INV and L.frt_tracker_get_motion(h, None) == INV and g.value == -7
    L.frt_tracker_destroy(h)


def test_the_accessor_refuses_before_any_device_work_and_writes_nothing(frt):
    L, INV, OK = frt.lib, frt.FRT_ERR_INVALID, frt.FRT_OK
    rc, h = _create(frt)                                                 # 3 streams, 4 tracks
    assert rc == OK
    vel = np.full(4 * 2 * 4, 0x55, np.uint8).view(np.int32)
    pred = np.full(4 * 20, 0x55, np.uint8).view(frt.BBOX_DTYPE)
    vel0, pred0 = vel.tobytes(), pred.tobytes()
    v, p = vel.ctypes.data, pred.ctypes.data
    assert L.frt_tracker_motion(h, 0, v, p) == INV and "off" in L.frt_last_error().decode()      # while motion is off
    assert L.frt_tracker_motion(h, 0, v, None) == INV
    assert L.frt_tracker_set_motion(h, 128) == OK
    assert L.frt_tracker_motion(None, 0, v, p) == INV
    assert L.frt_tracker_motion(h, 0, None, p) == INV
    for stream in (-1, 3, 1024):
        assert L.frt_tracker_motion(h, stream, v, p) == INV and "stream" in L.frt_last_error().decode(), stream
    assert L.frt_tracker_set_motion(h, 0) == OK
    assert L.frt_tracker_motion(h, 1, v, p) == INV                                               # on -> off: refused again
    assert vel.tobytes() == vel0 and pred.tobytes() == pred0
    L.frt_tracker_destroy(h)


def test_the_python_shell_maps_none_to_off(frt):
    t = frt.Tracker(2, 4, 3, 8)
    assert t.getMotion() == 0
    t.setMotion(200)
    assert t.getMotion() == 200
    try:
        t.setMotion(300)
        raise AssertionError("accepted")
    except frt.FrtError as e:
        assert e.code == frt.FRT_ERR_INVALID
    assert t.getMotion() == 200
    t.setMotion(None)
    assert t.getMotion() == 0
    try:
        t.motion(0)
        raise AssertionError("accepted")
    except frt.FrtError as e:
        assert e.code == frt.FRT_ERR_INVALID
    t.close()
    t = frt.Tracker(2, 4, 3, 8, motion_gain=256, reid_threshold=0.5)
    assert t.getMotion() == 256 and t.getAppearance() == (0.5, None)
    t.close()
    try:
        frt.Tracker(2, 4, 3, 8, motion_gain=-1)
        raise AssertionError("accepted")
    except frt.FrtError as e:
        assert e.code == frt.FRT_ERR_INVALID
