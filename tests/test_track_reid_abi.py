"""The tracker's appearance entry points (frt_tracker_set_appearance / _get_appearance, frt_tracker_update_assoc / _assoc_dev), the part that needs
no GPU: the symbols and their bindings, the record layout, the setter's range and NaN refusals, and the argument checks of the new update
entries - creation does no device work and every check runs before any, so a refused call returns its status here too and writes nothing."""
import ctypes
import os

import numpy as np

import track_reid_ref as rr
from conftest import ROOT
from test_track_abi import _c_struct, _create

_vp, _i, _f = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
SIGNATURES = {
    "frt_tracker_set_appearance": (_i, [_vp, _f, _f]),
    "frt_tracker_get_appearance": (_i, [_vp, _vp, _vp]),
    "frt_tracker_update_assoc_dev": (_i, [_vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp]),
    "frt_tracker_update_assoc": (_i, [_vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp]),
}


def test_entry_points_are_declared_exported_and_bound(frt):
    header = open(os.path.join(ROOT, "include", "frt.h")).read()
    for name, (res, args) in SIGNATURES.items():
        assert "int %s(" % name in header, name
        fn = getattr(frt.lib, name)
        assert frt.ABI[name] == (res, args) and fn.restype is res and list(fn.argtypes) == args, name
    for decl in ("int frt_tracker_set_appearance(frt_tracker *t, float reid_threshold, float iou_min_sim);",
                 "int frt_tracker_get_appearance(frt_tracker *t, float *reid_threshold_out, float *iou_min_sim_out);",
                 "int frt_tracker_update_assoc_dev(frt_tracker *t, frt_matcher *m, const void *results_dev, const void *embeds_dev, int n_frames,",
                 "int frt_tracker_update_assoc(frt_tracker *t, frt_matcher *m, const frt_face_result *results, const float *embeds, int n_frames,",
                 "#define FRT_TRACK_REID_OFF 2.0f", "#define FRT_TRACK_MIN_SIM_OFF -2.0f", "Nobody has measured S on real faces"):
        assert decl in header, decl
    assert callable(frt.Tracker.setAppearance) and callable(frt.Tracker.getAppearance)
    shell = open(os.path.join(ROOT, "include", "frt", "tracker.h")).read()
    assert "void setAppearance(float reidThreshold, float iouMinSim)" in shell and "void getAppearance(" in shell
    assert "std::vector<frt_track_assoc> &assoc" in shell


def test_assoc_record_layout(frt):
    header = open(os.path.join(ROOT, "include", "frt.h")).read()
    rec = _c_struct(header, "frt_track_assoc")
    assert rec == [("int32_t", "how"), ("int32_t", "gap"), ("float", "ovr"), ("float", "sim")]
    assert frt.TRACK_ASSOC_DTYPE.itemsize == 16 and frt.TRACK_ASSOC_DTYPE == rr.ASSOC_DTYPE
    assert [frt.TRACK_ASSOC_DTYPE.fields[n][1] for _, n in rec] == [0, 4, 8, 12]
    assert [frt.TRACK_ASSOC_DTYPE.fields[n][0] for _, n in rec] == [np.dtype("<i4")] * 2 + [np.dtype("<f4")] * 2
    for k, name in enumerate(("ABSENT", "IOU", "APPEARANCE", "BIRTH", "UNTRACKED")):
        assert "#define FRT_TRACK_ASSOC_%s %d " % (name, k) in header and getattr(frt, "TRACK_ASSOC_" + name) == k
    assert (rr.HOW_ABSENT, rr.HOW_IOU, rr.HOW_APPEARANCE, rr.HOW_BIRTH, rr.HOW_UNTRACKED) == (0, 1, 2, 3, 4)
    assert frt.TRACK_REID_OFF == 2.0 == rr.REID_OFF and frt.TRACK_MIN_SIM_OFF == -2.0 == rr.MIN_SIM_OFF


def _get(frt, h):
    r, m = _f(7.0), _f(7.0)
    assert frt.lib.frt_tracker_get_appearance(h, ctypes.addressof(r), ctypes.addressof(m)) == frt.FRT_OK
    return r.value, m.value


def test_the_setter_checks_ranges_and_a_refused_set_changes_nothing(frt):
    L, INV, OK = frt.lib, frt.FRT_ERR_INVALID, frt.FRT_OK
    rc, h = _create(frt)
    assert rc == OK and _get(frt, h) == (2.0, -2.0)                     # both off by default
    nan = float("nan")
    assert L.frt_tracker_set_appearance(h, 0.5, 0.25) == OK and _get(frt, h) == (0.5, 0.25)
    for bad in ((0.0, 0.2), (-0.5, 0.2), (1.5, 0.2), (nan, 0.2), (0.5, -1.5), (0.5, 1.5), (0.5, nan), (0.5, 2.0), (-2.0, 0.2), (3.0, -2.0), (nan, nan)):
        assert not rr.check_appearance(*bad)
        assert L.frt_tracker_set_appearance(h, *bad) == INV and "tracker" in L.frt_last_error().decode(), bad
        assert _get(frt, h) == (0.5, 0.25), bad                         # a refused call changes nothing, not even the half that was in range
    for ok in ((1.0, -1.0), (2.0 ** -20, 1.0), (2.0, 0.0), (0.25, -2.0), (2.0, -2.0)):
        assert rr.check_appearance(*ok)
        assert L.frt_tracker_set_appearance(h, *ok) == OK and _get(frt, h) == ok, ok
    assert L.frt_tracker_set_appearance(None, 0.5, 0.2) == INV
    r = _f(7.0)
    assert L.frt_tracker_get_appearance(None, ctypes.addressof(r), ctypes.addressof(r)) == INV
    assert L.frt_tracker_get_appearance(h, None, ctypes.addressof(r)) == INV and L.frt_tracker_get_appearance(h, ctypes.addressof(r), None) == INV
    assert r.value == 7.0
    L.frt_tracker_destroy(h)


def test_the_python_shell_maps_none_to_off(frt):
    t = frt.Tracker(2, 4, 3, 8)
    assert t.getAppearance() == (None, None)
    t.setAppearance(0.5, None)
    assert t.getAppearance() == (0.5, None)
    t.setAppearance(iou_min_sim=-0.25)
    assert t.getAppearance() == (None, -0.25)
    try:
        t.setAppearance(1.5, 0.0)
        raise AssertionError("accepted")
    except frt.FrtError as e:
        assert e.code == frt.FRT_ERR_INVALID
    assert t.getAppearance() == (None, -0.25)
    t.close()
    t = frt.Tracker(2, 4, 3, 8, reid_threshold=0.75, iou_min_sim=0.5)
    assert t.getAppearance() == (0.75, 0.5)
    t.close()
    try:
        frt.Tracker(2, 4, 3, 8, reid_threshold=-1.0)
        raise AssertionError("accepted")
    except frt.FrtError as e:
        assert e.code == frt.FRT_ERR_INVALID


def test_bad_arguments_of_the_assoc_updates_are_refused_before_any_device_work(frt):
    L = frt.lib
    INV, CAP = frt.FRT_ERR_INVALID, frt.FRT_ERR_CAPACITY
    rc, h = _create(frt)
    assert rc == frt.FRT_OK and L.frt_tracker_set_appearance(h, 0.5, 0.2) == frt.FRT_OK
    MF, D = 3, 8
    res = np.zeros(300 * MF, frt.RESULT_DTYPE)
    emb = np.zeros((300 * MF, D), np.float32)
    trk = np.full(300 * MF * 32, 0x55, np.uint8).view(frt.TRACK_DTYPE)
    tpl = np.full((300 * MF, D), 7.5, np.float32)
    assoc = np.full(300 * MF * 16, 0x55, np.uint8).view(frt.TRACK_ASSOC_DTYPE)
    trk0, tpl0, assoc0 = trk.tobytes(), tpl.tobytes(), assoc.tobytes()

    def update(t=h, m=None, r=res.ctypes.data, e=emb.ctypes.data, n=2, ids=None, out=trk.ctypes.data, tp=tpl.ctypes.data, a=assoc.ctypes.data, dev=False):
        ids_p = np.asarray(ids, np.int32).ctypes.data if ids is not None else None
        if dev:
            return L.frt_tracker_update_assoc_dev(t, m, r, e, n, ids_p, out, tp, a, None)
        return L.frt_tracker_update_assoc(t, m, r, e, n, ids_p, out, tp, a)

    for dev in (False, True):
        for a in (assoc.ctypes.data, None):                              # assoc may be NULL: the checks are the plain update's either way
            for kw in (dict(t=None), dict(r=None), dict(e=None), dict(out=None)):
                assert update(dev=dev, a=a, **kw) == INV, kw
            assert update(dev=dev, a=a, n=0) == INV and update(dev=dev, a=a, n=-1) == INV
            assert update(dev=dev, a=a, n=257) == CAP and "256" in L.frt_last_error().decode()
            assert update(dev=dev, a=a, n=4) == INV
            assert update(dev=dev, a=a, ids=[0, 3]) == INV and "outside" in L.frt_last_error().decode()
            assert update(dev=dev, a=a, ids=[1, 1]) == INV and "twice" in L.frt_last_error().decode()
    assert update(dev=True, e=emb.ctypes.data + 4) == INV and "aligned" in L.frt_last_error().decode()
    assert update(dev=True, tp=tpl.ctypes.data + 8) == INV
    assert trk.tobytes() == trk0 and tpl.tobytes() == tpl0 and assoc.tobytes() == assoc0
    L.frt_tracker_destroy(h)
