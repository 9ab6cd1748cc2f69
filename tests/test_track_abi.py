"""Face tracker (frt_tracker_* / frt_pipeline_run_tracked), the part that needs no GPU: the symbols and their bindings, the record layouts, and
the argument checks - every one of them runs before any device work, so on a machine without a device a refused call returns its status
(not FRT_ERR_DEVICE) and leaves the output buffers' sentinel bytes alone."""
import ctypes
import os
import re

import numpy as np

import track_ref as tk
from conftest import ROOT

_vp, _i = ctypes.c_void_p, ctypes.c_int
SIGNATURES = {
    "frt_tracker_create": (_i, [_i, _i, _i, _i, _vp, _i, ctypes.POINTER(_vp)]),
    "frt_tracker_destroy": (None, [_vp]),
    "frt_tracker_update_dev": (_i, [_vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp]),
    "frt_tracker_update": (_i, [_vp, _vp, _vp, _vp, _i, _vp, _vp, _vp]),
    "frt_tracker_tracks": (_i, [_vp, _i, _vp, _vp, _vp]),
    "frt_tracker_reset": (_i, [_vp, _i]),
    "frt_pipeline_run_tracked": (_i, [_vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp]),
}


def test_entry_points_are_declared_exported_and_bound(frt):
    header = open(os.path.join(ROOT, "include", "frt.h")).read()
    for name, (res, args) in SIGNATURES.items():
        assert "%s %s(" % ("void" if res is None else "int", name) in header, name
        fn = getattr(frt.lib, name)
        assert frt.ABI[name] == (res, args) and fn.restype is res and list(fn.argtypes) == args, name
    for decl in ("int frt_tracker_create(int n_streams, int max_tracks, int max_faces, int dim, const frt_track_options *options, int device, frt_tracker **out);",
                 "int frt_tracker_update_dev(frt_tracker *t, frt_matcher *m, const void *results_dev, const void *embeds_dev, int n_frames,",
                 "int frt_pipeline_run_tracked(frt_pipeline *p, frt_tracker *t, const uint8_t *frames, int n_frames, const int32_t *stream_ids,",
                 "Face tracker"):
        assert decl in header, decl
    assert callable(frt.Tracker.update) and callable(frt.Tracker.updateDev) and callable(frt.Tracker.tracks) and callable(frt.Tracker.reset)
    assert callable(frt.Pipeline.runTracked)
    shell = open(os.path.join(ROOT, "include", "frt", "tracker.h")).read()
    assert "class FaceTracker" in shell and "trackFaces(" in open(os.path.join(ROOT, "include", "frt", "arcface.h")).read()


def _c_struct(header, name):
    """the fields of `typedef struct name { ... } name;` in declaration order -> [(ctype, field)]"""
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for stmt in body.split(";"):
        stmt = stmt.strip()
        if stmt:
            ctype, names = stmt.split(None, 1)
            out += [(ctype, n.strip()) for n in names.split(",")]
    return out


def test_record_layouts(frt):
    header = open(os.path.join(ROOT, "include", "frt.h")).read()
    res = _c_struct(header, "frt_track_result")
    assert res == [("int32_t", n) for n in ("track_id", "slot", "age", "hits", "n_embeds", "confirmed", "match_idx")] + [("float", "match_sim")]
    assert frt.TRACK_DTYPE.itemsize == 32 and frt.TRACK_DTYPE == tk.TRACK_DTYPE
    assert [frt.TRACK_DTYPE.fields[n][1] for _, n in res] == list(range(0, 32, 4))       # the field offsets
    assert [frt.TRACK_DTYPE.fields[n][0] for _, n in res] == [np.dtype("<i4")] * 7 + [np.dtype("<f4")]
    st = _c_struct(header, "frt_track_state")
    assert [n for _, n in st] == ["live", "id", "box", "born", "hits", "missed", "n_embeds", "match_idx", "match_sim"]
    flat = [n for n in frt.TRACK_STATE_DTYPE.names]
    assert flat == ["live", "id", "x1", "y1", "x2", "y2", "score", "born", "hits", "missed", "n_embeds", "match_idx", "match_sim"]
    assert frt.TRACK_STATE_DTYPE.itemsize == 52 and frt.TRACK_STATE_DTYPE == tk.STATE_DTYPE and frt.RESULT_DTYPE == tk.RESULT_DTYPE
    assert [frt.TRACK_STATE_DTYPE.fields[n][1] for n in flat] == list(range(0, 52, 4))
    opt = _c_struct(header, "frt_track_options")
    assert opt == [("float", "iou_threshold"), ("int32_t", "max_missed"), ("int32_t", "min_hits"), ("float", "decay")]
    assert [f[0] for f in frt.TrackOptions._fields_] == [n for _, n in opt] and ctypes.sizeof(frt.TrackOptions) == 16


def _create(frt, n_streams=3, max_tracks=4, max_faces=3, dim=8, opt=None, device=0):
    h = _vp()
    rc = frt.lib.frt_tracker_create(n_streams, max_tracks, max_faces, dim, ctypes.addressof(opt) if opt is not None else None, device, ctypes.byref(h))
    return rc, h


def test_create_checks_ranges_and_options_without_a_device(frt):
    L, INV = frt.lib, frt.FRT_ERR_INVALID
    assert L.frt_tracker_create(3, 4, 3, 8, None, 0, None) == INV
    for kw in (dict(n_streams=0), dict(n_streams=1025), dict(max_tracks=0), dict(max_tracks=65), dict(max_faces=0), dict(max_faces=65), dict(dim=0),
               dict(dim=6), dict(dim=2052), dict(device=-1)):
        rc, h = _create(frt, **kw)
        assert rc == INV and not h.value, kw
    T = frt.TrackOptions
    for bad in (T(0.0, 5, 3, 1.0), T(-0.1, 5, 3, 1.0), T(1.5, 5, 3, 1.0), T(float("nan"), 5, 3, 1.0), T(0.3, -1, 3, 1.0), T(0.3, 5, 0, 1.0),
                T(0.3, 5, 3, 0.0), T(0.3, 5, 3, 1.25), T(0.3, 5, 3, float("nan"))):
        rc, h = _create(frt, opt=bad)
        assert rc == INV and not h.value and "tracker" in L.frt_last_error().decode()
    for kw in (dict(), dict(n_streams=1024, max_tracks=64, max_faces=64, dim=2048), dict(opt=T(1.0, 0, 1, 1.0)), dict(opt=T(1e-6, 5, 3, 0.5))):
        rc, h = _create(frt, **kw)   # (creation does no device work: it succeeds here too)
        assert rc == frt.FRT_OK and h.value, kw
        L.frt_tracker_destroy(h)
    L.frt_tracker_destroy(None)


def test_bad_arguments_are_refused_before_any_device_work(frt):
    L = frt.lib
    INV, CAP = frt.FRT_ERR_INVALID, frt.FRT_ERR_CAPACITY
    rc, h = _create(frt)
    assert rc == frt.FRT_OK
    MF, D = 3, 8
    res = np.zeros(300 * MF, frt.RESULT_DTYPE)
    emb = np.zeros((300 * MF, D), np.float32)
    trk = np.full(300 * MF, 0x55, np.uint8).view(np.uint8).repeat(32).view(frt.TRACK_DTYPE)
    tpl = np.full((300 * MF, D), 7.5, np.float32)
    trk0, tpl0 = trk.tobytes(), tpl.tobytes()

    def update(t=h, m=None, r=res.ctypes.data, e=emb.ctypes.data, n=2, ids=None, out=trk.ctypes.data, tp=tpl.ctypes.data, dev=False):
        ids_p = np.asarray(ids, np.int32).ctypes.data if ids is not None else None
        if dev:
            return L.frt_tracker_update_dev(t, m, r, e, n, ids_p, out, tp, None)
        return L.frt_tracker_update(t, m, r, e, n, ids_p, out, tp)

    for dev in (False, True):
        # ---- NULL pointers and ranges
        for kw in (dict(t=None), dict(r=None), dict(e=None), dict(out=None)):
            assert update(dev=dev, **kw) == INV, kw
        assert update(dev=dev, n=0) == INV and update(dev=dev, n=-1) == INV
        assert update(dev=dev, n=257) == CAP and "256" in L.frt_last_error().decode()
        assert update(dev=dev, n=300, ids=list(range(300))) == CAP
        # ---- stream ids: outside 0 .. n_streams - 1 (3 streams; NULL means frame i is stream i), or twice
        assert update(dev=dev, n=4) == INV
        assert update(dev=dev, ids=[0, 3]) == INV and "outside" in L.frt_last_error().decode()
        assert update(dev=dev, ids=[-1, 0]) == INV
        assert update(dev=dev, ids=[1, 1]) == INV and "twice" in L.frt_last_error().decode()
        assert update(dev=dev, n=3, ids=[2, 0, 2]) == INV
    assert update(dev=True, e=emb.ctypes.data + 4) == INV and "aligned" in L.frt_last_error().decode()
    assert update(dev=True, tp=tpl.ctypes.data + 8) == INV
    assert trk.tobytes() == trk0 and tpl.tobytes() == tpl0

    # ---- frt_tracker_tracks / frt_tracker_reset
    slots = np.full(4, 0x55, np.uint8).repeat(52).view(frt.TRACK_STATE_DTYPE)
    cnt = np.full(3, -7, np.int32)
    s0 = slots.tobytes()
    assert L.frt_tracker_tracks(None, 0, slots.ctypes.data, None, cnt.ctypes.data) == INV
    assert L.frt_tracker_tracks(h, 0, None, None, cnt.ctypes.data) == INV
    assert L.frt_tracker_tracks(h, -1, slots.ctypes.data, None, cnt.ctypes.data) == INV
    assert L.frt_tracker_tracks(h, 3, slots.ctypes.data, None, cnt.ctypes.data) == INV
    assert slots.tobytes() == s0 and (cnt == -7).all()
    assert L.frt_tracker_reset(None, 0) == INV and L.frt_tracker_reset(h, -2) == INV and L.frt_tracker_reset(h, 3) == INV

    # ---- frt_pipeline_run_tracked: a NULL pipeline / tracker
    frames = np.zeros((2, 4, 4, 3), np.uint8)
    r2 = np.full(2 * MF, 0x55, np.uint8).repeat(36).view(frt.RESULT_DTYPE)
    r0 = r2.tobytes()
    assert L.frt_pipeline_run_tracked(None, h, frames.ctypes.data, 2, None, r2.ctypes.data, trk.ctypes.data, emb.ctypes.data, tpl.ctypes.data) == INV
    assert L.frt_pipeline_run_tracked(None, None, frames.ctypes.data, 2, None, r2.ctypes.data, trk.ctypes.data, None, None) == INV
    assert r2.tobytes() == r0 and trk.tobytes() == trk0 and tpl.tobytes() == tpl0 and not emb.any()
    L.frt_tracker_destroy(h)
