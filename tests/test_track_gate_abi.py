"""The gate's entry points (frt_tracker_gate / _gate_dev, frt_pipeline_run_tracked_gated), the part that needs no GPU: the symbols and their
bindings, the layouts of frt_track_gate and frt_track_gate_options against the header, and every refusal - creation does no device work and
every check runs before any, so a refused call returns its status here too and writes nothing (the outputs keep their sentinel bytes).  The
pipeline entry's refusals that need a pipeline are in tests/test_gpu_track_gate.py."""
import ctypes
import os

import numpy as np

import track_gate_ref as gr
from conftest import ROOT
from test_track_abi import _c_struct, _create

_vp, _i = ctypes.c_void_p, ctypes.c_int
SIGNATURES = {
    "frt_tracker_gate_dev": (_i, [_vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _i, _vp]),
    "frt_tracker_gate": (_i, [_vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _i]),
    "frt_pipeline_run_tracked_gated": (_i, [_vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
}


def _header():
    return open(os.path.join(ROOT, "include", "frt.h")).read()


def test_entry_points_are_declared_exported_and_bound(frt):
    header = _header()
    for name, (res, args) in SIGNATURES.items():
        assert "int %s(" % name in header, name
        fn = getattr(frt.lib, name)
        assert frt.ABI[name] == (res, args) and fn.restype is res and list(fn.argtypes) == args, name
    for text in ("int frt_tracker_gate_dev(frt_tracker *t, const frt_track_gate_options *options, const void *boxes_dev, const void *n_boxes_dev, int n_frames,",
                 "int frt_tracker_gate(frt_tracker *t, const frt_track_gate_options *options, const frt_bbox *boxes, const int32_t *n_boxes /* may be NULL */,",
                 "int frt_pipeline_run_tracked_gated(frt_pipeline *p, frt_tracker *t, const frt_track_gate_options *options, const uint8_t *frames, int n_frames,",
                 "tests/track_gate_ref.py", "The peek is a PREDICTION, not a promise", "NO defaults and no recommended values"):
        assert text in header, text
    assert callable(frt.Tracker.gate) and callable(frt.Tracker.gateDev) and callable(frt.Pipeline.runTrackedGated)
    shell = open(os.path.join(ROOT, "include", "frt", "tracker.h")).read()
    assert "gate(" in shell and "frt_track_gate_options" in shell
    arc = open(os.path.join(ROOT, "include", "frt", "arcface.h")).read()
    assert "frt_pipeline_run_tracked_gated" in arc


def test_record_and_option_layouts(frt):
    header = _header()
    rec = _c_struct(header, "frt_track_gate")
    assert rec == [("int32_t", "decision"), ("int32_t", "slot"), ("float", "ovr"), ("int32_t", "why")]
    assert frt.TRACK_GATE_DTYPE.itemsize == 16 and frt.TRACK_GATE_DTYPE == gr.GATE_DTYPE
    assert [frt.TRACK_GATE_DTYPE.fields[n][1] for _, n in rec] == [0, 4, 8, 12]
    assert [frt.TRACK_GATE_DTYPE.fields[n][0] for _, n in rec] == [np.dtype("<i4"), np.dtype("<i4"), np.dtype("<f4"), np.dtype("<i4")]
    opt = _c_struct(header, "frt_track_gate_options")
    assert opt == [("int32_t", "refresh"), ("int32_t", "min_embeds"), ("float", "skip_iou")]
    O = frt.TrackGateOptions
    assert [(n, getattr(O, n).offset) for n, _ in O._fields_] == [("refresh", 0), ("min_embeds", 4), ("skip_iou", 8)] and ctypes.sizeof(O) == 12
    assert [t for _, t in O._fields_] == [ctypes.c_int32, ctypes.c_int32, ctypes.c_float]
    for k, name in enumerate(("ABSENT", "EMBED", "FOLLOW")):
        assert "#define FRT_TRACK_GATE_%s %d\n" % (name, k) in header and getattr(frt, "TRACK_GATE_" + name) == k
    for name, bit in (("NO_TRACK", 1), ("UNCONFIRMED", 2), ("FEW_EMBEDS", 4), ("LOW_OVERLAP", 8), ("REFRESH", 16)):
        assert "#define FRT_TRACK_GATE_%s %d\n" % (name, bit) in header and getattr(frt, "TRACK_GATE_" + name) == bit == getattr(gr, name)
    assert gr.BBOX_DTYPE == frt.BBOX_DTYPE and (gr.ABSENT, gr.EMBED, gr.FOLLOW) == (0, 1, 2)


BAD_OPTIONS = ((0, 1, 0.5), (-1, 1, 0.5), (1, 0, 0.5), (1, -2, 0.5), (1, 1, 0.0), (1, 1, -0.5), (1, 1, 1.5), (1, 1, float("nan")), (0, 0, 2.0))


def test_bad_arguments_of_the_gate_are_refused_before_any_device_work(frt):
    L = frt.lib
    INV, CAP = frt.FRT_ERR_INVALID, frt.FRT_ERR_CAPACITY
    rc, h = _create(frt)
    assert rc == frt.FRT_OK
    MF = 3
    boxes = np.zeros(300 * MF, frt.BBOX_DTYPE)
    nb = np.full(300, MF, np.int32)
    gate = np.full(300 * MF * 16, 0x55, np.uint8).view(frt.TRACK_GATE_DTYPE)
    lst = np.full(300 * MF, 0x55555555, np.int32)
    cnt = np.full(1, 0x55555555, np.int32)
    pc = np.full(300 * MF, 0x55555555, np.int32)
    sentinel = [x.tobytes() for x in (gate, lst, cnt, pc)]
    good = frt.TrackGateOptions(4, 2, 0.5)

    def call(t=h, o=good, b=boxes.ctypes.data, n_b=nb.ctypes.data, n=2, ids=None, g=gate.ctypes.data, li=lst.ctypes.data, c=cnt.ctypes.data,
             p=pc.ctypes.data, mb=4, dev=False):
        ids_p = np.asarray(ids, np.int32).ctypes.data if ids is not None else None
        o_p = ctypes.addressof(o) if o is not None else None
        if dev:
            return L.frt_tracker_gate_dev(t, o_p, b, n_b, n, ids_p, g, li, c, p, mb, None)
        return L.frt_tracker_gate(t, o_p, b, n_b, n, ids_p, g, li, c, p, mb)

    for dev in (False, True):
        for kw in (dict(t=None), dict(b=None), dict(g=None), dict(li=None), dict(c=None), dict(p=None)):
            assert call(dev=dev, **kw) == INV and "null" in L.frt_last_error().decode(), kw
        assert call(dev=dev, o=None) == INV and "no defaults" in L.frt_last_error().decode()      # there are no defaults
        for bad in BAD_OPTIONS:
            assert not gr.check_options(*bad)
            assert call(dev=dev, o=frt.TrackGateOptions(*bad)) == INV and "tracker gate" in L.frt_last_error().decode(), bad
        assert call(dev=dev, mb=0) == INV and call(dev=dev, mb=-4) == INV
        assert call(dev=dev, n=0) == INV and call(dev=dev, n=-1) == INV
        assert call(dev=dev, n=257) == CAP and "256" in L.frt_last_error().decode()
        assert call(dev=dev, n=4) == INV                                                           # stream 3 of a tracker for 3
        assert call(dev=dev, ids=[0, 3]) == INV and "outside" in L.frt_last_error().decode()
        assert call(dev=dev, ids=[1, 1]) == INV and "twice" in L.frt_last_error().decode()
    assert [x.tobytes() for x in (gate, lst, cnt, pc)] == sentinel
    L.frt_tracker_destroy(h)


def test_the_pipeline_entry_refuses_nulls_and_missing_options_before_it_looks_at_anything(frt):
    L, INV = frt.lib, frt.FRT_ERR_INVALID
    rc, h = _create(frt)
    assert rc == frt.FRT_OK
    frames = np.zeros((1, 8, 8, 3), np.uint8)
    res = np.full(64, 0x55, np.uint8)
    trk = np.full(64, 0x55, np.uint8)
    ne = np.full(1, 0x55555555, np.int32)
    good = frt.TrackGateOptions(4, 2, 0.5)
    # without a pipeline every call ends at the null check; the tracker alone is not enough
    for p, t, o, f, r, k, n in ((None, h, good, frames, res, trk, ne), (None, None, good, frames, res, trk, ne), (None, h, None, frames, res, trk, ne),
                                (None, h, good, None, res, trk, ne), (None, h, good, frames, None, trk, ne), (None, h, good, frames, res, None, ne),
                                (None, h, good, frames, res, trk, None)):
        rc = L.frt_pipeline_run_tracked_gated(p, t, ctypes.addressof(o) if o is not None else None, f.ctypes.data if f is not None else None, 1, None,
                                              r.ctypes.data if r is not None else None, k.ctypes.data if k is not None else None, None, None, None, None,
                                              n.ctypes.data if n is not None else None)
        assert rc == INV and "runTrackedGated" in L.frt_last_error().decode()
    assert (res == 0x55).all() and (trk == 0x55).all() and ne[0] == 0x55555555
    L.frt_tracker_destroy(h)


def test_the_python_shell_checks_shapes(frt):
    t = frt.Tracker(2, 4, 3, 8)
    for bad in (np.zeros(0, frt.BBOX_DTYPE), np.zeros(4, frt.BBOX_DTYPE)):
        try:
            t.gate(bad, 4, 2, 0.5)
            raise AssertionError("accepted")
        except ValueError:
            pass
    try:
        t.gate(np.zeros(6, frt.BBOX_DTYPE), 4, 2, 0.5, n_boxes=[1, 2, 3])
        raise AssertionError("accepted")
    except ValueError:
        pass
    try:
        t.gate(np.zeros(6, frt.BBOX_DTYPE), 0, 2, 0.5)
        raise AssertionError("accepted")
    except frt.FrtError as e:
        assert e.code == frt.FRT_ERR_INVALID
    t.close()
