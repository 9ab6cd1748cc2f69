"""Sighting book (frt_sightings_* / frt_pipeline_run_sighted), the part that needs no GPU: the symbols and their bindings, the record layout,
and the argument checks - every one of them runs before any device work, so on a machine without a device a refused call returns its own
status (not FRT_ERR_DEVICE) and leaves the output buffers' sentinel bytes alone."""
import ctypes
import os
import re

import numpy as np

import sightings_ref as sr
from conftest import ROOT

_vp, _i = ctypes.c_void_p, ctypes.c_int
SIGNATURES = {
    "frt_sightings_create": (_i, [_vp, _i, _vp, ctypes.POINTER(_vp)]),
    "frt_sightings_destroy": (None, [_vp]),
    "frt_sightings_update_dev": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp, _vp]),
    "frt_sightings_update": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp]),
    "frt_sightings_close": (_i, [_vp, _i]),
    "frt_sightings_drain": (_i, [_vp, _i, _vp, _vp, _vp, _vp, ctypes.POINTER(_i), _vp]),
    "frt_sightings_open": (_i, [_vp, _i, _vp, _vp, _vp, _vp]),
    "frt_pipeline_run_sighted": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp]),
}


def _header():
    return open(os.path.join(ROOT, "include", "frt.h")).read()


def test_entry_points_are_declared_exported_and_bound(frt):
    header = _header()
    for name, (res, args) in SIGNATURES.items():
        assert "%s %s(" % ("void" if res is None else "int", name) in header, name
        fn = getattr(frt.lib, name)
        assert frt.ABI[name] == (res, args) and fn.restype is res and list(fn.argtypes) == args, name
    for decl in ("int frt_sightings_create(frt_tracker *t, int capacity, const frt_sighting_options *options /* may be NULL */, frt_sightings **out);",
                 "int frt_sightings_update_dev(frt_sightings *b, const void *results_dev, const void *tracks_dev, const void *embeds_dev, const void *templates_dev,",
                 "int frt_sightings_drain(frt_sightings *b, int max_out, frt_sighting *records_out, uint8_t *crops_out, float *embeds_out, float *templates_out,",
                 "int frt_pipeline_run_sighted(frt_pipeline *p, frt_tracker *t, frt_sightings *b, const frt_quality_options *quality, const uint8_t *frames,",
                 "Sightings", "n_streams * max_tracks + capacity rows of 96 + 8 * dim", "keep_crops = 0 is the setting for trackers with many streams",
                 "NO RECOMMENDED THRESHOLDS"):
        assert decl in header, decl
    for m in ("update", "updateDev", "close", "drain", "open"):
        assert callable(getattr(frt.Sightings, m)), m
    assert callable(frt.Pipeline.runSighted)
    assert "class FaceSightings" in open(os.path.join(ROOT, "include", "frt", "sightings.h")).read()
    # the existing tracker and quality entry points keep their signatures
    assert frt.ABI["frt_pipeline_run_tracked"] == (_i, [_vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp])
    assert frt.ABI["frt_pipeline_run_quality"] == (_i, [_vp, _vp, _i, _vp, _vp, _vp, _vp, _vp])


def _c_struct(header, name):
    body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), header, re.S).group(1), flags=re.S)
    out = []
    for stmt in body.split(";"):
        stmt = stmt.strip()
        if stmt:
            ctype, names = stmt.split(None, 1)
            out += [(ctype, n.strip()) for n in names.split(",")]
    return out


def test_record_and_option_layouts(frt):
    header = _header()
    rec = _c_struct(header, "frt_sighting")
    box = ["x1", "y1", "x2", "y2", "score"]
    flat = [n for _, n in rec]
    assert flat == ["stream", "track_id", "first_tick", "last_tick", "close_tick", "reason", "hits", "n_embeds", "confirmed", "match_idx", "match_sim",
                    "n_shots", "best_tick", "best_box", "best_sharpness", "best_luma_var", "best_mean", "best_flags", "best_size", "reserved"]
    flat = flat[:13] + box + flat[14:]
    D = frt.SIGHTING_DTYPE
    assert D.itemsize == 96 and D == sr.SIGHTING_DTYPE and list(D.names) == flat
    assert [D.fields[n][1] for n in flat] == list(range(0, 96, 4))                      # every field 4 bytes, in declaration order
    ctypes_of = {"int32_t": "<i4", "float": "<f4", "uint32_t": "<u4"}
    for ctype, n in rec:
        if n != "best_box":
            assert D.fields[n][0] == np.dtype(ctypes_of[ctype]), n
    assert [D.fields[n][0] for n in box] == [np.dtype("<i4")] * 4 + [np.dtype("<f4")]
    opt = _c_struct(header, "frt_sighting_options")
    assert opt == [("int32_t", "rank"), ("int32_t", "min_hits"), ("int32_t", "keep_crops")]
    assert [f[0] for f in frt.SightingOptions._fields_] == [n for _, n in opt] and ctypes.sizeof(frt.SightingOptions) == 12
    for name, val in (("FRT_SHOT_RANK_SHARPNESS", 0), ("FRT_SHOT_RANK_SIZE", 1), ("FRT_SHOT_RANK_SCORE", 2), ("FRT_SIGHTING_EXPIRED", 1),
                      ("FRT_SIGHTING_REPLACED", 2), ("FRT_SIGHTING_CLOSED", 3)):
        assert re.search(r"#define %s %d\b" % (name, val), header), name
    assert (frt.SHOT_RANK_SHARPNESS, frt.SHOT_RANK_SIZE, frt.SHOT_RANK_SCORE) == (0, 1, 2) == (sr.RANK_SHARPNESS, sr.RANK_SIZE, sr.RANK_SCORE)
    assert (frt.SIGHTING_EXPIRED, frt.SIGHTING_REPLACED, frt.SIGHTING_CLOSED) == (1, 2, 3) == (sr.EXPIRED, sr.REPLACED, sr.CLOSED)


def _tracker(frt, n_streams=3):
    h = _vp()
    assert frt.lib.frt_tracker_create(n_streams, 4, 3, 8, None, 0, ctypes.byref(h)) == frt.FRT_OK
    return h


def _book(frt, t, capacity=4, opt=None):
    h = _vp()
    return frt.lib.frt_sightings_create(t, capacity, ctypes.addressof(opt) if opt is not None else None, ctypes.byref(h)), h


def test_create_checks_capacity_and_options_without_a_device(frt):
    L, INV, CAP = frt.lib, frt.FRT_ERR_INVALID, frt.FRT_ERR_CAPACITY
    t = _tracker(frt)
    O = frt.SightingOptions
    assert L.frt_sightings_create(None, 4, None, ctypes.byref(_vp())) == INV and L.frt_sightings_create(t, 4, None, None) == INV
    for cap in (0, -1, 65537):
        rc, h = _book(frt, t, cap)
        assert rc == CAP and not h.value and "capacity" in L.frt_last_error().decode(), cap
    for bad in (O(3, 1, 1), O(-1, 1, 1), O(0, 0, 1), O(0, -2, 1), O(0, 1, 2), O(0, 1, -1)):
        rc, h = _book(frt, t, opt=bad)
        assert rc == INV and not h.value and "sightings" in L.frt_last_error().decode()
    for cap, opt in ((1, None), (65536, O(2, 7, 0)), (4, O(1, 1, 1))):    # (creation does no device work: it succeeds here too)
        rc, h = _book(frt, t, cap, opt)
        assert rc == frt.FRT_OK and h.value
        L.frt_sightings_destroy(h)
    L.frt_sightings_destroy(None)
    L.frt_tracker_destroy(t)


def test_bad_arguments_are_refused_before_any_device_work(frt):
    L, INV, CAP = frt.lib, frt.FRT_ERR_INVALID, frt.FRT_ERR_CAPACITY
    t = _tracker(frt)
    rc, keep = _book(frt, t)
    rc2, lean = _book(frt, t, opt=frt.SightingOptions(0, 1, 0))
    assert rc == rc2 == frt.FRT_OK
    MF, D, N = 3, 8, 300
    res = np.zeros(N * MF, frt.RESULT_DTYPE)
    trk = np.zeros(N * MF, frt.TRACK_DTYPE)
    emb = np.zeros((N * MF, D), np.float32)
    tpl = np.zeros((N * MF, D), np.float32)
    qual = np.zeros(N * MF, frt.QUALITY_DTYPE)
    crops = np.zeros((2 * MF, 112, 112, 3), np.uint8)
    A = 4096   # stands for an aligned device address that is never touched

    def host(b=keep, r=res.ctypes.data, k=trk.ctypes.data, e=emb.ctypes.data, tp=tpl.ctypes.data, q=qual.ctypes.data, c=crops.ctypes.data, n=2, ids=None):
        return L.frt_sightings_update(b, r, k, e, tp, q, c, n, np.asarray(ids, np.int32).ctypes.data if ids is not None else None)

    def dev(b=keep, r=A, k=A, e=A, tp=A, q=A, c=A, n=2, ids=None):
        return L.frt_sightings_update_dev(b, r, k, e, tp, q, c, n, np.asarray(ids, np.int32).ctypes.data if ids is not None else None, None)

    for call in (host, dev):
        # ---- NULL pointers (templates may be NULL: its refusal is the crops' below)
        for kw in (dict(b=None), dict(r=None), dict(k=None), dict(e=None), dict(q=None)):
            assert call(**kw) == INV, kw
        # ---- crops are required iff the book keeps them
        assert call(c=None) == INV and "keeps crops" in L.frt_last_error().decode()
        assert call(b=lean) == INV and "keep_crops 0" in L.frt_last_error().decode()
        # ---- the tracker's id checks
        assert call(n=0) == INV and call(n=-1) == INV
        assert call(n=257) == CAP and "256" in L.frt_last_error().decode()
        assert call(n=4) == INV                                      # 3 streams; NULL ids: frame i is stream i
        assert call(ids=[0, 3]) == INV and "outside" in L.frt_last_error().decode()
        assert call(ids=[1, 1]) == INV and "twice" in L.frt_last_error().decode()
        assert call(b=lean, c=None, n=3, ids=[2, 0, 2]) == INV and "twice" in L.frt_last_error().decode()
    # ---- misaligned device pointers
    for kw in (dict(e=A + 4), dict(tp=A + 8), dict(c=A + 8), dict(q=A + 4), dict(r=A + 2), dict(k=A + 1)):
        assert dev(**kw) == INV and "aligned" in L.frt_last_error().decode(), kw

    # ---- close / drain / open
    rec = np.full(4 * 96, 0xA5, np.uint8)
    pay = np.full(4 * D * 4, 0xA5, np.uint8)
    big = np.full(16, 0xA5, np.uint8)          # never written: every call below is refused
    n, cnt = _i(-7), np.full(4, -7, np.int32)
    assert L.frt_sightings_close(None, 0) == INV and L.frt_sightings_close(keep, -2) == INV and L.frt_sightings_close(keep, 3) == INV
    drain = lambda b=keep, m=4, r=rec.ctypes.data, c=None, no=ctypes.byref(n): L.frt_sightings_drain(b, m, r, c, pay.ctypes.data, pay.ctypes.data, no, cnt.ctypes.data)
    assert drain(b=None) == INV and drain(r=None) == INV and drain(no=None) == INV and drain(m=0) == INV and drain(m=-3) == INV
    assert drain(b=lean, c=big.ctypes.data) == INV and "keep_crops 0" in L.frt_last_error().decode()
    opn = lambda b=keep, s=0, r=rec.ctypes.data, c=None: L.frt_sightings_open(b, s, r, pay.ctypes.data, pay.ctypes.data, c)
    assert opn(b=None) == INV and opn(r=None) == INV and opn(s=-1) == INV and opn(s=3) == INV and opn(b=lean, c=big.ctypes.data) == INV
    assert (rec == 0xA5).all() and (pay == 0xA5).all() and (big == 0xA5).all() and n.value == -7 and (cnt == -7).all()

    # ---- frt_pipeline_run_sighted: NULLs, a book of another tracker (looked at before the pipeline is), the quality options
    other = _tracker(frt)
    frames = np.zeros((2, 4, 4, 3), np.uint8)
    r2 = np.full(2 * MF * 36, 0xA5, np.uint8)
    k2 = np.full(2 * MF * 32, 0xA5, np.uint8)
    q2 = np.full(2 * MF * 56, 0xA5, np.uint8)
    run = lambda p=None, tt=t, b=keep, o=None: L.frt_pipeline_run_sighted(p, tt, b, o, frames.ctypes.data, 2, None, r2.ctypes.data, k2.ctypes.data,
                                                                             q2.ctypes.data, None)
    assert run(tt=None) == INV and run(b=None) == INV
    assert run(tt=other) == INV and "belongs to another tracker" in L.frt_last_error().decode()
    assert run() == INV and "null argument" in L.frt_last_error().decode()      # the NULL pipeline
    assert (r2 == 0xA5).all() and (k2 == 0xA5).all() and (q2 == 0xA5).all()
    for h in (keep, lean):
        L.frt_sightings_destroy(h)
    L.frt_tracker_destroy(t), L.frt_tracker_destroy(other)


def test_python_shell_refuses_bad_shapes_before_the_library(frt):
    import pytest
    trk = frt.Tracker(3, 4, 3, 8)
    with pytest.raises(frt.FrtError) as e:
        frt.Sightings(trk, 0)
    assert e.value.code == frt.FRT_ERR_CAPACITY
    book = frt.Sightings(trk, 4, rank=frt.SHOT_RANK_SIZE, min_hits=2, keep_crops=False)
    ok = dict(results=np.zeros(6, frt.RESULT_DTYPE), tracks=np.zeros(6, frt.TRACK_DTYPE), embeds=np.zeros((6, 8), np.float32),
              quality=np.zeros(6, frt.QUALITY_DTYPE))
    for bad in (dict(results=np.zeros(5, frt.RESULT_DTYPE)), dict(tracks=np.zeros(3, frt.TRACK_DTYPE)), dict(embeds=np.zeros((6, 4), np.float32)),
                dict(quality=np.zeros(7, frt.QUALITY_DTYPE)), dict(templates=np.zeros((6, 4), np.float32)), dict(crops=np.zeros((6, 112, 112), np.uint8)),
                dict(stream_ids=[0])):
        with pytest.raises(ValueError):
            book.update(**dict(ok, **bad))
    trk.close()                 # the tracker takes its books with it
    assert not book._h
    book.destroy()
