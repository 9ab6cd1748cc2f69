"""Large photos by tiles (frt_tile_plan / frt_cut_tiles / frt_merge_boxes / frt_detector_find_faces_tiled), the part that needs no GPU: the
symbols and their bindings, the host-only plan against tests/tiled_ref.py, and the argument checks that run before any device work."""
import ctypes
import os

import numpy as np

import tiled_ref as tr
from conftest import ROOT

_vp, _i, _sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t
SIGNATURES = {
    "frt_tile_plan": (_i, [_i, _i, _i, _i, _vp, _vp, _i, ctypes.POINTER(_i)]),
    "frt_cut_tiles": (_i, [_vp, _i, _i, _sz, _vp, _i, _i, _i, _vp, _i]),
    "frt_merge_boxes": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp, _i, _vp, _vp, ctypes.POINTER(_i), _i]),
    "frt_detector_find_faces_tiled": (_i, [_vp, _vp, _i, _i, _sz, _vp, _i, _vp, _vp, _vp, ctypes.POINTER(_i)]),
}


def test_entry_points_are_declared_exported_and_bound(frt):
    header = open(os.path.join(ROOT, "include", "frt.h")).read()
    for name, (res, args) in SIGNATURES.items():
        assert "int %s(" % name in header, name
        fn = getattr(frt.lib, name)
        assert frt.ABI[name] == (res, args) and fn.restype is res and list(fn.argtypes) == args, name
    for decl in ("int frt_tile_plan(int rows, int cols, int tile_rows, int tile_cols, const frt_tile_options *options, frt_tile *tiles_out, int capacity,",
                 "int frt_cut_tiles(const uint8_t *bgr, int rows, int cols, size_t row_stride, const frt_tile *tiles, int n_tiles, int tile_rows, int tile_cols,",
                 "typedef struct frt_tile { int32_t row0, col0, rows, cols, kind; } frt_tile;", "Large photos by tiles", "max_faces"):
        assert decl in header, decl
    assert ctypes.sizeof(frt.TileOptions) == 24 and frt.TILE_DTYPE.itemsize == 20 and frt.TILE_DTYPE == tr.TILE_DTYPE
    assert [f[0] for f in frt.TileOptions._fields_] == ["overlap_rows", "overlap_cols", "overview", "metric", "drop_cut", "merge_threshold"]
    assert callable(frt.tilePlan) and callable(frt.cutTiles) and callable(frt.mergeBoxes) and callable(frt.RetinaFace.findFaceTiled)
    shell = open(os.path.join(ROOT, "include", "frt", "retinaface.h")).read()
    assert "std::vector<struct Bbox> findFaceTiled(cv::Mat &photo" in shell


def test_plan_equals_the_restatement_over_a_sweep(frt):
    """photos of 1 .. 700 pixels per axis against tiles 96 x 160 and 640 x 640, overlaps 0, 1, T / 4 and T - 1, with and without overview"""
    tiles = np.zeros(4096, frt.TILE_DTYPE)
    n = _i(0)
    calls = 0
    for T_r, T_c in ((96, 160), (640, 640)):
        for frac in ("0", "1", "quarter", "most"):
            V_r, V_c = {"0": (0, 0), "1": (1, 1), "quarter": (T_r // 4, T_c // 4), "most": (T_r - 1, T_c - 1)}[frac]
            for overview in (0, 1):
                opt = frt.TileOptions(V_r, V_c, overview, 1, 1, -1.0)
                for L in range(1, 701):
                    # each axis runs 1 .. 700; an overlap of T - 1 makes a tile per pixel, so there the other axis stays within one tile
                    other = 1 + L % 37 if frac == "most" else 701 - L
                    for rows, cols in ((L, other), (other, L)):
                        want = tr.plan(rows, cols, T_r, T_c, V_r, V_c, overview)
                        assert len(want) <= 4096
                        rc = frt.lib.frt_tile_plan(rows, cols, T_r, T_c, ctypes.addressof(opt), tiles.ctypes.data, len(tiles), ctypes.byref(n))
                        assert rc == frt.FRT_OK and n.value == len(want) and np.array_equal(tiles[:n.value], want), (rows, cols, T_r, T_c, V_r, V_c, overview)
                        calls += 1
    assert calls > 20000
    assert np.array_equal(frt.tilePlan(200, 410, 96, 160, 32, True), tr.plan(200, 410, 96, 160, 32, 32, True))
    assert np.array_equal(frt.tilePlan(2160, 3840, 640, 640), tr.plan(2160, 3840, 640, 640, 160, 160, True))


def test_bad_arguments_are_refused_before_any_device_work(frt):
    L = frt.lib
    INV, CAP = frt.FRT_ERR_INVALID, frt.FRT_ERR_CAPACITY
    img = np.zeros((20, 30, 3), np.uint8)
    tiles = np.full(8, 77, frt.TILE_DTYPE)
    n = _i(-5)
    opt = frt.TileOptions(4, 4, 1, 1, 1, 0.4)
    o, t, im = ctypes.addressof(opt), tiles.ctypes.data, img.ctypes.data

    # ---- frt_tile_plan
    assert L.frt_tile_plan(20, 30, 16, 16, None, t, 8, ctypes.byref(n)) == INV
    assert L.frt_tile_plan(20, 30, 16, 16, o, None, 8, ctypes.byref(n)) == INV
    assert L.frt_tile_plan(20, 30, 16, 16, o, t, 8, None) == INV
    assert L.frt_tile_plan(0, 30, 16, 16, o, t, 8, ctypes.byref(n)) == INV and "rows < 1" in L.frt_last_error().decode()
    assert L.frt_tile_plan(20, 0, 16, 16, o, t, 8, ctypes.byref(n)) == INV
    for bad in (frt.TileOptions(-1, 4, 1, 1, 1, 0.4), frt.TileOptions(16, 4, 1, 1, 1, 0.4), frt.TileOptions(4, -1, 1, 1, 1, 0.4), frt.TileOptions(4, 16, 1, 1, 1, 0.4)):
        assert L.frt_tile_plan(20, 30, 16, 16, ctypes.addressof(bad), t, 8, ctypes.byref(n)) == INV and "overlap" in L.frt_last_error().decode()
    assert n.value == -5 and (tiles == np.full(8, 77, frt.TILE_DTYPE)).all()
    # 4096 tiles: a 64 x 64 grid is the most; one more column, or the overview on top, is too many
    opt0 = frt.TileOptions(0, 0, 0, 1, 1, 0.4)
    big = np.zeros(5000, frt.TILE_DTYPE)
    assert L.frt_tile_plan(64 * 16, 64 * 16, 16, 16, ctypes.addressof(opt0), big.ctypes.data, 5000, ctypes.byref(n)) == frt.FRT_OK and n.value == 4096
    assert L.frt_tile_plan(64 * 16, 64 * 16 + 1, 16, 16, ctypes.addressof(opt0), big.ctypes.data, 5000, ctypes.byref(n)) == CAP
    opt1 = frt.TileOptions(0, 0, 1, 1, 1, 0.4)
    assert L.frt_tile_plan(64 * 16, 64 * 16, 16, 16, ctypes.addressof(opt1), big.ctypes.data, 5000, ctypes.byref(n)) == CAP
    assert L.frt_tile_plan(2 ** 30, 2 ** 30, 16, 16, ctypes.addressof(opt1), big.ctypes.data, 5000, ctypes.byref(n)) == CAP
    # a plan larger than tiles_out: the count is reported, tiles_out untouched
    assert L.frt_tile_plan(20, 30, 16, 16, o, t, 3, ctypes.byref(n)) == CAP and n.value == len(tr.plan(20, 30, 16, 16, 4, 4, True)) == 7
    assert (tiles == np.full(8, 77, frt.TILE_DTYPE)).all()

    # ---- frt_cut_tiles
    plan = tr.plan(20, 30, 16, 16, 4, 4, True)
    out = np.full((len(plan), 16, 16, 3), 9, np.uint8)
    p, ou = plan.ctypes.data, out.ctypes.data
    assert L.frt_cut_tiles(None, 20, 30, 90, p, len(plan), 16, 16, ou, 0) == INV
    assert L.frt_cut_tiles(im, 20, 30, 90, None, len(plan), 16, 16, ou, 0) == INV
    assert L.frt_cut_tiles(im, 20, 30, 90, p, len(plan), 16, 16, None, 0) == INV
    assert L.frt_cut_tiles(im, 0, 30, 90, p, len(plan), 16, 16, ou, 0) == INV
    assert L.frt_cut_tiles(im, 20, 30, 89, p, len(plan), 16, 16, ou, 0) == INV and "row_stride" in L.frt_last_error().decode()
    assert L.frt_cut_tiles(im, 20, 30, 90, p, 0, 16, 16, ou, 0) == INV
    assert L.frt_cut_tiles(im, 20, 30, 90, p, 4097, 16, 16, ou, 0) == CAP
    assert (out == 9).all()

    # ---- frt_merge_boxes
    slots = 4
    boxes = np.zeros((len(plan), slots), frt.BBOX_DTYPE)
    nb = np.zeros(len(plan), np.int32)
    res = np.full(8, 5, frt.BBOX_DTYPE)
    src = np.full(8, 5, np.int32)
    cnt = _i(-5)

    def merge(boxes_p=boxes.ctypes.data, nb_p=nb.ctypes.data, tiles_p=p, n_tiles=len(plan), slots=slots, rows=20, cols=30, opt_p=o, max_out=8,
              out_p=res.ctypes.data, src_p=src.ctypes.data, cnt_p=ctypes.byref(cnt)):
        return L.frt_merge_boxes(boxes_p, nb_p, tiles_p, n_tiles, slots, rows, cols, 16, 16, opt_p, max_out, out_p, src_p, cnt_p, 0)

    for kw in ("boxes_p", "nb_p", "tiles_p", "opt_p", "out_p", "src_p", "cnt_p"):
        assert merge(**{kw: None}) == INV, kw
    assert merge(rows=0) == INV and merge(cols=0) == INV and merge(slots=0) == INV and merge(n_tiles=0) == INV
    for metric in (-1, 2):
        bad = frt.TileOptions(4, 4, 1, metric, 1, 0.4)
        assert merge(opt_p=ctypes.addressof(bad)) == INV and "metric" in L.frt_last_error().decode()
    neg = frt.TileOptions(4, 4, 1, 1, 1, -1.0)
    assert merge(opt_p=ctypes.addressof(neg)) == INV and "threshold" in L.frt_last_error().decode()
    # 16384 candidates and 16384 outputs are the most
    many = np.zeros(4096, frt.TILE_DTYPE)
    assert merge(tiles_p=many.ctypes.data, n_tiles=4096, slots=5) == CAP and "16384" in L.frt_last_error().decode()
    assert merge(tiles_p=many.ctypes.data, n_tiles=2049, slots=8) == CAP
    assert merge(tiles_p=many.ctypes.data, n_tiles=4097, slots=1) == CAP
    assert merge(max_out=0) == CAP and merge(max_out=16385) == CAP
    assert res.tobytes() == np.full(8, 5, frt.BBOX_DTYPE).tobytes() and (src == 5).all() and cnt.value == -5

    # ---- frt_detector_find_faces_tiled: no detector, nothing written
    assert L.frt_detector_find_faces_tiled(None, im, 20, 30, 90, o, 8, res.ctypes.data, None, src.ctypes.data, ctypes.byref(cnt)) == INV
    assert res.tobytes() == np.full(8, 5, frt.BBOX_DTYPE).tobytes() and (src == 5).all() and cnt.value == -5
