"""Recognising a large photo by tiles (frt_select_faces / frt_pipeline_run_photo_tiled), the part that needs no GPU: the symbols and their
bindings, the argument checks that run before any device work and before the pipeline handle is looked at, and the numpy restatement
(tests/tile_faces_ref.py) against hand-written cases of its own."""
import ctypes
import os

import numpy as np

import tile_faces_ref as tf
from conftest import ROOT

_vp, _i, _sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t
SIGNATURES = {
    "frt_select_faces": (_i, [_vp, _vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, ctypes.POINTER(_i), _i]),
    "frt_pipeline_run_photo_tiled": (_i, [_vp, _vp, _i, _i, _sz, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp, ctypes.POINTER(_i)]),
}


def test_entry_points_are_declared_exported_and_bound(frt):
    header = open(os.path.join(ROOT, "include", "frt.h")).read()
    for name, (res, args) in SIGNATURES.items():
        assert "int %s(" % name in header, name
        fn = getattr(frt.lib, name)
        assert frt.ABI[name] == (res, args) and fn.restype is res and list(fn.argtypes) == args, name
    for decl in ("int frt_select_faces(const frt_bbox *boxes, const int32_t *src /* may be NULL */, const float *landmarks /* may be NULL */, int n,",
                 "int frt_pipeline_run_photo_tiled(frt_pipeline *p, const uint8_t *bgr, int rows, int cols, size_t row_stride,",
                 "Recognising a large photo by tiles", "min(x2 - x1, y2 - y1) >= min_face"):
        assert decl in header, decl
    assert "no tiled frt_pipeline_run_images yet" not in header
    assert callable(frt.selectFaces) and callable(frt.Pipeline.runTiled)
    shell = open(os.path.join(ROOT, "include", "frt", "arcface.h")).read()
    assert "std::vector<struct Bbox> recognizeTiled(Detector &detector, cv::Mat &photo," in shell
    assert tf.BBOX_DTYPE == frt.BBOX_DTYPE and tf.RESULT_DTYPE == frt.RESULT_DTYPE


def test_select_is_refused_before_any_device_work(frt):
    L = frt.lib
    INV, CAP = frt.FRT_ERR_INVALID, frt.FRT_ERR_CAPACITY
    boxes = np.zeros(8, frt.BBOX_DTYPE)
    src = np.zeros(8, np.int32)
    ldm = np.zeros((8, 10), np.float32)
    out = np.full(8, 5, frt.BBOX_DTYPE)
    so, pos, passes = np.full(8, 5, np.int32), np.full(8, 5, np.int32), np.full(8, 5, np.int32)
    lo = np.full((8, 10), 5, np.float32)
    k = _i(-5)

    def sel(b=boxes.ctypes.data, s=src.ctypes.data, l=ldm.ctypes.data, n=8, max_batch=4, bo=out.ctypes.data, s_o=so.ctypes.data, l_o=lo.ctypes.data,
            p=pos.ctypes.data, pc=passes.ctypes.data, kk=ctypes.byref(k)):
        return L.frt_select_faces(b, s, l, n, 0, max_batch, bo, s_o, l_o, p, pc, kk, 0)

    assert sel(n=-1) == CAP and sel(n=16385) == CAP and "16384" in L.frt_last_error().decode()
    assert sel(max_batch=0) == INV and sel(max_batch=-3) == INV and "max_batch" in L.frt_last_error().decode()
    for kw in ("b", "bo", "p", "pc", "kk", "s_o", "l_o"):  # (src / landmarks given: their outputs are required too)
        assert sel(**{kw: None}) == INV, kw
    assert out.tobytes() == np.full(8, 5, frt.BBOX_DTYPE).tobytes() and (so == 5).all() and (pos == 5).all() and (passes == 5).all() and (lo == 5).all()
    assert k.value == -5


def test_run_photo_tiled_is_refused_with_a_null_pipeline_and_no_device(frt):
    L = frt.lib
    INV, CAP = frt.FRT_ERR_INVALID, frt.FRT_ERR_CAPACITY
    img = np.zeros((20, 30, 3), np.uint8)
    res = np.full(8, 5, frt.RESULT_DTYPE)
    src = np.full(8, 5, np.int32)
    emb = np.full((8, 512), 5, np.float32)
    cnt = _i(-5)
    opt = frt.TileOptions(4, 4, 1, 1, 1, 0.4)

    def run(pipe=None, bgr=img.ctypes.data, rows=20, cols=30, stride=90, o=ctypes.addressof(opt), min_face=0, max_out=8, r=res.ctypes.data,
            n=ctypes.byref(cnt)):
        return L.frt_pipeline_run_photo_tiled(pipe, bgr, rows, cols, stride, o, min_face, max_out, r, None, emb.ctypes.data, None, src.ctypes.data, n)

    def msg():
        return L.frt_last_error().decode()

    assert run(bgr=None) == INV and run(r=None) == INV and run(n=None) == INV and "null argument" in msg()
    assert run(rows=0) == INV and "rows < 1" in msg()
    assert run(cols=0) == INV and "cols < 1" in msg()
    assert run(stride=89) == INV and "row_stride" in msg()
    for bad in (frt.TileOptions(-1, 4, 1, 1, 1, 0.4), frt.TileOptions(4, -1, 1, 1, 1, 0.4)):
        assert run(o=ctypes.addressof(bad)) == INV and "overlap" in msg()
    # an overlap of the tile's size or more needs the detector's tile to be told from a legal one: it is refused all the same
    for bad in (frt.TileOptions(1 << 30, 4, 1, 1, 1, 0.4), frt.TileOptions(4, 1 << 30, 1, 1, 1, 0.4)):
        assert run(o=ctypes.addressof(bad)) == INV
    for metric in (-1, 2):
        bad = frt.TileOptions(4, 4, 1, metric, 1, 0.4)
        assert run(o=ctypes.addressof(bad)) == INV and "metric" in msg()
    assert run(max_out=0) == CAP and run(max_out=16385) == CAP and "16384" in msg()
    # the order: an invalid argument beside a max_out out of range is the invalid argument's code; everything fine but the handle: INVALID
    assert run(rows=0, max_out=0) == INV
    assert run() == INV and "null pipeline" in msg()
    assert run(o=None) == INV and "null pipeline" in msg()
    assert res.tobytes() == np.full(8, 5, frt.RESULT_DTYPE).tobytes() and (src == 5).all() and (emb == 5).all() and cnt.value == -5


def test_the_restatement_passes_hand_written_cases():
    def box(rows, cols, x1=3, y1=7, score=.5):
        return (x1, y1, x1 + rows, y1 + cols, score)

    b = np.array([box(20, 30, score=.9), box(19, 30, score=.8), box(30, 20, score=.7), box(30, 19, score=.6), box(0, 50, score=.5), box(21, 21, score=.4)],
                 tf.BBOX_DTYPE)
    src = np.array([40, 3, 17, 9, 2, 11], np.int32)
    ldm = np.arange(60, dtype=np.float32).reshape(6, 5, 2)
    # a side exactly min_face is kept; min_face - 1 keeps one more on each axis
    s = tf.select(b, src, ldm, min_face=20, max_batch=4)
    assert s["n_kept"] == 3 and s["keep_pos"].tolist() == [0, 2, 5, -1, -1, -1] and s["src"].tolist() == [40, 17, 11, -1, -1, -1]
    assert s["boxes"][:3].tobytes() == b[[0, 2, 5]].tobytes() and not s["boxes"][3:].tobytes().strip(b"\0")
    assert np.array_equal(s["landmarks"][:3], ldm[[0, 2, 5]]) and (s["landmarks"][3:] == 0).all()
    assert s["pass_count"].tolist() == [3, 0]
    s = tf.select(b, src, ldm, min_face=19, max_batch=4)
    assert s["n_kept"] == 5 and s["keep_pos"].tolist() == [0, 1, 2, 3, 5, -1] and s["pass_count"].tolist() == [4, 1]
    # min_face <= 0 keeps everything, the zero-extent box included; 1 drops it alone
    for mf in (0, -7):
        s = tf.select(b, min_face=mf, max_batch=128)
        assert s["n_kept"] == 6 and s["keep_pos"].tolist() == list(range(6)) and s["src"] is None and s["landmarks"] is None
        assert s["boxes"].tobytes() == b.tobytes() and s["pass_count"].tolist() == [6]
    assert tf.select(b, min_face=1)["keep_pos"].tolist() == [0, 1, 2, 3, 5, -1]
    assert tf.select(b, min_face=31)["n_kept"] == 0
    # pass_count at n = 0, n = max_batch, n = max_batch + 1 (cap 9: three passes of 4)
    assert tf.pass_count(0, 9, 4).tolist() == [0, 0, 0]
    assert tf.pass_count(4, 9, 4).tolist() == [4, 0, 0]
    assert tf.pass_count(5, 9, 4).tolist() == [4, 1, 0]
    assert tf.pass_count(9, 9, 4).tolist() == [4, 4, 1]
    assert tf.pass_count(0, 0, 4).tolist() == [] and tf.pass_count(3, 3, 1).tolist() == [1, 1, 1]
    e = tf.select(np.zeros(0, tf.BBOX_DTYPE), max_batch=4)
    assert e["n_kept"] == 0 and len(e["boxes"]) == 0 and len(e["pass_count"]) == 0


def test_tiled_faces_demo_is_well_formed_cpp11_and_links(tmp_path):
    """tests/cpp/tiled_faces_demo.cpp against cvlite and against the OpenCV declarations mock; every symbol recognizeTiled needs is exported"""
    import subprocess
    src = os.path.join(ROOT, "tests", "cpp", "tiled_faces_demo.cpp")
    pkg = os.path.join(ROOT, "face-recognition-cpp-tensorrt_amd")
    gxx = ["g++", "-std=c++11", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include")]
    mock = os.path.join(ROOT, "tests", "cpp", "opencv_decl_mock")
    out = subprocess.run(["g++", "-std=c++11", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-DFRT_EXPECT_OPENCV_BRANCH", "-I", mock, "-I",
                          os.path.join(ROOT, "include"), src], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    subprocess.check_call(gxx + [src, "-o", str(tmp_path / "tiled_faces_demo"), os.path.join(pkg, "libfrt.so"), "-Wl,-rpath," + pkg, "-Wl,-rpath,/opt/rocm/lib"])
