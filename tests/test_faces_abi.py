"""Face images instead of frames (frt_preprocess_faces / frt_embedder_embed_faces / frt_embedder_enrol_faces), the part that needs no GPU:
the chunk planner (csrc/frt_faces.hpp), the argument checks that run before any device work, and the shells."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "face-recognition-cpp-tensorrt_amd", "csrc")
GXX = ["g++", "-std=c++11", "-O1", "-Wall", "-Wextra", "-Werror"]


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_chunk_planner(tmp_path, sanitize):
    """tests/cpp/face_chunks_test.cpp: a plain host program with its own main, also built with AddressSanitizer + UBSan and run directly."""
    exe = str(tmp_path / "face_chunks_test")
    san = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"] if sanitize else []
    subprocess.check_call(GXX + san + ["-I", CSRC, os.path.join(ROOT, "tests", "cpp", "face_chunks_test.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.startswith("face chunks ok") and not out.stderr, (out.returncode, out.stdout, out.stderr)


def test_entry_points_are_declared_exported_and_bound(frt):
    header = open(os.path.join(ROOT, "include", "frt.h")).read()
    assert "typedef struct frt_face_image { const uint8_t *bgr; int32_t rows, cols; size_t row_stride; } frt_face_image;" in header
    for s in ("frt_preprocess_faces", "frt_embedder_embed_faces", "frt_embedder_enrol_faces"):
        assert s + "(" in header and hasattr(frt.lib, s) and s in frt.ABI, s
    assert ctypes.sizeof(frt.FaceImage) == 24 and frt.FaceImage.row_stride.offset == 16
    assert callable(frt.preprocessFaces) and callable(frt.ArcFaceIR50.forwardFaces) and callable(frt.ArcFaceIR50.enrolFaces)
    arc = open(os.path.join(ROOT, "include", "frt", "arcface.h")).read()
    assert "void forwardFaces(const std::vector<cv::Mat> &faces)" in arc
    assert "void enrolFaces(const std::vector<std::string> &names, const std::vector<cv::Mat> &faces" in arc


def test_bad_images_are_refused_before_any_device_work(frt):
    """NULL pixels, rows = 0, a short stride, n < 0: FRT_ERR_INVALID naming the image's index, outputs untouched; n == 0 does nothing.  None
    of it needs a device."""
    good = np.zeros((5, 4, 3), np.uint8)
    crops = np.full((3, 112, 112, 3), 7, np.uint8)
    chw = np.full((3, 3, 112, 112), 7, np.float32)

    def call(images, n=None):
        arr = (frt.FaceImage * len(images))(*images)
        rc = frt.lib.frt_preprocess_faces(arr, len(images) if n is None else n, crops.ctypes.data, chw.ctypes.data, 0)
        return rc, frt.lib.frt_last_error().decode()

    ok = frt.FaceImage(good.ctypes.data, 5, 4, 12)
    for bad, word in ((frt.FaceImage(None, 5, 4, 12), "null"), (frt.FaceImage(good.ctypes.data, 0, 4, 12), "rows < 1"),
                      (frt.FaceImage(good.ctypes.data, 5, 0, 12), "cols < 1"), (frt.FaceImage(good.ctypes.data, 5, 4, 11), "row_stride")):
        for at in (0, 2):
            images = [ok, ok, ok]
            images[at] = bad
            rc, msg = call(images)
            assert rc == frt.FRT_ERR_INVALID and "image %d" % at in msg and word in msg, (rc, msg)
    rc, msg = call([ok], n=-1)
    assert rc == frt.FRT_ERR_INVALID and "n < 0" in msg
    assert frt.lib.frt_preprocess_faces(None, 2, crops.ctypes.data, chw.ctypes.data, 0) == frt.FRT_ERR_INVALID
    assert frt.lib.frt_preprocess_faces(None, 0, crops.ctypes.data, chw.ctypes.data, 0) == frt.FRT_OK
    assert (crops == 7).all() and (chw == 7).all()
    # the object-level entry points check their handles first
    arr = (frt.FaceImage * 1)(ok)
    assert frt.lib.frt_embedder_embed_faces(None, arr, 1, chw.ctypes.data, None) == frt.FRT_ERR_INVALID
    assert frt.lib.frt_embedder_enrol_faces(None, None, arr, 1, None, None, None) == frt.FRT_ERR_INVALID


def test_binding_passes_strided_views_without_a_copy(frt):
    base = np.zeros((50, 80, 3), np.uint8)
    view = base[:, :61]
    arr, keep = frt._face_images([view, base[::2], base[:, ::-1]])
    assert keep[0] is view and (arr[0].bgr, arr[0].rows, arr[0].cols, arr[0].row_stride) == (base.ctypes.data, 50, 61, 240)
    assert (arr[1].rows, arr[1].cols, arr[1].row_stride) == (25, 80, 480) and arr[1].bgr == base.ctypes.data   # every second row: a stride
    assert arr[2].row_stride == 240 and arr[2].bgr == keep[2].ctypes.data != base.ctypes.data                   # mirrored columns: copied
    with pytest.raises(ValueError):
        frt._face_images([np.zeros((4, 4), np.uint8)])
    with pytest.raises(ValueError):
        frt._face_images([np.zeros((4, 4, 3), np.float32)])


def test_faces_demo_is_well_formed_cpp11(tmp_path):
    """tests/cpp/faces_demo.cpp (run on the GPU by tests/test_gpu_faces.py), against cvlite and against the OpenCV declarations mock."""
    src = os.path.join(ROOT, "tests", "cpp", "faces_demo.cpp")
    subprocess.check_call(GXX + ["-I", os.path.join(ROOT, "include"), "-c", src, "-o", str(tmp_path / "faces_demo.o")])
    mock = os.path.join(ROOT, "tests", "cpp", "opencv_decl_mock")
    out = subprocess.run(["g++", "-std=c++11", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-DFRT_EXPECT_OPENCV_BRANCH", "-I", mock, "-I",
                          os.path.join(ROOT, "include"), src], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
