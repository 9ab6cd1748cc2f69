"""Whole photos of any sizes (frt_resize_images / frt_enrol_select_dev / frt_pipeline_run_images / frt_pipeline_enrol_images), the part that
needs no GPU: the symbols and their bindings, the argument checks that run before any device work, and the C++ demo's syntax."""
import ctypes
import os
import subprocess

import numpy as np

from conftest import ROOT

GXX = ["g++", "-std=c++11", "-O1", "-Wall", "-Wextra", "-Werror"]
_vp, _i = ctypes.c_void_p, ctypes.c_int
SIGNATURES = {
    "frt_resize_images": (_i, [_vp, _i, _vp, _i, _i, _i]),
    "frt_enrol_select_dev": (_i, [_vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp]),
    "frt_pipeline_run_images": (_i, [_vp, _vp, _i, _vp, _vp, _vp]),
    "frt_pipeline_enrol_images": (_i, [_vp, _vp, _i, _vp, _vp, _vp, _vp, ctypes.POINTER(_i), ctypes.POINTER(_i)]),
}


def test_entry_points_are_declared_exported_and_bound(frt):
    header = open(os.path.join(ROOT, "include", "frt.h")).read()
    for name, (res, args) in SIGNATURES.items():
        assert "int %s(" % name in header, name
        fn = getattr(frt.lib, name)
        assert frt.ABI[name] == (res, args) and fn.restype is res and list(fn.argtypes) == args, name
    for decl in ("int frt_resize_images(const frt_face_image *images, int n, uint8_t *out, int out_rows, int out_cols, int device);",
                 "int frt_pipeline_run_images(frt_pipeline *p, const frt_face_image *images, int n, frt_face_result *results, float *embeds_out, "
                 "uint8_t *crops_out);"):
        assert decl in header, decl
    for word, value in (("FRT_ENROL_OK", 1), ("FRT_ENROL_MANY", 2), ("FRT_ENROL_NONE", 3), ("FRT_ENROL_EMPTY_ROI", 4)):
        assert "%s = %d" % (word, value) in header and getattr(frt, word) == value
    assert callable(frt.resizeImages) and callable(frt.Pipeline.runImages) and callable(frt.Pipeline.enrolImages) and callable(frt.enrol_select_dev)
    arc = open(os.path.join(ROOT, "include", "frt", "arcface.h")).read()
    assert "void enrolImages(Detector &detector, const std::vector<std::string> &names, const std::vector<cv::Mat> &images, std::vector<int> &status," in arc


def test_bad_images_are_refused_before_any_device_work(frt):
    """NULL pixels, rows = 0, cols = 0, a short stride, n < 0: FRT_ERR_INVALID naming the image's index from all three image entry points,
    outputs untouched; n == 0 does nothing; a NULL pipeline is refused.  None of it needs a device."""
    good = np.zeros((5, 4, 3), np.uint8)
    out = np.full((3, 6, 7, 3), 9, np.uint8)
    status = np.full(3, 9, np.int32)
    count = _i(9)

    def calls(arr, n, resize=True):
        if resize:
            yield "resize", frt.lib.frt_resize_images(arr, n, out.ctypes.data, 6, 7, 0), frt.lib.frt_last_error().decode()
        yield "run", frt.lib.frt_pipeline_run_images(None, arr, n, None, None, None), frt.lib.frt_last_error().decode()
        yield "enrol", frt.lib.frt_pipeline_enrol_images(None, arr, n, None, status.ctypes.data, None, None, None, ctypes.byref(count)), \
            frt.lib.frt_last_error().decode()

    ok = frt.FaceImage(good.ctypes.data, 5, 4, 12)
    for bad, word in ((frt.FaceImage(None, 5, 4, 12), "null"), (frt.FaceImage(good.ctypes.data, 0, 4, 12), "rows < 1"),
                      (frt.FaceImage(good.ctypes.data, 5, 0, 12), "cols < 1"), (frt.FaceImage(good.ctypes.data, 5, 4, 11), "row_stride")):
        for at in (0, 2):
            images = [ok, ok, ok]
            images[at] = bad
            for who, rc, msg in calls((frt.FaceImage * 3)(*images), 3):
                assert rc == frt.FRT_ERR_INVALID and "image %d" % at in msg and word in msg, (who, rc, msg)
    for who, rc, msg in calls((frt.FaceImage * 1)(ok), -1):
        assert rc == frt.FRT_ERR_INVALID and "n < 0" in msg, (who, rc, msg)
    for who, rc, msg in calls(None, 2):
        assert rc == frt.FRT_ERR_INVALID and "null image list" in msg, (who, rc, msg)
    # well-formed images, no pipeline (the resize of a well-formed image is no refusal: where there is a device it would write `out`)
    for who, rc, msg in calls((frt.FaceImage * 1)(ok), 1, resize=False):
        assert rc == frt.FRT_ERR_INVALID and "null pipeline" in msg, (who, rc, msg)
    # n == 0 does nothing (the pipeline calls still want their handle)
    assert frt.lib.frt_resize_images(None, 0, out.ctypes.data, 6, 7, 0) == frt.FRT_OK
    assert frt.lib.frt_resize_images(None, 0, None, 6, 7, -1) == frt.FRT_OK
    # a bad output size, and no output
    arr = (frt.FaceImage * 1)(ok)
    for rows, cols in ((0, 7), (6, 0), (-1, 7), (65536, 65536)):
        assert frt.lib.frt_resize_images(arr, 1, out.ctypes.data, rows, cols, 0) == frt.FRT_ERR_INVALID, (rows, cols)
    assert frt.lib.frt_resize_images(arr, 1, None, 6, 7, 0) == frt.FRT_ERR_INVALID
    assert (out == 9).all() and (status == 9).all() and count.value == 9
    # the selection's own arguments
    assert frt.lib.frt_enrol_select_dev(None, None, -1, 4, None, None, None, None, None) == frt.FRT_ERR_INVALID
    assert frt.lib.frt_enrol_select_dev(None, None, 3, 0, None, None, None, None, None) == frt.FRT_ERR_INVALID
    assert frt.lib.frt_enrol_select_dev(None, None, 3, 4, None, None, None, None, None) == frt.FRT_ERR_INVALID
    assert frt.lib.frt_enrol_select_dev(None, None, 0, 4, None, None, None, None, None) == frt.FRT_OK  # nothing to do
    assert frt.lib.frt_enrol_select_dev(16, 8, 1, 1, 16, None, 16, 16, None) == frt.FRT_ERR_INVALID    # rows of 16-byte vectors
    assert "16-byte" in frt.lib.frt_last_error().decode()


def test_photos_demo_is_well_formed_cpp11(tmp_path):
    """tests/cpp/photos_demo.cpp (run on the GPU by tests/test_gpu_images.py), against cvlite and against the OpenCV declarations mock."""
    src = os.path.join(ROOT, "tests", "cpp", "photos_demo.cpp")
    subprocess.check_call(GXX + ["-I", os.path.join(ROOT, "include"), "-c", src, "-o", str(tmp_path / "photos_demo.o")])
    mock = os.path.join(ROOT, "tests", "cpp", "opencv_decl_mock")
    out = subprocess.run(["g++", "-std=c++11", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-DFRT_EXPECT_OPENCV_BRANCH", "-I", mock, "-I",
                          os.path.join(ROOT, "include"), src], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
