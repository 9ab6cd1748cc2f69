"""Live gallery edits, the part that needs no GPU: the entry points exist, reject NULL handles, and the removal map (csrc/frt_holes.h) is the
order-preserving erase."""
import ctypes
import os
import subprocess

from conftest import ROOT

EDIT_SYMBOLS = ("frt_matcher_gallery_reserve", "frt_matcher_gallery_add", "frt_matcher_gallery_add_dev", "frt_matcher_gallery_remove",
                "frt_matcher_edit_stats")


def test_edit_entry_points_are_declared_exported_and_bound(frt):
    header = open(os.path.join(ROOT, "include", "frt.h")).read()
    for s in EDIT_SYMBOLS:
        assert s + "(" in header, s
        assert hasattr(frt.lib, s), "libfrt.so does not export %s" % s
        assert s in frt.ABI, "python binding misses %s" % s
    for name in ("galleryReserve", "galleryAdd", "galleryAddDev", "galleryRemove", "editStats"):
        assert callable(getattr(frt.MatMul, name))
    for name in ("enrolEmbedding", "removeClass"):
        assert callable(getattr(frt.ArcFaceIR50, name))


def test_edit_entry_points_reject_null_handles(frt):
    rows = (ctypes.c_float * 512)()
    idx = (ctypes.c_int32 * 1)(0)
    stats = (ctypes.c_long * 4)()
    assert frt.lib.frt_matcher_gallery_reserve(None, 10) == frt.FRT_ERR_INVALID
    assert frt.lib.frt_matcher_gallery_add(None, rows, 1) == frt.FRT_ERR_INVALID
    assert frt.lib.frt_matcher_gallery_add_dev(None, rows, 1) == frt.FRT_ERR_INVALID
    assert frt.lib.frt_matcher_gallery_remove(None, idx, 1) == frt.FRT_ERR_INVALID
    assert frt.lib.frt_matcher_edit_stats(None, stats) == frt.FRT_ERR_INVALID
    assert b"null" in frt.lib.frt_last_error()


def test_shell_headers_offer_the_edit_methods():
    mm = open(os.path.join(ROOT, "include", "frt", "matmul.h")).read()
    arc = open(os.path.join(ROOT, "include", "frt", "arcface.h")).read()
    for name in ("galleryReserve", "galleryAdd", "galleryAddDev", "galleryRemove"):
        assert "void %s(" % name in mm, name
    for name in ("void enrolEmbedding(", "void enrolEmbeddings(", "int removeClass("):
        assert name in arc, name


def test_hole_map_is_the_order_preserving_erase(tmp_path):
    """tests/cpp/hole_map_test.cpp: the header the compaction kernels use, compiled for the host alone."""
    exe = str(tmp_path / "hole_map_test")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "face-recognition-cpp-tensorrt_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "hole_map_test.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.startswith("hole map ok"), (out.returncode, out.stdout, out.stderr)


def test_shell_program_compiles_as_cxx11(tmp_path):
    """tests/cpp/enrol_demo.cpp (run on the GPU by tests/test_gpu_gallery_edit.py) is well-formed C++11 under -Wall -Wextra -Werror."""
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-c",
                           os.path.join(ROOT, "tests", "cpp", "enrol_demo.cpp"), "-o", str(tmp_path / "enrol_demo.o")])
