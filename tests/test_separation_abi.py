"""frt_matcher_separation (include/frt.h), the part that needs no GPU: the two entry points as the header, the library
and the Python binding declare them, the drop-in shells' methods, the demo as C++11, and the kernel file's place in the build."""
import ctypes
import os
import subprocess

from conftest import ROOT

CSRC = os.path.join(ROOT, "face-recognition-cpp-tensorrt_amd", "csrc")
DEMO = os.path.join(ROOT, "tests", "cpp", "separation_demo.cpp")
GXX = ["g++", "-std=c++11", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include")]


def test_separation_is_declared_exported_and_bound(frt):
    header = open(os.path.join(ROOT, "include", "frt.h")).read()
    for s, n_args in (("frt_matcher_separation", 9), ("frt_matcher_separation_dev", 10)):
        assert "int " + s + "(" in header
        assert hasattr(frt.lib, s), "libfrt.so does not export %s" % s
        assert s in frt.ABI and len(frt.ABI[s][1]) == n_args, "python binding misses %s" % s
        assert frt.ABI[s][0] is ctypes.c_int and frt.ABI[s][1][6] is ctypes.c_int  # (n_thresholds)
    assert callable(frt.MatMul.separation) and callable(frt.MatMul.separation_dev)
    assert len(frt.MatMul.SEPARATION_STATS) == 5
    # the header states what makes the call the calibration of the clustering threshold
    block = header[header.index("Leave-one-out genuine / impostor"):header.index("int frt_matcher_separation(")]
    for words in ("t* = max_i imp_sim[i]", "puts no two labels into one component", "merges the two identities of the arg-max pair",
                  "singleton component exactly when gen_sim[i] < t"):
        assert words in block


def test_separation_rejects_a_null_matcher(frt):
    assert frt.lib.frt_matcher_separation(None, None, None, None, None, None, 0, None, None) == frt.FRT_ERR_INVALID
    assert b"null argument" in frt.lib.frt_last_error()
    assert frt.lib.frt_matcher_separation_dev(None, None, None, None, None, None, 0, None, None, None) == frt.FRT_ERR_INVALID


def test_shell_headers_offer_the_separation_methods():
    mm = open(os.path.join(ROOT, "include", "frt", "matmul.h")).read()
    arc = open(os.path.join(ROOT, "include", "frt", "arcface.h")).read()
    assert "void separation(std::vector<float> &genSim, std::vector<int> &genRow, std::vector<float> &impSim, std::vector<int> &impRow," in mm
    assert "gallerySeparation(const std::vector<float> &thresholds" in arc


def test_separation_demo_is_well_formed_cpp11(tmp_path):
    subprocess.check_call(GXX + ["-c", DEMO, "-o", str(tmp_path / "separation_demo.o")])


def test_kernel_file_is_part_of_the_library_build():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "kernels_separation" in mk
    src = open(os.path.join(CSRC, "kernels_separation.hip")).read()
    for k in ("separation_genuine_kernel", "separation_reduce_kernel", "exact_row_dot("):
        assert k in src
    # the chain is shared with the pair re-rank, not restated
    assert "exact_row_dot(" in open(os.path.join(CSRC, "kernels_match.hip")).read()
    assert "__builtin_fmaf" not in src
