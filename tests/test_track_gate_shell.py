"""FaceTracker::gate (include/frt/tracker.h) and the ArcFaceIR50::trackFaces overload with the gate's options (include/frt/arcface.h) through
tests/cpp/track_gate_demo.cpp: well-formed C++11 against cvlite and against the OpenCV declarations mock, and linkable against the library
without a GPU."""
import os
import subprocess

from conftest import ROOT

PKG = os.path.join(ROOT, "face-recognition-cpp-tensorrt_amd")
SRC = os.path.join(ROOT, "tests", "cpp", "track_gate_demo.cpp")
GXX = ["g++", "-std=c++11", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include")]
LINK = [os.path.join(PKG, "libfrt.so"), "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"]


def test_track_gate_demo_is_well_formed_cpp11(tmp_path):
    subprocess.check_call(GXX + ["-c", SRC, "-o", str(tmp_path / "track_gate_demo.o")])
    mock = os.path.join(ROOT, "tests", "cpp", "opencv_decl_mock")
    out = subprocess.run(["g++", "-std=c++11", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-DFRT_EXPECT_OPENCV_BRANCH", "-I", mock, "-I",
                          os.path.join(ROOT, "include"), SRC], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr


def test_track_gate_demo_links_against_the_library(tmp_path):
    """every symbol the shell needs is exported: the demo links without a GPU"""
    subprocess.check_call(GXX + [SRC, "-o", str(tmp_path / "track_gate_demo")] + LINK)


def test_shell_headers_offer_the_method_and_the_overload():
    shell = open(os.path.join(ROOT, "include", "frt", "tracker.h")).read()
    assert "std::vector<frt_track_gate> gate(const std::vector<frt_bbox> &boxes, const frt_track_gate_options &options" in shell
    arc = open(os.path.join(ROOT, "include", "frt", "arcface.h")).read()
    assert "trackFaces(Detector &detector, FaceTracker &tracker, const frt_track_gate_options &options, const std::vector<cv::Mat> &frames" in arc
