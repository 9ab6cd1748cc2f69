"""ArcFaceIR50::faceQuality and the gated enrolImages overload (include/frt/arcface.h) through tests/cpp/quality_demo.cpp: well-formed C++11
against cvlite and against the OpenCV declarations mock, and linkable against the library without a GPU.  Compile-only: what the calls
compute is tests/test_gpu_quality.py's."""
import os
import subprocess

from conftest import ROOT

PKG = os.path.join(ROOT, "face-recognition-cpp-tensorrt_amd")
SRC = os.path.join(ROOT, "tests", "cpp", "quality_demo.cpp")
GXX = ["g++", "-std=c++11", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include")]
LINK = [os.path.join(PKG, "libfrt.so"), "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"]


def test_quality_demo_is_well_formed_cpp11(tmp_path):
    subprocess.check_call(GXX + ["-c", SRC, "-o", str(tmp_path / "quality_demo.o")])
    mock = os.path.join(ROOT, "tests", "cpp", "opencv_decl_mock")
    out = subprocess.run(["g++", "-std=c++11", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-DFRT_EXPECT_OPENCV_BRANCH", "-I", mock, "-I",
                          os.path.join(ROOT, "include"), SRC], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr


def test_quality_demo_links_against_the_library(tmp_path):
    """every symbol the shell needs is exported: the demo links without a GPU"""
    subprocess.check_call(GXX + [SRC, "-o", str(tmp_path / "quality_demo")] + LINK)


def test_the_header_is_plain_c(tmp_path):
    """struct frt_face_quality shares its name with the host entry point: the header must still be C, and say how to spell the type"""
    src = tmp_path / "c.c"
    src.write_text('#include "frt.h"\nint main(void) { struct frt_face_quality q; frt_quality_options o; (void)o; return (int)sizeof q - 56; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "c")])
    assert subprocess.call([str(tmp_path / "c")]) == 0


def test_shell_header_offers_the_records_and_the_methods():
    arc = open(os.path.join(ROOT, "include", "frt", "arcface.h")).read()
    assert "struct FaceQuality : frt_face_quality" in arc and "struct QualityOptions : frt_quality_options" in arc
    assert "std::vector<FaceQuality> faceQuality(const QualityOptions &options = QualityOptions(), const std::vector<struct Bbox> *boxes = nullptr)" in arc
    assert "const QualityOptions &quality, std::vector<FaceQuality> &qualityOut, float *embeddingsOut = nullptr)" in arc
