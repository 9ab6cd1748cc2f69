"""RetinaFace::findFaceTiled (include/frt/retinaface.h) through tests/cpp/tiled_demo.cpp: well-formed C++11 against cvlite and against the
OpenCV declarations mock, and on the GPU the same boxes as the Python binding's findFaceTiled for a row-strided cv::Mat."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

PKG = os.path.join(ROOT, "face-recognition-cpp-tensorrt_amd")
SRC = os.path.join(ROOT, "tests", "cpp", "tiled_demo.cpp")
GXX = ["g++", "-std=c++11", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include")]


def test_tiled_demo_is_well_formed_cpp11(tmp_path):
    subprocess.check_call(GXX + ["-c", SRC, "-o", str(tmp_path / "tiled_demo.o")])
    mock = os.path.join(ROOT, "tests", "cpp", "opencv_decl_mock")
    out = subprocess.run(["g++", "-std=c++11", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-DFRT_EXPECT_OPENCV_BRANCH", "-I", mock, "-I",
                          os.path.join(ROOT, "include"), SRC], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr


def test_tiled_demo_links_against_the_library(tmp_path):
    """every symbol the method needs is exported: the demo links without a GPU"""
    subprocess.check_call(GXX + [SRC, "-o", str(tmp_path / "tiled_demo"), os.path.join(PKG, "libfrt.so"), "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])


def test_shell_header_offers_the_method_and_the_route_to_embeddings():
    shell = open(os.path.join(ROOT, "include", "frt", "retinaface.h")).read()
    assert "std::vector<struct Bbox> findFaceTiled(cv::Mat &photo, const frt_tile_options *options = nullptr, int maxOut = 256," in shell
    assert "rec.forward(photo, boxes)" in shell and "forwardAligned(photo, boxes, landmarks)" in shell


@pytest.mark.gpu
def test_shell_finds_what_the_python_binding_finds(frt, synth, blobs, tmp_path):
    dpath, _ = blobs("det")
    exe = str(tmp_path / "tiled_demo")
    subprocess.check_call(GXX + [SRC, "-o", exe, os.path.join(PKG, "libfrt.so"), "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    photo = synth.make_frames(1, 200, 410)[0]
    wide = np.zeros((200, 410 * 3 + 7), np.uint8)
    wide[:, :410 * 3] = photo.reshape(200, -1)
    (tmp_path / "photo.bin").write_bytes(wide.tobytes())
    det = frt.RetinaFace(dpath, 160, 96, (3, 96, 160), 4, 8, 0.4, 0.02)
    boxes, src = det.findFaceTiled(photo, overlap=32, overview=True, metric=1, drop_cut=False, max_out=64, sources=True)
    n_default = len(det.findFaceTiled(photo))
    det.close()
    assert len(boxes) > 3
    out = subprocess.run([exe, dpath, str(tmp_path / "photo.bin"), "200", "410", str(wide.shape[1]), "160", "96", "4", "8", "32", "1", "1", "0", "64"],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = [l.split() for l in out.stdout.splitlines()]
    got = [[int(v) for v in l[1:]] for l in lines if l[0] == "box"]
    want = [[int(b["x1"]), int(b["y1"]), int(b["x2"]), int(b["y2"]), int(np.float32(b["score"]).view(np.uint32)), int(s)] for b, s in zip(boxes, src)]
    assert got == want
    assert [l[1] for l in lines if l[0] == "default"] == [str(n_default)]
