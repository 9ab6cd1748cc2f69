"""FaceTracker::setMotion / getMotion / motion (include/frt/tracker.h) through tests/cpp/track_motion_demo.cpp: well-formed C++11 under -Wall
-Wextra -Werror, the settings part runs without a GPU (creation and the setter do no device work), and on the GPU one coasting return
through the shell."""
import os
import subprocess

import pytest

from conftest import ROOT

PKG = os.path.join(ROOT, "face-recognition-cpp-tensorrt_amd")
SRC = os.path.join(ROOT, "tests", "cpp", "track_motion_demo.cpp")
GXX = ["g++", "-std=c++11", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include")]
LINK = [os.path.join(PKG, "libfrt.so"), "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"]


def _build(tmp_path):
    exe = str(tmp_path / "track_motion_demo")
    subprocess.check_call(GXX + [SRC, "-o", exe] + LINK)
    return exe


def test_settings_round_trip_and_a_refused_set_throws(tmp_path):
    out = subprocess.run([_build(tmp_path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.splitlines() == ["motion 256"]


def test_shell_header_offers_the_methods():
    shell = open(os.path.join(ROOT, "include", "frt", "tracker.h")).read()
    assert "void setMotion(int gain)" in shell and "int getMotion()" in shell
    assert "std::vector<int32_t> motion(int stream, std::vector<frt_bbox> *predicted = nullptr)" in shell


@pytest.mark.gpu
def test_one_coasting_return_through_the_shell(tmp_path):
    out = subprocess.run([_build(tmp_path), "update"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.splitlines()[-1] == "track 0 0 how 1 gap 4 ovr 1 vel 2048 0 pred 56 103"
