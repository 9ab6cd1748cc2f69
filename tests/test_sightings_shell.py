"""FaceSightings (include/frt/sightings.h) through tests/cpp/sightings_demo.cpp: well-formed C++11, linkable against the library without a
GPU - where creating a tracker and a book, and a refused creation, do no device work -, and on the GPU one face followed, closed and drained."""
import os
import subprocess

import pytest

from conftest import ROOT

PKG = os.path.join(ROOT, "face-recognition-cpp-tensorrt_amd")
SRC = os.path.join(ROOT, "tests", "cpp", "sightings_demo.cpp")
GXX = ["g++", "-std=c++11", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include")]
LINK = [os.path.join(PKG, "libfrt.so"), "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"]


def test_sightings_demo_compiles_links_and_runs_its_host_part(tmp_path):
    exe = str(tmp_path / "sightings_demo")
    subprocess.check_call(GXX + [SRC, "-o", exe] + LINK)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stdout == "book created\n", out.stdout + out.stderr


def test_shell_header_offers_the_class():
    shell = open(os.path.join(ROOT, "include", "frt", "sightings.h")).read()
    for decl in ("class FaceSightings", "std::vector<Sighting> drain(int maxOut", "void close(int stream = -1)", "std::vector<frt_sighting> open(int stream"):
        assert decl in shell, decl


@pytest.mark.gpu
def test_sightings_demo_follows_closes_and_drains_one_face(tmp_path):
    exe = str(tmp_path / "sightings_demo")
    subprocess.check_call(GXX + [SRC, "-o", exe] + LINK)
    out = subprocess.run([exe, "update"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.splitlines()[1] == "sighting track 0 ticks 0..2 reason 3 hits 3 shots 3 best tick 1 sharpness 9 crop 2 embed 1"
