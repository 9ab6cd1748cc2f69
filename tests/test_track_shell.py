"""FaceTracker (include/frt/tracker.h) and ArcFaceIR50::trackFaces (include/frt/arcface.h) through tests/cpp/track_demo.cpp: well-formed C++11
against cvlite and against the OpenCV declarations mock, linkable against the library without a GPU, and on the GPU the same track ids and
names as the Python binding's Pipeline.runTracked."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

PKG = os.path.join(ROOT, "face-recognition-cpp-tensorrt_amd")
SRC = os.path.join(ROOT, "tests", "cpp", "track_demo.cpp")
GXX = ["g++", "-std=c++11", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include")]
LINK = [os.path.join(PKG, "libfrt.so"), "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"]


def test_track_demo_is_well_formed_cpp11(tmp_path):
    subprocess.check_call(GXX + ["-c", SRC, "-o", str(tmp_path / "track_demo.o")])
    mock = os.path.join(ROOT, "tests", "cpp", "opencv_decl_mock")
    out = subprocess.run(["g++", "-std=c++11", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-DFRT_EXPECT_OPENCV_BRANCH", "-I", mock, "-I",
                          os.path.join(ROOT, "include"), SRC], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr


def test_track_demo_links_against_the_library(tmp_path):
    """every symbol the shell needs is exported: the demo links without a GPU"""
    subprocess.check_call(GXX + [SRC, "-o", str(tmp_path / "track_demo")] + LINK)


def test_shell_headers_offer_the_class_and_the_method():
    shell = open(os.path.join(ROOT, "include", "frt", "tracker.h")).read()
    assert "class FaceTracker" in shell and "std::vector<frt_track_result> update(" in shell and "void reset(int stream = -1)" in shell
    arc = open(os.path.join(ROOT, "include", "frt", "arcface.h")).read()
    assert "std::vector<frt_face_result> trackFaces(Detector &detector, FaceTracker &tracker, const std::vector<cv::Mat> &frames" in arc


@pytest.mark.gpu
def test_shell_reports_the_ids_and_names_of_the_python_binding(frt, synth, blobs, tmp_path):
    dpath, _ = blobs("det")
    rpath, _ = blobs("ir")
    exe = str(tmp_path / "track_demo")
    subprocess.check_call(GXX + [SRC, "-o", exe] + LINK)
    H, W, MF, CALLS, PER = 96, 160, 4, 3, 2
    first = synth.make_frames(PER, H, W)
    frames = np.stack([np.roll(first, 3 * c, axis=2) for c in range(CALLS)])      # [calls][frames][H][W][3]: the scene drifts 3 columns per call
    names = ["person%d" % i for i in range(9)]
    rng = np.random.default_rng(11)
    gal = rng.standard_normal((9, 512)).astype(np.float32)
    gal /= np.linalg.norm(gal, axis=1, keepdims=True)
    (tmp_path / "frames.bin").write_bytes(frames.tobytes())
    (tmp_path / "gallery.bin").write_bytes(gal.tobytes())
    (tmp_path / "names.txt").write_text("".join(n + "\n" for n in names))

    det = frt.RetinaFace(dpath, W, H, (3, H, W), PER, MF, 0.4, 0.02)
    rec = frt.ArcFaceIR50(rpath, W, H, (3, 112, 112), 512, PER * MF, MF, 0.65)
    rec.setGallery(gal, names)
    rec.initMatMul()
    pipe = frt.Pipeline(det, rec, PER)
    trk = frt.Tracker(PER, 8, MF)
    want = []
    for c in range(CALLS):
        res, _, tr, _ = pipe.runTracked(trk, frames[c])
        for k in range(PER * MF):
            t, r = tr.reshape(-1)[k], res[k]
            ok = 0 <= t["match_idx"] < len(names)
            want.append(["track", c, k // MF, k % MF, r["x1"], r["y1"], r["x2"], r["y2"], t["track_id"], t["slot"], t["age"], t["hits"], t["n_embeds"],
                         t["confirmed"], names[t["match_idx"]] if ok else "-", int(np.float32(t["match_sim"] if ok else 0).view(np.uint32))])
    for s in range(PER):
        slots, cnt = trk.tracks(s)
        want.append(["stream", s, cnt["next_id"], cnt["tick"], cnt["dropped"], int((slots["live"] != 0).sum())])
    assert any(row[0] == "track" and row[8] >= 0 and row[10] == CALLS for row in want)   # a track lived through every call
    trk.close(), pipe.close(), rec.close(), det.close()

    out = subprocess.run([exe, dpath, rpath, str(tmp_path / "frames.bin"), str(CALLS), str(PER), str(W), str(H), str(MF), str(PER * MF),
                          str(tmp_path / "gallery.bin"), "9", str(tmp_path / "names.txt"), "8"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    got = [l.split() for l in out.stdout.splitlines() if l.split()[0] in ("track", "stream")]
    assert got == [[str(v) for v in row] for row in want]
