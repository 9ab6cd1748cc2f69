"""MatMul::cluster (include/frt/matmul.h) and ArcFaceIR50::clusterGallery (include/frt/arcface.h) through tests/cpp/cluster_demo.cpp, against
the Python binding's cluster on the same rows: a photo dump enrolled under one name per row comes back grouped into persons, and with
install the shell's template audit lists exactly those persons."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

PKG = os.path.join(ROOT, "face-recognition-cpp-tensorrt_amd")
SRC = os.path.join(ROOT, "tests", "cpp", "cluster_demo.cpp")
GXX = ["g++", "-std=c++11", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include")]


def test_cluster_demo_is_well_formed_cpp11(tmp_path):
    subprocess.check_call(GXX + ["-c", SRC, "-o", str(tmp_path / "cluster_demo.o")])


def test_shell_headers_offer_the_cluster_methods():
    mm = open(os.path.join(ROOT, "include", "frt", "matmul.h")).read()
    arc = open(os.path.join(ROOT, "include", "frt", "arcface.h")).read()
    assert "void cluster(float threshold, std::vector<int> &labels, bool install = false" in mm
    assert "std::vector<int> clusterGallery(float threshold, bool install = false)" in arc


@pytest.mark.gpu
def test_shells_cluster_like_the_python_binding(frt, blobs, tmp_path):
    rpath, _ = blobs("ir")
    exe = str(tmp_path / "cluster_demo")
    subprocess.check_call(GXX + [SRC, "-o", exe, os.path.join(PKG, "libfrt.so"), "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    # 90 persons with 1 to 5 photos each, interleaved: unit centre + 0.5 x unit noise, re-normalised (photos of a person at 0.8, strangers near 0)
    rng = np.random.Generator(np.random.PCG64(404))
    rows = []
    for p in range(90):
        c = rng.standard_normal(512)
        c /= np.linalg.norm(c)
        for _ in range(1 + p % 5):
            u = rng.standard_normal(512)
            r = c + 0.5 * u / np.linalg.norm(u)
            rows.append(r / np.linalg.norm(r))
    rows = np.ascontiguousarray(np.array(rows)[rng.permutation(len(rows))], np.float32)
    n, t = len(rows), np.float32(0.5)
    s = (rows.astype(np.float64) @ rows.astype(np.float64).T)[np.triu_indices(n, 1)]
    assert np.abs(s - 0.5).min() > 1e-4
    (tmp_path / "gal.bin").write_bytes(rows.tobytes())
    out = subprocess.run([exe, rpath, str(tmp_path / "gal.bin"), str(n), "%.9g" % t], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = [l.split() for l in out.stdout.splitlines()]
    mm = frt.MatMul(0)
    mm.init(rows)
    labels, stats = mm.cluster(t)
    mm.close()
    assert stats["clusters"] == 90 and stats["edges"] == sum(m * (m - 1) // 2 for m in (1 + p % 5 for p in range(90)))
    got = {l[0]: l[1:] for l in lines if l[0] in ("matmul", "labels", "shell")}
    assert [int(v) for v in got["matmul"]] == [stats[k] for k in frt.MatMul.CLUSTER_STATS]
    assert [int(v) for v in got["labels"]] == labels.tolist() and [int(v) for v in got["shell"]] == labels.tolist()
    # the audit after install: one entry per person in first-appearance order, named by its first row, with its number of photos
    first = [int(l) for i, l in enumerate(labels.tolist()) if l == i]
    counts = np.bincount(labels)
    assert [(l[1], int(l[2])) for l in lines if l[0] == "person"] == [("u%d" % r, int(counts[r])) for r in first]
