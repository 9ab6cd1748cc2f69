"""MatMul::separation (include/frt/matmul.h) and ArcFaceIR50::gallerySeparation (include/frt/arcface.h) through tests/cpp/separation_demo.cpp,
against the Python binding's separation on the same rows and labels: 90 persons enrolled under one name per person."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

PKG = os.path.join(ROOT, "face-recognition-cpp-tensorrt_amd")
SRC = os.path.join(ROOT, "tests", "cpp", "separation_demo.cpp")
GXX = ["g++", "-std=c++11", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include")]


@pytest.mark.gpu
def test_shells_report_what_the_python_binding_reports(frt, blobs, tmp_path):
    rpath, _ = blobs("ir")
    exe = str(tmp_path / "separation_demo")
    subprocess.check_call(GXX + [SRC, "-o", exe, os.path.join(PKG, "libfrt.so"), "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    # 90 persons with 1 to 5 photos each, shuffled: unit centre + 0.5 x unit noise, re-normalised
    rng = np.random.Generator(np.random.PCG64(405))
    rows, labels = [], []
    for p in range(90):
        c = rng.standard_normal(512)
        c /= np.linalg.norm(c)
        for _ in range(1 + p % 5):
            u = rng.standard_normal(512)
            r = c + 0.5 * u / np.linalg.norm(u)
            rows.append(r / np.linalg.norm(r))
            labels.append(p)
    perm = rng.permutation(len(rows))
    rows = np.ascontiguousarray(np.array(rows)[perm], np.float32)
    labels = np.ascontiguousarray(np.array(labels)[perm], np.int32)
    n = len(rows)
    thr = np.array([0.3, 0.5, 0.9], np.float32)
    (tmp_path / "gal.bin").write_bytes(rows.tobytes())
    (tmp_path / "lab.bin").write_bytes(labels.tobytes())
    out = subprocess.run([exe, rpath, str(tmp_path / "gal.bin"), str(tmp_path / "lab.bin"), str(n)] + ["%.9g" % t for t in thr], capture_output=True,
                         text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = [l.split() for l in out.stdout.splitlines()]
    mm = frt.MatMul(0)
    mm.init(rows)
    mm.set_labels(labels)
    gs, gr, is_, ir, counts, stats = mm.separation(thr)
    mm.close()
    assert stats["genuine_rows"] == n - 18 and stats["impostor_rows"] == n  # 18 of the 90 persons have one photo
    got = {l[0]: l[1:] for l in lines if l[0] != "row"}
    want_stats = [stats[k] for k in frt.MatMul.SEPARATION_STATS]
    assert [int(v) for v in got["stats"]] == want_stats and [int(v) for v in got["shell_stats"]] == want_stats
    assert [int(v) for v in got["counts"]] == counts.reshape(-1).tolist() and [int(v) for v in got["shell_counts"]] == counts.reshape(-1).tolist()
    assert [int(v) for v in got["gen_row"]] == gr.tolist() and [int(v) for v in got["imp_row"]] == ir.tolist()
    # %.9g round-trips a float32; "-inf" parses as -inf
    assert np.array_equal(np.array([float(v) for v in got["gen_sim"]], np.float32), gs)
    assert np.array_equal(np.array([float(v) for v in got["imp_sim"]], np.float32), is_)
    shell = [l[1:] for l in lines if l[0] == "row"]
    assert [s[0] for s in shell] == ["p%d" % l for l in labels.tolist()]
    assert np.array_equal(np.array([float(s[1]) for s in shell], np.float32), gs) and np.array_equal(np.array([float(s[2]) for s in shell], np.float32), is_)
    assert [s[3] for s in shell] == ["p%d" % labels[r] for r in ir.tolist()]
