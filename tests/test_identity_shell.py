"""ArcFaceIR50::matchTopIdentities (include/frt/arcface.h) through tests/cpp/identity_demo.cpp: a gallery whose classNames repeat, edited
with enrolEmbeddings / removeClass / a reload, against the Python binding's topk_labels on the same rows and names."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

PKG = os.path.join(ROOT, "face-recognition-cpp-tensorrt_amd")
SRC = os.path.join(ROOT, "tests", "cpp", "identity_demo.cpp")
GXX = ["g++", "-std=c++11", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include")]


def test_identity_demo_is_well_formed_cpp11(tmp_path):
    subprocess.check_call(GXX + ["-c", SRC, "-o", str(tmp_path / "identity_demo.o")])


def intern(names):
    """labels in first-appearance order, as the shell hands them to the matcher"""
    table = {}
    return np.array([table.setdefault(n, len(table)) for n in names], np.int32)


def python_answer(frt, mm, rows, names, emb, k):
    mm.init(np.ascontiguousarray(rows, np.float32))
    mm.set_labels(intern(names))
    lab, idx, sim = mm.topk_labels(emb, k)
    return [(names[i], float(s)) for l, i, s in zip(lab[0], idx[0], sim[0]) if l >= 0]


@pytest.mark.gpu
@pytest.mark.parametrize("k", [3, 16])
def test_match_top_identities_names_equal_the_python_result(frt, synth, blobs, tmp_path, k):
    rpath, _ = blobs("ir")
    exe = str(tmp_path / "identity_demo")
    subprocess.check_call(GXX + [SRC, "-o", exe, os.path.join(PKG, "libfrt.so"), "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    N = 400
    face = synth.make_frame(11, 112, 112)
    boxes = np.zeros(1, frt.BBOX_DTYPE)
    boxes[0] = (0, 0, 112, 112, 1.0)
    rec = frt.ArcFaceIR50(rpath, 640, 480, (3, 112, 112), 512, 1, 4, 0.65)
    emb = rec.forward(face, boxes).copy()
    rec.close()
    # four faces per user ("u<i % 100>"); the face itself is row 10, a second photo of that user is row 110, user 55 looks alike, and for
    # k = 16 > 10 users of the half-size reload the lists run short there
    gal = synth.make_gallery(N)
    gal[10] = emb[0]
    gal[110] = synth.make_queries(emb, [0], noise=0.01, seed=1)[0]
    gal[55] = synth.make_queries(emb, [0], noise=0.03, seed=2)[0]
    names = ["u%d" % (i % (100 if k == 3 else 10)) for i in range(N)]
    (tmp_path / "face.bin").write_bytes(face.tobytes())
    (tmp_path / "gal.bin").write_bytes(gal.tobytes())
    (tmp_path / "emb.bin").write_bytes(emb[0].tobytes())
    (tmp_path / "names.txt").write_text("".join(n + "\n" for n in names))
    out = subprocess.run([exe, rpath, str(tmp_path / "face.bin"), str(tmp_path / "gal.bin"), str(N), str(tmp_path / "names.txt"), str(k),
                          str(tmp_path / "emb.bin")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    got = []
    for l in (l.split() for l in out.stdout.splitlines() if l.startswith("step")):
        assert len(l) == 3 + 2 * int(l[2])
        got.append([(l[3 + 2 * j], float(l[4 + 2 * j])) for j in range(int(l[2]))])
    assert len(got) == 4
    # the same four galleries through the Python binding
    mm = frt.MatMul(0)
    rows, who = [gal], list(names)
    want = [python_answer(frt, mm, gal, who, emb, k)]
    rows = np.concatenate([gal, emb[:1], gal[7:8]])
    who = who + [names[55], "zed"]
    want.append(python_answer(frt, mm, rows, who, emb, k))
    keep = [i for i, n in enumerate(who) if n != names[10]]
    rows, who = rows[keep], [who[i] for i in keep]
    want.append(python_answer(frt, mm, rows, who, emb, k))
    want.append(python_answer(frt, mm, gal[:N // 2], names[:N // 2], emb, k))
    mm.close()
    for step, (g, w) in enumerate(zip(got, want)):
        assert [n for n, _ in g] == [n for n, _ in w], step
        assert np.abs(np.array([s for _, s in g]) - np.array([s for _, s in w])).max() < 1e-5, step
    assert got[0][0][0] == names[10] and got[1][1][0] == names[55] and got[2][0][0] == names[55]
    assert len(got[0]) == min(k, len(set(names))) and len(got[3]) == min(k, len(set(names[:N // 2])))
