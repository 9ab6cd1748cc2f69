"""Face images instead of frames: frt_preprocess_faces / frt_embedder_embed_faces / frt_embedder_enrol_faces and their shells
(preprocessFaces, ArcFaceIR50.forwardFaces / enrolFaces) - what /recognize (src/app.cpp:243-287), /insert/face with api_imgIsCropped
(:148-162) and the gen mode (:69-99) do per image, for ragged batches."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, face_input

pytestmark = pytest.mark.gpu

PKG = os.path.join(ROOT, "face-recognition-cpp-tensorrt_amd")
SIZES = [(1, 1), (1, 7), (9, 1), (56, 56), (112, 112), (224, 224), (448, 448), (113, 111), (37, 201), (333, 500)]


def intern(names):
    """labels in first-appearance order, as the C++ shell hands them to the matcher"""
    table = {}
    return np.array([table.setdefault(n, len(table)) for n in names], np.int32)


@pytest.fixture(scope="module")
def ragged(synth, orc):
    """The eleven images of the issue - ten sizes and one 50x61 view of a 50x80 array (padded stride) - with the oracle's
    cv::resize(INTER_LINEAR) + preprocessFace of each.  Shared, never modified."""
    rng = np.random.default_rng(20240611)
    imgs = [synth.make_frame(100 + i, r, c) if min(r, c) >= 32 else rng.integers(0, 256, (r, c, 3), dtype=np.uint8) for i, (r, c) in enumerate(SIZES)]
    imgs.append(synth.make_frame(77, 50, 80)[:, :61])
    assert imgs[-1].strides[0] == 240 and not imgs[-1].flags.c_contiguous
    crops = np.stack([orc.resize_linear(im, 112, 112) for im in imgs])
    chw = orc.face_normalize(crops)
    for a in imgs + [crops, chw]:
        a.flags.writeable = False
    return imgs, crops, chw


def test_prepare_kernel_is_the_oracle_bit_for_bit(frt, ragged):
    """One ragged call: crops == oracle.resize_linear, chw == oracle.face_normalize(crops); 112^2 is a copy, 224^2 the 2x2 mean, 1x1 constant."""
    imgs, ocrops, ochw = ragged
    crops, chw = frt.preprocessFaces(imgs)
    for i, im in enumerate(imgs):
        assert np.array_equal(crops[i], ocrops[i]), (i, im.shape)
        assert np.array_equal(chw[i], ochw[i]), (i, im.shape)
    assert np.array_equal(crops[4], imgs[4])
    assert (crops[0] == imgs[0][0, 0]).all()
    q = imgs[5].astype(np.int32)
    assert np.array_equal(crops[5], ((q[0::2, 0::2] + q[0::2, 1::2] + q[1::2, 0::2] + q[1::2, 1::2] + 2) >> 2).astype(np.uint8))
    # either output alone
    only = np.zeros_like(crops)
    arr, keep = frt._face_images(imgs)
    assert frt.lib.frt_preprocess_faces(arr, len(keep), only.ctypes.data, None, 0) == frt.FRT_OK and np.array_equal(only, ocrops)
    only_chw = np.zeros_like(chw)
    assert frt.lib.frt_preprocess_faces(arr, len(keep), None, only_chw.ctypes.data, 0) == frt.FRT_OK and np.array_equal(only_chw, ochw)


@pytest.mark.parametrize("kind", ["ir", "ir_se"])
def test_forward_faces_is_the_existing_path_on_the_same_crops(frt, ragged, blobs, kind):
    """forwardFaces with maxBatchSize 4 (chunks 4 + 4 + 3) == doInference(face_input(crops)) on the same object, bit for bit, and agrees with
    the oracle's network as test_gpu_embedder.py asks of forward()."""
    from oracle import nets
    imgs, ocrops, ochw = ragged
    path, sd = blobs(kind)
    rec = frt.ArcFaceIR50(path, maxBatchSize=4)
    emb = rec.forwardFaces(imgs).copy()
    assert len(rec.croppedFaces) == len(imgs)
    for i, c in enumerate(rec.croppedFaces):
        assert np.array_equal(c["face"], ocrops[i]) and (c["x1"], c["y1"], c["x2"], c["y2"]) == (0, 0, 112, 112)
    assert np.array_equal(emb, rec.doInference(face_input(ocrops)))
    cos = (emb * nets.arcface_forward(sd, ochw.copy())).sum(1)
    print("cosine vs oracle (%s): min %.8f" % (kind, cos.min()))
    assert cos.min() > 1 - 1e-4
    assert np.array_equal(rec.forwardFaces(imgs), emb)                   # a second call reuses the staging
    assert rec.forwardFaces([]).shape == (0, 512) and rec.croppedFaces == []
    rec.close()


def test_forward_faces_in_fp32_mode(frt, ragged, blobs):
    from oracle import nets
    imgs, ocrops, ochw = ragged
    path, sd = blobs("ir")
    rec = frt.ArcFaceIR50(path, maxBatchSize=4)
    rec.setPrecision(True)
    pick = [3, 7, 10]
    emb = rec.forwardFaces([imgs[i] for i in pick])
    assert np.array_equal(emb, rec.doInference(face_input(ocrops[pick])))
    cos = (emb * nets.arcface_forward(sd, ochw[pick])).sum(1)
    print("cosine vs oracle (fp32): min %.8f" % cos.min())
    assert cos.min() > 1 - 1e-4
    rec.close()


def test_byte_cap_cuts_a_batch_of_large_images(frt, orc, blobs):
    """Twelve 1080x1920 images are 75 MB: over the 64 MiB staging cap, so maxBatchSize 16 does not decide the chunks (10 + 2)."""
    rng = np.random.default_rng(7)
    imgs = [rng.integers(0, 256, (1080, 1920, 3), dtype=np.uint8) for _ in range(12)]
    path, _ = blobs("ir")
    rec = frt.ArcFaceIR50(path, maxBatchSize=16)
    emb = rec.forwardFaces(imgs)
    crops = np.stack([c["face"] for c in rec.croppedFaces])
    for i, im in enumerate(imgs):
        assert np.array_equal(crops[i], orc.resize_linear(im, 112, 112)), i
    want = rec.doInference(face_input(crops))  # one pass of 12: another chunking
    cos, diff = (emb * want).sum(1).min(), np.abs(emb - want).max()
    print("chunks 10 + 2 vs one pass of 12: min cosine %.8f, max |d| %.3g" % (cos, diff))
    assert cos > 1 - 1e-5 and diff < 1e-3
    rec.close()


@pytest.mark.parametrize("labelled", [False, True], ids=["unlabelled", "labelled"])
def test_enrol_faces_is_one_gallery_edit(frt, synth, ragged, blobs, labelled):
    imgs, _, _ = ragged
    faces = [imgs[3], imgs[4], imgs[7], imgs[9], imgs[10]]
    new_names = ["u3", "new", "new", "u7", "zed"]
    path, _ = blobs("ir")
    N = 400
    gal = synth.make_gallery(N)
    names = ["u%d" % (i % 100) for i in range(N)]
    rec = frt.ArcFaceIR50(path, maxBatchSize=2)
    rec.setGallery(gal, list(names))
    rec.initMatMul()
    mm = rec.matmul
    all_labels = intern(names + new_names)
    if labelled:
        mm.set_labels(all_labels[:N])
    else:  # a labelled call on an unlabelled gallery: refused, nothing changed
        with pytest.raises(frt.FrtError) as err:
            rec.enrolFaces(new_names, faces, labels=all_labels[N:])
        assert err.value.code == frt.FRT_ERR_INVALID and frt.lib.frt_matcher_num_rows(mm._h) == N and rec.classCount == N
    gen = mm.generation()
    first, emb = rec.enrolFaces(new_names, faces, labels=all_labels[N:] if labelled else None)
    assert first == N and frt.lib.frt_matcher_num_rows(mm._h) == N + 5 == mm.m and mm.generation() == gen + 1
    assert rec.classNames[N:] == new_names and rec.classCount == N + 5
    assert np.array_equal(emb, rec.forwardFaces(faces))
    fresh = frt.MatMul(0)
    fresh.init(np.concatenate([gal, emb]))
    idx, sim = mm.top1(emb)
    assert idx.tolist() == list(range(N, N + 5)) and sim.min() > 0.999
    widx, wsim = fresh.top1(emb)
    assert np.array_equal(idx, widx) and np.array_equal(sim, wsim)
    if labelled:
        fresh.set_labels(all_labels)
        lab, idx, sim = mm.topk_labels(emb, 3)
        assert idx[:, 0].tolist() == list(range(N, N + 5)) and sim[:, 0].min() > 0.999 and lab[:, 0].tolist() == all_labels[N:].tolist()
        wlab, widx, wsim = fresh.topk_labels(emb, 3)
        assert np.array_equal(lab, wlab) and np.array_equal(idx, widx) and np.array_equal(sim, wsim)
        with pytest.raises(frt.FrtError) as err:  # and the reverse mismatch
            rec.enrolFaces(new_names, faces)
        assert err.value.code == frt.FRT_ERR_INVALID and frt.lib.frt_matcher_num_rows(mm._h) == N + 5
    # too many images for one call: refused before anything runs
    arr, keep = frt._face_images([imgs[0]])
    many = (frt.FaceImage * 65537)(*([arr[0]] * 65537))
    assert frt.lib.frt_embedder_enrol_faces(rec._h, mm._h, many, 65537, None, None, None) == frt.FRT_ERR_CAPACITY
    assert frt.lib.frt_matcher_num_rows(mm._h) == N + 5
    fresh.close()
    rec.close()


def test_forward_faces_beside_a_pipeline_in_flight(frt, synth, ragged, blobs):
    import torch
    imgs, _, _ = ragged
    dpath, _ = blobs("det")
    rpath, _ = blobs("ir")
    B, K, H, W = 2, 4, 160, 224
    det = frt.RetinaFace(dpath, W, H, (3, H, W), B, K, 0.4, 0.6)
    rec = frt.ArcFaceIR50(rpath, W, H, maxBatchSize=B * K, maxFacesPerScene=K)
    rec.setGallery(synth.make_gallery(2000))
    rec.initMatMul()
    pipe = frt.Pipeline(det, rec, B)
    batches = [synth.make_frames(B, H, W, start=5 * i) for i in range(3)]
    want = [tuple(a.copy() for a in pipe.run(b)) for b in batches]
    want_emb = rec.forwardFaces(imgs).copy()  # chunks 8 + 3
    pinned = [torch.from_numpy(b).pin_memory() for b in batches]
    res = [torch.zeros(B * K * frt.RESULT_DTYPE.itemsize, dtype=torch.uint8).pin_memory() for _ in batches]
    emb = [torch.zeros(B * K, 512).pin_memory() for _ in batches]
    tickets = [pipe.submit(pinned[i].numpy(), res[i].numpy().view(frt.RESULT_DTYPE), emb[i].numpy()) for i in range(3)]
    got_emb = rec.forwardFaces(imgs)
    for t in tickets:
        pipe.wait(t)
    assert np.array_equal(got_emb, want_emb)
    for i in range(3):
        assert np.array_equal(res[i].numpy().view(frt.RESULT_DTYPE), want[i][0]), i
        assert np.array_equal(emb[i].numpy(), want[i][1]), i
    pipe.close()
    det.close()
    rec.close()


def test_cpp_shell_answers_equal_the_python_binding(frt, synth, ragged, blobs, tmp_path):
    """tests/cpp/faces_demo.cpp: forwardFaces + matchTopIdentities, then enrolFaces, on the same bytes as the Python binding."""
    imgs, _, _ = ragged
    faces = [imgs[4], imgs[8], imgs[10], imgs[5]]  # 112^2, 37x201, the strided view, 224^2
    enrol_names = ["u3", "new", "new", "zed"]
    rpath, _ = blobs("ir")
    exe = str(tmp_path / "faces_demo")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "faces_demo.cpp"), "-o", exe, os.path.join(PKG, "libfrt.so"), "-Wl,-rpath," + PKG,
                           "-Wl,-rpath,/opt/rocm/lib"])
    N, k = 400, 3
    rec = frt.ArcFaceIR50(rpath, 640, 480, (3, 112, 112), 512, 2, 4, 0.65)
    emb = rec.forwardFaces(faces).copy()
    rec.close()
    gal = synth.make_gallery(N)
    gal[10] = emb[0]
    gal[110] = synth.make_queries(emb, [0], noise=0.01, seed=1)[0]
    gal[55] = synth.make_queries(emb, [1], noise=0.02, seed=2)[0]
    names = ["u%d" % (i % 100) for i in range(N)]
    blob = [np.int32(len(faces)).tobytes()]
    for f in faces:  # rows, cols, row stride, then the rows with their padding
        padded = np.zeros((f.shape[0], f.strides[0]), np.uint8)
        padded[:, :f.shape[1] * 3] = f.reshape(f.shape[0], -1)
        blob.append(np.array([f.shape[0], f.shape[1], f.strides[0]], np.int32).tobytes())
        blob.append(padded.tobytes())
    (tmp_path / "faces.bin").write_bytes(b"".join(blob))
    (tmp_path / "gal.bin").write_bytes(gal.tobytes())
    (tmp_path / "names.txt").write_text("".join(n + "\n" for n in names))
    (tmp_path / "enrol.txt").write_text("".join(n + "\n" for n in enrol_names))
    out = subprocess.run([exe, rpath, str(tmp_path / "faces.bin"), str(tmp_path / "gal.bin"), str(N), str(tmp_path / "names.txt"), str(k),
                          str(tmp_path / "enrol.txt"), "2"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    got = {"forward": [], "enrol": []}
    for l in (l.split() for l in out.stdout.splitlines() if l.split(" ")[0] in got):
        assert len(l) == 3 + 2 * int(l[2]) and int(l[1]) == len(got[l[0]])
        got[l[0]].append([(l[3 + 2 * j], float(l[4 + 2 * j])) for j in range(int(l[2]))])
    mm = frt.MatMul(0)
    for tag, rows, who in (("forward", gal, names), ("enrol", np.concatenate([gal, emb]), names + enrol_names)):
        mm.init(np.ascontiguousarray(rows, np.float32))
        mm.set_labels(intern(who))
        lab, idx, sim = mm.topk_labels(emb, k)
        assert len(got[tag]) == len(faces), out.stdout
        for i in range(len(faces)):
            want = [(who[r], float(s)) for l, r, s in zip(lab[i], idx[i], sim[i]) if l >= 0]
            assert [n for n, _ in got[tag][i]] == [n for n, _ in want], (tag, i)
            assert np.abs(np.array([s for _, s in got[tag][i]]) - np.array([s for _, s in want])).max() < 1e-5, (tag, i)
    mm.close()
    assert got["forward"][0][0][0] == names[10] and got["forward"][1][0][0] == names[55]
    assert [g[0][0] for g in got["enrol"]][1:] == ["new", "new", "zed"] and got["enrol"][0][0][0] in ("u3", names[10])
