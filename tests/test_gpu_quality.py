"""Face quality on the GPU (frt_face_quality*, frt_enrol_select_gated_dev, frt_pipeline_run_quality, frt_pipeline_enrol_images_gated and
their Python shells) against tests/quality_ref.py, the numpy restatement of include/frt.h "Face quality".  Whole records are compared by
their bytes: the sums are integers and the three floats are one float64 division of exact integers each, so there is no tolerance."""
import numpy as np
import pytest

import quality_ref as qr
from test_gpu_images import B, H, K, PHOTOS, W, close, injected, make_pipeline

pytestmark = pytest.mark.gpu

OK, LOW = qr.ENROL_OK, qr.ENROL_LOW_QUALITY
N_MAX = 130  # not a multiple of anything the kernel counts in
# thresholds that raise every bit on some crop of the set below and leave others passing (asserted on the ref's side, before the GPU is asked)
GATE = dict(min_size=30, min_sharpness=1000.0, min_luma_var=100.0, min_mean=20.0, max_mean=200.0, max_clipped=6000, min_score=0.5)


def same_bytes(got, want, what):
    if got.tobytes() == want.tobytes():
        return
    for i in range(len(want)):
        if got[i].tobytes() != want[i].tobytes():
            raise AssertionError("%s: record %d differs\n got  %s\n want %s" % (what, i, got[i], want[i]))
    raise AssertionError("%s: %d records against %d" % (what, len(got), len(want)))


@pytest.fixture(scope="module")
def crop_set():
    """130 crops - the hand cases of tests/test_quality_ref.py, seeded noise, the same noise box-blurred, a crop with one channel constant,
    then more noise and blurred noise under other seeds - and their records: every fifth small, every seventh with a low score, every
    third (i % 3 == 2) absent.  The ref's answers are computed once per call shape and shared."""
    hand = [qr.constant(255, 255, 255), qr.constant(0, 0, 0), qr.checkerboard(), qr.constant(255, 0, 0), qr.constant(0, 255, 0), qr.constant(0, 0, 255),
            qr.single_pixel(0, 0), qr.single_pixel(1, 1), qr.single_pixel(0, 1), qr.noise(7), qr.box_blur5(qr.noise(7)), qr.one_channel_constant()]
    more = [qr.noise(100 + i) if i % 2 else qr.box_blur5(qr.noise(100 + i)) for i in range(N_MAX - len(hand))]
    crops = np.stack(hand + more)
    rec = np.zeros(N_MAX, qr.RESULT_DTYPE)
    i = np.arange(N_MAX)
    side = np.where(i % 5 == 0, 20, 60)
    rec["x1"], rec["y1"], rec["x2"], rec["y2"] = 10, 20, 10 + side, 20 + side + 5
    rec["score"] = np.where(i % 7 == 0, np.float32(0.3), np.float32(0.9))
    rec["frame"], rec["match_idx"], rec["match_sim"] = i % 4, -1, 0
    rec["valid"] = np.where(i % 3 == 2, 0, 1)
    masked = crops.copy()
    masked[rec["valid"] == 0] = 0xFF      # an absent slot's crop is not read: whatever it holds, the record is zero
    want = {(r, g): qr.quality(crops, rec if r else None, qr.options(**GATE) if g else None) for r in (False, True) for g in (False, True)}
    # the gate does what the test needs it to do
    for r in (False, True):
        assert want[r, False]["flags"].max() == 0                                      # the defaults flag nothing
        assert qr.passes(want[r, True]).any() and not qr.passes(want[r, True]).all()
    seen = int(np.bitwise_or.reduce(want[True, True]["flags"]))
    assert seen == 127, seen                                                           # every bit on some crop
    assert int(np.bitwise_or.reduce(want[False, True]["flags"])) == 127 & ~(qr.SMALL | qr.LOW_SCORE)
    assert (want[True, False][rec["valid"] == 0].view(np.uint8) == 0).all() and (want[True, False]["present"] == rec["valid"]).all()
    sharp, soft = want[False, False]["sharpness"][9], want[False, False]["sharpness"][10]
    print("sharpness of the noise crop %.1f, of the same crop blurred %.1f" % (sharp, soft))
    assert soft < GATE["min_sharpness"] < sharp
    for a in (crops, masked, rec):
        a.flags.writeable = False
    return dict(crops=crops, masked=masked, rec=rec, want=want)


@pytest.mark.parametrize("n", [1, 3, N_MAX])
def test_the_kernel_alone_by_its_bytes(frt, crop_set, n):
    opt = frt.QualityOptions(**GATE)
    for records in (False, True):
        crops = crop_set["masked" if records else "crops"][:n]
        rec = crop_set["rec"][:n] if records else None
        for gate in (False, True):
            got = frt.faceQuality(crops, rec, opt if gate else None)
            same_bytes(got, crop_set["want"][records, gate][:n], "n %d records %s gate %s" % (n, records, gate))
    assert frt.faceQuality(np.zeros((0, 112, 112, 3), np.uint8)).shape == (0,)


def test_the_hand_cases_on_the_device(frt, crop_set):
    q = frt.faceQuality(crop_set["crops"][:12])
    assert q["sum_y2"][0] == 815673600 and q["n_bright"][0] == 12544 and q["luma_var"][0] == 0 and q["sharpness"][0] == 0
    assert q[1]["present"] == 1 and q["sum_y"][1] == 0 and q["n_dark"][1] == 12544
    c = q[2]
    assert (c["sum_y"], c["sum_lap"], c["sum_lap2"], c["n_dark"], c["n_bright"]) == (1599360, 0, 12588840000, 6272, 6272)
    assert c["luma_var"] == np.float32(16256.25) and c["sharpness"] == np.float32(1040400.0)
    assert [int(v) // 12544 for v in q["sum_y"][3:6]] == [29, 149, 77]
    assert q["sum_lap2"][6] == 0 and q["sum_lap2"][7] == 1020 * 1020 + 2 * 255 * 255 and q["sum_lap2"][8] == 255 * 255


def test_the_device_form_on_another_stream(frt, crop_set):
    import torch
    dev = torch.device("cuda:0")
    side = torch.cuda.Stream(device=dev)
    n = 37
    opt = frt.QualityOptions(**GATE)
    d_crops = torch.from_numpy(crop_set["masked"][:n].copy()).to(dev)
    d_rec = torch.from_numpy(crop_set["rec"][:n].view(np.uint8).reshape(-1).copy()).to(dev)
    for records in (False, True):
        src = d_crops if records else torch.from_numpy(crop_set["crops"][:n].copy()).to(dev)
        for stream in (None, side):
            out = torch.full((n * 56 + 56,), 0xA5, dtype=torch.uint8, device=dev)
            torch.cuda.synchronize()
            frt.face_quality_dev(src.data_ptr(), d_rec.data_ptr() if records else None, n, out.data_ptr(), opt, stream.cuda_stream if stream else None)
            torch.cuda.synchronize()
            got = out.cpu().numpy()
            same_bytes(got[:n * 56].view(qr.QUALITY_DTYPE), crop_set["want"][records, True][:n], "dev records %s stream %s" % (records, stream is not None))
            assert (got[n * 56:] == 0xA5).all()        # nothing behind record n - 1
    out = torch.full((56,), 0xA5, dtype=torch.uint8, device=dev)
    frt.face_quality_dev(d_crops.data_ptr(), None, 0, out.data_ptr())   # n == 0 does nothing
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 0xA5).all()


@pytest.mark.parametrize("max_faces", [1, 4])
def test_the_gated_selection_alone(frt, max_faces):
    import torch
    rng = np.random.default_rng(501 + max_faces)
    dev = torch.device("cuda:0")
    n = 61
    rec, emb, status, face, rows = injected(frt, rng, n, max_faces)
    ok = np.flatnonzero(status == OK)
    assert len(ok) >= 6
    ql = np.zeros((n, max_faces), qr.QUALITY_DTYPE)
    ql["present"] = rec["valid"] != 0
    on0 = ok[::3]                                     # flags on slot 0 of some OK frames ...
    ql["flags"][on0, 0] = qr.BLURRED
    if max_faces > 1:
        ql["flags"][ok[1::3], 1] = qr.DARK | qr.FLAT  # ... on slot 1 of others: only slot 0 counts
    not_ok = np.flatnonzero(status != OK)
    ql["flags"][not_ok, 0] = qr.CLIPPED               # a frame that is not OK keeps its status
    want_status = qr.enrol_select(rec, ql)
    assert np.array_equal(want_status, np.where(np.isin(np.arange(n), on0), LOW, status)) and np.array_equal(qr.enrol_select(rec), status)
    keep = np.ones(len(ok), bool)
    keep[::3] = False

    d_rec = torch.from_numpy(rec.view(np.uint8).reshape(-1).copy()).to(dev)
    d_emb = torch.from_numpy(emb).to(dev)
    d_ql = torch.from_numpy(ql.view(np.uint8).reshape(-1).copy()).to(dev)

    def run(fn, *tail):
        d_rows = torch.full((n + 2, 512), -7.0, device=dev)
        d_count = torch.tensor([1], dtype=torch.int32, device=dev)
        d_status = torch.full((n,), -1, dtype=torch.int32, device=dev)
        d_face = torch.zeros(n * frt.RESULT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        fn(d_rec.data_ptr(), d_emb.data_ptr(), n, max_faces, d_status.data_ptr(), d_face.data_ptr(), d_rows.data_ptr(), d_count.data_ptr(), None, *tail)
        torch.cuda.synchronize()
        return d_status.cpu().numpy(), d_face.cpu().numpy(), d_rows.cpu().numpy(), int(d_count.item())

    plain = run(frt.enrol_select_dev)
    null = run(frt.enrol_select_gated_dev, None)
    for a, b in zip(plain[:3], null[:3]):
        assert a.tobytes() == b.tobytes()              # a null quality_dev: frt_enrol_select_dev's bytes
    assert plain[3] == null[3] == 1 + len(ok) and np.array_equal(plain[0], status)
    gst, gface, grows, gcount = run(frt.enrol_select_gated_dev, d_ql.data_ptr())
    assert np.array_equal(gst, want_status)
    assert gface.tobytes() == plain[1].tobytes()       # the face of a LOW_QUALITY frame is written as for OK
    assert gcount == 1 + int(keep.sum()) and np.array_equal(grows[1:gcount], rows[keep]) and (grows[gcount:] == -7.0).all() and (grows[0] == -7.0).all()


def test_run_quality_is_run_with_the_records_behind_it(frt, synth, blobs):
    det, rec, pipe = make_pipeline(frt, blobs, gallery=synth.make_gallery(400))
    frames = synth.make_frames(2, H, W)
    opt = frt.QualityOptions(min_size=40, min_sharpness=50.0, max_clipped=3000)
    ropt = qr.options(min_size=40, min_sharpness=50.0, max_clipped=3000)
    for part, o, ro in ((frames, opt, ropt), (frames[:1], None, None), (frames, None, None)):   # the second call: fewer frames on the same staging
        n = len(part)
        wres, wemb = pipe.run(part)
        res, emb, ql, crops = pipe.runQuality(part, o, want_crops=True)
        assert res.tobytes() == wres.tobytes() and emb.tobytes() == wemb.tobytes()
        r2 = np.zeros(n * K, frt.RESULT_DTYPE)
        c2 = np.zeros((n * K, 112, 112, 3), np.uint8)
        pipe.wait(pipe.submit(np.ascontiguousarray(part), r2, None, c2))
        used = res["valid"] != 0
        print("%d frames: %d of %d slots hold a face" % (n, int(used.sum()), n * K))
        assert used.any() and r2.tobytes() == wres.tobytes()
        assert np.array_equal(crops[used], c2[used])
        same_bytes(ql, qr.quality(crops, res, ro), "runQuality, %d frames" % n)
        assert (ql[~used].view(np.uint8) == 0).all() and (ql["present"][used] == 1).all()
        assert np.array_equal(ql["size"][used], np.minimum(res["x2"] - res["x1"], res["y2"] - res["y1"])[used])
        assert ql["score"][used].tobytes() == res["score"][used].tobytes()
        res3, none, ql3 = pipe.runQuality(part, o, want_embeds=False)
        assert none is None and res3.tobytes() == wres.tobytes() and ql3.tobytes() == ql.tobytes()
    with pytest.raises(frt.FrtError) as err:
        pipe.runQuality(synth.make_frames(B + 1, H, W))
    assert err.value.code == frt.FRT_ERR_CAPACITY
    close(pipe, det, rec)


def test_gated_enrolment(frt, synth, blobs):
    imgs = [synth.make_frame(300 + i, r, c) for i, (r, c) in PHOTOS]
    names = ["p%d" % i for i in range(10)]
    N = 400
    gal = synth.make_gallery(N)
    probe = synth.make_queries(gal, [5, 250], noise=0.02, seed=9)
    det, rec, pipe = make_pipeline(frt, blobs, gallery=gal)
    det2, rec2, pipe2 = make_pipeline(frt, blobs, gallery=gal)
    mm = rec.matmul

    def answers(m, extra):
        return m.calculate(np.concatenate([extra, probe]) if len(extra) else probe)

    def fresh_answers(rows):
        fresh = frt.MatMul(0)
        fresh.init(np.concatenate([gal, rows]) if len(rows) else gal)
        out = fresh.calculate(np.concatenate([rows, probe]) if len(rows) else probe)
        fresh.close()
        return out

    def reset():
        if mm.m > N:
            mm.galleryRemove(list(range(N, mm.m)))
        rec.classNames, rec.classCount = rec.classNames[:N], N

    # ---- options NULL: frt_pipeline_enrol_images on an identical fresh gallery, byte for byte, plus the records
    status0, first0, e0, faces0, q0 = pipe.enrolImages(names, imgs, want_quality=True)
    wstatus, wfirst, we, wfaces = pipe2.enrolImages(names, imgs)
    assert status0.tobytes() == wstatus.tobytes() and first0 == wfirst == N and e0.tobytes() == we.tobytes() and faces0.tobytes() == wfaces.tobytes()
    assert np.array_equal(answers(mm, e0), answers(rec2.matmul, we)) and rec.classNames == rec2.classNames
    ok = np.flatnonzero(status0 == OK)
    assert len(ok) >= 2, status0
    res, _, crops = pipe.runImages(imgs, want_crops=True)
    slot0 = np.arange(10) * K
    same_bytes(q0, qr.quality(crops[slot0], res[slot0]), "quality_out, no gate")
    assert (q0["present"] == (res["valid"][slot0] != 0)).all() and (q0["flags"] == 0).all()

    # ---- the median sharpness of the accepted photos splits them
    thr = float(np.float32(np.median(q0["sharpness"][ok].astype(np.float64))))
    below = q0["sharpness"][ok] < np.float32(thr)
    print("sharpness of the accepted photos %s, threshold %r" % (q0["sharpness"][ok].tolist(), thr))
    assert below.any() and not below.all()
    gate = frt.QualityOptions(min_sharpness=thr)
    want_status = status0.copy()
    want_status[ok[below]] = LOW
    want_q = qr.quality(crops[slot0], res[slot0], qr.options(min_sharpness=thr))
    assert np.array_equal(want_q["flags"][ok], np.where(below, qr.BLURRED, 0))
    reset()
    gen = mm.generation()
    status, first, e, faces, q = pipe.enrolImages(names, imgs, quality=gate, want_quality=True)
    assert np.array_equal(status, want_status) and first == N
    assert faces.tobytes() == faces0.tobytes()                       # a LOW_QUALITY photo's face record is filled as for OK
    assert (faces["valid"][ok] == 1).all()
    same_bytes(q, want_q, "quality_out, gated")
    assert e.tobytes() == e0[~below].tobytes() and len(e) == int((~below).sum())
    assert mm.m == N + len(e) and frt.lib.frt_matcher_num_rows(mm._h) == N + len(e) and mm.generation() != gen
    assert rec.classNames[N:] == [names[i] for i in ok[~below]] and rec.classCount == N + len(e)
    assert np.array_equal(answers(mm, e), fresh_answers(e))
    idx, _ = mm.top1(e)
    assert idx.tolist() == list(range(N, N + len(e)))

    # ---- twenty photos through a pipeline of four frames: the selection appends across the chunks
    reset()
    status, first, e, faces, q = pipe.enrolImages(names + ["r%d" % i for i in range(10)], imgs + imgs, quality=gate, want_quality=True)
    assert np.array_equal(status, np.tile(want_status, 2)) and first == N and np.array_equal(faces["frame"], np.arange(20))
    same_bytes(q, np.tile(want_q, 2), "quality_out, five chunks")
    assert e.tobytes() == np.tile(e0[~below], (2, 1)).tobytes()
    assert np.array_equal(answers(mm, e), fresh_answers(e))
    # without the flag for the records, and without a gate that bites: the same rows as ungated
    reset()
    out = pipe.enrolImages(names, imgs, quality=frt.QualityOptions())
    assert len(out) == 4 and out[0].tobytes() == status0.tobytes() and out[2].tobytes() == e0.tobytes()

    # ---- a gate nobody passes: no edit
    reset()
    gen = mm.generation()
    status, first, e, faces, q = pipe.enrolImages(names, imgs, quality=frt.QualityOptions(min_sharpness=1e12), want_quality=True)
    assert np.array_equal(status, np.where(status0 == OK, LOW, status0)) and first == N and e.shape == (0, 512)
    assert mm.generation() == gen and frt.lib.frt_matcher_num_rows(mm._h) == N and rec.classCount == N
    assert (q["flags"][ok] == qr.BLURRED).all() and faces.tobytes() == faces0.tobytes()
    close(pipe, det, rec, pipe2, det2, rec2)
