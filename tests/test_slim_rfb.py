"""Slim / RFB detectors on the CPU: the restatement against the reference-module goldens and the oracle, anchor tables, the exporter's
detector kinds and frt_detector_describe (no device needed)."""
import os

import numpy as np
import pytest

import slim_ref
from conftest import GOLDEN


def _input(synth, n, h, w, start=0):
    fr = synth.make_frames(n, h, w, start=start)
    return np.ascontiguousarray((fr.astype(np.float32) - np.array([104, 117, 123], np.float32)).transpose(0, 3, 1, 2))


@pytest.mark.parametrize("name", ["slim", "rfb"])
@pytest.mark.parametrize("tag,hw", [("96x160", (96, 160)), ("288x320", (288, 320)), ("640", (640, 640))])
def test_restatement_matches_reference_goldens(synth, name, tag, hw):
    g = np.load(os.path.join(GOLDEN, "retinaface_%s.npz" % name))
    sd = synth.slim_state(int(g["seed"]), rfb=name == "rfb")
    loc, conf, ldm = slim_ref.forward(sd, _input(synth, 2, *hw, start=int(g["frame_seed"])), rfb=name == "rfb")
    assert loc.shape[1] == slim_ref.anchor_count(hw[1], hw[0])
    step = int(g["step_" + tag])
    assert np.abs(loc[:, ::step] - g["loc_" + tag]).max() <= 1e-5
    assert np.abs(ldm[:, ::step] - g["ldm_" + tag]).max() <= 1e-5
    assert np.abs(conf[:, ::step] - g["conf_" + tag]).max() <= 1e-6
    assert np.array_equal((conf[..., 1] > 0.6).sum(1), g["npass_" + tag])


@pytest.mark.parametrize("geom", [(640, 640, 640, 640), (320, 288, 640, 480), (320, 288, 480, 640), (160, 96, 161, 97)])
def test_restated_postprocess_with_the_mnet_table_equals_the_oracle(orc, geom):
    in_w, in_h, fw, fh = geom
    A = len(orc.anchors(in_w, in_h))
    assert A == slim_ref.anchor_count(in_w, in_h, slim_ref.MNET)
    assert np.array_equal(orc.anchors(in_w, in_h), slim_ref.anchors(in_w, in_h, slim_ref.MNET))
    for seed in range(3):
        r = np.random.default_rng(seed)
        loc = (r.standard_normal((A, 4)) * 1.5).astype(np.float32)
        conf = np.zeros((A, 2), np.float32)
        conf[:, 1] = r.random(A).astype(np.float32) ** 8
        conf[r.integers(0, A, 40), 1] = np.float32(0.75)  # ties: lower anchor index first
        conf[:, 0] = 1 - conf[:, 1]
        for k in (4, 64):
            want = orc.postprocess(loc, conf, in_w, in_h, fw, fh, 0.4, 0.6, k)
            got = slim_ref.postprocess(loc, conf, in_w, in_h, fw, fh, 0.4, 0.6, k, table=slim_ref.MNET)
            assert len(got) == len(want) > 0
            for f in ("x1", "y1", "x2", "y2", "score"):
                assert np.array_equal(got[f], want[f]), (geom, seed, k, f)


def test_anchor_counts_of_the_four_level_table():
    assert slim_ref.anchor_count(640, 640) == 23500
    assert slim_ref.anchor_count(320, 288) == 5295
    assert slim_ref.feature_maps(172, 100, slim_ref.SLIM) == [(13, 22), (7, 11), (4, 6), (2, 3)]
    assert slim_ref.anchor_count(172, 100) == 13 * 22 * 3 + 7 * 11 * 2 + 4 * 6 * 2 + 2 * 3 * 3
    a = slim_ref.anchors(640, 640)
    assert np.allclose(a[0], [4 / 640, 4 / 640, 10 / 640, 10 / 640]) and np.allclose(a[2, 2:], [24 / 640, 24 / 640])
    assert np.allclose(a[-1], [608 / 640, 608 / 640, 256 / 640, 256 / 640])


def _save_pth(tmp_path, sd, prefix="", wrap=False):
    import torch
    t = {prefix + k: torch.from_numpy(v) for k, v in sd.items()}
    p = str(tmp_path / "ckpt.pth")
    torch.save({"state_dict": t} if wrap else t, p)
    return p


@pytest.mark.parametrize("kind,rfb", [("slim", False), ("rfb", True), ("RFB", True)])
def test_exporter_detector_kinds(frt, synth, tmp_path, kind, rfb):
    sd = synth.slim_state(5, rfb=rfb)
    pth = _save_pth(tmp_path, sd, prefix="module.", wrap=True)
    out = frt.weights_io.export_pth(pth, str(tmp_path / "det.frtw"), kind)
    k, got = frt.weights_io.read_blob(out)
    assert k == (frt.weights_io.KIND_RETINAFACE_RFB if rfb else frt.weights_io.KIND_RETINAFACE_SLIM) == (5 if rfb else 4)
    assert list(got) == [n for n in sd if not n.endswith("num_batches_tracked")]
    assert all(np.array_equal(got[n], sd[n]) for n in got)


def test_exporter_refuses_the_wrong_family(frt, synth, tmp_path):
    rfb = _save_pth(tmp_path, synth.slim_state(5, rfb=True))
    with pytest.raises(ValueError, match="RFB"):
        frt.weights_io.export_pth(rfb, str(tmp_path / "a.frtw"), "slim")
    with pytest.raises(ValueError, match="RFB"):
        frt.weights_io.export_pth(rfb, str(tmp_path / "a.frtw"), "retinaface")
    slim = _save_pth(tmp_path, synth.slim_state(5))
    for kind in ("retinaface", "rfb"):
        with pytest.raises(ValueError, match="Slim"):
            frt.weights_io.export_pth(slim, str(tmp_path / "a.frtw"), kind)
    mnet = _save_pth(tmp_path, synth.retinaface_state(1))
    with pytest.raises(ValueError, match="mobilenet0.25"):
        frt.weights_io.export_pth(mnet, str(tmp_path / "a.frtw"), "slim")


def test_describe_detector_blobs(frt, synth, tmp_path):
    w = frt.weights_io
    cases = [(synth.retinaface_state(1), w.KIND_RETINAFACE_MNET025, "mnet0.25", 3, False),
             (synth.retinaface_state(1, landmarks=True), w.KIND_RETINAFACE_MNET025, "mnet0.25", 3, True),
             (synth.slim_state(5), w.KIND_RETINAFACE_SLIM, "slim", 4, True),
             (synth.slim_state(5, landmarks=False), w.KIND_RETINAFACE_SLIM, "slim", 4, False),
             (synth.slim_state(5, rfb=True), w.KIND_RETINAFACE_RFB, "rfb", 4, True)]
    for i, (sd, kind, fam, levels, ldm) in enumerate(cases):
        p = frt.write_weights(str(tmp_path / ("d%d.frtw" % i)), sd, kind)
        assert frt.describe_detector_weights(p) == dict(family=fam, kind=kind, levels=levels, hasLandmarks=ldm)


def test_describe_refuses_recogniser_and_broken_detector_blobs(frt, synth, tmp_path):
    w = frt.weights_io
    rec = frt.write_weights(str(tmp_path / "rec.frtw"), synth.arcface_state(2, "ir"), w.KIND_ARCFACE_IR50)
    with pytest.raises(frt.FrtError) as e:
        frt.describe_detector_weights(rec)
    assert e.value.code == frt.FRT_ERR_FORMAT
    for rfb, kind, drop in ((False, w.KIND_RETINAFACE_SLIM, "conv11.3.weight"), (True, w.KIND_RETINAFACE_RFB, "conv8.branch2.3.bn.running_var"),
                            (False, w.KIND_RETINAFACE_SLIM, "conf.3.bias")):
        sd = synth.slim_state(5, rfb=rfb)
        del sd[drop]
        p = frt.write_weights(str(tmp_path / "t.frtw"), sd, kind)
        with pytest.raises(frt.FrtError, match="missing tensor " + drop.replace(".", r"\.")) as e:
            frt.describe_detector_weights(p)
        assert e.value.code == frt.FRT_ERR_FORMAT
    sd = synth.slim_state(5)
    sd["loc.1.2.weight"] = sd["loc.1.2.weight"][:4]
    p = frt.write_weights(str(tmp_path / "s.frtw"), sd, w.KIND_RETINAFACE_SLIM)
    with pytest.raises(frt.FrtError, match=r"wrong shape for loc\.1\.2\.weight"):
        frt.describe_detector_weights(p)
    # an RFB checkpoint written as a Slim blob (and the other way round)
    p = frt.write_weights(str(tmp_path / "x.frtw"), synth.slim_state(5, rfb=True), w.KIND_RETINAFACE_SLIM)
    with pytest.raises(frt.FrtError, match=r"missing tensor conv8\.0\.weight"):
        frt.describe_detector_weights(p)
    p = frt.write_weights(str(tmp_path / "y.frtw"), synth.slim_state(5), w.KIND_RETINAFACE_RFB)
    with pytest.raises(frt.FrtError, match=r"missing tensor conv8\.branch0\.0\.conv\.weight"):
        frt.describe_detector_weights(p)
