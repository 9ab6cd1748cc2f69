"""The recogniser's backbone is read from the blob: IR-50 / IR-100 / IR-152, with or without SE (model_irse.py:102-124, 193-240).
No device needed: frt_embedder_describe runs the loader's validation on the host, the exporter and the fp32 oracle are CPU code."""
import ctypes
import os

import numpy as np
import pytest

from conftest import GOLDEN, face_input

BACKBONES = [("ir", 50), ("ir", 100), ("ir", 152), ("ir_se", 50), ("ir_se", 100), ("ir_se", 152)]
DEEP = [b for b in BACKBONES if b[1] != 50]
TABLES = {50: (3, 4, 14, 3), 100: (3, 13, 30, 3), 152: (3, 8, 36, 3)}


def kind_of(frt, mode):
    return frt.weights_io.KIND_ARCFACE_IR_SE if mode == "ir_se" else frt.weights_io.KIND_ARCFACE_IR


def describe_raw(frt, path):
    n, se, units = ctypes.c_int(-1), ctypes.c_int(-1), (ctypes.c_int * 4)()
    rc = frt.lib.frt_embedder_describe(os.fsencode(path), ctypes.byref(n), ctypes.byref(se), units)
    return rc, frt.lib.frt_last_error().decode(), (n.value, se.value, tuple(units))


@pytest.fixture(scope="module")
def ir100(synth):
    return synth.arcface_state(2, "ir", num_layers=100)


@pytest.mark.parametrize("mode,layers", BACKBONES)
def test_describe_reads_every_backbone_from_its_tensors(frt, synth, tmp_path, mode, layers):
    path = frt.write_weights(str(tmp_path / "w.frtw"), synth.arcface_state(2, mode, num_layers=layers), kind_of(frt, mode))
    rc, err, got = describe_raw(frt, path)
    assert rc == frt.FRT_OK, err
    assert got == (layers, int(mode == "ir_se"), TABLES[layers])
    assert frt.describe_weights(path) == dict(numLayers=layers, se=mode == "ir_se", unitsPerStage=TABLES[layers])
    assert frt.lib.frt_embedder_describe(os.fsencode(path), None, None, None) == frt.FRT_OK  # every output is optional


def test_describe_reports_a_missing_file_like_create(frt):
    rc, err, _ = describe_raw(frt, "/nonexistent/arc.frtw")
    assert rc == frt.FRT_ERR_NOT_FOUND and err == "Cant find engine file"


def test_describe_refuses_a_detector_blob(frt, synth, tmp_path):
    path = frt.write_weights(str(tmp_path / "d.frtw"), synth.retinaface_state(1), frt.weights_io.KIND_RETINAFACE_MNET025)
    rc, err, _ = describe_raw(frt, path)
    assert rc == frt.FRT_ERR_FORMAT and "IR" in err


def malformed(ir100, synth):
    """name -> (state dict, text frt_last_error() must contain)"""
    out = {}
    sd = dict(ir100)
    del sd["body.20.res_layer.3.weight"]                          # one unit's tensor dropped
    out["dropped conv"] = (sd, "missing tensor body.20.res_layer.3.weight")
    sd = dict(ir100)
    for k in [k for k in sd if k.startswith("body.33.")]:         # a whole unit dropped from the middle: the units after it are left over
        del sd[k]
    out["dropped unit"] = (sd, "body.34.")
    sd = dict(ir100)
    del sd["body.16.shortcut_layer.1.running_var"]                # the stage-3 opener's shortcut BN incomplete
    out["dropped shortcut bn"] = (sd, "missing tensor body.16.shortcut_layer.1.running_var")
    sd = dict(ir100)
    for k in [k for k in ir100 if k.startswith("body.48.")]:      # an extra body.49: four 512-wide units
        sd[k.replace("body.48.", "body.49.")] = ir100[k]
    out["extra unit"] = (sd, "body.49")
    sd = dict(ir100)
    sd["body.60.res_layer.2.weight"] = ir100["body.48.res_layer.2.weight"]  # a stray body.* tensor past the last unit
    out["stray tensor"] = (sd, "unexpected tensor body.60.res_layer.2.weight")
    sd = dict(ir100)
    se = synth.arcface_state(2, "ir_se", num_layers=100)
    for k in ("body.7.res_layer.5.fc1.weight", "body.7.res_layer.5.fc2.weight"):  # SE mixed into a plain unit
        sd[k] = se[k]
    out["se mixed in"] = (sd, "body.7.res_layer.5.fc1.weight")
    sd = dict(ir100)
    sd["body.5.res_layer.4.weight"] = ir100["body.5.res_layer.4.weight"][:100]  # mis-sized
    out["wrong size"] = (sd, "wrong size for body.5.res_layer.4.weight")
    return out


@pytest.mark.parametrize("case", ["dropped conv", "dropped unit", "dropped shortcut bn", "extra unit", "stray tensor", "se mixed in", "wrong size"])
def test_malformed_blobs_are_refused_naming_the_tensor(frt, synth, ir100, tmp_path, case):
    sd, what = malformed(ir100, synth)[case]
    path = frt.write_weights(str(tmp_path / "w.frtw"), sd, frt.weights_io.KIND_ARCFACE_IR)
    rc, err, _ = describe_raw(frt, path)
    assert rc == frt.FRT_ERR_FORMAT, (case, rc, err)
    assert what in err, (case, err)
    # create runs the same validation before it touches a device: the same code and message with or without one
    h = ctypes.c_void_p()
    assert frt.lib.frt_embedder_create(os.fsencode(path), 3, 112, 112, 512, 1, 0, ctypes.byref(h)) == frt.FRT_ERR_FORMAT and not h
    assert what in frt.lib.frt_last_error().decode()


def test_an_se_blob_with_a_plain_unit_is_refused(frt, synth, tmp_path):
    sd = synth.arcface_state(2, "ir_se", num_layers=152)
    del sd["body.40.res_layer.5.fc1.weight"], sd["body.40.res_layer.5.fc2.weight"]
    path = frt.write_weights(str(tmp_path / "w.frtw"), sd, frt.weights_io.KIND_ARCFACE_IR_SE)
    rc, err, _ = describe_raw(frt, path)
    assert rc == frt.FRT_ERR_FORMAT and "body.40.res_layer.5.fc1.weight" in err, err


def test_exporter_kinds_and_refusal(frt, synth, tmp_path):
    torch = pytest.importorskip("torch")
    wio = frt.weights_io
    assert set(wio.ARCFACE_KINDS) == {"ir50", "ir100", "ir152", "ir_se50", "ir_se100", "ir_se152"}
    for mode, layers in BACKBONES:
        assert wio.arcface_layout(synth.arcface_state(2, mode, num_layers=layers)) == (layers, mode == "ir_se")
    sd = synth.arcface_state(2, "ir_se", num_layers=100)
    pth = tmp_path / "irse100.pth"
    torch.save({"state_dict": {"module." + k: torch.from_numpy(v) for k, v in sd.items()}}, str(pth))
    for wrong in ("ir100", "ir_se152", "ir_se50", "ir50"):
        with pytest.raises(ValueError, match="IR-SE-100"):
            wio.export_pth(str(pth), str(tmp_path / "x.frtw"), wrong)
    assert not os.path.exists(tmp_path / "x.frtw")
    out = wio.export_pth(str(pth), str(tmp_path / "ok.frtw"), "ir_se100")
    kind, back = wio.read_blob(out)
    assert kind == wio.KIND_ARCFACE_IR_SE and set(back) == set(sd)
    assert frt.describe_weights(out) == dict(numLayers=100, se=True, unitsPerStage=TABLES[100])
    bad = dict(sd)
    del bad["body.30.res_layer.5.fc1.weight"]
    with pytest.raises(ValueError, match="body.30"):
        wio.arcface_layout(bad)


@pytest.mark.parametrize("mode,layers", DEEP)
def test_oracle_matches_the_deep_goldens(synth, mode, layers):
    """The fp32 oracle (oracle/nets.py) against the reference module's output (make_golden_deep.py), both on CPU."""
    from oracle import nets
    g = np.load(os.path.join(GOLDEN, "arcface_%s%d.npz" % (mode, layers)))
    assert int(g["num_layers"]) == layers and str(g["mode"]) == mode
    sd = synth.arcface_state(int(g["seed"]), mode, num_layers=layers, calib=(g["calib_mean"], g["calib_var"]))
    x = face_input(synth.make_faces(int(g["n_faces"])))
    emb, blocks, _ = nets.arcface_forward(sd, x, return_blocks=True)
    cos = (emb.astype(np.float64) * g["embeddings"]).sum(1)
    assert cos.min() >= 1 - 1e-6, 1 - cos
    assert np.abs(emb @ emb.T - g["cos"]).max() < 1e-5
    stats = np.array([[b.mean(), b.std(), np.abs(b).max()] for b in blocks])
    assert stats.shape == g["block_stats"].shape == (1 + sum(TABLES[layers]), 3)
    assert np.allclose(stats, g["block_stats"], rtol=1e-4, atol=1e-4)
