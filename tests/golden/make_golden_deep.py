"""Generate the goldens of the deep recogniser backbones by running the REFERENCE's own PyTorch module (build container only).

    python tests/golden/make_golden_deep.py        # -> tests/golden/arcface_{ir100,ir152,ir_se100,ir_se152}.npz

The companion of make_golden.py (IR-50 / IR-SE-50, left as it is) for IR_101 / IR_152 / IR_SE_101 / IR_SE_152 of
conversion/arcface/model_irse.py, read from the reference checkout in place (make_golden.REF; never copied).  Each fixture holds its own BatchNorm1d
calibration (the running statistics of output_layer.4, measured over 96 synthetic faces like ``make_golden.py --calib``), so the
state dict is ``synth.arcface_state(2, mode, num_layers, calib=(calib_mean, calib_var))``: regenerated from the seed, never stored.
Per fixture: seed, n_faces, num_layers, mode, embeddings [8, 512], their cos matrix, per-block statistics (mean, std, max |x| after
the input layer and after every unit) and the calibration - about 25 KB.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF, face_input, load_sd, synth  # noqa: E402

VARIANTS = (("ir", 100), ("ir", 152), ("ir_se", 100), ("ir_se", 152))
N_FACES = 8


def arcface_module(mode, layers):
    sys.path.insert(0, os.path.join(REF, "arcface"))
    import model_irse
    name = ("IR_SE_%d" if mode == "ir_se" else "IR_%d") % (101 if layers == 100 else layers)  # model_irse.py:193-240 calls 100 layers IR_101
    return getattr(model_irse, name)([112, 112])


def calibration(mode, layers):
    m = load_sd(arcface_module(mode, layers), synth.arcface_state(2, mode, num_layers=layers))
    feats = []
    h = m.output_layer[3].register_forward_hook(lambda mod, i, o: feats.append(o.detach().numpy().copy()))
    with torch.no_grad():
        for s in range(0, 96, 16):
            m(torch.from_numpy(face_input(synth.make_faces(96)[s:s + 16])))
    h.remove()
    f = np.concatenate(feats).astype(np.float64)
    return f.mean(0).astype(np.float32), f.var(0).astype(np.float32)


def golden(mode, layers):
    calib = calibration(mode, layers)
    sd = synth.arcface_state(2, mode, num_layers=layers, calib=calib)
    m = load_sd(arcface_module(mode, layers), sd)
    x = face_input(synth.make_faces(N_FACES))
    blocks = []
    hooks = [m.input_layer.register_forward_hook(lambda mod, i, o: blocks.append(o.detach().numpy().copy()))]
    for u in m.body:
        hooks.append(u.register_forward_hook(lambda mod, i, o: blocks.append(o.detach().numpy().copy())))
    with torch.no_grad():
        emb = m(torch.from_numpy(x)).numpy()
    for h in hooks:
        h.remove()
    stats = np.array([[b.mean(), b.std(), np.abs(b).max()] for b in blocks], np.float32)
    tag = "%s%d" % (mode, layers)
    np.savez(os.path.join(HERE, "arcface_%s.npz" % tag), seed=2, n_faces=N_FACES, num_layers=layers, mode=mode, embeddings=emb,
             cos=(emb @ emb.T).astype(np.float32), block_stats=stats, calib_mean=calib[0], calib_var=calib[1])
    off = (emb @ emb.T)[~np.eye(N_FACES, dtype=bool)]
    print("arcface", tag, "emb", emb.shape, "units", len(blocks) - 1, "max |block| %.1f" % stats[:, 2].max(),
          "off-diagonal cos: mean %.3f max %.3f" % (off.mean(), off.max()))


if __name__ == "__main__":
    torch.manual_seed(0)
    for mode, layers in VARIANTS:
        golden(mode, layers)
