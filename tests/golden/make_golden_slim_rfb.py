"""Goldens of the Slim / RFB detectors from the REFERENCE's own modules (build container only).

    python tests/golden/make_golden_slim_rfb.py     # -> tests/golden/retinaface_slim.npz, retinaface_rfb.npz

Imports conversion/retina/models/net_slim.py and net_rfb.py in place (never copied), with make_golden.torchvision_standin() for
their unused torchvision imports.  Weights come from synth.slim_state(seed) and frames from synth.make_frames(n, h, w, start=frame
seed): only the seeds and the expected outputs are stored - loc / conf / ldm in full at 96x160, strided samples at 288x320 and 640x640.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402

SEED, FRAME_SEED = 5, 0


def main():
    mg.torchvision_standin()
    sys.path.insert(0, os.path.join(mg.REF, "retina"))
    from config import cfg_rfb, cfg_slim
    from models.net_rfb import RFB
    from models.net_slim import Slim
    for name, cls, cfg, rfb in (("slim", Slim, cfg_slim, False), ("rfb", RFB, cfg_rfb, True)):
        m = mg.load_sd(cls(cfg, "test"), mg.synth.slim_state(SEED, rfb=rfb))
        out = {}
        for tag, (h, w), step in (("96x160", (96, 160), 1), ("288x320", (288, 320), 5), ("640", (640, 640), 23)):
            fr = mg.synth.make_frames(2, h, w, start=FRAME_SEED)
            x = np.ascontiguousarray((fr.astype(np.float32) - np.array([104, 117, 123], np.float32)).transpose(0, 3, 1, 2))
            with torch.no_grad():
                loc, conf, ldm = (t.numpy() for t in m(torch.from_numpy(x)))
            out["loc_" + tag], out["conf_" + tag], out["ldm_" + tag] = loc[:, ::step], conf[:, ::step], ldm[:, ::step]
            out["step_" + tag] = step
            out["npass_" + tag] = (conf[..., 1] > 0.6).sum(1)
            print(name, tag, loc.shape, "anchors > 0.6:", out["npass_" + tag])
        np.savez_compressed(os.path.join(HERE, "retinaface_%s.npz" % name), seed=SEED, frame_seed=FRAME_SEED, **out)


if __name__ == "__main__":
    main()
