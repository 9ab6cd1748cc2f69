"""Recogniser-only cost of the flip-augmented embeddings (frt_embedder_set_flip): device time of one forward() over F faces (the "embed_network"
profiling scope: from the first launch of the pass to the last, no upload or download in it), flip against plain on the same object in the same
run, on alternating legs.  Also: the two launches the mode adds, per sub-pass (kernel-level profiling scopes), and what the simpler design - the
faces and their mirror images as two separate passes of F / 2 faces each - would pay per pass, from a plain embedder of half the batch.

    python tools/flip_timing.py [--faces 128] [--legs 5] [--reps 10] [--mode ir|ir_se]      prints one JSON line"""
import argparse
import json
import os
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as entry  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--faces", type=int, default=128)
    ap.add_argument("--legs", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--mode", default="ir", choices=["ir", "ir_se"])
    a = ap.parse_args()
    frt = entry.load_pkg()
    s = frt.synth
    tmp = tempfile.mkdtemp()
    path = frt.write_weights(os.path.join(tmp, "rec.frtw"), s.arcface_state(2, a.mode, calib=s.load_calibration(a.mode)), 2 if a.mode == "ir" else 3)
    F = a.faces
    x = np.random.default_rng(0).standard_normal((F, 3, 112, 112)).astype(np.float32) * 0.5

    def passes(rec, n, reps, kind, want):
        """ms of every scope named in `want` over `reps` doInference calls of n faces at profiling level `kind`: label -> list"""
        frt.profile_enable(kind)
        try:
            for _ in range(reps):
                rec.doInference(x[:n])
            labels, ms, _ = frt.profile_collect()
        finally:
            frt.profile_enable(0)
        return {w: [float(m) for l, m in zip(labels, ms) if l == w] for w in want}

    rec = frt.ArcFaceIR50(path, maxBatchSize=F)
    half = frt.ArcFaceIR50(path, maxBatchSize=max(F // 2, 1))
    for flip in (False, True):  # warm-up of both modes: tables, code objects, clocks
        rec.setFlip(flip)
        for _ in range(3):
            rec.doInference(x)
    for _ in range(3):
        half.doInference(x[:max(F // 2, 1)])
    t = {"plain": [], "flip": [], "half": []}
    for _ in range(a.legs):
        rec.setFlip(False)
        t["plain"] += passes(rec, F, a.reps, 2, ["embed_network"])["embed_network"]
        rec.setFlip(True)
        t["flip"] += passes(rec, F, a.reps, 2, ["embed_network"])["embed_network"]
        t["half"] += passes(half, max(F // 2, 1), a.reps, 2, ["embed_network"])["embed_network"]
    k = passes(rec, F, a.reps, 1, ["flip_pair_up", "fc_finalize_pair"])  # (flip is on: the last leg left it so)
    med = {n: float(np.median(v)) for n, v in t.items()}
    out = {
        "mode": a.mode, "faces": F, "legs": a.legs, "reps": a.reps,
        "plain_ms": round(med["plain"], 4), "flip_ms": round(med["flip"], 4), "ratio": round(med["flip"] / med["plain"], 4),
        "plain_faces_per_s": round(F / med["plain"] * 1e3, 1), "flip_faces_per_s": round(F / med["flip"] * 1e3, 1),
        "plain_ms_min_max": [round(min(t["plain"]), 4), round(max(t["plain"]), 4)], "flip_ms_min_max": [round(min(t["flip"]), 4), round(max(t["flip"]), 4)],
        # flip runs F faces as two sub-passes of F / 2 faces + their mirror images = two network passes of F faces
        "sub_passes": 2 if F >= 2 else 1,
        "pair_up_us_per_sub_pass": round(float(np.median(k["flip_pair_up"])) * 1e3, 2) if k["flip_pair_up"] else None,
        "finalize_pair_us_per_sub_pass": round(float(np.median(k["fc_finalize_pair"])) * 1e3, 2) if k["fc_finalize_pair"] else None,
        # the simpler design: per F / 2 faces, two plain passes of F / 2 faces instead of one of F
        "half_batch_plain_ms": round(med["half"], 4), "two_half_passes_over_one_full": round(2 * med["half"] / med["plain"], 4),
    }
    rec.close()
    half.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
