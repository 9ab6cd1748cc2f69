"""Faces per second of the three ways to embed a batch of face images (DESIGN section "Face images instead of frames").

One process, one recogniser (IR-50, synthetic weights, maxBatchSize 128), --faces images (default 4096) in two mixes - all 112x112, and
112x112 / 160x160 / 250x250 in turn - and three legs, alternated --repeat times so that each leg's own spread is seen beside the difference
between legs:

  a  the reference's loop (src/app.cpp:79-97): per image, resize on the host (the oracle's cv::resize restatement) + preprocessFace +
     doInference of one face.  Run on the first --a-faces images (default 512): its rate does not depend on the count.
  b  the best the library offered before forwardFaces: resize and normalise on the host OUTSIDE the timed region, then doInference of the
     whole fp32 batch (chunks of 128, 150 KB per face over PCIe, synchronous per chunk).
  c  forwardFaces: u8 images up (37 KB per 112x112 face), resize + preprocessFace in one kernel, passes of 128 while the next chunk uploads.

Host clock around calls that return when their device work is complete.  Afterwards one forwardFaces call with the stage profile on gives
the prepare kernel's time per pass beside the network's.  Needs the GPU: without one the recogniser cannot be created and the script fails.

    python tools/face_batch_timing.py [--faces 4096] [--repeat 5] [--out profiles/...json]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import __graft_entry__ as entry


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--faces", type=int, default=4096)
    ap.add_argument("--a-faces", type=int, default=512)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    frt = entry.load_pkg()
    import oracle
    s = frt.synth
    tmp = tempfile.mkdtemp(prefix="frt_faces_")
    path = frt.write_weights(os.path.join(tmp, "rec.frtw"), s.arcface_state(2, "ir", calib=s.load_calibration("ir")), 2)
    rec = frt.ArcFaceIR50(path, maxBatchSize=a.batch)
    n, na = a.faces, min(a.a_faces, a.faces)
    base = [s.make_frame(i, 250, 250) for i in range(16)]  # a few distinct images, cut and reused: the timing does not depend on the pixels

    def image(i, size):
        return np.ascontiguousarray(base[i % len(base)][:size, :size])

    mixes = {"all_112": [image(i, 112) for i in range(n)], "mix_112_160_250": [image(i, (112, 160, 250)[i % 3]) for i in range(n)]}
    out = {"faces": n, "faces_leg_a": na, "batch": a.batch, "repeat": a.repeat, "unit": "faces/s", "mixes": {}}

    def timed(fn):
        t0 = time.perf_counter()
        r = fn()
        return time.perf_counter() - t0, r

    for name, imgs in mixes.items():
        crops = np.stack([im if im.shape[:2] == (112, 112) else oracle.resize_linear(im, 112, 112) for im in imgs])
        chw = np.ascontiguousarray((crops[..., ::-1].astype(np.float32) - 127.5).transpose(0, 3, 1, 2) * np.float32(0.0078125))

        def leg_a():
            e = np.empty((na, 512), np.float32)
            for i in range(na):
                im = imgs[i]
                if im.shape[:2] != (112, 112):
                    im = oracle.resize_linear(im, 112, 112)
                e[i] = rec.doInference(rec.preprocessFace(im), 1)[0]
            return e

        legs = {"a": (leg_a, na), "b": (lambda: rec.doInference(chw), n), "c": (lambda: rec.forwardFaces(imgs), n)}
        results = {k: fn() for k, (fn, _) in legs.items()}  # warm-up of every shape, and the answers: all three embed the same crops
        same = {"c_vs_b_max_abs": float(np.abs(results["c"] - results["b"]).max()),
                "a_vs_b_min_cos": float((results["a"] * results["b"][:na]).sum(1).min())}
        rates = {k: [] for k in legs}
        for _ in range(a.repeat):
            for k in ("b", "c", "a"):
                fn, cnt = legs[k]
                t, _r = timed(fn)
                rates[k].append(cnt / t)
        rec_mix = {"agreement": same, "bytes_up_per_face": {"b": 3 * 112 * 112 * 4, "c": sum(im.nbytes for im in imgs) / n}}
        for k in ("a", "b", "c"):
            r = rates[k]
            rec_mix[k] = {"median": statistics.median(r), "min": min(r), "max": max(r), "all": r}
            print("%-16s leg %s  median %9.0f faces/s  (min %9.0f  max %9.0f)" % (name, k, statistics.median(r), min(r), max(r)), flush=True)
        # one profiled call: the prepare kernel and the network, per pass
        frt.profile_enable(2)
        rec.forwardFaces(imgs)
        labels, ms, _work = frt.profile_collect()
        frt.profile_enable(0)
        prof = {}
        for lab in sorted(set(labels)):
            v = [m for l, m in zip(labels, ms) if l == lab]
            prof[lab] = {"passes": len(v), "median_ms": statistics.median(v), "total_ms": float(sum(v))}
            print("%-16s profile %-16s %4d passes  median %.3f ms  total %.1f ms" % (name, lab, len(v), statistics.median(v), sum(v)), flush=True)
        rec_mix["profile"] = prof
        out["mixes"][name] = rec_mix
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    rec.close()


if __name__ == "__main__":
    main()
