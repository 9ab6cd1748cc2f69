#!/usr/bin/env python3
"""Detector families on one GPU: RetinaFace mobilenet0.25 (the reference's detector), Slim and RFB.

  network    device time of one 32-frame 640x640 detector pass from the library's own HIP event bracket around the network
             (frt_profile_enable(2): "det_network"; upload, preprocess and post-processing excluded), median over --reps passes
  pipeline   the bench.py-shaped step - B = 32 frames x K = 4 faces at 640x640, IR-50, a 100k-row gallery - through Pipeline.submit / wait
             with 3 tickets in flight: wall time per step after warm-up

Families alternate within one run (round r times every family once), so clock or thermal drift spreads over all of them.

    python tools/detector_bench.py --out profiles/r08/r08_detectors.json
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FAMILIES = ["mnet0.25", "slim", "rfb"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10, help="detector passes per family and round")
    ap.add_argument("--steps", type=int, default=10, help="pipeline steps per family and round")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    import __graft_entry__ as entry
    frt = entry.load_pkg()
    sy, wio = frt.synth, frt.weights_io
    tmp = tempfile.mkdtemp(prefix="frt_detectors_")
    B, K, H, W = 32, 4, 640, 640
    rec_path = frt.write_weights(os.path.join(tmp, "ir50.frtw"), sy.arcface_state(2, "ir", calib=sy.load_calibration("ir")), 2)
    states = {"mnet0.25": (sy.retinaface_state(1), wio.KIND_RETINAFACE_MNET025), "slim": (sy.slim_state(5), wio.KIND_RETINAFACE_SLIM),
              "rfb": (sy.slim_state(5, rfb=True), wio.KIND_RETINAFACE_RFB)}
    frames = sy.make_frames(B, H, W)
    x = np.ascontiguousarray((frames.astype(np.float32) - np.array([104, 117, 123], np.float32)).transpose(0, 3, 1, 2))
    gal = sy.make_gallery(100_000)
    objs = {}
    for fam in FAMILIES:
        sd, kind = states[fam]
        path = frt.write_weights(os.path.join(tmp, fam + ".frtw"), sd, kind)
        det = frt.RetinaFace(path, W, H, (3, H, W), B, K, 0.4, 0.6)
        assert det.family == fam
        rec = frt.ArcFaceIR50(rec_path, W, H, maxBatchSize=B * K, maxFacesPerScene=K)
        rec.setGallery(gal)
        rec.initMatMul()
        objs[fam] = (det, rec, frt.Pipeline(det, rec, B))
        os.remove(path)
    pinned = torch.from_numpy(frames).pin_memory()
    res = [np.zeros(B * K, frt.RESULT_DTYPE) for _ in range(3)]
    emb = [np.zeros((B * K, 512), np.float32) for _ in range(3)]

    def pipeline_steps(pipe, n):
        tickets = []
        for i in range(n):
            if len(tickets) == 3:
                pipe.wait(tickets.pop(0))
            tickets.append(pipe.submit(pinned.numpy(), res[i % 3], emb[i % 3]))
        for t in tickets:
            pipe.wait(t)

    for fam, (det, _, pipe) in objs.items():  # warm-up: first-use setup, graph capture
        for _ in range(3):
            det.doInference(x)
        pipeline_steps(pipe, 6)
    ms = {f: [] for f in objs}
    step = {f: [] for f in objs}
    faces = {}
    for _ in range(args.rounds):
        for fam, (det, _, pipe) in objs.items():
            frt.profile_enable(2)
            for _ in range(args.reps):
                det.doInference(x)
            labels, t_ms, _ = frt.profile_collect()
            frt.profile_enable(-1)
            ms[fam] += [m for lab, m in zip(labels, t_ms) if lab == "det_network"]
            frt.profile_enable(0)
            t0 = time.perf_counter()
            pipeline_steps(pipe, args.steps)
            step[fam].append((time.perf_counter() - t0) / args.steps)
            faces[fam] = int((res[0]["valid"] != 0).sum())
    rows = []
    for fam in FAMILIES:
        m = float(np.median(ms[fam]))
        st = float(np.median(step[fam]))
        rows.append({"family": fam, "anchors": objs[fam][0].numAnchors, "network_us_per_32": round(m * 1e3, 1), "passes": len(ms[fam]),
                     "network_us_per_32_min": round(float(np.min(ms[fam])) * 1e3, 1), "pipeline_ms_per_step": round(st * 1e3, 3),
                     "pipeline_frames_per_s": round(B / st, 1), "valid_faces_last_step": faces[fam]})
    for r in rows:
        r["network_time_vs_mnet"] = round(r["network_us_per_32"] / rows[0]["network_us_per_32"], 3)
        print(json.dumps(r), flush=True)
    for det, rec, pipe in objs.values():
        pipe.close()
        rec.close()
        det.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"what": __doc__.split("\n\n")[0], "command": "python tools/detector_bench.py " + " ".join(sys.argv[1:]),
                       "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
