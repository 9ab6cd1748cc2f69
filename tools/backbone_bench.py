#!/usr/bin/env python3
"""Throughput of the six recogniser backbones (IR-50 / 100 / 152, with and without SE) on one GPU.

  recogniser   faces/s of ArcFaceIR50.doInference at 128 faces per call; device time of each pass from the library's own HIP event
               bracket around the network (frt_profile_enable(2): "embed_network", upload / download excluded), median over --reps passes
  pipeline     the B = 32 frames x K = 4 faces, 640x640 step of bench.py through Pipeline.submit / wait with 3 tickets in flight and a
               100k-row gallery: wall time per step after warm-up (the stages run on the library's own streams)

Backbones alternate within one run (round r times every backbone once), so clock or thermal drift spreads over all of them.  GFLOP/face is
the algorithmic count from the layer shapes (convs, shortcut convs, the Linear); TF/s and the share of the fp16 MFMA dense peak (2.5 PF/s,
MI355X) follow from it.

    python tools/backbone_bench.py --out profiles/r07/r07_deep_backbones.json
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
BACKBONES = [("ir", 50), ("ir", 100), ("ir", 152), ("ir_se", 50), ("ir_se", 100), ("ir_se", 152)]
PEAK_FP16_TFS = 2500.0


def gflop_per_face(layers):
    """multiply-adds x 2 of the convolutions and the Linear (BN / PReLU / SE / pooling are not counted)"""
    from importlib import util
    spec = util.spec_from_file_location("synth_only", os.path.join(ROOT, "face-recognition-cpp-tensorrt_amd", "synth.py"))
    sy = util.module_from_spec(spec)
    spec.loader.exec_module(sy)
    f, h = 2.0 * 27 * 64 * 112 * 112, 112
    for cin, depth, stride in sy.ir_units(layers):
        ho = h // stride
        f += 2.0 * 9 * cin * depth * h * h + 2.0 * 9 * depth * depth * ho * ho
        if cin != depth:
            f += 2.0 * cin * depth * ho * ho
        h = ho
    return (f + 2.0 * 25088 * 512) / 1e9


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10, help="recogniser passes per backbone and round")
    ap.add_argument("--steps", type=int, default=10, help="pipeline steps per backbone and round")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    import __graft_entry__ as entry
    frt = entry.load_pkg()
    sy = frt.synth
    tmp = tempfile.mkdtemp(prefix="frt_backbones_")
    F, B, K, H, W = 128, 32, 4, 640, 640
    det_path = frt.write_weights(os.path.join(tmp, "det.frtw"), sy.retinaface_state(1), 1)
    det = frt.RetinaFace(det_path, W, H, (3, H, W), B, K, 0.4, 0.6)
    x = np.random.default_rng(0).standard_normal((F, 3, 112, 112)).astype(np.float32) * 0.5
    frames = sy.make_frames(B, H, W)
    gal = sy.make_gallery(100_000)
    objs = {}
    for mode, layers in BACKBONES:
        tag = "%s%d" % (mode, layers)
        path = frt.write_weights(os.path.join(tmp, tag + ".frtw"), sy.arcface_state(2, mode, num_layers=layers), 3 if mode == "ir_se" else 2)
        rec_one = frt.ArcFaceIR50(path, maxBatchSize=F)
        rec = frt.ArcFaceIR50(path, W, H, maxBatchSize=B * K, maxFacesPerScene=K)
        rec.setGallery(gal)
        rec.initMatMul()
        pipe = frt.Pipeline(det, rec, B)
        assert (rec_one.numLayers, rec_one.se) == (layers, mode == "ir_se")
        objs[tag] = (rec_one, rec, pipe)
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

    for tag, (rec_one, _, pipe) in objs.items():  # warm-up: first-use setup, graph capture
        for _ in range(3):
            rec_one.doInference(x)
        pipeline_steps(pipe, 6)
    ms = {t: [] for t in objs}
    step = {t: [] for t in objs}
    for _ in range(args.rounds):
        for tag, (rec_one, _, pipe) in objs.items():
            frt.profile_enable(2)
            for _ in range(args.reps):
                rec_one.doInference(x)
            labels, t_ms, _ = frt.profile_collect()
            frt.profile_enable(-1)
            ms[tag] += [m for lab, m in zip(labels, t_ms) if lab == "embed_network"]
            frt.profile_enable(0)
            t0 = time.perf_counter()
            pipeline_steps(pipe, args.steps)
            step[tag].append((time.perf_counter() - t0) / args.steps)
    rows = []
    for mode, layers in BACKBONES:
        tag = "%s%d" % (mode, layers)
        g = gflop_per_face(layers)
        m = float(np.median(ms[tag]))
        tfs = g * F / m  # GFLOP / ms = TF/s
        st = float(np.median(step[tag]))
        rows.append({"backbone": tag, "units": sum({50: (3, 4, 14, 3), 100: (3, 13, 30, 3), 152: (3, 8, 36, 3)}[layers]),
                     "gflop_per_face": round(g, 2), "recogniser_ms_per_128": round(m, 3), "recogniser_faces_per_s": round(F / m * 1e3, 1),
                     "recogniser_tf_s": round(tfs, 1), "share_of_fp16_mfma_peak": round(tfs / PEAK_FP16_TFS, 4), "passes": len(ms[tag]),
                     "pipeline_ms_per_step": round(st * 1e3, 3), "pipeline_faces_per_s": round(B * K / st, 1)})
        print(json.dumps(rows[-1]), flush=True)
    base = {r["backbone"][:-2]: r for r in rows if r["backbone"].endswith("50")}
    for r in rows:
        b = base.get(r["backbone"].rstrip("0123456789"))
        r["recogniser_time_vs_50"] = round(r["recogniser_ms_per_128"] / b["recogniser_ms_per_128"], 3)
    for tag, (rec_one, rec, pipe) in objs.items():
        pipe.close()
        rec.close()
        rec_one.close()
    det.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"what": __doc__.split("\n\n")[0], "command": "python tools/backbone_bench.py " + " ".join(sys.argv[1:]),
                       "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
