"""What scoring the face crops costs on the device.

  a  the quality kernel alone over --faces (128) crops resident in HBM, every slot present: per launch by the library's profiling hooks
     (frt_profile_enable(2), the bracket named face_quality around the launch of frt_face_quality_dev), --repeat launches after a warm-up;
     the same with every third slot absent
  b  Pipeline.runQuality against frt_pipeline_submit_crops + wait of the same frames - the call a caller who wants the crops makes today -
     on alternating legs in one process: --legs pairs of --repeat calls each; per leg the median call, then the spread of the leg medians.
     The two differ by the quality launch, the 56-byte records' download and the route (serial under the run mutex against the staged
     submit), so only a difference outside the legs' spread means anything
Needs the GPU.  Run it under a time limit, one process:

    timeout 600 python tools/quality_timing.py [--faces 128] [--frames 32] [--frame 640] [--repeat 30] [--legs 3] --out result.json
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

import __graft_entry__ as entry


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--faces", type=int, default=128)
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--frame", type=int, default=640)
    ap.add_argument("--repeat", type=int, default=30)
    ap.add_argument("--legs", type=int, default=3)
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    import torch
    import quality_ref as qr
    frt = entry.load_pkg()
    F, MF = a.faces, 4
    out = {"faces": F, "frames": a.frames, "frame": a.frame, "max_faces": MF, "repeat": a.repeat, "legs": a.legs, "cases": {}}

    def stats(ts):
        return {"median": statistics.median(ts), "min": min(ts), "max": max(ts)}

    def report(name, r):
        out["cases"][name] = r
        print("%-34s %s" % (name, json.dumps(r)), flush=True)

    # ---- a: the kernel alone
    rng = np.random.default_rng(3)
    crops = rng.integers(0, 256, (F, 112, 112, 3), dtype=np.uint8)
    rec = np.zeros(F, qr.RESULT_DTYPE)
    rec["x2"], rec["y2"], rec["score"] = 80, 90, 0.9
    rec["valid"] = np.where(np.arange(F) % 3 == 2, 0, 1)
    d_crops = torch.from_numpy(crops).cuda()
    d_rec = torch.from_numpy(rec.view(np.uint8).copy()).cuda()
    d_out = torch.zeros(F * 56, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    for name, recs in (("a_kernel_us_all_present", None), ("a_kernel_us_every_third_absent", d_rec.data_ptr())):
        launch = lambda: frt.face_quality_dev(d_crops.data_ptr(), recs, F, d_out.data_ptr(), None, stream)  # noqa: E731
        for _ in range(5):
            launch()
        torch.cuda.synchronize()
        got = d_out.cpu().numpy().view(qr.QUALITY_DTYPE)
        want = qr.quality(crops[:8], rec[:8] if recs else None)
        assert got[:8].tobytes() == want.tobytes(), name        # the launch that is timed is the one that is right
        frt.profile_enable(2)
        for _ in range(a.repeat):
            launch()
        torch.cuda.synchronize()
        names, ms, _ = frt.profile_collect()
        frt.profile_enable(0)
        ks = [float(t) * 1e3 for n, t in zip(names, ms) if n == "face_quality"]
        assert len(ks) == a.repeat, (len(ks), set(names))
        r = stats(ks)
        r["bytes_read"] = int(F * 37632 if recs is None else int(rec["valid"].sum()) * 37632)
        report(name, r)

    # ---- b: the pipeline with the records against the pipeline with the crops, alternating legs
    tmp = tempfile.mkdtemp(prefix="frt_quality_timing_")
    s = frt.synth
    det_path = frt.write_weights(os.path.join(tmp, "det.frtw"), s.retinaface_state(1), 1)
    rec_path = frt.write_weights(os.path.join(tmp, "rec.frtw"), s.arcface_state(2, "ir", calib=s.load_calibration("ir")), 2)
    W = H = a.frame
    S = a.frames
    det = frt.RetinaFace(det_path, W, H, (3, H, W), S, MF, 0.4, 0.6)
    rcg = frt.ArcFaceIR50(rec_path, W, H, (3, 112, 112), 512, S * MF, MF, 0.65)
    rcg.setGallery(s.make_gallery(1000))
    rcg.initMatMul()
    pipe = frt.Pipeline(det, rcg, S)
    frames = np.ascontiguousarray(s.make_frames(S, H, W))
    res = np.zeros(S * MF, frt.RESULT_DTYPE)
    emb = np.zeros((S * MF, 512), np.float32)
    crp = np.zeros((S * MF, 112, 112, 3), np.uint8)

    def submit_crops():
        pipe.wait(pipe.submit(frames, res, emb, crp))

    def run_quality():
        pipe.runQuality(frames, None, want_crops=True)

    def leg(fn):
        for _ in range(3):
            fn()
        ts = []
        for _ in range(a.repeat):
            t0 = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(ts)

    legs = {"submit_crops_ms": [], "run_quality_ms": []}
    for _ in range(a.legs):
        legs["submit_crops_ms"].append(leg(submit_crops))
        legs["run_quality_ms"].append(leg(run_quality))
    for name, v in legs.items():
        report("b_" + name, {"leg_medians": v, "median": statistics.median(v), "min": min(v), "max": max(v)})
    out["b_faces_per_call"] = int((res["valid"] != 0).sum())
    out["b_ratio_of_medians"] = statistics.median(legs["run_quality_ms"]) / statistics.median(legs["submit_crops_ms"])
    lo, hi = min(legs["submit_crops_ms"]), max(legs["submit_crops_ms"])
    out["b_difference_inside_the_spread"] = bool(lo <= statistics.median(legs["run_quality_ms"]) <= hi)
    print("ratio of medians %.4f, inside the submit_crops legs' spread: %s" % (out["b_ratio_of_medians"], out["b_difference_inside_the_spread"]), flush=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    pipe.close(), rcg.close(), det.close()


if __name__ == "__main__":
    main()
