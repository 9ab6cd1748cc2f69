"""What the sighting book costs on the device.

  a  the two launches of a book update (brackets sightings_plan / sightings_copy of frt_profile_enable(2)) at --streams (32) x 4 faces x 16
     tracks, dim 512, crops kept, everything resident in HBM: every face is on a track and the quality records cycle, so that some best shots
     are replaced in every update; --repeat updates after a warm-up
  b  the worst case: 256 streams x 64 tracks, every slot filled, then one empty update with max_missed 0 that ends 16 384 tracks in one launch,
     without crops; and the same with crops at --crop-streams (64) streams x 64 tracks (4 096 closes: max_tracks ends at 64)
  c  Pipeline.runSighted against Pipeline.runTracked of the same --frames (32) frames of --frame (640) pixels on alternating legs in one
     process: --legs pairs of --repeat calls each, per leg the median call, then the spread of the leg medians; the stage brackets of one
     runSighted beside them, and Pipeline.runQuality with and without the crop download runSighted does not do
  d  a drain of 64 sightings with crops, wall clock
Needs the GPU.  Run it under a time limit, one process:

    timeout 600 python tools/sightings_timing.py [--repeat 30] [--legs 3] --out result.json
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
    ap.add_argument("--streams", type=int, default=32)
    ap.add_argument("--crop-streams", type=int, default=64)
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--frame", type=int, default=640)
    ap.add_argument("--repeat", type=int, default=30)
    ap.add_argument("--legs", type=int, default=3)
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    import torch
    frt = entry.load_pkg()
    out = {"args": vars(a), "cases": {}}
    stream = torch.cuda.current_stream().cuda_stream

    def stats(ts):
        return {"median": statistics.median(ts), "min": min(ts), "max": max(ts), "n": len(ts)}

    def report(name, r):
        out["cases"][name] = r
        print("%-40s %s" % (name, json.dumps(r)), flush=True)

    def dev(arr):
        return torch.from_numpy(np.ascontiguousarray(arr).view(np.uint8).reshape(-1).copy()).cuda()

    def brackets(fn, n):
        """n calls of fn under frt_profile_enable(2) -> {bracket name: [us]}"""
        frt.profile_enable(2)
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
        names, ms, _ = frt.profile_collect()
        frt.profile_enable(0)
        got = {}
        for nm, t in zip(names, ms):
            got.setdefault(nm, []).append(float(t) * 1e3)
        return got

    def grid_results(S, MF, side):
        """S frames of MF faces on a grid of boxes that do not overlap"""
        res = np.zeros((S, MF), frt.RESULT_DTYPE)
        k = np.arange(MF)
        res["x1"], res["y1"] = (k % side) * 30, (k // side) * 30
        res["x2"], res["y2"], res["score"], res["match_idx"], res["valid"] = res["x1"] + 20, res["y1"] + 20, 0.9, -1, 1
        return res.reshape(-1)

    def quality(rng, F):
        q = np.zeros(F, frt.QUALITY_DTYPE)
        q["present"], q["sharpness"], q["size"], q["score"] = 1, rng.random(F) * 100, 20, 0.9
        return q

    class Resident:
        """a tracker and its book driven from buffers in HBM"""

        def __init__(self, S, T, MF, D, capacity, keep_crops, max_missed, rng):
            self.S, self.MF, F = S, MF, S * MF
            self.trk = frt.Tracker(S, T, MF, D, 0.3, max_missed, 1)
            self.book = frt.Sightings(self.trk, capacity, keep_crops=keep_crops)
            self.res = dev(grid_results(S, MF, 8))
            self.none = torch.zeros_like(self.res)
            self.emb = torch.randn(F, D, device="cuda")
            self.tpl = torch.zeros(F, D, device="cuda")
            self.tracks = torch.zeros(F * 32, dtype=torch.uint8, device="cuda")
            self.qual = [dev(quality(rng, F)) for _ in range(4)]
            self.crops = torch.randint(0, 256, (F, 112, 112, 3), dtype=torch.uint8, device="cuda") if keep_crops else None
            self.i = 0

        def update(self, faces=True):
            r = self.res if faces else self.none
            self.i += 1
            self.trk.updateDev(r.data_ptr(), self.emb.data_ptr(), self.S, self.tracks.data_ptr(), self.tpl.data_ptr(), hip_stream=stream)
            self.book.updateDev(r.data_ptr(), self.tracks.data_ptr(), self.emb.data_ptr(), self.qual[self.i % 4].data_ptr(), self.S, self.tpl.data_ptr(),
                                self.crops.data_ptr() if self.crops is not None else None, hip_stream=stream)

        def close(self):
            self.trk.close()

    rng = np.random.default_rng(3)
    # ---- a: the steady state
    r = Resident(a.streams, 16, 4, 512, 1024, True, 5, rng)
    for _ in range(5):
        r.update()
    got = brackets(r.update, a.repeat)
    open0 = r.book.open(0)[0]
    assert (open0["close_tick"][:4] == -1).all() and (open0["n_shots"][:4] == 5 + a.repeat).all()      # what is timed is the update that works
    for k in ("sightings_plan", "sightings_copy"):
        report("a_%s_us" % k, stats(got[k]))
    r.close()

    # ---- b: every track of the call ends in one launch
    for name, S, keep in (("b_close_16384_no_crops", 256, False), ("b_close_%d_with_crops" % (a.crop_streams * 64), a.crop_streams, True)):
        plan, copy = [], []
        r = Resident(S, 64, 64, 4, S * 64, keep, 0, rng)
        for _ in range(5):
            r.update()
            got = brackets(lambda: r.update(faces=False), 1)
            plan += got["sightings_plan"]
            copy += got["sightings_copy"]
            n = 0
            while True:
                k = len(r.book.drain(8192, want_embeds=False, want_templates=False, want_crops=False)[0])
                n += k
                if k == 0:
                    break
            assert n == S * 64, (name, n)
        report(name + "_plan_us", stats(plan))
        report(name + "_copy_us", stats(copy))
        r.close()

    # ---- d: a drain of 64 sightings with crops
    r = Resident(16, 4, 4, 512, 64, True, 0, rng)
    ts = []
    for _ in range(a.repeat):
        r.update()
        r.update(faces=False)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = r.book.drain(64)
        ts.append((time.perf_counter() - t0) * 1e3)
        assert len(got[0]) == 64 and got[3].any()
    report("d_drain_64_with_crops_ms", stats(ts))
    r.close()

    # ---- c: the pipeline with the book against the pipeline with the tracker alone, alternating legs
    tmp = tempfile.mkdtemp(prefix="frt_sightings_timing_")
    s = frt.synth
    det_path = frt.write_weights(os.path.join(tmp, "det.frtw"), s.retinaface_state(1), 1)
    rec_path = frt.write_weights(os.path.join(tmp, "rec.frtw"), s.arcface_state(2, "ir", calib=s.load_calibration("ir")), 2)
    W = H = a.frame
    S, MF = a.frames, 4
    det = frt.RetinaFace(det_path, W, H, (3, H, W), S, MF, 0.4, 0.6)
    rcg = frt.ArcFaceIR50(rec_path, W, H, (3, 112, 112), 512, S * MF, MF, 0.65)
    rcg.setGallery(s.make_gallery(1000))
    rcg.initMatMul()
    pipe = frt.Pipeline(det, rcg, S)
    frames = np.ascontiguousarray(s.make_frames(S, H, W))
    t_plain, t_book = frt.Tracker(S, 16, MF), frt.Tracker(S, 16, MF)
    book = frt.Sightings(t_book, 1024)

    def leg(fn):
        for _ in range(3):
            fn()
        ts = []
        for _ in range(a.repeat):
            t0 = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(ts)

    calls = {"run_tracked_ms": lambda: pipe.runTracked(t_plain, frames), "run_sighted_ms": lambda: pipe.runSighted(t_book, book, frames),
             "run_quality_ms": lambda: pipe.runQuality(frames), "run_quality_with_crops_ms": lambda: pipe.runQuality(frames, want_crops=True)}
    legs = {k: [] for k in calls}
    for _ in range(a.legs):
        for k, fn in calls.items():
            legs[k].append(leg(fn))
    for k, v in legs.items():
        report("c_" + k, {"leg_medians": v, "median": statistics.median(v), "min": min(v), "max": max(v)})
    res = pipe.runSighted(t_book, book, frames)[0]
    out["c_faces_per_call"] = int((res["valid"] != 0).sum())
    out["c_ratio_of_medians"] = statistics.median(legs["run_sighted_ms"]) / statistics.median(legs["run_tracked_ms"])
    lo, hi = min(legs["run_tracked_ms"]), max(legs["run_tracked_ms"])
    out["c_difference_inside_the_spread"] = bool(lo <= statistics.median(legs["run_sighted_ms"]) <= hi)
    got = brackets(lambda: pipe.runSighted(t_book, book, frames), 5)
    for k in ("face_quality", "sightings_plan", "sightings_copy", "track_update"):
        report("c_stage_%s_us" % k, stats(got[k]))
    print("runSighted / runTracked %.4f, inside the runTracked legs' spread: %s" % (out["c_ratio_of_medians"], out["c_difference_inside_the_spread"]), flush=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    t_plain.close(), t_book.close(), pipe.close(), rcg.close(), det.close()


if __name__ == "__main__":
    main()
