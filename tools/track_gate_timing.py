"""What the gate in front of the recogniser saves, or costs (include/frt.h "Gate").

The shape of tools/track_timing.py's pipeline legs: 32 streams, synthetic 640 x 640 frames, max_faces 4, max_tracks 16, one 1M x 512
gallery, one process.  The same frames are repeated, so after the warm-up calls every face sits on a confirmed track with embeddings: the
steady state of a still camera, the best case of the gate.
  legs     Pipeline.runTracked (the route without the gate) and Pipeline.runTrackedGated at refresh 1 (skips nothing: the host read, the
           compaction and the smaller passes are all it adds), 4 and 16, on alternating legs in one process: --legs rounds of --repeat calls
           each, every leg with a tracker of its own.  Per leg the calls' median, mean, min and max - with refresh r one call in r embeds
           every face and the others none, so the mean is the cost per call of the stream and the median that of the common call - and
           n_embed of every call.
  --profile  instead of the legs: the gate, the gather crop and the scatter by the library's profiling hooks (frt_profile_enable(2)), which
           run every call serially; a run of its own, so that the legs above are not taken with the hooks on.
  --motion GAIN  instead of the legs: a MOVING scene - the frames rolled --roll pixels further on every call, a
           demonstration of the mechanism and not a rate anyone will see on video -, runTrackedGated at --refresh[0] with motion off and on,
           alternating legs, the roll itself outside the timed region: the mean time per call and n_embed per call; then, hooks on, the gate
           kernel alone (track_gate) off and on, alternating legs.
The measurement's own settings, not recommendations: --min-embeds 1, --skip-iou 0.5.
Needs the GPU.  Run it under a time limit, one process per mode:

    timeout 900 python tools/track_gate_timing.py [--rows 1000000] [--streams 32] [--repeat 32] [--legs 3] [--profile] --out result.json
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
import numpy as np

import __graft_entry__ as entry


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--streams", type=int, default=32)
    ap.add_argument("--repeat", type=int, default=32)
    ap.add_argument("--legs", type=int, default=3)
    ap.add_argument("--frame", type=int, default=640)
    ap.add_argument("--refresh", type=int, nargs="+", default=[1, 4, 16])
    ap.add_argument("--min-embeds", dest="min_embeds", type=int, default=1)
    ap.add_argument("--skip-iou", dest="skip_iou", type=float, default=0.5)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--motion", type=int, default=0, help="the moving-scene legs, motion off against this gain (1 .. 256)")
    ap.add_argument("--roll", type=int, default=8, help="--motion: pixels per call")
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    frt = entry.load_pkg()
    S, MF, T, N = a.streams, 4, 16, a.rows
    F = S * MF
    out = {"streams": S, "max_faces": MF, "max_tracks": T, "gallery_rows": N, "repeat": a.repeat, "legs": a.legs, "unit": "ms",
           "min_embeds": a.min_embeds, "skip_iou": a.skip_iou, "cases": {}}

    def report(name, r):
        out["cases"][name] = r
        print("%-28s %s" % (name, json.dumps(r)), flush=True)

    s = frt.synth
    g = s.make_gallery(N)
    tmp = tempfile.mkdtemp(prefix="frt_track_gate_timing_")
    det_path = frt.write_weights(os.path.join(tmp, "det.frtw"), s.retinaface_state(1), 1)
    rec_path = frt.write_weights(os.path.join(tmp, "rec.frtw"), s.arcface_state(2, "ir", calib=s.load_calibration("ir")), 2)
    W = H = a.frame
    det = frt.RetinaFace(det_path, W, H, (3, H, W), S, MF, 0.4, 0.6)
    rec = frt.ArcFaceIR50(rec_path, W, H, (3, 112, 112), 512, F, MF, 0.65)
    rec.setGallery(g)
    rec.initMatMul()
    pipe = frt.Pipeline(det, rec, S)
    frames = s.make_frames(S, H, W)
    out["faces_per_call"] = int((pipe.run(frames)[0]["score"] > 0).sum())
    if a.motion:
        out["motion_gain"], out["roll"], out["refresh"] = a.motion, a.roll, a.refresh[0]
        trk = {"gated_off": frt.Tracker(S, T, MF, 512), "gated_on": frt.Tracker(S, T, MF, 512, motion_gain=a.motion)}
        at = {n: 0 for n in trk}

        def moving(n):
            at[n] += 1
            return np.roll(frames, a.roll * at[n], axis=2)

        def gated(n, f):
            return pipe.runTrackedGated(trk[n], f, a.refresh[0], a.min_embeds, a.skip_iou, want_embeds=False, want_templates=False)[4]

        times, embedded, leg_means = {n: [] for n in trk}, {n: [] for n in trk}, {n: [] for n in trk}
        for _ in range(a.legs):
            for n in trk:
                for _ in range(5):
                    gated(n, moving(n))
                ts = []
                for _ in range(a.repeat):
                    f = moving(n)
                    t0 = time.perf_counter()
                    ne = gated(n, f)
                    ts.append((time.perf_counter() - t0) * 1e3)
                    embedded[n].append(ne)
                times[n] += ts
                leg_means[n].append(statistics.mean(ts))
        for n in trk:
            e, t = np.asarray(embedded[n]), np.asarray(times[n])
            report(n, {"calls": len(t), "mean": float(t.mean()), "median": float(np.median(t)), "min": float(t.min()), "max": float(t.max()),
                       "leg_means": leg_means[n], "n_embed_mean": float(e.mean()), "n_embed_min": int(e.min()), "n_embed_max": int(e.max())})
        gate_medians = {n: [] for n in trk}
        for _ in range(a.legs):
            for n in trk:
                frt.profile_enable(2)
                for _ in range(a.repeat):
                    gated(n, moving(n))
                kn, ms, _ = frt.profile_collect()
                frt.profile_enable(0)
                gate_medians[n].append(statistics.median([float(t) for k, t in zip(kn, ms) if k == "track_gate"]))
        for n, v in gate_medians.items():
            report("p_track_gate_" + n.split("_")[1], {"leg_medians": v, "median": statistics.median(v), "min": min(v), "max": max(v)})
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
        for t in trk.values():
            t.close()
        pipe.close(), rec.close(), det.close()
        return
    names = ["run_tracked"] + ["gated_refresh_%d" % r for r in a.refresh]
    trackers = {n: frt.Tracker(S, T, MF, 512) for n in names}
    embedded = {n: [] for n in names}

    def call(name):
        if name == "run_tracked":
            pipe.runTracked(trackers[name], frames, want_embeds=False, want_templates=False)
            return out["faces_per_call"]
        r = int(name.rsplit("_", 1)[1])
        return pipe.runTrackedGated(trackers[name], frames, r, a.min_embeds, a.skip_iou, want_embeds=False, want_templates=False)[4]

    for n in names:  # every track confirmed and embedded before anything is timed
        for _ in range(5):
            call(n)

    if a.profile:
        frt.profile_enable(2)
        for n in names[1:]:
            for _ in range(a.repeat):
                embedded[n].append(call(n))
        kn, ms, _ = frt.profile_collect()
        frt.profile_enable(0)
        for part in ("track_gate", "crop_faces_gather", "track_gate_scatter", "embed_network", "match_top1", "track_update"):
            ks = [float(t) for k, t in zip(kn, ms) if k == part]
            if ks:
                report("p_" + part, {"launches": len(ks), "median": statistics.median(ks), "min": min(ks), "max": max(ks)})
        for n in names[1:]:
            out["cases"]["p_n_embed_" + n] = {"mean": statistics.mean(embedded[n]), "min": min(embedded[n]), "max": max(embedded[n])}
    else:
        times = {n: [] for n in names}
        leg_medians = {n: [] for n in names}
        for _ in range(a.legs):
            for n in names:
                for _ in range(3):
                    call(n)
                ts = []
                for _ in range(a.repeat):
                    t0 = time.perf_counter()
                    ne = call(n)
                    ts.append((time.perf_counter() - t0) * 1e3)
                    embedded[n].append(ne)
                times[n] += ts
                leg_medians[n].append(statistics.median(ts))
        for n in names:
            e = np.asarray(embedded[n])
            t = np.asarray(times[n])
            r = {"calls": len(t), "median": float(np.median(t)), "mean": float(t.mean()), "min": float(t.min()), "max": float(t.max()),
                 "leg_medians": leg_medians[n], "n_embed_mean": float(e.mean()), "n_embed_min": int(e.min()), "n_embed_max": int(e.max())}
            if n != "run_tracked":  # the two kinds of call of a gated leg apart
                for kind, m in (("calls_that_embed_nothing", e == 0), ("calls_that_embed", e > 0)):
                    if m.any():
                        r[kind] = {"calls": int(m.sum()), "median": float(np.median(t[m])), "min": float(t[m].min()), "max": float(t[m].max())}
            report(n, r)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    for t in trackers.values():
        t.close()
    pipe.close(), rec.close(), det.close()


if __name__ == "__main__":
    main()
