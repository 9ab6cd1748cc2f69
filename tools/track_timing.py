"""What following faces across frames costs on the device, against doing it on the host.

32 streams, max_faces 4, max_tracks 16, one 1M x 512 gallery, one process.  The tracker alone (a, b) is fed the records and embeddings of a
seeded random walk (4 faces per stream, resident in HBM); the pipeline legs (c) run synthetic 640 x 640 frames.
  a  frt_tracker_update_dev alone: the whole call by device events on its stream, and split by the library's profiling hooks
     (frt_profile_enable(2)) into track_update (the update kernel), match_top1 (the extra search) and track_identity
  b  the same update done the only way possible without the tracker: records and embeddings to the host, tests/track_ref.py, MatMul.top1 of
     the templates (host wall time, the downloads included)
  c  frt_pipeline_run_tracked - appearance off, and on - against frt_pipeline_run of the same frames, on alternating legs in one process:
     --legs triples of --repeat calls each; per leg the median call, then the spread of the leg medians
With appearance on (--reid / --min-sim, 0.5 / 0.2):
  a_on_*  leg a again: the whole call, and its split into track_similarity (the similarity kernel), track_update and the rest
  w_*     the similarity kernel's worst case, once: 256 frames x 64 detections x 64 live tracks, dim 512, no matcher
With --motion GAIN (a run of its own, instead of everything above, same shape, no gallery):
  m_update_*   the update kernel alone (frt_profile_enable(2): track_update) over the same walk, motion off and on - and, with --parent-lib,
               the kernel of another build of the library (the parent commit's) - on alternating legs in one process
  m_tracked_*  frt_pipeline_run_tracked with motion off and on, alternating legs
Needs the GPU.  Run it under a time limit, one process:

    timeout 900 python tools/track_timing.py [--rows 1000000] [--streams 32] [--repeat 30] [--legs 3] --out result.json
    timeout 600 python tools/track_timing.py --motion 128 [--parent-lib old/libfrt.so] [--legs 5] --out result.json
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


def walk(rng, n_streams, max_faces, updates):
    """records of a random walk: max_faces faces per stream drifting over a 640 x 640 frame, nine in ten seen -> [updates][n_streams * max_faces]"""
    import track_ref as tk
    pos = rng.uniform(40, 500, (n_streams, max_faces, 2))
    vel = rng.uniform(-5, 5, (n_streams, max_faces, 2))
    out = []
    for _ in range(updates):
        pos += vel
        vel[(pos < 10) | (pos > 540)] *= -1
        r = np.zeros((n_streams, max_faces), tk.RESULT_DTYPE)
        r["match_idx"] = -1
        for s in range(n_streams):
            seen = [f for f in range(max_faces) if rng.random() < 0.9]
            for d, f in enumerate(seen):
                x, y = int(pos[s, f, 0]), int(pos[s, f, 1])
                r[s, d] = (x, y, x + 80, y + 80, 0.9 - 0.1 * d, s, -1, 0.0, 1)
        out.append(r.reshape(-1))
    return out


def load_other_build(path):
    """the binding once more, over another build of the library (symbols it lacks are skipped, as bench.py --ab-old-lib loads it)"""
    import importlib.util
    import types
    os.environ["FRT_LIB"] = os.path.abspath(path)
    sys.modules["frt_amd_ab_old_library"] = types.ModuleType("frt_amd_ab_old_library")
    try:
        spec = importlib.util.spec_from_file_location("frt_amd_other", os.path.join(entry.PKG_DIR, "__init__.py"), submodule_search_locations=[entry.PKG_DIR])
        mod = importlib.util.module_from_spec(spec)
        sys.modules["frt_amd_other"] = mod
        spec.loader.exec_module(mod)
    finally:
        del os.environ["FRT_LIB"], sys.modules["frt_amd_ab_old_library"]
    return mod


def motion_legs(a, frt, report, out):
    """--motion: the update kernel and frt_pipeline_run_tracked with motion off and on, alternating legs (see the module docstring)"""
    import torch
    S, MF, T, D = a.streams, 4, 16, 512
    F = S * MF
    rng = np.random.default_rng(1)
    steps = walk(rng, S, MF, a.repeat + 5)
    emb = rng.standard_normal((F, D)).astype(np.float32)
    emb /= np.linalg.norm(emb, axis=1, keepdims=True)
    d_res = [torch.from_numpy(r.view(np.uint8).copy()).cuda() for r in steps]
    d_emb = torch.from_numpy(emb).cuda()
    d_trk = torch.zeros(F * 32, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    builds = {"off": (frt, None), "on": (frt, a.motion)}
    if a.parent_lib:
        builds["parent"] = (load_other_build(a.parent_lib), None)
    trackers = {n: (lib, lib.Tracker(S, T, MF, D) if gain is None else lib.Tracker(S, T, MF, D, motion_gain=gain)) for n, (lib, gain) in builds.items()}
    medians = {n: [] for n in trackers}
    for _ in range(a.legs):
        for n, (lib, trk) in trackers.items():
            trk.reset()
            for k in range(5):
                trk.updateDev(d_res[k].data_ptr(), d_emb.data_ptr(), S, d_trk.data_ptr(), None, None, None, stream)
            torch.cuda.synchronize()
            lib.profile_enable(2)
            for k in range(5, 5 + a.repeat):
                trk.updateDev(d_res[k].data_ptr(), d_emb.data_ptr(), S, d_trk.data_ptr(), None, None, None, stream)
            torch.cuda.synchronize()
            names, ms, _ = lib.profile_collect()
            lib.profile_enable(0)
            ks = [float(t) for nm, t in zip(names, ms) if nm == "track_update"]
            assert len(ks) == a.repeat, (n, len(ks))
            medians[n].append(statistics.median(ks))
    for n, v in medians.items():
        report("m_update_" + n, {"leg_medians": v, "median": statistics.median(v), "min": min(v), "max": max(v)})
    out["m_live_tracks"] = {n: sum(int((trk.tracks(s)[0]["live"] != 0).sum()) for s in range(S)) for n, (_, trk) in trackers.items()}
    for _, trk in trackers.values():
        trk.close()
    # ---- the pipeline, the frames repeated (a still scene: the velocities stay zero, the cost is the instantiation's)
    tmp = tempfile.mkdtemp(prefix="frt_track_timing_")
    s = frt.synth
    det_path = frt.write_weights(os.path.join(tmp, "det.frtw"), s.retinaface_state(1), 1)
    rec_path = frt.write_weights(os.path.join(tmp, "rec.frtw"), s.arcface_state(2, "ir", calib=s.load_calibration("ir")), 2)
    W = H = a.frame
    det = frt.RetinaFace(det_path, W, H, (3, H, W), S, MF, 0.4, 0.6)
    rec = frt.ArcFaceIR50(rec_path, W, H, (3, 112, 112), 512, F, MF, 0.65)
    pipe = frt.Pipeline(det, rec, S, match=False)
    frames = s.make_frames(S, H, W)
    trk = {"off": frt.Tracker(S, T, MF, D), "on": frt.Tracker(S, T, MF, D, motion_gain=a.motion)}
    legs = {n: [] for n in trk}
    for _ in range(a.legs):
        for n in trk:
            for _ in range(3):
                pipe.runTracked(trk[n], frames)
            ts = []
            for _ in range(a.repeat):
                t0 = time.perf_counter()
                pipe.runTracked(trk[n], frames)
                ts.append((time.perf_counter() - t0) * 1e3)
            legs[n].append(statistics.median(ts))
    for n, v in legs.items():
        report("m_tracked_" + n, {"leg_medians": v, "median": statistics.median(v), "min": min(v), "max": max(v)})
    for t in trk.values():
        t.close()
    pipe.close(), rec.close(), det.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--streams", type=int, default=32)
    ap.add_argument("--repeat", type=int, default=30)
    ap.add_argument("--legs", type=int, default=3)
    ap.add_argument("--frame", type=int, default=640)
    ap.add_argument("--reid", type=float, default=0.5, help="reid_threshold of the legs with appearance on")
    ap.add_argument("--min-sim", dest="min_sim", type=float, default=0.2, help="iou_min_sim of the legs with appearance on")
    ap.add_argument("--motion", type=int, default=0, help="the motion legs alone, with this gain (1 .. 256) for the legs with motion on")
    ap.add_argument("--parent-lib", dest="parent_lib", default=None, help="--motion: another build of libfrt.so whose update kernel joins the legs")
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    import torch
    import track_ref as tk
    frt = entry.load_pkg()
    S, MF, T, D, N = a.streams, 4, 16, 512, a.rows
    F = S * MF
    if a.motion:
        out = {"streams": S, "max_faces": MF, "max_tracks": T, "repeat": a.repeat, "legs": a.legs, "unit": "ms", "motion_gain": a.motion, "cases": {}}

        def report(name, r):
            out["cases"][name] = r
            print("%-28s %s" % (name, json.dumps(r)), flush=True)

        motion_legs(a, frt, report, out)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
        return
    rng = np.random.default_rng(1)
    g = frt.synth.make_gallery(N)
    mm = frt.MatMul(0)
    mm.init(g)
    out = {"streams": S, "max_faces": MF, "max_tracks": T, "gallery_rows": N, "repeat": a.repeat, "legs": a.legs, "unit": "ms", "cases": {}}

    def stats(ts):
        return {"median": statistics.median(ts), "min": min(ts), "max": max(ts)}

    def report(name, r):
        out["cases"][name] = r
        print("%-28s %s" % (name, json.dumps(r)), flush=True)

    # ---- the walk, resident in HBM: each face's embeddings are a gallery row plus noise, so the screened search sees queries that match
    steps = walk(rng, S, MF, a.repeat + 5)
    who = rng.integers(0, N, (S, MF))
    embeds = [frt.synth.make_queries(g, who.reshape(-1), noise=0.05).astype(np.float32) for _ in range(4)]
    d_res = [torch.from_numpy(r.view(np.uint8).copy()).cuda() for r in steps]
    d_emb = [torch.from_numpy(e).cuda() for e in embeds]
    d_trk = torch.zeros(F * 32, dtype=torch.uint8, device="cuda")
    d_tpl = torch.zeros((F, D), dtype=torch.float32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream

    # ---- a: update_dev alone
    trk = frt.Tracker(S, T, MF, D)
    upd = lambda k: trk.updateDev(d_res[k].data_ptr(), d_emb[k % 4].data_ptr(), S, d_trk.data_ptr(), d_tpl.data_ptr(), None, mm, stream)
    for k in range(5):
        upd(k)
    torch.cuda.synchronize()
    ts = []
    for k in range(5, 5 + a.repeat):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        upd(k)
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    report("a_update_dev", stats(ts))
    trk.reset()
    frt.profile_enable(2)
    for k in range(a.repeat):
        upd(k)
    torch.cuda.synchronize()
    names, ms, _ = frt.profile_collect()
    frt.profile_enable(0)
    for part in ("track_update", "match_top1", "track_identity"):
        ks = [float(t) for n, t in zip(names, ms) if n == part]
        assert len(ks) == a.repeat, (part, len(ks), set(names))
        report("a_" + part, stats(ks))
    live = sum(int((trk.tracks(s)[0]["live"] != 0).sum()) for s in range(S))
    out["live_tracks_after_a"] = live

    # ---- a, appearance on: the same updates with reid_threshold 0.5 / iou_min_sim 0.2 - the similarity kernel in
    #      front of the update kernel's other instantiation
    on = frt.Tracker(S, T, MF, D, reid_threshold=a.reid, iou_min_sim=a.min_sim)
    upd_on = lambda k: on.updateDev(d_res[k].data_ptr(), d_emb[k % 4].data_ptr(), S, d_trk.data_ptr(), d_tpl.data_ptr(), None, mm, stream)
    for k in range(5):
        upd_on(k)
    torch.cuda.synchronize()
    ts = []
    for k in range(5, 5 + a.repeat):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        upd_on(k)
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    report("a_on_update_dev", stats(ts))
    on.reset()
    frt.profile_enable(2)
    for k in range(a.repeat):
        upd_on(k)
    torch.cuda.synchronize()
    names, ms, _ = frt.profile_collect()
    frt.profile_enable(0)
    for part in ("track_similarity", "track_update", "match_top1", "track_identity"):
        ks = [float(t) for n, t in zip(names, ms) if n == part]
        assert len(ks) == a.repeat, (part, len(ks), set(names))
        report("a_on_" + part, stats(ks))
    on.close()

    # ---- w: the worst case of the similarity kernel, once: 256 frames x 64 detections x 64 live tracks with embeddings (no matcher)
    WF, WS = 256, 64
    wrng = np.random.default_rng(2)
    wres = np.zeros((WF, WS), tk.RESULT_DTYPE)
    wres["match_idx"] = -1
    for d in range(WS):
        x, y = 80 * (d % 8), 80 * (d // 8)
        wres[:, d] = (x, y, x + 60, y + 60, 0.99 - 0.01 * d, 0, -1, 0.0, 1)
    wemb = wrng.standard_normal((WF * WS, D)).astype(np.float32)
    wemb /= np.linalg.norm(wemb, axis=1, keepdims=True)
    w_res, w_emb = torch.from_numpy(wres.reshape(-1).view(np.uint8).copy()).cuda(), torch.from_numpy(wemb).cuda()
    w_trk = torch.zeros(WF * WS * 32, dtype=torch.uint8, device="cuda")
    worst = frt.Tracker(WF, WS, WS, D, reid_threshold=a.reid, iou_min_sim=a.min_sim)
    upd_w = lambda: worst.updateDev(w_res.data_ptr(), w_emb.data_ptr(), WF, w_trk.data_ptr(), None, None, None, stream)
    for _ in range(3):   # the first one gives every slot a track with an embedding
        upd_w()
    torch.cuda.synchronize()
    frt.profile_enable(2)
    for _ in range(10):
        upd_w()
    torch.cuda.synchronize()
    names, ms, _ = frt.profile_collect()
    frt.profile_enable(0)
    for part in ("track_similarity", "track_update"):
        report("w_" + part, stats([float(t) for n, t in zip(names, ms) if n == part]))
    out["w_live_tracks"] = sum(int((worst.tracks(s)[0]["n_embeds"] > 0).sum()) for s in (0, WF - 1))
    worst.close()

    # ---- b: the same update on the host
    ref = tk.Tracker(S, T, MF, D)
    ts, parts = [], {"download": [], "track_ref": [], "top1": []}
    for k in range(a.repeat):
        t0 = time.perf_counter()
        res = d_res[k].cpu().numpy().view(tk.RESULT_DTYPE)
        emb = d_emb[k % 4].cpu().numpy()
        t1 = time.perf_counter()
        tracks, tpl = ref.update(res, emb)
        t2 = time.perf_counter()
        idx, sim = mm.top1(tpl.reshape(-1, D).astype(np.float32))
        ref.apply_identity(tracks, None, idx, sim)
        t3 = time.perf_counter()
        ts.append((t3 - t0) * 1e3)
        for name, dt in (("download", t1 - t0), ("track_ref", t2 - t1), ("top1", t3 - t2)):
            parts[name].append(dt * 1e3)
    report("b_host_update", stats(ts))
    for name, v in parts.items():
        report("b_" + name, stats(v))
    trk.close()
    mm.close()

    # ---- c: the pipeline with and without the tracker behind it, alternating legs
    tmp = tempfile.mkdtemp(prefix="frt_track_timing_")
    s = frt.synth
    det_path = frt.write_weights(os.path.join(tmp, "det.frtw"), s.retinaface_state(1), 1)
    rec_path = frt.write_weights(os.path.join(tmp, "rec.frtw"), s.arcface_state(2, "ir", calib=s.load_calibration("ir")), 2)
    W = H = a.frame
    det = frt.RetinaFace(det_path, W, H, (3, H, W), S, MF, 0.4, 0.6)
    rec = frt.ArcFaceIR50(rec_path, W, H, (3, 112, 112), 512, F, MF, 0.65)
    rec.setGallery(g)
    rec.initMatMul()
    pipe = frt.Pipeline(det, rec, S)
    frames = s.make_frames(S, H, W)
    trk = frt.Tracker(S, T, MF, D)
    trk_on = frt.Tracker(S, T, MF, D, reid_threshold=a.reid, iou_min_sim=a.min_sim)
    legs = {"run": [], "run_tracked": [], "run_tracked_on": []}

    def leg(fn):
        for _ in range(3):
            fn()
        ts = []
        for _ in range(a.repeat):
            t0 = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(ts)

    for _ in range(a.legs):
        legs["run"].append(leg(lambda: pipe.run(frames)))
        legs["run_tracked"].append(leg(lambda: pipe.runTracked(trk, frames)))
        legs["run_tracked_on"].append(leg(lambda: pipe.runTracked(trk_on, frames)))
    for name, v in legs.items():
        report("c_" + name, {"leg_medians": v, "median": statistics.median(v), "min": min(v), "max": max(v)})
    out["c_faces_per_call"] = int((pipe.run(frames)[0]["score"] > 0).sum())
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    trk.close(), trk_on.close(), pipe.close(), rec.close(), det.close()


if __name__ == "__main__":
    main()
