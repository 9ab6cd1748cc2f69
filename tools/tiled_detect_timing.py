"""Large photos by tiles: wall time of RetinaFace.findFaceTiled on one synthetic photo against the loop a user writes today - numpy cut,
findFaceBatch per chunk of max_batch tiles, numpy merge (tests/tiled_ref.py) - on the same detector object in the same run, on alternating
legs, with the spread.  Also the device time of the cut and of the merge inside the call (profiling scopes "tiles_cut" / "tiles_merge" of
frt_profile_*), and the merge alone at 16384 candidates (frt_merge_boxes: wall time, which includes its upload, download and allocation, and
the device time of its four launches).

    python tools/tiled_detect_timing.py [--rows 2160] [--cols 3840] [--frame 640] [--batch 32] [--faces 32] [--legs 5] [--reps 5]
                                        [--family mnet]                                                      prints one JSON line"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as entry  # noqa: E402
import tiled_ref as tr  # noqa: E402


def spread(v):
    v = np.asarray(v, np.float64)
    return {"median_ms": round(float(np.median(v)), 3), "min_ms": round(float(v.min()), 3), "max_ms": round(float(v.max()), 3), "n": int(len(v))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=2160)
    ap.add_argument("--cols", type=int, default=3840)
    ap.add_argument("--frame", type=int, default=640)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--faces", type=int, default=32)
    ap.add_argument("--legs", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    frt = entry.load_pkg()
    s = frt.synth
    tmp = tempfile.mkdtemp()
    path = frt.write_weights(os.path.join(tmp, "det.frtw"), s.retinaface_state(1), 1)
    T = a.frame
    det = frt.RetinaFace(path, T, T, (3, T, T), a.batch, a.faces, 0.4, 0.6)
    photo = s.make_frame(0, a.rows, a.cols)
    tiles = tr.plan(a.rows, a.cols, T, T, T // 4, T // 4, True)
    max_out = 1024

    def tiled():
        return det.findFaceTiled(photo, max_out=max_out, sources=True)

    def user_loop():
        """cut with numpy (the overview through resizeFrame), findFaceBatch per chunk, merge with numpy"""
        frames = tr.cut(photo, tiles, T, T, resize=frt.resizeFrame)
        boxes = np.zeros((len(tiles), a.faces), tr.BBOX_DTYPE)
        n = np.zeros(len(tiles), np.int32)
        for first in range(0, len(tiles), a.batch):
            for i, bx in enumerate(det.findFaceBatch(frames[first:first + a.batch])):
                boxes[first + i, :len(bx)] = bx
                n[first + i] = len(bx)
        out, src, cnt = tr.merge(boxes, n, tiles, a.rows, a.cols, T, T, 1, True, np.float32(0.4), max_out)
        return out[:cnt], src[:cnt]

    def timed(fn, reps):
        ms = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            ms.append((time.perf_counter() - t0) * 1e3)
        return ms

    got, want = tiled(), user_loop()  # warm-up of both, and the answers agree
    same = got[0].tobytes() == want[0].tobytes() and np.array_equal(got[1], want[1])
    for _ in range(2):
        tiled()
    t = {"tiled": [], "loop": []}
    for _ in range(a.legs):
        t["tiled"] += timed(tiled, a.reps)
        t["loop"] += timed(user_loop, max(1, a.reps // 2))
    # device time of the cut (one scope per chunk: summed per call) and of the merge inside the call
    frt.profile_enable(2)
    try:
        for _ in range(a.reps):
            tiled()
        labels, ms, _ = frt.profile_collect()
    finally:
        frt.profile_enable(0)
    by = {}
    for l, m in zip(labels, ms):
        by.setdefault(l, []).append(float(m))
    chunks = -(-len(tiles) // a.batch)
    per_call = {k: [sum(v[i * (len(v) // a.reps):(i + 1) * (len(v) // a.reps)]) for i in range(a.reps)] for k, v in by.items()}
    # the merge alone at the most candidates there may be: 2048 tiles x 8 slots at random origins of a 4000 x 4000 photo
    rng = np.random.Generator(np.random.PCG64(7))
    mt = np.zeros(2048, tr.TILE_DTYPE)
    mt["row0"], mt["col0"] = rng.integers(0, 4000 - T, 2048), rng.integers(0, 4000 - T, 2048)
    mt["rows"] = mt["cols"] = T
    mb = np.zeros((2048, 8), tr.BBOX_DTYPE)
    mb["x1"], mb["y1"] = rng.integers(0, T - 64, mb.shape), rng.integers(0, T - 64, mb.shape)
    mb["x2"], mb["y2"] = mb["x1"] + rng.integers(16, 64, mb.shape), mb["y1"] + rng.integers(16, 64, mb.shape)
    mb["score"] = rng.random(mb.shape, np.float32)
    mn = np.full(2048, 8, np.int32)

    def merge_alone():
        return frt.mergeBoxes(mb, mn, mt, 4000, 4000, T, T, 1, False, 0.4, 16384)

    kept = len(merge_alone()[0])
    merge_wall = timed(merge_alone, 2 * a.reps)
    frt.profile_enable(2)
    try:
        for _ in range(a.reps):
            merge_alone()
        labels, ms, _ = frt.profile_collect()
    finally:
        frt.profile_enable(0)
    merge_dev = [float(m) for l, m in zip(labels, ms) if l == "tiles_merge"]
    out = {
        "photo": [a.rows, a.cols], "frame": T, "max_batch": a.batch, "max_faces": a.faces, "tiles": int(len(tiles)), "chunks": int(chunks),
        "boxes": int(len(got[0])), "answers_equal": bool(same), "legs": a.legs,
        "tiled_wall": spread(t["tiled"]), "user_loop_wall": spread(t["loop"]),
        "speedup_median": round(float(np.median(t["loop"]) / np.median(t["tiled"])), 2),
        "device_per_call": {k: spread(per_call[k]) for k in ("tiles_cut", "tiles_merge", "det_network", "det_postprocess") if k in per_call},
        "merge_16384": {"kept": int(kept), "wall": spread(merge_wall), "device": spread(merge_dev)},
    }
    det.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
