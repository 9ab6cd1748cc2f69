"""Recognising a large photo by tiles: wall time of Pipeline.runTiled on one synthetic photo against the loop a user writes without it -
findFaceTiled, the gate on the host, forward on the kept boxes (the photo goes up a second time, one synchronisation per recogniser pass),
MatMul.top1 - on the same three objects in the same process, on alternating legs, with the spread.  Also the device time of the select
launch, of the crop launches and of the other stages inside the call (profiling scopes of frt_profile_enable(2)).

    python tools/tiled_recognise_timing.py [--rows 2160] [--cols 3840] [--frame 640] [--batch 32] [--faces 32] [--rec-batch 128]
                                           [--gallery 100000] [--bbox 0.6] [--min-face 0] [--legs 5] [--reps 5]     prints one JSON line"""
import argparse
import ctypes
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
import tile_faces_ref as tf  # noqa: E402


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
    ap.add_argument("--rec-batch", type=int, default=128)
    ap.add_argument("--gallery", type=int, default=100000)
    ap.add_argument("--bbox", type=float, default=0.6)
    ap.add_argument("--min-face", type=int, default=0)
    ap.add_argument("--legs", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    frt = entry.load_pkg()
    s = frt.synth
    tmp = tempfile.mkdtemp()
    dpath = frt.write_weights(os.path.join(tmp, "det.frtw"), s.retinaface_state(1), frt.weights_io.KIND_RETINAFACE_MNET025)
    rpath = frt.write_weights(os.path.join(tmp, "ir.frtw"), s.arcface_state(2, "ir", calib=s.load_calibration("ir")), frt.weights_io.KIND_ARCFACE_IR50)
    T = a.frame
    det = frt.RetinaFace(dpath, T, T, (3, T, T), a.batch, a.faces, 0.4, a.bbox)
    rec = frt.ArcFaceIR50(rpath, T, T, maxBatchSize=a.rec_batch, maxFacesPerScene=a.faces)
    rec.setGallery(s.make_gallery(a.gallery))
    rec.initMatMul()
    pipe = frt.Pipeline(det, rec, a.batch)
    photo = np.ascontiguousarray(s.make_frame(0, a.rows, a.cols))
    max_out = 1024
    p = lambda arr: ctypes.c_void_p(arr.ctypes.data)

    def call():
        return pipe.runTiled(photo, min_face=a.min_face, max_out=max_out)

    def user_loop():
        boxes = det.findFaceTiled(photo, max_out=max_out)
        kb = np.ascontiguousarray(boxes[tf.gate(boxes, a.min_face)])
        n = len(kb)
        emb = np.zeros((n, 512), np.float32)
        if n == 0:
            return kb, emb, np.zeros(0, np.int32), np.zeros(0, np.float32)
        rc = frt.lib.frt_embedder_forward(rec._h, p(photo), a.rows, a.cols, photo.strides[0], p(kb), n, p(emb), None)
        assert rc in (frt.FRT_OK, frt.FRT_ERR_EMPTY_ROI)
        idx, sim = rec.matmul.top1(emb)
        return kb, emb, idx, sim

    def timed(fn, reps):
        ms = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            ms.append((time.perf_counter() - t0) * 1e3)
        return ms

    got, want = call(), user_loop()  # warm-up of both, and the answers agree
    res, emb = got
    ok = res["valid"] != 0
    same = (len(res) == len(want[0]) and emb.tobytes() == want[1].tobytes() and all(res[c].tobytes() == want[0][c].tobytes() for c in ("x1", "y1", "x2", "y2", "score"))
            and np.array_equal(res["match_idx"][ok], want[2][ok]) and res["match_sim"][ok].tobytes() == want[3][ok].tobytes())
    for _ in range(2):
        call()
        user_loop()
    t = {"call": [], "loop": []}
    for _ in range(a.legs):
        t["call"] += timed(call, a.reps)
        t["loop"] += timed(user_loop, a.reps)
    detect = timed(lambda: det.findFaceTiled(photo, max_out=max_out), a.reps)  # the first stage alone, for scale
    frt.profile_enable(2)
    try:
        for _ in range(a.reps):
            call()
        labels, ms, _ = frt.profile_collect()
    finally:
        frt.profile_enable(0)
    by = {}
    for l, m in zip(labels, ms):
        by.setdefault(l, []).append(float(m))
    per_call = {k: [sum(v[i * (len(v) // a.reps):(i + 1) * (len(v) // a.reps)]) for i in range(a.reps)] for k, v in by.items() if len(v) >= a.reps}
    call_med, loop_med = float(np.median(t["call"])), float(np.median(t["loop"]))
    out = {
        "photo": [a.rows, a.cols], "frame": T, "det_max_batch": a.batch, "max_faces": a.faces, "rec_max_batch": a.rec_batch, "gallery_rows": a.gallery,
        "bbox_threshold": a.bbox, "min_face": a.min_face, "faces": int(len(res)), "passes": int(-(-len(res) // a.rec_batch)), "answers_equal": bool(same),
        "legs": a.legs, "call_wall": spread(t["call"]), "user_loop_wall": spread(t["loop"]), "detect_alone_wall": spread(detect),
        "saved_ms_median": round(loop_med - call_med, 3), "speedup_median": round(loop_med / call_med, 3),
        # beyond the spread: the slowest call is still faster than the fastest loop
        "faster_beyond_spread": bool(max(t["call"]) < min(t["loop"])),
        "device_per_call": {k: spread(v) for k, v in sorted(per_call.items())},
    }
    pipe.close()
    det.close()
    rec.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
