"""Photos per second of the two ways to enrol whole photos (DESIGN section "Whole photos of any sizes").

One process, one detector (640 x 640 frames, max batch 32, 4 faces per scene), one recogniser (IR-50, synthetic weights, maxBatchSize 128), a
--gallery row gallery (default 1M), --photos photos (default 1024) of 480x640, 720x1280 and 1080x1920 in turn, and two legs, alternated
--repeat times so that each leg's own spread is seen beside the difference between the legs:

  loop   what a caller had to write before enrolImages: per photo resizeFrame (host -> device -> host), Pipeline.run of that one frame,
         the box count on the host, enrolEmbedding of the one face's embedding (its gallery edit, MatMul.galleryAdd; the Python name list
         is left out of the timed loop: the one difference from the loop a caller writes).  --loop-photos runs it on fewer photos.
  batch  Pipeline.enrolImages: the photos' bytes up once per chunk of 32, one resize kernel per chunk, the chunks back to back through the
         three-stage pipeline, the rule on the device, ONE gallery edit.

Both legs end with their device work complete; the host clock is around them.  After each leg the rows it added are removed again (outside
the timed region), so every repeat starts from the same gallery.  Afterwards one enrolImages call with the stage profile on gives the
resize kernel's time per chunk beside the other stages'.  Needs the GPU: without one the objects cannot be created and the script fails.

    python tools/enrol_images_timing.py [--photos 1024] [--repeat 5] [--gallery 1000000] [--out profiles/...json]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as entry

SIZES = [(480, 640), (720, 1280), (1080, 1920)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--photos", type=int, default=1024)
    ap.add_argument("--loop-photos", type=int, default=0, help="photos of the per-photo leg (0: all of them)")
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--gallery", type=int, default=1000000)
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    frt = entry.load_pkg()
    s = frt.synth
    tmp = tempfile.mkdtemp(prefix="frt_photos_")
    dpath = frt.write_weights(os.path.join(tmp, "det.frtw"), s.retinaface_state(1), 1)
    rpath = frt.write_weights(os.path.join(tmp, "rec.frtw"), s.arcface_state(2, "ir", calib=s.load_calibration("ir")), 2)
    H = W = 640
    B, K = a.frames, 4
    det = frt.RetinaFace(dpath, W, H, (3, H, W), B, K, 0.4, 0.6)
    rec = frt.ArcFaceIR50(rpath, W, H, maxBatchSize=B * K, maxFacesPerScene=K)
    N = a.gallery
    rec.setGallery(s.make_gallery(N))
    rec.initMatMul()
    mm = rec.matmul
    mm.galleryReserve(N + a.photos)
    pipe = frt.Pipeline(det, rec, B)
    n = a.photos
    nl = min(a.loop_photos, n) if a.loop_photos > 0 else n
    base = [[s.make_frame(900 + 8 * k + i, r, c) for i in range(8)] for k, (r, c) in enumerate(SIZES)]  # a few distinct photos per size, reused
    photos = [base[i % 3][(i // 3) % 8] for i in range(n)]
    names = ["p%d" % i for i in range(n)]

    def restore():
        rows = int(frt.lib.frt_matcher_num_rows(mm._h))
        if rows > N:
            mm.galleryRemove(list(range(N, rows)))
        rec.classNames = list(rec.classNames)[:N]
        rec.classCount = N

    def leg_loop():
        added = 0
        for i in range(nl):
            frame = frt.resizeFrame(photos[i], W, H)
            res, emb = pipe.run(frame[None])
            if int((res["score"] > 0).sum()) == 1 and res["valid"][0]:
                mm.galleryAdd(emb[0])  # (enrolEmbedding without its name list: copying a 1M-entry Python list per photo is not the library's time)
                added += 1
        return added

    def leg_batch():
        return int((pipe.enrolImages(names, photos)[0] == frt.FRT_ENROL_OK).sum())

    legs = {"loop": (leg_loop, nl), "batch": (leg_batch, n)}
    accepted = {}
    for k, (fn, _) in legs.items():  # warm-up of every shape, and the answers
        accepted[k] = fn()
        restore()
    status = pipe.enrolImages(names, photos)[0]
    restore()
    out = {"photos": n, "photos_leg_loop": nl, "frames_per_chunk": B, "gallery_rows": N, "repeat": a.repeat, "unit": "photos/s", "accepted": accepted,
           "status_counts": {str(k): int((status == k).sum()) for k in (1, 2, 3, 4)},
           "bytes_up_per_photo": sum(p.nbytes for p in photos) / n}
    rates = {k: [] for k in legs}
    for _ in range(a.repeat):
        for k in ("batch", "loop"):
            fn, cnt = legs[k]
            t0 = time.perf_counter()
            fn()
            rates[k].append(cnt / (time.perf_counter() - t0))
            restore()
    for k in legs:
        r = rates[k]
        out[k] = {"median": statistics.median(r), "min": min(r), "max": max(r), "all": r}
        print("leg %-5s  median %8.1f photos/s  (min %8.1f  max %8.1f)" % (k, statistics.median(r), min(r), max(r)), flush=True)
    out["ratio_of_medians"] = out["batch"]["median"] / out["loop"]["median"]
    # one profiled call (the stages then run one after the other on one stream): the resize kernel per chunk beside the other stages
    frt.profile_enable(2)
    pipe.enrolImages(names, photos)
    labels, ms, _work = frt.profile_collect()
    frt.profile_enable(0)
    restore()
    prof = {}
    for lab in sorted(set(labels)):
        v = [m for l, m in zip(labels, ms) if l == lab]
        prof[lab] = {"launches": len(v), "median_ms": statistics.median(v), "total_ms": float(sum(v))}
    for lab in ("images_resize", "enrol_select"):
        if lab in prof:
            print("profile %-14s %4d chunks  median %.3f ms  total %.1f ms" % (lab, prof[lab]["launches"], prof[lab]["median_ms"], prof[lab]["total_ms"]),
                  flush=True)
    out["profile"] = prof
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    pipe.close()
    det.close()
    rec.close()


if __name__ == "__main__":
    main()
