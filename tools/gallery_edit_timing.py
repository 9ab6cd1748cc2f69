"""What a live gallery edit costs beside the only alternative, a full reload.

One 1M x 512 fp32 gallery, one process: medians of repeated edits (frt_matcher_gallery_add / add_dev / remove; host clock around calls
that return when their device work is complete), the edit_stats increments of each case, and the full frt_matcher_init of the same rows -
the path before live edits, what bench.py reports as config.gallery_load_s.  After every timed edit the gallery is brought back to its size
outside the timed window (an add is undone by removing the new rows, a remove by adding the rows back), so every repetition edits a gallery of
--rows rows.  Needs the GPU: without one the matcher cannot be created and the script fails.

    python tools/gallery_edit_timing.py [--rows 1000000] [--repeat 9] [--out profiles/...json]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import __graft_entry__ as entry


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--repeat", type=int, default=9)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    frt = entry.load_pkg()
    N, D = a.rows, 512
    g = frt.synth.make_gallery(N)
    extra = frt.synth.make_gallery(1024, seed=77)
    extra_dev = torch.from_numpy(extra).cuda()
    torch.cuda.synchronize()
    mm = frt.MatMul(0)
    mm.galleryReserve(N + 4096)
    q = frt.synth.make_queries(g, [0, N // 2, N - 1], noise=0.01)

    def timed(fn):
        t0 = time.perf_counter()
        fn()
        return (time.perf_counter() - t0) * 1e3

    def stats_delta(before):
        after = mm.editStats()
        return {k: after[k] - before[k] for k in after}

    out = {"rows": N, "cols": D, "repeat": a.repeat, "unit": "ms", "cases": {}}
    # the alternative: the whole gallery again
    loads = [timed(lambda: mm.init(g)) for _ in range(3)]
    out["full_init_ms"] = {"median": statistics.median(loads), "all": loads, "bytes": N * D * 4}
    mm.top1(q)  # scratch, code objects

    def case(name, edit, undo):
        edit()  # warm-up of every kernel and buffer the case uses
        undo()
        ts, st = [], None
        for _ in range(a.repeat):
            before = mm.editStats()
            ts.append(timed(edit))
            st = stats_delta(before)
            undo()
            assert mm.m == N
        out["cases"][name] = {"median": statistics.median(ts), "min": min(ts), "max": max(ts), "edit_stats": st}
        print("%-28s median %9.3f ms  (min %9.3f  max %9.3f)  %s" % (name, statistics.median(ts), min(ts), max(ts), st), flush=True)

    for n in (1, 4, 128):
        case("add_%d_host" % n, lambda n=n: mm.galleryAdd(extra[:n]), lambda n=n: mm.galleryRemove(np.arange(N, N + n)))
        case("add_%d_dev" % n, lambda n=n: mm.galleryAddDev(extra_dev.data_ptr(), n), lambda n=n: mm.galleryRemove(np.arange(N, N + n)))
    # removes: the undo appends the removed rows again (the gallery keeps its size; its order changes, the cost does not depend on it)
    scattered = np.random.Generator(np.random.PCG64(1)).choice(N, 1000, replace=False)
    case("remove_1_near_end", lambda: mm.galleryRemove([N - 10]), lambda: mm.galleryAdd(extra[:1]))
    case("remove_1_at_0", lambda: mm.galleryRemove([0]), lambda: mm.galleryAdd(extra[:1]))
    case("remove_1000_scattered", lambda: mm.galleryRemove(scattered), lambda: mm.galleryAdd(extra[:1000]))
    i, s = mm.top1(q[1:2])
    out["sanity_top1_sim"] = float(s[0])
    out["scan_bytes"] = mm.scanBytes()
    print("full frt_matcher_init          median %9.3f ms  %s" % (out["full_init_ms"]["median"], ["%.1f" % t for t in loads]))
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    mm.close()


if __name__ == "__main__":
    main()
