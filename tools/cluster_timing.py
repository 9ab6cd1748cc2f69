"""What grouping a gallery into persons costs (frt_matcher_cluster), stage by stage, and what the cheapest loop over
the older entry points would cost.

Galleries, fp32 storage, 512 columns, threshold 0.5, one process:
  persons    --rows (1M) rows, --per-person (4) photos per person, the photos of a person rows / per-person apart: unit centre + 0.5 x unit
             noise, re-normalised (photos of a person near 0.8, strangers near 0)
  templates  --template-rows (250 000) rows of different persons (what frt_matcher_build_templates leaves: nothing to join)
Per gallery, once with the triangular walk (chunk c's coarse scan begins at tile c while 256 tiles are left: the product's walk) and once with
FRT_CLUSTER_FULL_WALK=1 in the environment (every chunk scans from tile 0; the library reads the variable at every call, for this tool):
  call       frt_matcher_cluster as a whole, host wall time (the call returns when its device work is complete); median of --repeat calls
             after one warm-up call, with the result's statistics
  stages     one more call under frt_profile_enable(3): device events around every chunk's coarse scan, selection, edge re-rank (and dense
             pass, if any chunk took it); the sum over the chunks per stage.  The events sit between the launches, so this call is a little
             slower than the untimed ones: the sums say which stage dominates, `call` says what a user waits for.
  floor      rows / 128 times one frt_matcher_top1_dev call with 128 stored rows as queries (device events, median over --floor-calls
             different chunks): the least any loop over the top-1 / top-k entry points pays before it stitches anything together.  With
             --old-lib this figure is taken from another build of the library (the commit before clustering existed), nothing else runs.
Needs the GPU.  Run it under a time limit, one process:

    timeout 900 python tools/cluster_timing.py --out result.json [--rows 1000000] [--template-rows 250000] [--old-lib path/to/libfrt.so]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np


def person_gallery(n, per_person, seed=3):
    rng = np.random.Generator(np.random.PCG64(seed))
    persons = (n + per_person - 1) // per_person
    centres = rng.standard_normal((persons, 512), dtype=np.float32)
    centres /= np.linalg.norm(centres, axis=1, keepdims=True)
    g = np.empty((n, 512), np.float32)
    for r0 in range(0, n, 65536):
        r1 = min(r0 + 65536, n)
        u = rng.standard_normal((r1 - r0, 512), dtype=np.float32)
        u *= 0.5 / np.linalg.norm(u, axis=1, keepdims=True)
        u += centres[np.arange(r0, r1) % persons]
        g[r0:r1] = u / np.linalg.norm(u, axis=1, keepdims=True)
    return g, persons


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--per-person", type=int, default=4)
    ap.add_argument("--template-rows", type=int, default=250_000)
    ap.add_argument("--threshold", type=float, default=0.5)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--floor-calls", type=int, default=40)
    ap.add_argument("--old-lib", default=None)
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    if a.old_lib:
        import types
        os.environ["FRT_LIB"] = os.path.abspath(a.old_lib)
        sys.modules["frt_amd_ab_old_library"] = types.ModuleType("frt_amd_ab_old_library")  # (the binding's import is strict otherwise)
    import torch
    import __graft_entry__ as entry
    frt = entry.load_pkg()
    out = {"threshold": a.threshold, "repeat": a.repeat, "unit": "ms", "library": a.old_lib or "this build", "cases": {}}

    def report(name, r):
        out["cases"][name] = r
        print("%-28s %s" % (name, json.dumps(r)), flush=True)

    def floor(mm, n, tag):
        di = torch.zeros(128, dtype=torch.int32, device="cuda")
        ds = torch.zeros(128, device="cuda")
        stream = torch.cuda.current_stream().cuda_stream
        ts = []
        for c in np.linspace(0, n // 128 - 1, a.floor_calls + 3).astype(np.int64):
            dq = torch.from_numpy(gallery[c * 128:(c + 1) * 128]).cuda()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            mm.top1_dev(dq.data_ptr(), 128, di.data_ptr(), ds.data_ptr(), stream)
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1))
        ts = ts[3:]  # (warm-up)
        calls = (n + 127) // 128
        report("floor_top1_loop_" + tag, {"per_call_median": statistics.median(ts), "per_call_min": min(ts), "per_call_max": max(ts), "calls": calls,
                                          "loop_total": statistics.median(ts) * calls})

    for tag, n, per in (("persons", a.rows, a.per_person), ("templates", a.template_rows, 1)):
        if n <= 0:
            continue
        gallery, persons = person_gallery(n, per)
        mm = frt.MatMul(0)
        mm.init(gallery)
        floor(mm, n, tag)
        for walk in (() if a.old_lib else ("triangular", "from_tile_0")):
            if walk == "from_tile_0":
                os.environ["FRT_CLUSTER_FULL_WALK"] = "1"
            else:
                os.environ.pop("FRT_CLUSTER_FULL_WALK", None)
            mm.cluster(a.threshold)
            ts, stats = [], None
            for _ in range(a.repeat):
                t0 = time.perf_counter()
                _, stats = mm.cluster(a.threshold)
                ts.append((time.perf_counter() - t0) * 1e3)
            r = {"rows": n, "persons": persons, "median": statistics.median(ts), "min": min(ts), "max": max(ts)}
            r.update(stats)
            report("call_%s_%s" % (tag, walk), r)
            frt.profile_enable(3)
            t0 = time.perf_counter()
            mm.cluster(a.threshold)
            wall = (time.perf_counter() - t0) * 1e3
            names, ms, _ = frt.profile_collect(cap=4 * ((n + 127) // 128) + 16)
            frt.profile_enable(0)
            r = {"call_under_events": wall}
            for k in sorted(set(names)):
                v = [float(t) for nm, t in zip(names, ms) if nm == k]
                r[k] = {"sum": sum(v), "chunks": len(v), "median": statistics.median(v)}
            report("stages_%s_%s" % (tag, walk), r)
        os.environ.pop("FRT_CLUSTER_FULL_WALK", None)
        mm.close()
        del gallery
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
