"""What the leave-one-out genuine / impostor scores of a labelled gallery cost (frt_matcher_separation), stage by stage,
and what the loop a user could write before it existed would cost.

Galleries, fp32 storage, 512 columns, one process - those of tools/cluster_timing.py, labelled by person:
  persons    --rows (1M) rows, --per-person (4) photos per person, the photos of a person rows / per-person apart
  templates  --template-rows (250 000) rows of different persons (every row a person of its own: no genuine candidate anywhere)
Per gallery:
  call       frt_matcher_separation as a whole with 5 thresholds, host wall time (the call returns when its device work is complete); median
             of --repeat calls after one warm-up call, with the result's statistics
  stages     one more call under frt_profile_enable(3): device events around the genuine kernel, every chunk's coarse scan, selection and
             re-rank (or exact scan), and the reduction; the sum per stage.  The events sit between the launches, so this call is a little
             slower than the untimed ones: the sums say which stage dominates, `call` says what a user waits for.
  floor      rows / 128 times one frt_matcher_topk_labels_dev call with k = 2 and 128 stored rows as queries (device events, median over
             --floor-calls different chunks): what a loop over the gallery paid for the impostor side alone (entry 0 is the query's own
             person, entry 1 the best other one; nothing about the genuine side).  With --old-lib this figure is taken from another build
             of the library (the commit before the call existed), nothing else runs.
Needs the GPU.  Run it under a time limit, one process:

    timeout 900 python tools/separation_timing.py --out result.json [--rows 1000000] [--template-rows 250000] [--old-lib path/to/libfrt.so]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from cluster_timing import person_gallery

THRESHOLDS = np.array([0.2, 0.35, 0.5, 0.65, 0.8], np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--per-person", type=int, default=4)
    ap.add_argument("--template-rows", type=int, default=250_000)
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
    out = {"thresholds": THRESHOLDS.tolist(), "repeat": a.repeat, "unit": "ms", "library": a.old_lib or "this build", "cases": {}}

    def report(name, r):
        out["cases"][name] = r
        print("%-28s %s" % (name, json.dumps(r)), flush=True)

    def floor(mm, n, tag):
        dl = torch.zeros((128, 2), dtype=torch.int32, device="cuda")
        di = torch.zeros((128, 2), dtype=torch.int32, device="cuda")
        ds = torch.zeros((128, 2), device="cuda")
        stream = torch.cuda.current_stream().cuda_stream
        ts = []
        for c in np.linspace(0, n // 128 - 1, a.floor_calls + 3).astype(np.int64):
            dq = torch.from_numpy(gallery[c * 128:(c + 1) * 128]).cuda()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            mm.topk_labels_dev(dq.data_ptr(), 128, 2, dl.data_ptr(), di.data_ptr(), ds.data_ptr(), stream)
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1))
        ts = ts[3:]  # (warm-up)
        calls = (n + 127) // 128
        report("floor_topk_labels_loop_" + tag, {"per_call_median": statistics.median(ts), "per_call_min": min(ts), "per_call_max": max(ts), "calls": calls,
                                                 "loop_total": statistics.median(ts) * calls})

    for tag, n, per in (("persons", a.rows, a.per_person), ("templates", a.template_rows, 1)):
        if n <= 0:
            continue
        gallery, persons = person_gallery(n, per)
        mm = frt.MatMul(0)
        mm.init(gallery)
        mm.set_labels((np.arange(n) % persons).astype(np.int32))
        floor(mm, n, tag)
        if not a.old_lib:
            mm.separation(THRESHOLDS)
            ts, stats = [], None
            for _ in range(a.repeat):
                t0 = time.perf_counter()
                res = mm.separation(THRESHOLDS)
                ts.append((time.perf_counter() - t0) * 1e3)
                stats = res[5]
            r = {"rows": n, "persons": persons, "median": statistics.median(ts), "min": min(ts), "max": max(ts), "t_star": float(res[2].max()),
                 "counts": res[4].tolist()}
            r.update(stats)
            report("call_" + tag, r)
            frt.profile_enable(3)
            t0 = time.perf_counter()
            mm.separation(THRESHOLDS)
            wall = (time.perf_counter() - t0) * 1e3
            names, ms, _ = frt.profile_collect(cap=4 * ((n + 127) // 128) + 16)
            frt.profile_enable(0)
            r = {"call_under_events": wall}
            for k in sorted(set(names)):
                v = [float(t) for nm, t in zip(names, ms) if nm == k]
                r[k] = {"sum": sum(v), "brackets": len(v), "median": statistics.median(v)}
            report("stages_" + tag, r)
        mm.close()
        del gallery
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
