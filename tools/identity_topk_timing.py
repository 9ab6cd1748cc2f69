"""What the k best IDENTITIES cost beside the row search plus a host dedupe.

One 1M x 512 fp32 gallery, 128 queries, one process.  Timed on the device with events around the `_dev` calls (queries and outputs
resident), medians of --repeat calls after a warm-up:
  topk_labels  k = 4, M = 1 and 4   (M = rows per label; (k - 1) M + 1 <= 16: one screened search)
  topk_labels  k = 4, M = 8         ((k - 1) M + 1 = 25: k exact scans)
  topk         k = 4 and k = 16     (the row search a caller over-asks today) + the host dedupe of its lists (download + first-of-each-label)
and, for every (k, M), whether 16 rows - the most the row search returns - can hold k identities at all: only when (k - 1) M + 1 <= 16.
Needs the GPU.  Run it under a time limit, one process:

    timeout 600 python tools/identity_topk_timing.py [--rows 1000000] [--queries 128] [--repeat 20] --out result.json
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


def host_dedupe(idx, sim, labels, k):
    """what a caller of the row search does today: walk every list, keep the first row of every label"""
    out = []
    for q in range(idx.shape[0]):
        seen, keep = set(), []
        for i, s in zip(idx[q], sim[q]):
            l = int(labels[i]) if i >= 0 else -1
            if l < 0 or l in seen:
                continue
            seen.add(l)
            keep.append((l, int(i), float(s)))
            if len(keep) == k:
                break
        out.append(keep)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--queries", type=int, default=128)
    ap.add_argument("--repeat", type=int, default=20)
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    import torch
    frt = entry.load_pkg()
    N, D, F = a.rows, 512, a.queries
    g = frt.synth.make_gallery(N)
    q = frt.synth.make_queries(g, np.linspace(0, N - 1, F).astype(np.int64), noise=0.01)
    dq = torch.from_numpy(q).cuda()
    dl = torch.zeros(F, 16, dtype=torch.int32, device="cuda")
    di = torch.zeros(F, 16, dtype=torch.int32, device="cuda")
    ds = torch.zeros(F, 16, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    mm = frt.MatMul(0)
    mm.init(g)

    def device_ms(fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(a.repeat):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1))
        return {"median": statistics.median(ts), "min": min(ts), "max": max(ts)}

    out = {"rows": N, "cols": D, "queries": F, "repeat": a.repeat, "unit": "ms", "cases": {}}

    def report(name, r):
        out["cases"][name] = r
        print("%-34s %s" % (name, json.dumps(r)), flush=True)

    for k, m in ((4, 1), (4, 4), (4, 8)):
        labels = (np.arange(N) % ((N + m - 1) // m)).astype(np.int32)
        mm.set_labels(labels)
        n_id, m_max = mm.labels_info()
        r = device_ms(lambda: mm.topk_labels_dev(dq.data_ptr(), F, k, dl.data_ptr(), di.data_ptr(), ds.data_ptr(), stream))
        r.update(k=k, M=m_max, identities=n_id, screened=(k - 1) * m_max + 1 <= 16)
        report("topk_labels_k%d_M%d" % (k, m), r)
    mm.set_labels(None)
    labels4 = (np.arange(N) % ((N + 3) // 4)).astype(np.int32)
    for k in (4, 16):
        r = device_ms(lambda: mm.topk_dev(dq.data_ptr(), F, k, di.data_ptr(), ds.data_ptr(), stream))
        hs = []
        for _ in range(5):
            t0 = time.perf_counter()
            hi = di.view(-1)[:F * k].view(F, k).cpu().numpy()  # (the call wrote [F][k] contiguously)
            hv = ds.view(-1)[:F * k].view(F, k).cpu().numpy()
            host_dedupe(hi, hv, labels4, 4)
            hs.append((time.perf_counter() - t0) * 1e3)
        r.update(k=k, host_download_and_dedupe_ms=statistics.median(hs))
        report("topk_rows_k%d" % k, r)
    # where over-asking cannot work whatever it costs: 16 rows hold k identities for certain only if (k - 1) M + 1 <= 16
    out["row_search_cannot_guarantee"] = [[k, m] for k in range(2, 17) for m in (1, 2, 4, 8, 16) if (k - 1) * m + 1 > 16]
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    mm.close()


if __name__ == "__main__":
    main()
