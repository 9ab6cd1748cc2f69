"""What building the template gallery costs, and what matching against it saves.

One 1M x 512 gallery with M = 4 rows per identity (rows of an identity 250 000 rows apart), fp32 and fp16 storage, one process.  Medians of
--repeat calls after a warm-up:
  kernel   template_build_kernel alone, device events around the launch (the library's profiling hooks, frt_profile_enable(2))
  call     frt_matcher_build_templates as a whole, audit only and with a destination: the call returns when its device work is complete,
           so this is host wall time - grouping on the host, uploads, the kernel, downloads, the ingest into the destination
  copy     a device-to-device copy of the kernel's byte count (N D (4 | 2) read + I D 4 written, halved: a copy reads and writes every
           byte it is given), device events, in the same run: the rate the kernel's rate is held against
  top1     128 queries against the row gallery and against the template gallery (device events around top1_dev)
Needs the GPU.  Run it under a time limit, one process:

    timeout 900 python tools/template_build_timing.py [--rows 1000000] [--per-identity 4] [--repeat 50] --out result.json
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
    ap.add_argument("--per-identity", type=int, default=4)
    ap.add_argument("--queries", type=int, default=128)
    ap.add_argument("--repeat", type=int, default=50)
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    import torch
    frt = entry.load_pkg()
    N, D, F, M = a.rows, 512, a.queries, a.per_identity
    I = (N + M - 1) // M
    g = frt.synth.make_gallery(N)
    labels = (np.arange(N) % I).astype(np.int32)
    q = frt.synth.make_queries(g, np.linspace(0, N - 1, F).astype(np.int64), noise=0.01)
    dq = torch.from_numpy(q).cuda()
    di = torch.zeros(F, dtype=torch.int32, device="cuda")
    ds = torch.zeros(F, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream

    def stats(ts):
        return {"median": statistics.median(ts), "min": min(ts), "max": max(ts)}

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
        return stats(ts)

    def wall_ms(fn):
        for _ in range(3):
            fn()
        ts = []
        for _ in range(a.repeat):
            t0 = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        return stats(ts)

    out = {"rows": N, "cols": D, "per_identity": M, "identities": I, "queries": F, "repeat": a.repeat, "unit": "ms", "cases": {}}

    def report(name, r):
        out["cases"][name] = r
        print("%-34s %s" % (name, json.dumps(r)), flush=True)

    src, dst = frt.MatMul(0), frt.MatMul(0)
    for fp16 in (False, True):
        tag = "fp16" if fp16 else "fp32"
        src.setStorage(fp16)
        src.init(g)
        src.setStorage(False)
        src.set_labels(labels)
        nbytes = N * D * (2 if fp16 else 4) + I * D * 4
        # the kernel alone: the library brackets the launch with events of its own
        for _ in range(3):
            src.buildTemplates()
        frt.profile_enable(2)
        for _ in range(a.repeat):
            src.buildTemplates()
        names, ms, _ = frt.profile_collect()
        frt.profile_enable(0)
        ks = [float(t) for n, t in zip(names, ms) if n == "template_build"]
        assert len(ks) == a.repeat, (len(ks), set(names))
        r = stats(ks)
        r.update(bytes=nbytes, TBps=nbytes / (r["median"] * 1e-3) / 1e12)
        report("kernel_" + tag, r)
        # a copy of the same byte count (half read, half written)
        a_, b_ = torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda"), torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda")
        r = device_ms(lambda: b_.copy_(a_))
        r.update(bytes=nbytes, TBps=nbytes / (r["median"] * 1e-3) / 1e12)
        report("copy_" + tag, r)
        del a_, b_
        out["cases"]["kernel_" + tag]["fraction_of_copy_rate"] = out["cases"]["kernel_" + tag]["TBps"] / r["TBps"]
        print("kernel_%s runs at %.2f of the copy's rate" % (tag, out["cases"]["kernel_" + tag]["fraction_of_copy_rate"]), flush=True)
        report("call_audit_only_" + tag, wall_ms(lambda: src.buildTemplates()))
        report("call_with_destination_" + tag, wall_ms(lambda: src.buildTemplates(dst)))
        if not fp16:
            for name, mm in (("top1_rows", src), ("top1_templates", dst)):
                r = device_ms(lambda: mm.top1_dev(dq.data_ptr(), F, di.data_ptr(), ds.data_ptr(), stream))
                r.update(gallery_rows=mm.m, scan_bytes=mm.scanBytes())
                report("%s_%s" % (name, tag), r)
            for name, mm in (("top1_rows_exact", src), ("top1_templates_exact", dst)):
                mm.setScreening(False)
                r = device_ms(lambda: mm.top1_dev(dq.data_ptr(), F, di.data_ptr(), ds.data_ptr(), stream))
                r.update(gallery_rows=mm.m, scan_bytes=mm.scanBytes())
                report("%s_%s" % (name, tag), r)
                mm.setScreening(True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    src.close()
    dst.close()


if __name__ == "__main__":
    main()
