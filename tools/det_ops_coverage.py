#!/usr/bin/env python3
"""Which kernel ran each detector op in each case of tests/test_gpu_det_ops.py: one rocprofv3 kernel trace (no counters) of the harness
process per (blob, geometry, batch).  Needs a GPU and a built libfrt.so.

    python tools/det_ops_coverage.py [OUTDIR = profiles/det_ops]

Writes OUTDIR/<case>.txt ("<step>\t<kernel symbols>", the steps of the harness's results.txt: op0 .. op22, the range-edge runs, u8conv, u8stem)
and OUTDIR/kernels.txt: every distinct detector kernel symbol that ran with the cases it ran in, then every __global__ of csrc/kernels_det*.hip
that no case reached.  The steps are told apart by the fills the harness issues before each of them (runtime kernels, named *rocclr*).  A harness
process that fails ends the run."""
import csv
import glob
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import launch_harness  # noqa: E402
import test_gpu_det_ops as T  # noqa: E402
from conftest import load_pkg  # noqa: E402


def steps_of(trace_csv):
    """The product kernels of a trace in dispatch order, cut into steps at the runtime's fill / copy kernels."""
    rows = sorted(csv.DictReader(open(trace_csv)), key=lambda r: int(r["Start_Timestamp"]))
    steps, cur = [], None
    for r in rows:
        name = r["Kernel_Name"]
        if "rocclr" in name:
            if cur:
                steps.append(cur)
            cur = []
        elif cur is not None:
            cur.append(re.sub(r"^void |\(anonymous namespace\)::|\(.*\)$|\[clone.*$|\.kd$", "", name).strip())
    if cur:
        steps.append(cur)
    return [s for s in steps if s]


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "det_ops")
    os.makedirs(out, exist_ok=True)
    frt = load_pkg()
    tmp = tempfile.mkdtemp(prefix="det_ops_cov_")
    harness = launch_harness.build(tmp, "det_op_check", opt="-O2")
    blobs = {}

    def blob(kind):
        if kind not in blobs:
            sd = frt.synth.retinaface_state(1, landmarks=kind == "det_ldm")
            blobs[kind] = (frt.write_weights(os.path.join(tmp, kind + ".frtw"), sd, frt.weights_io.KIND_RETINAFACE_MNET025), sd)
        return blobs[kind]

    class Tmp:  # (stands in for pytest's tmp_path_factory)
        def mktemp(self, name):
            import pathlib
            return pathlib.Path(tempfile.mkdtemp(prefix=name, dir=tmp))

    def prepare_slim(wd, rfb, B):
        path, _, ops = T._slim_reference(frt, frt.synth, Tmp(), rfb)
        T.prepare_slim(wd, path, ops, B)

    jobs = [("%s-%s-B%d" % c[:3], lambda wd, c=c: T.prepare(wd, blob(c[0])[0], T._reference(frt.synth, blob, c[0], c[1]), c[1], c[2], c[3], c[4])) for c in T.CASES]
    jobs += [("%s-100x172-B%d" % ("rfb" if r else "slim", b), lambda wd, r=r, b=b: prepare_slim(wd, r, b)) for r, b in T.SLIM_CASES]
    ran = {}
    for cid, prep in jobs:
        wd = os.path.join(tmp, cid)
        os.makedirs(wd)
        prep(wd)
        prof = os.path.join(tmp, cid + "_prof")
        run = subprocess.run(["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", prof, "--", harness, wd], capture_output=True, text=True, timeout=300)
        if run.returncode != 0:
            sys.exit("%s: exit status %d: %s" % (cid, run.returncode, run.stderr.strip()[-800:]))
        traces = glob.glob(os.path.join(prof, "**", "*kernel_trace.csv"), recursive=True)
        assert len(traces) == 1, traces
        steps = steps_of(traces[0])
        names = [ln.split("\t")[0] for ln in open(os.path.join(wd, "results.txt")).read().splitlines() if not ln.endswith("n/a")]
        with open(os.path.join(out, cid + ".txt"), "w") as f:
            if len(steps) != len(names):
                f.write("# %d steps in the trace, %d in results.txt: not matched\n" % (len(steps), len(names)))
                names = ["step%d" % i for i in range(len(steps))]
            for n, s in zip(names, steps):
                f.write("%s\t%s\n" % (n, " + ".join(s)))
                for k in s:
                    ran.setdefault(k, []).append("%s:%s" % (cid, n))
        print(cid, len(steps), "steps", flush=True)
        for fn in glob.glob(os.path.join(wd, "*")):
            os.remove(fn)
    src = ""
    for fn in sorted(glob.glob(os.path.join(ROOT, "face-recognition-cpp-tensorrt_amd", "csrc", "kernels_det*.hip"))):
        src += open(fn).read()
    globals_ = sorted(set(re.findall(r"__global__[^;{]*?void\s+(\w+)\s*\(", src)))
    with open(os.path.join(out, "kernels.txt"), "w") as f:
        for k in sorted(ran):
            cases = sorted({c.split(":")[0] for c in ran[k]})
            f.write("%s\t%d launches in %s\n" % (k, len(ran[k]), ", ".join(cases)))
        f.write("\n# __global__ functions of kernels_det*.hip with no instantiation in any case:\n")
        for g in globals_:
            if not any(re.match(r"%s(<|$)" % g, k) for k in ran):
                f.write("%s\n" % g)


if __name__ == "__main__":
    main()
