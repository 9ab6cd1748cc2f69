#!/usr/bin/env python3
"""Which kernel ran in each launch of tests/test_gpu_match_exact.py: one rocprofv3 kernel trace (no counters, no other tracing) of the harness
process of every group.  Needs a GPU and a built libfrt.so.

    python tools/match_exact_coverage.py [OUTDIR = profiles/match_exact]

Writes OUTDIR/kernels.txt: every match_kernel / match_reduce_kernel / merge_topk* symbol that ran, with the number of launches and the cases (and
launches) it ran in, then every such symbol compiled into libfrt.so (tools/codeobj_meta.py) that no case reached.  A trace's product kernels are
attributed in dispatch order: the op list says which launcher ran, match_exact_ref.kernel_launches() how many kernels it starts.  A harness process
that fails ends the run."""
import csv
import glob
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

import codeobj_meta  # noqa: E402
import launch_harness  # noqa: E402
import match_exact_ref as X  # noqa: E402
import match_stage_ref as R  # noqa: E402

FAMILY = re.compile(r"^(match_kernel|match_reduce_kernel|merge_topk\w*)(<|$)")


def normal(name):
    """a demangled kernel name without return type, namespace, arguments and blanks"""
    name = re.sub(r"\[clone.*$|\.kd$", "", name).strip()
    name = re.sub(r"^void |\(anonymous namespace\)::", "", name)
    depth = 0
    for i, c in enumerate(name):   # cut at the argument list: the first "(" outside the template arguments
        depth += (c == "<") - (c == ">")
        if c == "(" and depth == 0:
            name = name[:i]
            break
    return re.sub(r"\b(_Float16|half)\b", "half_t", name.replace(" ", ""))


def normal_names(names):
    """{name: normal() form} of mangled or demangled names.  A demangler (binutils', the profiler's) may not know DF16_ (_Float16) yet and leave
    the whole name mangled: it is handed the older Dh (half), which is no substitution candidate either, so the rest of the name is unchanged"""
    mangled = {n: n.replace("DF16_", "Dh") for n in names if n.startswith("_Z")}
    dm = codeobj_meta.demangle(sorted(set(mangled.values()))) if mangled else {}
    return {n: normal(dm[mangled[n]] if n in mangled else n) for n in names}


def compiled_family(lib):
    """the family's symbols in libfrt.so, in normal() form"""
    return sorted({n for n in normal_names(list(codeobj_meta.kernels(lib))).values() if FAMILY.match(n)})


def describe(tok):
    """one launch line of ops.txt -> (op, k, a short description)"""
    op, a = tok[0], tok[1:]
    if op == "top1":
        return op, 1, "top1 F=%s pb=%s off=%s" % (a[5], a[7], a[10])
    if op == "full":
        return op, 1, "full F=%s" % a[5]
    if op == "topk":
        return op, int(a[6]), "topk F=%s k=%s pb=%s off=%s" % (a[5], a[6], a[8], a[11])
    if op == "topk_labels":
        return op, int(a[6]), "topk_labels F=%s k=%s pb=%s off=%s" % (a[5], a[6], a[8], a[14])
    if op == "top1_excl":
        return op, 1, "top1_excl F=%s pb=%s" % (a[5], a[7])
    return op, 1, op


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "match_exact")
    os.makedirs(out, exist_ok=True)
    compiled = compiled_family(os.path.join(launch_harness.PKG, "libfrt.so"))
    tmp = tempfile.mkdtemp(prefix="match_exact_cov_")
    harness = launch_harness.build(tmp, "match_exact_check", opt="-O2")
    ran = {}   # symbol -> [(case, launch description)]
    for group, make in X.GROUPS.items():
        wd = os.path.join(tmp, group)
        os.makedirs(wd)
        ops = R.Ops(wd)
        make(ops)
        ops.write()
        prof = os.path.join(tmp, group + "_prof")
        run = subprocess.run(["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", prof, "--", harness, wd], capture_output=True, text=True, timeout=300)
        if run.returncode != 0:
            sys.exit("%s: exit status %d: %s" % (group, run.returncode, run.stderr.strip()[-800:]))
        traces = glob.glob(os.path.join(prof, "**", "*kernel_trace.csv"), recursive=True)
        assert len(traces) == 1, traces
        rows = sorted(csv.DictReader(open(traces[0])), key=lambda r: int(r["Start_Timestamp"]))
        names = normal_names({r["Kernel_Name"] for r in rows})
        kernels = [n for n in (names[r["Kernel_Name"]] for r in rows) if FAMILY.match(n)]
        cid, pos = None, 0
        for ln in ops.lines:
            tok = ln.split()
            if tok[0] == "case":
                cid = tok[1]
            elif tok[0] in ("top1", "full", "topk", "topk_labels", "top1_excl", "merge", "merge_labels"):
                op, k, what = describe(tok)
                n = X.kernel_launches(op, k)
                for name in kernels[pos:pos + n]:
                    ran.setdefault(name, []).append((cid, what))
                pos += n
        if pos != len(kernels):
            sys.exit("%s: the op list accounts for %d kernels, the trace holds %d of the family (names in the trace: %s)"
                     % (group, pos, len(kernels), ", ".join(sorted({r["Kernel_Name"] for r in rows})[:6])))
        print(group, len(kernels), "kernels", flush=True)
        for fn in glob.glob(os.path.join(wd, "*")):
            os.remove(fn)
    with open(os.path.join(out, "kernels.txt"), "w") as f:
        f.write("# %d symbols of the family compiled into libfrt.so, %d of them reached\n" % (len(compiled), len(set(ran) & set(compiled))))
        for name in sorted(ran):
            cases = {}
            for cid, what in ran[name]:
                cases.setdefault(cid, [])
                if what not in cases[cid] and what not in ("merge", "merge_labels"):
                    cases[cid].append(what)
            f.write("%s\t%d launches in %d cases\n" % (name, len(ran[name]), len(cases)))
            if name.startswith("merge_topk"):
                f.write("    %s\n" % ", ".join(sorted(cases)))
            else:
                for cid in sorted(cases):
                    f.write("    %s: %s\n" % (cid, "; ".join(cases[cid])))
        f.write("\n# compiled into libfrt.so, reached by no case:\n")
        for name in compiled:
            if name not in ran:
                f.write("%s\n" % name)
        f.write("\n# ran, but not found among the compiled symbols (names did not match):\n")
        for name in sorted(ran):
            if name not in compiled:
                f.write("%s\n" % name)


if __name__ == "__main__":
    main()
