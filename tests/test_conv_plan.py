"""The recogniser's dispatch over its whole launch space, without a GPU: tests/cpp/conv_plan_dump.cpp (host code against libfrt.so's
conv_plan) must print tests/golden/arc_conv_plan.txt line for line.  The golden file was written by the same enumeration built against the
commit before conv_plan existed, asking that commit's three walks (conv_kernel_label, conv_small_applies || conv_s2_applies, conv_se_fused
with the per-device occupancy gate taken as passed): a kernel family or instantiation that moves, for any unit shape, launch description
or batch from 1 to 256, changes a line."""
import os
import subprocess

from conftest import ROOT
from launch_harness import build


def test_conv_plan_matches_the_recorded_dispatch(tmp_path):
    exe = build(tmp_path, "conv_plan_dump")
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    got = out.stdout.splitlines()
    want = open(os.path.join(ROOT, "tests", "golden", "arc_conv_plan.txt")).read().splitlines()
    assert len(want) > 100
    for g, w in zip(got, want):
        assert g == w
    assert len(got) == len(want)
