"""What one residual unit of the recogniser launches (arc_unit_schedule, csrc/frt_arc_launches.hpp - the function frt_embedder::forward()
runs per unit and frt_embedder::warm_strip_tables() walks), without a GPU.  tests/cpp/arc_schedule_dump.cpp prints it for the eight unit
shapes x network with / without SE x SE tail allowed in conv2's epilogue or not x batches 1 .. 256.  The expected launches are put together
here from tests/golden/arc_conv_plan.txt and the schedule rule, never from the code under test:

  conv1; then, without SE, conv2_scx alone where the golden says the plan consumes the fused shortcut, else shortcut1x1 (units that change
  the width) and conv2; with SE, shortcut1x1 (the same units), then conv2_se on its twin instantiation where the tail may be fused and the
  golden says the plan can carry it, else conv2_res and the stand-alone SE launches.

The twin's label is what conv_plan itself says about the conv2_se description (the dump's `twin` lines).  The strip geometries the scheduled
launches read tables of must be the ones tests/cpp/strip_tables_dump.cpp enumerates over the description space."""
import os
import re
import subprocess

import pytest

from conftest import ROOT
from launch_harness import build

BATCHES = range(1, 257)


def run_host_program(tmp, name):
    exe = build(tmp, name)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    return out.stdout.splitlines()


@pytest.fixture(scope="module")
def dumped(tmp_path_factory):
    """(sched, twin, geoms): {(shape, se, fuse): [launches at F = 1 .. 256]}, {shape: [se_label or None]}, the set of geometry tuples."""
    sched, twin, geoms = {}, {}, set()
    for line in run_host_program(tmp_path_factory.mktemp("arc_schedule"), "arc_schedule_dump"):
        if line.startswith("geom "):
            geoms.add(tuple(int(v) for v in line.split()[1:]))
            continue
        f = line.split("\t")
        if f[0] == "sched":
            per_f = sched.setdefault((f[1], int(f[2]), int(f[3])), [None] * 256)
            lo, hi, value = int(f[4]), int(f[5]), tuple(f[6:])
        else:
            assert f[0] == "twin" and len(f) == 5, line
            per_f = twin.setdefault(f[1], [None] * 256)
            lo, hi, value = int(f[2]), int(f[3]), f[4]
        assert 1 <= lo <= hi <= 256, line
        for F in range(lo, hi + 1):
            assert per_f[F - 1] is None, line  # ranges do not overlap
            per_f[F - 1] = value
    return sched, twin, geoms


@pytest.fixture(scope="module")
def golden():
    """{(shape, description): [(label, scx, se) at F = 1 .. 256]}"""
    plan = {}
    for line in open(os.path.join(ROOT, "tests", "golden", "arc_conv_plan.txt")).read().splitlines():
        m = re.fullmatch(r"(\d+->\d+ \d+x\d+ s\d) (\w+) F=(\d+)\.\.(\d+) (.+) scx=([01]) se=([01])", line)
        assert m, line
        per_f = plan.setdefault((m.group(1), m.group(2)), [None] * 256)
        for F in range(int(m.group(3)), int(m.group(4)) + 1):
            per_f[F - 1] = (m.group(5), int(m.group(6)), int(m.group(7)))
    assert all(None not in v for v in plan.values())
    return plan


def test_twin_labels_sit_where_the_golden_says_the_plan_can_carry_the_tail(dumped, golden):
    _, twin, _ = dumped
    shapes = {s for s, _ in golden}
    assert len(shapes) == 8
    for shape in shapes:
        for F in BATCHES:
            label, _, se = golden[(shape, "conv2_se")][F - 1]
            got = twin.get(shape, [None] * 256)[F - 1]
            assert (got is not None) == bool(se), (shape, F)
            assert got != label  # another instantiation


def test_schedule_is_the_rule_applied_to_the_recorded_plans(dumped, golden):
    sched, twin, _ = dumped
    shapes = sorted({s for s, _ in golden})
    assert len(sched) == 8 * 2 * 2
    for shape in shapes:
        cin, depth = (int(v) for v in re.match(r"(\d+)->(\d+)", shape).groups())

        def conv(desc, F, final=None):
            label = golden[(shape, desc)][F - 1][0]
            return "%s;%s;%d;%s" % (desc, label, final is not None, final if final is not None else label)

        for se in (0, 1):
            for fuse in (0, 1):
                for F in BATCHES:
                    want = [conv("conv1", F)]
                    scx = golden.get((shape, "conv2_scx"))
                    if not se and scx is not None and scx[F - 1][1]:
                        want.append(conv("conv2_scx", F))
                    else:
                        if cin != depth:
                            want.append(conv("shortcut1x1", F))
                        if not se:
                            want.append(conv("conv2", F))
                        elif fuse and golden[(shape, "conv2_se")][F - 1][2]:
                            want.append(conv("conv2_se", F, final=twin[shape][F - 1]))
                        else:
                            want += [conv("conv2_res", F), "launch_se"]
                    assert sched[(shape, se, fuse)][F - 1] == tuple(want), (shape, se, fuse, F)
    # the rule's branches are all taken somewhere
    seen = {launch.split(";")[0] for per_f in sched.values() for launches in per_f for launch in launches}
    assert seen == {"conv1", "conv2", "conv2_scx", "conv2_se", "conv2_res", "shortcut1x1", "launch_se"}


def test_scheduled_strip_geometries_are_the_enumerated_ones(dumped, tmp_path):
    _, _, geoms = dumped
    enumerated = {tuple(int(v) for v in line.split()[1:10]) for line in run_host_program(tmp_path, "strip_tables_dump") if line.startswith("geom ")}
    assert len(enumerated) >= 4
    assert geoms == enumerated  # every enumerated geometry is scheduled; every scheduled launch that reads a table has an enumerated one
