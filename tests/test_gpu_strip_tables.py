"""The strip kernels' table path at the batches where a table index wraps or the last strip is ragged: single conv launches through the
stand-alone per-launch checker (tests/cpp/arc_launch_check.cpp, cases and float64 reference: tests/arc_launch_ref.py), class A exact
inputs - out0 and out1 must equal float64 bit for bit - on buffers with guard patterns around every tensor.

  14x14x256 compact strips (7 strips = 8 images), conv1 and conv2:  F = 112 (whole periods), 113 (one image into a new period, last strip
      partial), 120 / 121 (period boundary), 128
  7x7x512 compact strips (49 strips = 128 images), conv1 and conv2:  F = 112, 113, 128 (exactly one period), 129 (wrap)
  28x28x128 (conv1, conv2) and 56x56 64 -> 128 (conv1) padded strips:  the first batch of every plan line's range and first + 1 (ragged last
      strip of an image, every instantiation of the family)
One process runs F = 128 and then F = 113 on the same geometry: the table cached by the first launch serves the second, so it cannot depend on
the batch.  One harness process per group, each under its own timeout; a process that ends on an error ends the module."""
import shutil

import numpy as np
import pytest

import arc_launch_ref as R
from launch_harness import Runner, build

_runner = Runner()


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return build(tmp_path_factory.mktemp("strip_table_check"), "arc_launch_check")


def _label(shape, desc, F):
    (ln,) = [ln for ln in R.plan_lines() if ln.shape == shape and ln.desc == desc and ln.first <= F <= ln.last]
    return ln.label


def _case(shape, desc, F):
    return R.Case("t%d_%s_F%d_A" % (shape, desc, F), shape, desc, F, "A", _label(shape, desc, F))


def _padded_cases(shape, descs):
    out = []
    for ln in R.plan_lines():
        if ln.shape == shape and ln.desc in descs and ln.label.startswith("conv_patch_kernel"):
            out += [_case(shape, ln.desc, F) for F in (ln.first, ln.first + 1) if F <= ln.last]
    return out


GROUPS = {
    "14x14x256_compact": [_case(5, d, F) for d in ("conv1", "conv2") for F in (112, 113, 120, 121, 128)],
    "7x7x512_compact": [_case(7, d, F) for d in ("conv1", "conv2") for F in (112, 113, 128, 129)],
    "28x28x128_padded": _padded_cases(3, ("conv1", "conv2")),
    "56x56_64to128_padded": _padded_cases(2, ("conv1",)),
    "one_process_F128_then_F113": [_case(5, "conv1", 128), _case(5, "conv1", 113)],
}


def test_the_groups_select_the_strip_kernels():
    """(no GPU) the batches above are planned onto the kernels this file is about"""
    assert {c.label for c in GROUPS["14x14x256_compact"]} == {"conv_patchc_kernel<7>"}
    assert {c.label for c in GROUPS["7x7x512_compact"]} == {"conv_patchc_kernel<4>"}
    assert len({c.label for c in GROUPS["28x28x128_padded"]}) == 4 and len(GROUPS["28x28x128_padded"]) == 16
    assert {c.label for c in GROUPS["56x56_64to128_padded"]} == {"conv_patch_kernel<3, 5, 5, true, false, 7, 1, 3, false>"}


@pytest.mark.gpu
@pytest.mark.parametrize("group", list(GROUPS))
def test_strip_launches_at_table_boundaries(group, harness, tmp_path):
    _runner.require_running()
    cases = GROUPS[group]
    work = tmp_path / "cases"
    work.mkdir()
    want = {}
    try:
        for c in cases:
            d = R.inputs(c)
            want[c.id] = R.exact_case(c, d, R.reference(c, d))
            R.write_case(str(work), c, d)
        R.write_manifest(str(work), cases)  # (the harness runs the cases in this order, in one process)
        _runner.run(harness, work, group, 300)
        failures = []
        for c in cases:
            got = R.read_outputs(str(work), c)
            if got is None:
                failures.append("%s: not reached" % c.id)
                continue
            outs, changed, label = got
            if label != c.label:
                failures.append("%s: planned %s, the plan golden says %s" % (c.id, label, c.label))
            if changed:
                failures.append("%s: %d halves outside the logical output changed" % (c.id, changed))
            if sorted(outs) != sorted(want[c.id]):
                failures.append("%s: outputs %s, expected %s" % (c.id, sorted(outs), sorted(want[c.id])))
                continue
            for k in sorted(want[c.id]):
                ne = outs[k].view(np.uint16) != want[c.id][k].view(np.uint16)
                if ne.any():
                    i = tuple(int(v) for v in np.argwhere(ne)[0])
                    failures.append("%s %s: %d of %d values differ, first at [f, oh, ow, c] = %s: %r, reference %r" %
                                    (c.id, k, ne.sum(), ne.size, i, float(outs[k][i]), float(want[c.id][k][i])))
        _runner.require_ended_well()
        assert not failures, "%d failures:\n%s" % (len(failures), "\n".join(failures[:40]))
    finally:
        shutil.rmtree(str(work), ignore_errors=True)
