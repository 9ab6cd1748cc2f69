"""Every planned conv launch of the recogniser, ALONE, against float64 (cases and reference: tests/arc_launch_ref.py; the program that runs
them: tests/cpp/arc_launch_check.cpp).  The network-level tests see these kernels through 48 launches, a 25088 -> 512 Linear and an L2
normalisation; here each selected line of tests/golden/arc_conv_plan.txt runs once per batch size on tensors of its own:
  * the planned label is the golden line's, and every label of the selected lines has run;
  * class A (exact inputs): out0 and out1 equal the reference bit for bit;
  * class B (realistic inputs): every element is inside the error bound derived in arc_launch_ref's docstring; max(err / bound) is printed;
  * no half outside an output's logical tensor has changed (the buffers have the embedder's sizes, with a margin in front).
The seven conv2_se lines with se=1 run as the twin instantiation with the whole SE tail in its epilogue (test_fused_se_launches_alone).
One harness process per unit shape, each under its own timeout.  A process that ends on a HIP error ends the module: the remaining
parameters fail with its message and launch nothing.
The batches here are the smallest that select each instantiation, and at those the three persistent kernels walk nothing: a workgroup of
conv64_kernel owns one strip, a wave of arc_input_mfma_kernel one tile, a workgroup of conv_s2c64_kernel one or two output rows.  Their walks -
what they carry from one work item to the next - are checked by tests/test_gpu_conv64_walk.py (conv64_kernel) and
tests/test_gpu_persistent_walks.py (the input layer and the 112 -> 56 conv), with this harness, these references and these bounds."""
import shutil

import numpy as np
import pytest

import arc_launch_ref as R
from launch_harness import Runner, build

_runner = Runner()
_ran = {}  # unit shape -> labels that ran and passed


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return build(tmp_path_factory.mktemp("arc_launch_check"), "arc_launch_check")


def _compare(case, want, outs, changed, label):
    """Failure messages of one case ([] = passed) and, for class B, max(err / bound)."""
    bad = []
    if label != case.label:
        bad.append("planned %s, the plan golden says %s" % (label, case.label))
    if changed:
        bad.append("%d halves outside the logical output changed" % changed)
    more, ratio = R.compare_outputs(case.cls, want, outs)
    bad += more
    return bad, ratio


@pytest.mark.gpu
@pytest.mark.parametrize("shape", range(len(R.SHAPES)), ids=["%d-%d_%dx%d_s%d" % (s[0], s[1], s[2], s[2], s[3]) for s in R.SHAPES])
def test_conv_launches_alone(shape, harness, tmp_path):
    _runner.require_running()
    cases = [c for c in R.cases() if c.shape == shape]
    work = tmp_path / "cases"
    work.mkdir()
    want = {}
    try:
        for c in cases:
            d = R.inputs(c)
            ref = R.reference(c, d, bound=c.cls == "B")
            if c.cls == "A":
                want[c.id] = R.exact_case(c, d, ref)
            else:
                want[c.id] = {k: (ref[k], ref["bound" + k[-1]]) for k in ("out0", "out1") if k in ref}
            R.write_case(str(work), c, d)
        R.write_manifest(str(work), cases)
        _runner.run(harness, work, R.SHAPES[shape], 300)
        failures, labels = [], set()
        for c in cases:
            got = R.read_outputs(str(work), c)
            if got is None:
                failures.append("%s: not reached" % c.id)
                continue
            bad, ratio = _compare(c, want[c.id], *got)
            if ratio is not None:
                print("%s %s: max(err / bound) = %.3f" % (c.id, c.label, ratio))
            failures += ["%s (%s): %s" % (c.id, c.label, b) for b in bad]
            if not bad:
                labels.add(got[2])
        _runner.require_ended_well()
        assert not failures, "%d of %d cases failed:\n%s" % (len({f.split(" ")[0] for f in failures}), len(cases), "\n".join(failures[:40]))
        _ran[shape] = labels
    finally:
        shutil.rmtree(str(work), ignore_errors=True)


@pytest.mark.gpu
def test_every_selected_plan_line_ran():
    """The labels that ran (and passed) are the labels of the selected plan lines: none left out, for any unit shape."""
    assert sorted(_ran) == list(range(len(R.SHAPES))), "the launch checks of some unit shapes did not pass (this test runs behind them)"
    for shape in range(len(R.SHAPES)):
        assert _ran[shape] == {ln.label for ln in R.plan_lines() if ln.shape == shape}


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["input", "fc", "se"])
def test_small_launches_alone(kind, harness, tmp_path):
    """launch_arc_input, launch_fc_slices + launch_fc_finalize and launch_se through the same harness (cases, references and bounds:
    arc_launch_ref, "the three small launches").  The SE gate's allowance for the device expf is measured, not derived: largest |gate - float64|
    seen on an MI355X 4.1e-7 (7x7x512, F = 3), allowed 4 x that = 1.64e-6 on top of the derived part."""
    _runner.require_running()
    cases = R.small_cases(kind)
    work = tmp_path / "cases"
    work.mkdir()
    try:
        inputs = {}
        for c in cases:
            inputs[c.id] = R.small_inputs(c)
            R.write_small(str(work), c, inputs[c.id])
        R.write_small_manifest(str(work), cases)
        _runner.run(harness, work, kind, 300)
        failures = []
        for c in cases:
            got = R.read_small_outputs(str(work), c)
            if got is None:
                failures.append("%s: not reached" % c.id)
                continue
            outs, changed, _ = got
            if changed:
                failures.append("%s: %d elements outside a logical output (or arrival counters) changed" % (c.id, changed))
            want = R.small_reference(c, inputs[c.id], gate_dev=outs.get("gate"))
            assert sorted(want) == sorted(outs)
            for k in sorted(want):
                ref, bound = want[k]
                if bound is None:
                    ne = outs[k] != ref.astype(outs[k].dtype)
                    if ne.any() or not np.array_equal(ref.astype(outs[k].dtype), ref):
                        failures.append("%s %s: %d of %d values differ from the exact reference" % (c.id, k, ne.sum(), ne.size))
                    continue
                err = np.abs(outs[k].astype(np.float64) - ref)
                live = bound > 0
                print("%s %s: max(err / bound) = %.3f, max err %.3g" % (c.id, k, (err[live] / bound[live]).max(), err.max()))
                if not (err <= bound).all():
                    i = tuple(int(v) for v in np.argwhere(~(err <= bound))[0])
                    failures.append("%s %s: %d values outside the bound, first at %s: %r, reference %r, bound %.3g" % (c.id, k, (~(err <= bound)).sum(), i, float(outs[k][i]), ref[i], bound[i]))
        _runner.require_ended_well()
        assert not failures, "\n".join(failures[:40])
    finally:
        shutil.rmtree(str(work), ignore_errors=True)


_ran_fused = {}  # unit shape -> (twin label, F) of the fused cases that ran and passed
FUSED_SHAPES = sorted({ln.shape for ln in R.fused_plan_lines()})


@pytest.mark.gpu
@pytest.mark.parametrize("shape", FUSED_SHAPES, ids=["%d-%d_%dx%d_s%d" % (R.SHAPES[s][:3] + R.SHAPES[s][2:]) for s in FUSED_SHAPES])
def test_fused_se_launches_alone(shape, harness, tmp_path):
    """conv2 with the whole SE tail in its epilogue (se_tail_epilogue, csrc/frt_se_device.h), built the way arc_unit_schedule builds it and launched
    alone (arc_launch_ref, "conv2 with the SE tail in its epilogue"): behind a primer launch with other tensors on the same scratch, class A bit
    for bit, class S inside its derived bound (max(err / bound) is printed), nothing outside the logical outputs, the partial sums, the counters
    and the flags written, every counter back at zero, every flag at the launch's epoch, and a third launch that writes the same bits."""
    _runner.require_running()
    cases = [c for c in R.fused_cases() if c.shape == shape]
    work = tmp_path / "cases"
    work.mkdir()
    want = {}
    try:
        for c in cases:
            d = R.fused_inputs(c)
            ref = R.fused_reference(c, d, bound=c.cls == "S")
            if c.cls == "A":
                want[c.id] = R.fused_exact(c, d, ref)
            else:
                R.fused_gate_condition(c, ref)
                want[c.id] = {k: (ref[k], ref["bound" + k[-1]]) for k in ("out0", "out1")}
            R.write_case(str(work), c, d)
        R.write_manifest(str(work), cases)
        _runner.run(harness, work, R.SHAPES[shape], 300)
        failures, passed = [], set()
        for c in cases:
            got = R.read_fused_outputs(str(work), c)
            if got is None:
                failures.append("%s: not reached" % c.id)
                continue
            bad = []
            if got.label != c.label:
                bad.append("ran %s, the twin of the plan golden's line is %s" % (got.label, c.label))
            if not got.fits:
                bad.append("conv_se_fits_device() is false on this device: the fused tail was not launched")
            if got.n_parts != R.fused_twin(c).n_parts:
                bad.append("%d strips per image, the derived bound assumes %d" % (got.n_parts, R.fused_twin(c).n_parts))
            for n, what in ((got.slack, "halves outside a logical output changed"), (got.outside, "scratch words outside the partial sums, counters and flags changed"),
                            (got.unwritten, "partial sums were not written"), (got.counters, "arrival counters are not back at zero"),
                            (got.flags, "flags are not at the launch's epoch"), (got.repeat, "halves differ between the second and the third launch")):
                if n:
                    bad.append("%d %s" % (n, what))
            more, ratio = R.compare_outputs(c.cls, want[c.id], got.outs)
            if ratio is not None:
                print("%s %s: max(err / bound) = %.3f" % (c.id, c.label, ratio))
            failures += ["%s (%s): %s" % (c.id, c.label, b) for b in bad + more]
            if not bad + more:
                passed.add((got.label, c.F))
        _runner.require_ended_well()
        assert not failures, "%d of %d cases failed:\n%s" % (len({f.split(" ")[0] for f in failures}), len(cases), "\n".join(failures[:40]))
        _ran_fused[shape] = passed
    finally:
        shutil.rmtree(str(work), ignore_errors=True)


@pytest.mark.gpu
def test_every_fused_plan_line_ran():
    """The twins that ran alone (and passed) are the labels a fused IR-SE pass shows and a stand-alone one does not (tests/golden/arc_conv_labels.json):
    four of them; and each of the seven se=1 plan lines ran at its first F and at first + 1."""
    import json
    import os
    assert sorted(_ran_fused) == FUSED_SHAPES, "the fused launch checks of some unit shapes did not pass (this test runs behind them)"
    seqs = json.load(open(os.path.join(R.ROOT, "tests", "golden", "arc_conv_labels.json")))
    only_fused = {l for k, v in seqs.items() if k.startswith("ir_se fused") for l in v} - {l for k, v in seqs.items() if k.startswith("ir_se standalone") for l in v}
    assert len(only_fused) == 4
    assert {label for ran in _ran_fused.values() for label, _ in ran} == only_fused
    lines = R.fused_plan_lines()
    assert len(lines) == 7
    for ln in lines:
        twin = R.FUSED[(ln.shape, ln.label)].label
        assert {(twin, ln.first), (twin, ln.first + 1)} <= _ran_fused[ln.shape], ln
