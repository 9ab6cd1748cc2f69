"""Every planned conv launch of the recogniser, ALONE, against float64 (cases and reference: tests/arc_launch_ref.py; the program that runs
them: tests/cpp/arc_launch_check.cpp).  The network-level tests see these kernels through 48 launches, a 25088 -> 512 Linear and an L2
normalisation; here each selected line of tests/golden/arc_conv_plan.txt runs once per batch size on tensors of its own:
  * the planned label is the golden line's, and every label of the selected lines has run;
  * class A (exact inputs): out0 and out1 equal the reference bit for bit;
  * class B (realistic inputs): every element is inside the error bound derived in arc_launch_ref's docstring; max(err / bound) is printed;
  * no half outside an output's logical tensor has changed (the buffers have the embedder's sizes, with a margin in front).
One harness process per unit shape, each under its own timeout.  A process that ends on a HIP error ends the module: the remaining
parameters fail with its message and launch nothing."""
import shutil
import subprocess

import numpy as np
import pytest

import arc_launch_ref as R

_stopped = []  # the message of the harness process that ended on an error
_ran = {}      # unit shape -> labels that ran and passed


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return R.build_harness(tmp_path_factory.mktemp("arc_launch_check"))


def _compare(case, want, outs, changed, label):
    """Failure messages of one case ([] = passed) and, for class B, max(err / bound)."""
    bad, ratio = [], None
    if label != case.label:
        bad.append("planned %s, the plan golden says %s" % (label, case.label))
    if changed:
        bad.append("%d halves outside the logical output changed" % changed)
    for k in sorted(want):
        if k not in outs:
            bad.append("%s was not written" % k)
        elif case.cls == "A":
            ne = outs[k].view(np.uint16) != want[k].view(np.uint16)
            if ne.any():
                i = tuple(int(v) for v in np.argwhere(ne)[0])
                bad.append("%s: %d of %d values differ, first at [f, oh, ow, c] = %s: %r, reference %r" % (k, ne.sum(), ne.size, i, float(outs[k][i]), float(want[k][i])))
        else:
            ref, bound = want[k]
            err = np.abs(outs[k].astype(np.float64) - ref)
            ratio = max(ratio or 0.0, float((err / bound).max()))
            if not (err <= bound).all():  # (also catches a NaN)
                i = tuple(int(v) for v in np.argwhere(~(err <= bound))[0])
                bad.append("%s: %d values outside the bound, first at %s: %r, reference %r, bound %.3g" % (k, (~(err <= bound)).sum(), i, float(outs[k][i]), ref[i], bound[i]))
    if set(outs) - set(want):
        bad.append("unexpected outputs %s" % sorted(set(outs) - set(want)))
    return bad, ratio


@pytest.mark.gpu
@pytest.mark.parametrize("shape", range(len(R.SHAPES)), ids=["%d-%d_%dx%d_s%d" % (s[0], s[1], s[2], s[2], s[3]) for s in R.SHAPES])
def test_conv_launches_alone(shape, harness, tmp_path):
    assert not _stopped, "not run: an earlier harness process ended on an error: " + _stopped[0]
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
        try:
            run = subprocess.run([harness, str(work)], capture_output=True, text=True, timeout=300)
            if run.returncode != 0:
                _stopped.append("%s: exit status %d: %s" % (R.SHAPES[shape], run.returncode, run.stderr.strip()[-500:]))
        except subprocess.TimeoutExpired:
            _stopped.append("%s: no end after 300 s" % (R.SHAPES[shape],))
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
        assert not _stopped, _stopped[0]
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
    assert not _stopped, "not run: an earlier harness process ended on an error: " + _stopped[0]
    cases = R.small_cases(kind)
    work = tmp_path / "cases"
    work.mkdir()
    try:
        inputs = {}
        for c in cases:
            inputs[c.id] = R.small_inputs(c)
            R.write_small(str(work), c, inputs[c.id])
        R.write_small_manifest(str(work), cases)
        try:
            run = subprocess.run([harness, str(work)], capture_output=True, text=True, timeout=300)
            if run.returncode != 0:
                _stopped.append("%s: exit status %d: %s" % (kind, run.returncode, run.stderr.strip()[-500:]))
        except subprocess.TimeoutExpired:
            _stopped.append("%s: no end after 300 s" % kind)
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
        assert not _stopped, _stopped[0]
        assert not failures, "\n".join(failures[:40])
    finally:
        shutil.rmtree(str(work), ignore_errors=True)
