"""Every launch of the recogniser's fp32 mode (frt_embedder::forward_f32, csrc/kernels_arc_f32.hip), ALONE, against float64 (cases and reference:
tests/arc_launch_ref.py, "the fp32 mode, launch by launch"; the program that runs them: tests/cpp/arc32_launch_check.cpp).  The mode is the
accuracy reference of the build, and the network-level tests see conv32_kernel through 52 launches, a 25088 -> 512 Linear and an L2
normalisation; here each description forward_f32 builds (csrc/frt_arc_launches.hpp, arc32_*) runs at each unit shape on tensors of its own:
  * class A (exact inputs): the fp32 output equals the reference bit for bit;
  * class B (realistic inputs): every element is inside the derived error bound; max(err / bound) is printed;
  * no float outside an output's logical tensor has changed (buffers of the embedder's sizes between two sentinel margins), and the inputs lie
    between NaNs.
One harness process per unit shape and one for the three small launches, each under its own timeout.  A process that ends on a HIP error, a
signal or the timeout ends the module: the remaining parameters fail with its message and launch nothing."""
import shutil

import pytest

import arc_launch_ref as R
from launch_harness import Runner, build

_runner = Runner()
_ran = set()   # (unit shape, description, F, class) of the conv cases that ran and passed


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return build(tmp_path_factory.mktemp("arc32_launch_check"), "arc32_launch_check")


@pytest.mark.gpu
@pytest.mark.parametrize("shape", range(len(R.SHAPES)), ids=["%d-%d_%dx%d_s%d" % (s[0], s[1], s[2], s[2], s[3]) for s in R.SHAPES])
def test_conv32_launches_alone(shape, harness, tmp_path):
    _runner.require_running()
    cases = [c for c in R.cases32() if c.shape == shape]
    work = tmp_path / "cases"
    work.mkdir()
    want = {}
    try:
        for c in cases:
            d = R.inputs32(c)
            ref = R.reference32(c, d, bound=c.cls == "B")
            want[c.id] = R.exact_case32(c, d, ref) if c.cls == "A" else {"out0": (ref["out0"], ref["bound0"])}
            R.write_case32(str(work), c, d)
        R.write_manifest32(str(work), cases)
        _runner.run(harness, work, R.SHAPES[shape], 300)
        failures, passed = [], set()
        for c in cases:
            got = R.read_outputs32(str(work), c)
            if got is None:
                failures.append("%s: not reached" % c.id)
                continue
            outs, changed, label = got
            bad = []
            if label != c.desc:
                bad.append("ran as %s" % label)
            if changed:
                bad.append("%d floats outside the logical output changed" % changed)
            more, ratio = R.compare_outputs(c.cls, want[c.id], outs)
            if ratio is not None:
                print("%s: max(err / bound) = %.4f" % (c.id, ratio))
            failures += ["%s: %s" % (c.id, b) for b in bad + more]
            if not bad + more:
                passed.add((c.shape, c.desc, c.F, c.cls))
        _runner.require_ended_well()
        assert not failures, "%d of %d cases failed:\n%s" % (len({f.split(":")[0] for f in failures}), len(cases), "\n".join(failures[:40]))
        _ran.update(passed)
    finally:
        shutil.rmtree(str(work), ignore_errors=True)


@pytest.mark.gpu
def test_every_listed_conv32_case_ran():
    """The (shape, description, F, class) that ran and passed are the ones listed: none left out, for any unit shape."""
    assert _ran == {(c.shape, c.desc, c.F, c.cls) for c in R.cases32()}, "some fp32 launch checks did not pass (this test runs behind them)"


@pytest.mark.gpu
def test_small_fp32_launches_alone(harness, tmp_path):
    """launch_arc32_input, launch_fc32 + launch_fc_finalize(splits = 1) and launch_se32 through the same harness, in one process (arc_launch_ref,
    "The three small fp32 launches").  The SE gate's allowance for the device expf, addition and division is measured, not derived:
    R.SE32_GATE_SEEN is the largest |gate - float64 gate| beyond the derived part seen on an MI355X, 4 x that is allowed.  Seen: nothing beyond it
    (largest error 1.18e-6, at least 2.1e-5 inside the derived part everywhere), so the allowance is 0."""
    _runner.require_running()
    cases = R.small_cases32()
    work = tmp_path / "cases"
    work.mkdir()
    try:
        inputs = {}
        for c in cases:
            inputs[c.id] = R.small_inputs32(c)
            R.write_small32(str(work), c, inputs[c.id])
        R.write_manifest32(str(work), [], cases)
        _runner.run(harness, work, "the small launches", 300)
        failures, beyond, raw = [], 0.0, 0.0
        for c in cases:
            got = R.read_small_outputs32(str(work), c)
            if got is None:
                failures.append("%s: not reached" % c.id)
                continue
            outs, changed, _ = got
            if changed:
                failures.append("%s: %d floats outside a logical output changed" % (c.id, changed))
            want = R.small_reference32(c, inputs[c.id], gate_dev=outs.get("gate"))
            assert sorted(k for k in want if k != "gate_derived") == sorted(outs)
            bad, ratios = R.compare_small32(c, want, outs)
            for k in sorted(ratios):
                print("%s %s: max(err / bound) = %.4f" % (c.id, k, ratios[k]))
            if "gate_derived" in want:
                ref, derived = want["gate_derived"]
                err = abs(outs["gate"].astype("float64") - ref)
                beyond, raw = max(beyond, float((err - derived).max())), max(raw, float(err.max()))
                print("%s gate: max |err| = %.3g, max(err - derived part) = %.3g" % (c.id, err.max(), (err - derived).max()))
            failures += ["%s %s" % (c.id, b) for b in bad]
        print("SE gates: largest |gate - float64 gate| %.3g, beyond the derived part %.3g (allowed %.3g)" % (raw, beyond, R.SE32_GATE_ALLOW))
        _runner.require_ended_well()
        assert not failures, "\n".join(failures[:40])
    finally:
        shutil.rmtree(str(work), ignore_errors=True)
