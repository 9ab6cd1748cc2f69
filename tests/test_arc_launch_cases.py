"""The case list of the stand-alone conv launch check (tests/arc_launch_ref.py, tests/cpp/arc_launch_check.cpp), without a GPU: the list
covers every selected line of tests/golden/arc_conv_plan.txt, the harness compiles and plans for each case the instantiation the golden line
names, and every class A case keeps the premises under which its launch must be bit-equal to the float64 reference."""
import subprocess

import numpy as np
import pytest

import arc_launch_ref as R


def test_cases_cover_every_selected_plan_line():
    lines = R.plan_lines()
    cases = R.cases()
    assert len(lines) == 89  # 114 lines less the 25 conv2_se ones
    assert len({c.id for c in cases}) == len(cases)
    a = [c for c in cases if c.cls == "A"]
    for ln in lines:
        fs = sorted(c.F for c in a if (c.shape, c.desc, c.label) == (ln.shape, ln.desc, ln.label) and ln.first <= c.F <= ln.last)
        assert fs == [ln.first] + ([ln.first + 1] if ln.last > ln.first else []), ln
    assert len(a) == sum(1 + (ln.last > ln.first) for ln in lines)  # and nothing above the first F + 1 of a range
    assert {c.label for c in cases} == {ln.label for ln in lines}
    b = [c for c in cases if c.cls == "B"]
    assert {(c.label, c.desc) for c in b} == {(ln.label, ln.desc) for ln in lines} and len(b) == len({(c.label, c.desc) for c in b})


def test_harness_plans_the_golden_label_for_every_case(tmp_path):
    exe = R.build_harness(tmp_path)
    cases = R.cases()
    R.write_manifest(str(tmp_path), cases)
    out = subprocess.run([exe, "--plan", str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    got = dict(line.split("\t") for line in out.stdout.splitlines())
    assert len(got) == len(cases)
    for c in cases:
        assert got[c.id] == c.label, c.id


@pytest.mark.parametrize("shape", range(len(R.SHAPES)), ids=["%d-%d_%dx%d_s%d" % (s[0], s[1], s[2], s[2], s[3]) for s in R.SHAPES])
def test_class_a_cases_are_exact_in_fp16(shape):
    n = 0
    for c in R.cases():
        if c.shape != shape or c.cls != "A":
            continue
        d = R.inputs(c)
        ref = R.reference(c, d)
        R.exact_case(c, d, ref)
        # the inputs are what the docstring says they are: a quarter of x and w non-zero, distinct biases
        assert set(np.unique(d["x"])) <= {-1.0, 0.0, 1.0} and 0.2 < np.count_nonzero(d["w"]) / d["w"].size < 0.3
        if R.geometry(c.shape, c.desc).mode != "prelu":
            assert len(np.unique(d["p"][1])) == d["p"].shape[1]
        n += 1
    assert n >= 8


def test_small_launch_cases_keep_their_exactness_premises():
    """Output Linear: every slice sum is an integer fp32 holds; SE tail with w2 = 0: gate 1/2, y and z fp16-exact (asserted by the reference)."""
    for c in R.small_cases("fc")[:2]:
        d = R.small_inputs(c)
        parts, bound = R.small_reference(c, d)["out1"]
        assert bound is None and np.array_equal(parts, np.rint(parts)) and np.abs(parts).max() <= 512
        assert (d["valid"] == 0).sum() == (c.F > 1)
    for c in R.small_cases("se"):
        if c.cls == "A" and c.F == 1:
            ref = R.small_reference(c, R.small_inputs(c))
            assert all(ref[k][1] is None for k in ("gate", "out0", "out1"))
