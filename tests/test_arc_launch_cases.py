"""The case list of the stand-alone conv launch check (tests/arc_launch_ref.py, tests/cpp/arc_launch_check.cpp), without a GPU: the list
covers every selected line of tests/golden/arc_conv_plan.txt, the harness compiles and plans for each case the instantiation the golden line
names, and every class A case keeps the premises under which its launch must be bit-equal to the float64 reference.  The same for the fused SE
conv2 launches (the se=1 lines), whose class S inputs must also keep the gates of neighbouring images apart, and whose comparison must fail
two deliberately wrong references."""
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


# ------------------------------------------------------------------------------------------------ conv2 with the SE tail in its epilogue
def test_fused_cases_cover_every_se_plan_line():
    lines = R.fused_plan_lines()
    cases = R.fused_cases()
    assert len(lines) == 7 and len({c.id for c in cases}) == len(cases) == 21
    assert sorted((ln.shape, ln.first) for ln in lines) == [(2, 23), (3, 56), (4, 23), (5, 56), (5, 112), (6, 96), (7, 111)]
    for ln in lines:
        twin = R.FUSED[(ln.shape, ln.label)].label
        mine = [c for c in cases if (c.shape, c.label) == (ln.shape, twin) and ln.first <= c.F <= ln.last]
        assert sorted(c.F for c in mine if c.cls == "A") == [ln.first, ln.first + 1], ln
        assert [c.F for c in mine if c.cls == "S"] == [ln.first + 1], ln
    assert len({c.label for c in cases}) == 4 and all(c.desc == "conv2_se" for c in cases)
    assert not {c.id for c in cases} & {c.id for c in R.cases()}


def test_harness_plans_the_four_twins_for_the_fused_cases(tmp_path):
    exe = R.build_harness(tmp_path)
    cases = R.fused_cases()
    R.write_manifest(str(tmp_path), cases)
    out = subprocess.run([exe, "--plan", str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    got = dict(line.split("\t") for line in out.stdout.splitlines())
    assert len(got) == len(cases)
    for c in cases:
        assert got[c.id] == c.label, c.id
    assert len(set(got.values())) == 4 and all(", true" in v for v in got.values())


@pytest.fixture(scope="module")
def class_s():
    """case id -> (case, inputs, reference with bounds) of the class S fused cases, computed once."""
    out = {}
    for c in R.fused_cases():
        if c.cls == "S":
            d = R.fused_inputs(c)
            out[c.id] = (c, d, R.fused_reference(c, d, bound=True))
    return out


def test_fused_class_a_cases_keep_their_exactness_premises():
    n = 0
    for c in R.fused_cases():
        if c.cls == "A":
            d = R.fused_inputs(c)
            R.fused_exact(c, d, R.fused_reference(c, d))
            assert set(np.unique(d["x"])) <= {-1.0, 0.0, 1.0} and set(np.unique(d["sc"])) <= {-1.0, 0.0, 1.0} and len(np.unique(d["p"][1])) == d["p"].shape[1]
            assert not np.array_equal(d["x0"], d["x"]) and not np.array_equal(d["sc0"], d["sc"])  # the primer launch has other tensors
            n += 1
    assert n == 14


def test_fused_class_s_gates_differ_between_the_images_of_a_pair(class_s):
    assert len(class_s) == 7
    for c, d, ref in class_s.values():
        worst, share = R.fused_gate_condition(c, ref)
        print("%s: largest gate bound %.2e, share of gate pairs more than 0.02 apart %.3f, %d roundings of res that may go either way" % (c.id, worst, share, ref["flipped"]))
        assert np.array_equal(ref["acc"], np.rint(ref["acc"])) and 0.5 < ref["res"].std() < 2  # integer accumulators, res is O(1)
        assert ref["flipped"] < ref["res"].size / 1000


def test_a_wrong_fused_reference_fails_the_comparison(class_s):
    """The comparison the GPU test makes tells a right tail from the two wrong ones the cosine tests cannot see: the fp16-rounded right reference
    passes its own bounds; it fails against a reference whose two images of a strip have swapped gates, and against one that divides the pooled
    sums by the pixels of a strip instead of the image's."""
    swapped = rescaled = 0
    for c, d, ref in class_s.values():
        outs = {k: ref[k].astype(np.float16) for k in ("out0", "out1")}
        want = lambda r: {k: (r[k], r["bound" + k[-1]]) for k in ("out0", "out1")}
        bad, ratio = R.compare_outputs("S", want(ref), outs)
        assert not bad and ratio <= 1
        t = R.fused_twin(c)
        g = R.geometry(c.shape, c.desc)
        if t.n_img == 2:
            bad, _ = R.compare_outputs("S", want(R.fused_reference(c, d, bound=True, acc=ref["acc"], swap_gates=True)), outs)
            assert len(bad) == 2, c.id
            swapped += 1
        strip_px = g.Ho * g.Ho * t.n_img // t.n_parts
        if strip_px != g.Ho * g.Ho:
            bad, _ = R.compare_outputs("S", want(R.fused_reference(c, d, bound=True, acc=ref["acc"], pool_hw=strip_px)), outs)
            assert len(bad) == 2, c.id
            rescaled += 1
    assert swapped == 2 and rescaled == 5
