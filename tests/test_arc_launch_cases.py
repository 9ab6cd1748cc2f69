"""The case list of the stand-alone conv launch check (tests/arc_launch_ref.py, tests/cpp/arc_launch_check.cpp), without a GPU: the list
covers every selected line of tests/golden/arc_conv_plan.txt, the harness compiles and plans for each case the instantiation the golden line
names, and every class A case keeps the premises under which its launch must be bit-equal to the float64 reference.  The same for the fused SE
conv2 launches (the se=1 lines), whose class S inputs must also keep the gates of neighbouring images apart, and whose comparison must fail
two deliberately wrong references."""
import subprocess

import numpy as np
import pytest

import arc_launch_ref as R
from launch_harness import build


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
    exe = build(tmp_path, "arc_launch_check")
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
    exe = build(tmp_path, "arc_launch_check")
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


# ------------------------------------------------------------------------------------------------ the fp32 mode, launch by launch
def test_fp32_cases_cover_every_description_of_every_unit_shape():
    cases = R.cases32()
    assert len({c.id for c in cases}) == len(cases)
    assert not {c.id for c in cases} & ({c.id for c in R.cases()} | {c.id for c in R.fused_cases()})
    n = 0
    for shape, (cin, depth, h, stride) in enumerate(R.SHAPES):
        descs = ["conv1", "conv2", "conv2_res"] + (["shortcut1x1"] if cin != depth else [])
        assert sorted(R.descs32(shape)) == sorted(descs)
        fs = [1, 2, 8] if h in (14, 7) else [1, 2]
        for desc in descs:
            mine = [c for c in cases if (c.shape, c.desc) == (shape, desc)]
            assert sorted(c.F for c in mine if c.cls == "A") == fs and [c.F for c in mine if c.cls == "B"] == [2], (shape, desc)
            n += len(mine)
            g = R.geometry32(shape, desc)
            if h in (28, 14, 7):  # M % 32 != 0 at some F: a tile straddles two faces, the last one is ragged
                assert any(c.F * g.Ho * g.Ho % 32 for c in mine), (shape, desc)
            if 8 in fs and g.Ho == 7:  # the mode's chunk leaves a tail of 8 pixels wherever the output is 7x7
                assert 8 * g.Ho * g.Ho % 32 == 8
    assert n == len(cases) == 91
    # the block counts the kernel's ring and wave split can go wrong at are among the cases
    nb = {(R.geometry32(c.shape, c.desc).ks ** 2 * R.geometry32(c.shape, c.desc).Cin // 32, R.geometry32(c.shape, c.desc).pro) for c in cases}
    assert (18, True) in nb and (18, False) in nb and (2, False) in nb  # NB % 4 == 2; NI = 5 against the 6-step unroll of the ring of 3; NB = 2 < 4 waves
    small = R.small_cases32()
    assert len({c.id for c in small}) == len(small) == 6 + 3 + 16


def test_fp32_harness_describes_every_case_as_the_reference_does(tmp_path):
    """The harness compiles here, and the Conv32Args the product's descriptions (csrc/frt_arc_launches.hpp, the text forward_f32 compiles) give for
    each case are the geometry the float64 reference restates."""
    exe = build(tmp_path, "arc32_launch_check")
    cases = R.cases32()
    R.write_manifest32(str(tmp_path), cases, R.small_cases32())
    out = subprocess.run([exe, "--describe", str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    got = dict(line.split("\t") for line in out.stdout.splitlines())
    assert len(got) == len(cases)
    for c in cases:
        assert got[c.id] == R.describe32_line(c), c.id


@pytest.fixture(scope="module")
def fp32_refs():
    """case id -> (case, inputs, reference) of the fp32 conv cases the wrong-reference tests use, computed once."""
    out = {}
    for c in R.cases32():
        if (c.shape, c.desc, c.F) in ((0, "conv2", 2), (4, "shortcut1x1", 2), (7, "conv1", 2), (6, "conv1", 8)):
            d = R.inputs32(c)
            out[c.id] = (c, d, R.reference32(c, d, bound=c.cls == "B"))
    return out


@pytest.mark.parametrize("shape", range(len(R.SHAPES)), ids=["%d-%d_%dx%d_s%d" % (s[0], s[1], s[2], s[2], s[3]) for s in R.SHAPES])
def test_fp32_class_a_cases_are_exact_in_fp32(shape):
    n = 0
    for c in R.cases32():
        if c.shape == shape and c.cls == "A":
            d = R.inputs32(c)
            R.exact_case32(c, d, R.reference32(c, d))
            assert 0.2 < np.count_nonzero(d["w"]) / d["w"].size < 0.3 and 0.2 < np.count_nonzero(d["x"]) / d["x"].size < 0.3
            n += 1
    assert n >= 6


def _want32(c, d, ref):
    return R.exact_case32(c, d, ref) if c.cls == "A" else {"out0": (ref["out0"], ref["bound0"])}


def test_a_wrong_fp32_conv_reference_fails_the_comparison(fp32_refs):
    """The comparison the GPU test makes tells a right launch from the wrong ones a cosine of 1 - 1e-6 can absorb: the fp32-rounded right reference
    passes (class B: ratio <= 1), and as the device output it fails against a reference that pads before the leading BatchNorm, one that samples
    the shortcut at stride 1 in a stride-2 unit, and one that takes the 1x1 shortcut's tap at the un-strided position - in both classes."""
    seen = set()
    for c, d, ref in fp32_refs.values():
        outs = {"out0": ref["out0"].astype(np.float32)}
        bad, ratio = R.compare_outputs(c.cls, _want32(c, d, ref), outs)
        assert not bad and (ratio is None or ratio <= 1), c.id
        wrong = {"conv1": "pad_raw", "conv2": "sc_stride1", "shortcut1x1": "tap_unstrided"}[c.desc]
        wref = R.reference32(c, d, bound=c.cls == "B", wrong=wrong)
        bad, _ = R.compare_outputs(c.cls, {"out0": wref["out0"].astype(np.float32)} if c.cls == "A" else {"out0": (wref["out0"], wref["bound0"])}, outs)
        assert len(bad) == 1, (c.id, wrong)
        if wrong == "pad_raw":  # every border output moves, no interior one
            ne = wref["out0"] != ref["out0"]
            assert not ne[:, 1:-1, 1:-1].any() and (c.cls == "B" or ne[:, 0].any(-1).all() and ne[:, :, -1].any(-1).all())
        seen.add((wrong, c.cls))
    assert seen == {(w, cls) for w in ("pad_raw", "sc_stride1", "tap_unstrided") for cls in "AB"}


def test_small_fp32_cases_keep_their_premises_and_a_wrong_se_reference_fails():
    """Input layer class A and the Linear's sums are exact (asserted by the reference); the SE tail with w2 = 0 has gate 1/2; the right SE reference
    passes its own bounds and a pooled sum divided by the wrong pixel count does not."""
    for c in R.small_cases32():
        if c.F > 2:
            continue
        d = R.small_inputs32(c)
        want = R.small_reference32(c, d)
        if c.cls == "A":
            assert all(want[k][1] is None for k in ({"input32": ["out0"], "fc32": ["out1"], "se32": ["gate", "out0"]}[c.kind]))
        if c.kind == "fc32":
            assert (d["valid"] == 0).sum() == (c.F > 1) and not want["out0"][0][d["valid"] == 0].any()
        outs = {k: v[0].astype(np.float32) for k, v in want.items() if k != "gate_derived"}
        bad, ratios = R.compare_small32(c, want, outs)
        assert not bad and all(v <= 1 for v in ratios.values()), c.id
        if c.kind == "se32" and c.cls == "B":
            bad, _ = R.compare_small32(c, R.small_reference32(c, d, gate_dev=outs["gate"], pool_hw=c.H * c.H + c.H), outs)
            assert len(bad) == 1 and bad[0].startswith("gate"), (c.id, bad)
