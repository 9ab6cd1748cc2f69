"""conv64_kernel (csrc/kernels_arc_c64.hip) ALONE at batches where a workgroup walks MORE THAN ONE strip.

The launch-alone cases of tests/test_gpu_arc_launches.py run this kernel at the first batch of its plan lines and at first + 1: 4 faces at
112x112 (448 strips) and 11 at 56x56 (308 strips).  The launcher's grid is min(512, strips), so there every workgroup owns exactly one strip:
the persistent walk, the hand-over of the two patch buffers and the rotation of the two accumulator halves (a strip's second half drains
under the NEXT strip's first K loop, the last one behind the loop) are never reached.  (The walks of the recogniser's other two persistent
kernels, arc_input_mfma_kernel over tiles and conv_s2c64_kernel over output rows: tests/test_gpu_persistent_walks.py.)  Here the same harness (tests/cpp/arc_launch_check.cpp,
tests/launch_harness.py), the same cases, references and bounds (tests/arc_launch_ref.py) run the plan lines whose label is
conv64_kernel<0 | 1 | 2> at four other batches, all inside the lines' ranges.  A strip is 2 rows x 56 columns, so with a grid of 512:

    shape     faces  strips   walk
    56x56      19      532    20 workgroups walk two strips, 492 one      (ragged remainder, one hand-over)
    56x56      37    1 036    12 walk three, 500 two                      (both parities of the rotation, the remainder on the last round)
    112x112     5      560    48 walk two, 464 one
    112x112    10    1 120    96 walk three, 416 two

Class A (exact inputs) at every batch, all three modes: out0 and out1 equal the float64 reference bit for bit.  Class B (realistic inputs)
once per mode: every element inside the bound arc_launch_ref derives; max(err / bound) is printed.  Every case: the planned label is the
plan golden's and no half outside the logical outputs has changed.  test_walk_cases needs no GPU: it checks the table above and, on the
reference alone, the premises of class A at these batches (arc_launch_ref.exact_case); the references it computes are kept for the GPU cases."""
import shutil

import pytest

import arc_launch_ref as R
from launch_harness import Runner, build

GRID = 512                                   # launch_c64_t
BATCHES = {0: (5, 10), 1: (19, 37)}          # unit shape (arc_launch_ref.SHAPES) -> faces
WALK = {(1, 19): (532, {2: 20, 1: 492}), (1, 37): (1036, {3: 12, 2: 500}), (0, 5): (560, {2: 48, 1: 464}), (0, 10): (1120, {3: 96, 2: 416})}
CLASS_B = {"conv64_kernel<0>": (0, 10), "conv64_kernel<1>": (1, 37), "conv64_kernel<2>": (1, 37)}  # label -> (shape, faces) of its realistic case

_runner = Runner()
_want = {}  # case id -> what compare_outputs takes


def _lines():
    return [ln for ln in R.plan_lines() if ln.label.startswith("conv64_kernel<")]


def _cases():
    out = []
    for ln in _lines():
        for F in BATCHES[ln.shape]:
            assert ln.first <= F <= ln.last, (ln, F)
            out.append(R.Case("walk_s%d_%s_F%d_A" % (ln.shape, ln.desc, F), ln.shape, ln.desc, F, "A", ln.label))
            if CLASS_B[ln.label] == (ln.shape, F):
                out.append(R.Case("walk_s%d_%s_F%d_B" % (ln.shape, ln.desc, F), ln.shape, ln.desc, F, "B", ln.label))
    return out


CASES = _cases()


def _prepare(case):
    """(inputs, expected outputs) of one case; the expected outputs are computed once per process."""
    d = R.inputs(case)
    if case.id not in _want:
        ref = R.reference(case, d, bound=case.cls == "B")
        if case.cls == "A":
            _want[case.id] = R.exact_case(case, d, ref)  # asserts the premises of class A on the reference
        else:
            _want[case.id] = {k: (ref[k], ref["bound" + k[-1]]) for k in ("out0", "out1") if k in ref}
    return d, _want[case.id]


def _walk(strips):
    """{strips walked: workgroups} of conv64_kernel's persistent walk over a grid of GRID"""
    full, rem = divmod(strips, GRID)
    return {n: c for n, c in ((full + 1, rem), (full, GRID - rem)) if c and n}


def test_walk_cases():
    """The batches give the four situations of the module docstring, every mode has its cases, and the premises of class A hold there."""
    assert sorted({ln.label for ln in _lines()}) == ["conv64_kernel<%d>" % m for m in (0, 1, 2)]
    for (shape, F), (strips, walk) in WALK.items():
        h = R.SHAPES[shape][2]
        assert h % 2 == 0 and h % 56 == 0
        assert F * (h // 2) * (h // 56) == strips and _walk(strips) == walk, (shape, F)
    assert sorted(WALK) == sorted((s, F) for s, fs in BATCHES.items() for F in fs)
    labels = {(c.label, c.shape, c.F, c.cls) for c in CASES}
    assert {l for l, _, _, cls in labels if cls == "B"} == set(CLASS_B) and len([c for c in CASES if c.cls == "B"]) == 3
    for m in (0, 1, 2):  # class A: every mode at both 56x56 batches, mode 0 at both 112x112 batches too
        assert {(s, F) for l, s, F, cls in labels if cls == "A" and l == "conv64_kernel<%d>" % m} >= {(1, 19), (1, 37)}
    assert {(s, F) for l, s, F, cls in labels if cls == "A" and l == "conv64_kernel<0>"} >= {(0, 5), (0, 10)}
    for c in CASES:
        if c.cls == "A":
            _prepare(c)


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return build(tmp_path_factory.mktemp("conv64_walk"), "arc_launch_check")


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_conv64_walks_strips(case, harness, tmp_path):
    _runner.require_running()
    work = tmp_path / "cases"
    work.mkdir()
    try:
        d, want = _prepare(case)
        R.write_case(str(work), case, d)
        R.write_manifest(str(work), [case])
        _runner.run(harness, work, case.id, 120)
        got = R.read_outputs(str(work), case)
        _runner.require_ended_well()
        assert got is not None, "%s: not reached" % case.id
        outs, changed, label = got
        bad, ratio = R.compare_outputs(case.cls, want, outs)
        if ratio is not None:
            print("%s %s: max(err / bound) = %.3f" % (case.id, case.label, ratio))
        if label != case.label:
            bad.append("planned %s, the plan golden says %s" % (label, case.label))
        if changed:
            bad.append("%d halves outside the logical output changed" % changed)
        assert not bad, "%s (%s):\n%s" % (case.id, case.label, "\n".join(bad))
    finally:
        shutil.rmtree(str(work), ignore_errors=True)
