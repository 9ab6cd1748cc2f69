"""arc_input_mfma_kernel (csrc/kernels_arc_input.hip) and conv_s2c64_kernel (csrc/kernels_arc_s2.hip) ALONE at batches where they WALK.

Both are persistent: a fixed grid walks a list of work items and carries state from one item to the next.  The launch-alone cases of
tests/test_gpu_arc_launches.py run them where nothing is carried (conv64_kernel, the third such kernel: tests/test_gpu_conv64_walk.py):

  * The input layer: every wave walks tiles of 32 pixels with a stride of gridDim.x * 4 waves; launch_arc_input_mfma shrinks the grid to
    (n_tiles + 3) / 4 until n_tiles reaches 2048 (512 workgroups x 4 waves).  arc_launch_ref.small_cases("input") runs F = 1, 2, 3 - 392, 784,
    1176 tiles, one per wave - so the one-tile-deep software pipeline (tile t + stride's 16 tap loads and four border ballots taken before tile
    t's MFMAs, the hand-over xv = xn, edge = edge_n, the per-wave transpose tiles reused without a barrier) never executes.
  * The 112 -> 56 conv: workgroup lid of 768 walks the output rows [lid n / 768, (lid + 1) n / 768), n = 56 F, with input rows in three LDS
    slots, slot(y) = (y + 1) % 3; a step inherits row 2 oy - 1 from the step before and fetches two new rows behind the second barrier -
    three at an image's first row -, and ends on a hand-counted wait.  The launch-alone cases run F = 23 and 24: ranges of one or two rows, so
    no step inherits a row that was itself fetched inside the loop, and no new image begins behind a second or third step.

Here the same harness (tests/cpp/arc_launch_check.cpp, tests/launch_harness.py) and the same references and bounds (tests/arc_launch_ref.py)
run them at:

    launch    F    items          walk
    input      6   2 352 tiles    304 waves walk two tiles, 1 744 one
    input     11   4 312 tiles    216 walk three, 1 832 two               (both buffer parities, the remainder on the last round)
    112->56   37   2 072 rows     536 ranges of three rows, 232 of two
    112->56   42   2 352 rows     720 ranges of three, 48 of four

    image boundaries strictly inside a range, {(range length, offset of the new image's first row): count}
    F = 37: {(2, 1): 4, (3, 1): 9, (3, 2): 10};  13 ranges start at the first row of an image b > 0, 14 end at an image's last row
    F = 42: {(3, 1): 12, (3, 2): 12};            17 and 18

The 112 -> 56 conv has three plan lines (tests/golden/arc_conv_plan.txt, label conv_s2c64_kernel); what each launch is, from the descriptions in
csrc/frt_arc_launches.hpp:

    line                  epilogue                                 the wait that ends a step
    conv2                 BN + shortcut, two outputs               vmcnt(8)
    conv2_se with se=0    conv2's launch with the SE scratch       vmcnt(8)   (planned only: a pass launches conv2_res + the stand-alone tail)
    conv2_res             BN, no shortcut, one output              vmcnt(4)

Each line: class A (exact inputs) at F = 37 and 42, out0 and out1 bit for bit against arc_launch_ref.exact_case; class B (realistic inputs) at
F = 37 inside the bound arc_launch_ref derives, max(err / bound) printed.  The conv2_se line runs as the harness's case kind "conv_plain": the
description launched as it is planned (kind "conv" moves conv2_se to its twin with the SE tail, which these lines do not have).
The input launch: class B at F = 6 and 11 with small_reference's bound, and class A - new in arc_launch_ref, "the three small launches" - at
F = 1, 6 and 11: z and y bit for bit.  Every case: the planned label is the golden's (the input: the launcher's name) and nothing outside the
logical outputs - z and the even-position y for the input - has changed.  One harness process per case, each under its own timeout; a process
that ends on a HIP error, a signal or its timeout ends the module.  test_walk_tables needs no GPU: it restates the two launchers' walks, asserts
the tables above, and on the reference alone the premises of every class A case, whose references it keeps for the GPU cases."""
import collections
import shutil
import subprocess

import numpy as np
import pytest

import arc_launch_ref as R
from launch_harness import Runner, build

INPUT_WAVES = 2048  # launch_arc_input_mfma: 512 workgroups x 4 waves; fewer while there are fewer tiles
INPUT_TILE = 32     # pixels
S2_GRID = 768       # launch_s2c64; fewer while there are fewer rows
S2_LABEL = "conv_s2c64_kernel"

INPUT_WALK = {6: (2352, {2: 304, 1: 1744}), 11: (4312, {3: 216, 2: 1832})}         # F -> (tiles, {tiles walked: waves})
S2_WALK = {37: (2072, {3: 536, 2: 232}), 42: (2352, {3: 720, 4: 48})}               # F -> (rows, {range length: workgroups})
S2_INSIDE = {37: {(2, 1): 4, (3, 1): 9, (3, 2): 10}, 42: {(3, 1): 12, (3, 2): 12}}  # F -> {(range length, offset of an image's first row): ranges}
S2_ENDS = {37: (13, 14), 42: (17, 18)}  # F -> (ranges that start at the first row of an image b > 0, ranges that end at an image's last row)
INPUT_A, INPUT_B = (1, 6, 11), (6, 11)
S2_A, S2_B = (37, 42), 37

_runner = Runner()
_want = {}  # class A case id -> the exact outputs, fp16


def input_walk(F, waves=INPUT_WAVES):
    """(tiles, {tiles walked: waves}) of arc_input_mfma_kernel: wave w of the grid takes tiles w, w + waves, ..."""
    tiles, rem = divmod(F * 112 * 112, INPUT_TILE)
    assert rem == 0
    waves = min(waves, (tiles + 3) // 4 * 4)
    return tiles, dict(collections.Counter(len(range(w, tiles, waves)) for w in range(waves) if w < tiles))


def s2_ranges(F, grid=S2_GRID):
    """The row ranges [begin, end) of conv_s2c64_kernel's workgroups (as logical ids: blockIdx.x only permutes them)."""
    n = 56 * F
    g = min(grid, n)
    return [(lid * n // g, (lid + 1) * n // g) for lid in range(g)]


def s2_walk(F):
    """(rows, {range length: workgroups}, {(range length, offset): ranges with an image's first row at that offset > 0}, (ranges that start at the
    first row of an image b > 0, ranges that end at an image's last row))"""
    rs = s2_ranges(F)
    assert rs[0][0] == 0 and rs[-1][1] == 56 * F and all(a[1] == b[0] for a, b in zip(rs, rs[1:]))
    inside = collections.Counter((e - b, row - b) for b, e in rs for row in range(b + 1, e) if row % 56 == 0)
    return 56 * F, dict(collections.Counter(e - b for b, e in rs)), dict(inside), (sum(b > 0 and b % 56 == 0 for b, e in rs if e > b), sum(e % 56 == 0 for b, e in rs if e > b))


def _s2_lines():
    return R.plan_lines_of(S2_LABEL)


def _s2_cases():
    out = []
    for ln in _s2_lines():
        for F in S2_A:
            out.append(R.Case("walk_s%d_%s_F%d_A" % (ln.shape, ln.desc, F), ln.shape, ln.desc, F, "A", ln.label))
        out.append(R.Case("walk_s%d_%s_F%d_B" % (ln.shape, ln.desc, S2_B), ln.shape, ln.desc, S2_B, "B", ln.label))
    return out


S2_CASES = _s2_cases()
INPUT_CASES = R.input_cases(INPUT_A, "A") + R.input_cases(INPUT_B, "B")


def _prepare_conv(case):
    """(inputs, what compare_outputs takes); the exact outputs of a class A case are computed once per process."""
    d = R.inputs(case)
    if case.cls == "A":
        if case.id not in _want:
            _want[case.id] = R.exact_case(case, d, R.reference(case, d))  # asserts the premises of class A on the reference
        return d, _want[case.id]
    ref = R.reference(case, d, bound=True)
    return d, {k: (ref[k], ref["bound" + k[-1]]) for k in ("out0", "out1") if k in ref}


def _prepare_input(c):
    d = R.small_inputs(c)
    if c.cls == "A":
        if c.id not in _want:
            ref = R.small_reference(c, d)  # asserts the premises of class A
            assert all(bound is None for _, bound in ref.values())
            _want[c.id] = {k: v.astype(np.float16) for k, (v, _) in ref.items()}
            assert all(np.array_equal(_want[c.id][k], v) for k, (v, _) in ref.items())
        return d, _want[c.id]
    return d, R.small_reference(c, d)


def test_walk_tables():
    """The walks of the module docstring, restated from the two launchers; the premise of this file - the existing cases walk nothing -; every
    chosen batch inside its plan line; the premises of every class A case, on the reference alone."""
    for F, want in INPUT_WALK.items():
        assert input_walk(F) == want, F
    assert sorted(INPUT_WALK) == sorted(INPUT_B) and set(INPUT_B) < set(INPUT_A)
    for F, (rows, lengths) in S2_WALK.items():
        assert s2_walk(F) == (rows, lengths, S2_INSIDE[F], S2_ENDS[F]), (F, s2_walk(F))
        assert S2_ENDS[F][0] > 0 and S2_ENDS[F][1] > 0
    assert sorted(S2_WALK) == sorted(S2_A) and S2_B in S2_A
    # what the launch-alone cases of tests/test_gpu_arc_launches.py run: no wave walks two tiles, no range is longer than two rows
    small = [c.F for c in R.small_cases("input")]
    assert small == [1, 2, 3] and all(set(input_walk(F)[1]) == {1} for F in small)
    alone = sorted({c.F for c in R.cases() if c.label == S2_LABEL})
    assert alone == [23, 24] and all(set(s2_walk(F)[1]) <= {1, 2} for F in alone)
    # the three plan lines, every chosen batch inside their ranges
    lines = _s2_lines()
    assert sorted(ln.desc for ln in lines) == ["conv2", "conv2_res", "conv2_se"] and all(ln.shape == 0 for ln in lines)
    for ln in lines:
        assert all(ln.first <= F <= ln.last for F in S2_A), ln
    assert len(S2_CASES) == 9 and len({c.id for c in S2_CASES}) == 9 and len([c for c in S2_CASES if c.cls == "B"]) == 3
    assert [(c.F, c.cls) for c in INPUT_CASES] == [(1, "A"), (6, "A"), (11, "A"), (6, "B"), (11, "B")]
    assert not {c.id for c in INPUT_CASES} & {c.id for c in R.small_cases("input")}
    # the two epilogues of the kernel: two outputs with a shortcut (conv2, and conv2_se as planned), one output without (conv2_res)
    assert [R.geometry(0, desc)[6:9] for desc in ("conv2", "conv2_se", "conv2_res")] == [("add", "sc", 56), ("add", "sc", 56), ("bn", None, 0)]
    for c in S2_CASES:
        if c.cls == "A":
            _prepare_conv(c)
    for c in INPUT_CASES:
        if c.cls == "A":
            _prepare_input(c)


def test_harness_plans_the_walk_cases(tmp_path):
    """Without a GPU: the harness compiles, and plans conv_s2c64_kernel for all nine conv cases - the conv2_se line through the case kind that
    launches a description as it is planned."""
    exe = build(tmp_path, "arc_launch_check")
    R.write_manifest(str(tmp_path), S2_CASES, kind="conv_plain")
    out = subprocess.run([exe, "--plan", str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert dict(line.split("\t") for line in out.stdout.splitlines()) == {c.id: S2_LABEL for c in S2_CASES}


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return build(tmp_path_factory.mktemp("persistent_walks"), "arc_launch_check")


@pytest.mark.gpu
@pytest.mark.parametrize("case", S2_CASES, ids=[c.id for c in S2_CASES])
def test_conv_s2c64_walks_rows(case, harness, tmp_path):
    _runner.require_running()
    work = tmp_path / "cases"
    work.mkdir()
    try:
        d, want = _prepare_conv(case)
        R.write_case(str(work), case, d)
        R.write_manifest(str(work), [case], kind="conv_plain")
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


@pytest.mark.gpu
@pytest.mark.parametrize("case", INPUT_CASES, ids=[c.id if c.cls == "A" else c.id + "_B" for c in INPUT_CASES])
def test_input_layer_walks_tiles(case, harness, tmp_path):
    _runner.require_running()
    work = tmp_path / "cases"
    work.mkdir()
    try:
        d, want = _prepare_input(case)
        R.write_small(str(work), case, d)
        R.write_small_manifest(str(work), [case])
        _runner.run(harness, work, case.id, 120)
        got = R.read_small_outputs(str(work), case)
        _runner.require_ended_well()
        assert got is not None, "%s: not reached" % case.id
        outs, changed, label = got
        bad, ratio = R.compare_outputs(case.cls, want, outs)
        if ratio is not None:
            print("%s %s: max(err / bound) = %.3f" % (case.id, label, ratio))
        if label != "launch_arc_input":
            bad.append("ran %s" % label)
        if changed:
            bad.append("%d halves outside the logical z and the even-position y changed" % changed)
        assert not bad, "%s:\n%s" % (case.id, "\n".join(bad))
    finally:
        shutil.rmtree(str(work), ignore_errors=True)
