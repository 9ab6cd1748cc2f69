"""Every instantiation of the exact fp32 scan (match_kernel x 18, match_reduce_kernel x 2) and the two device merges, each launched ALONE through its
launcher on guarded buffers (cases, references and the case table: tests/match_exact_ref.py; the program that runs them:
tests/cpp/match_exact_check.cpp; which kernel ran in which case: tools/match_exact_coverage.py -> profiles/match_exact/kernels.txt).
tests/test_gpu_match.py holds these kernels to 1e-5 on unit rows with a winner far ahead; here
  * class A (exact inputs): index, similarity bits, labels and the full matrix equal float64 bit for bit, with the winner duplicated across lane
    halves, waves, tiles and workgroups, a NaN row and an all-zero query;
  * class C (realistic inputs, rows within a few ulps of the winner): every similarity equals the fma chain restated in NumPy bit for bit, every
    index and label its ranking;
  * class B (the class C data): every similarity is within gamma(D) sum |q_k g_k| of float64; max(err / bound) is printed;
  * the merges equal oracle.match.merge_topk / test_identity_merge.reference_merge bit for bit;
  * partial_blocks 3 / 4 / 6 at 4 tiles: a workgroup walks two tiles, workgroups without a tile leave -1 partials;
  * no guard byte in front of or behind any buffer, and no byte of an input, has changed.
Seen on an MI355X: every class passes; class B max(err / bound) 0.028 at D = 512, 0.071 at D = 96, 0.137 at D = 32 (N = 461), 0.170 over the 33 x
65 869 full matrix at D = 32 (match_exact_ref.RATIOS_SEEN).  With the terms s and s ^ 1 of match_kernel's inner loop swapped, class C fails in every
group (similarity bits, and winners: e.g. row 14 for row 224) while classes A and B and the merges pass; with better() preferring the higher index
on a tie, classes A and C and both merges fail.
One harness process per group, each under its own timeout.  A process that ends on a HIP error or at its timeout ends the module: the remaining
parameters fail with its message and launch nothing."""
import shutil

import pytest

import match_exact_ref as X
import match_stage_ref as R
from launch_harness import Runner, build

_runner = Runner()


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return build(tmp_path_factory.mktemp("match_exact_check"), "match_exact_check")


@pytest.mark.gpu
@pytest.mark.parametrize("group", list(X.GROUPS))
def test_match_exact_alone(group, harness, tmp_path):
    _runner.require_running()
    work = tmp_path / "cases"
    work.mkdir()
    try:
        ops = R.Ops(work)
        check = X.GROUPS[group](ops)
        ops.write()
        _runner.run(harness, work, group, 120)
        failures = check()
        _runner.require_ended_well()
        assert not failures, "%d checks failed:\n%s" % (len(failures), "\n".join(failures[:40]))
    finally:
        shutil.rmtree(str(work), ignore_errors=True)
