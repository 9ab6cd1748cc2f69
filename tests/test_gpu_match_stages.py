"""Every stage of the matcher's screened search ALONE against float64 (cases, references and bounds: tests/match_stage_ref.py; the program that
runs them: tests/cpp/match_stage_check.cpp).  tests/test_gpu_match.py sees these kernels only through the final answer, which the exact re-rank
repairs whenever the stages in front of it keep the winning block; here the shadow build, the coarse scan, the k-th entry, the pair selection and
the re-rank each run on buffers of their own:
  * class A (exact inputs): every output word equals the reference bit for bit;
  * class B (realistic inputs): every coarse entry is within the product's own delta of the float64 block maximum; max(err / delta) is printed;
  * the chained cases: every row at or above the float64 k-th best similarity lies in a listed block, without the overflow fallback;
  * no guard byte in front of or behind any buffer, and no byte of an input, has changed.
Seen on an MI355X: class B and chained max(err / delta) 0.707 for the int8 shadow (the rows aligned with query 9), 0.064 - 0.080 for the fp16
shadow; sqrt(max_err2) 1.0000500 x the float64 error norm.  The figure of every case: match_stage_ref's docstring.
One harness process per stage group, each under its own timeout.  A process that ends on a HIP error or at its timeout ends the module: the
remaining parameters fail with its message and launch nothing."""
import shutil

import pytest

import match_stage_ref as R
from launch_harness import Runner, build

_runner = Runner()


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return build(tmp_path_factory.mktemp("match_stage_check"), "match_stage_check")


@pytest.mark.gpu
@pytest.mark.parametrize("group", list(R.GROUPS))
def test_match_stage_alone(group, harness, tmp_path):
    _runner.require_running()
    work = tmp_path / "cases"
    work.mkdir()
    try:
        ops = R.Ops(work)
        check = R.GROUPS[group](ops)
        ops.write()
        _runner.run(harness, work, group, 120)
        failures = check()
        _runner.require_ended_well()
        assert not failures, "%d checks failed:\n%s" % (len(failures), "\n".join(failures[:40]))
    finally:
        shutil.rmtree(str(work), ignore_errors=True)
