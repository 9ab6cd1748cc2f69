"""The two launches of the recogniser's flip mode (csrc/kernels_arc_flip.hip), ALONE, against tests/flip_ref.py; the program that runs them:
tests/cpp/flip_launch_check.cpp (named guarded buffers, check_common.hpp).  One harness process under its own timeout for all cases.
  * pair-up, n = 1, 2, 3 (and the mirror-only launch the one-face passes use): bit for bit;
  * pair finalize, n = 1, 2, 33, 64 with 49 slices and n = 1, 2 with one: partials in {-1, 0, 1}, so the sums are exact and every embedding lies
    inside the reference's fp32 bound; the last row of n > 1 has valid == 0 and is zeros.  n = 1 also as two one-face passes kept apart;
  * no guard byte changed and every input is still what was loaded: nothing is written past 2n faces / n rows."""
import shutil

import numpy as np
import pytest

import flip_ref as FR
from launch_harness import Ops, Runner, bit_diff, build

pytestmark = pytest.mark.gpu
_runner = Runner()


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return build(tmp_path_factory.mktemp("flip_launch_check"), "flip_launch_check")


def test_flip_launches_alone(harness, tmp_path):
    _runner.require_running()
    work = tmp_path / "cases"
    work.mkdir()
    try:
        ops = Ops(work)
        exact, bounded = [], []  # (case, dump file, reference[, bound])
        for n in FR.PAIR_UP_N:
            x = FR.pair_up_input(n)
            want = FR.pair_up_reference(x)
            ops.case("pair_up_n%d" % n)
            ops.rbuf("in", x)
            ops.buf("out", want.nbytes)
            ops.op("pair_up", "in", "out", n)
            exact.append((ops.cid, ops.dump("out"), want))
            ops.end()
            ops.case("mirror_n%d" % n)
            ops.rbuf("in", x)
            ops.buf("out", x.nbytes)
            ops.op("mirror", "in", "out", n)
            exact.append((ops.cid, ops.dump("out"), want[n:]))
            ops.end()
        for c in FR.FINALIZE_CASES:
            d = FR.finalize_inputs(c)
            ref, bound = FR.finalize_case_reference(c, d)
            ops.case(c.id)
            ops.rbuf("partial", d["partial"])
            ops.rbuf("par", d["p"])
            ops.rbuf("valid", d["valid"])
            ops.buf("out", c.n * 512 * 4)
            ops.op("finalize", "partial", "par", "valid", "out", c.n, c.splits)
            bounded.append((ops.cid, ops.dump("out"), ref, bound, d["valid"]))
            ops.end()
            if c.n == 1:  # the same sums as two one-face passes kept apart
                ops.case(c.id + "_apart")
                ops.rbuf("pa", d["partial"][:, :1])
                ops.rbuf("pb", d["partial"][:, 1:])
                ops.rbuf("par", d["p"])
                ops.rbuf("valid", d["valid"])
                ops.buf("out", 512 * 4)
                ops.op("finalize2", "pa", "pb", "par", "valid", "out", 1, c.splits)
                bounded.append((ops.cid, ops.dump("out"), ref, bound, d["valid"]))
                ops.end()
        ops.write()
        _runner.run(harness, work, "the flip launches", 120)
        changed = ops.results()
        failures = []
        for cid in ops.cases:
            if cid not in changed:
                failures.append("%s: not reached" % cid)
            elif changed[cid]:
                failures.append("%s: %d guard bytes / inputs changed" % (cid, changed[cid]))
        for cid, fn, want in exact:
            failures += ["%s: %s" % (cid, m) for m in bit_diff("out", ops.read(fn, np.float32), want)]
        for cid, fn, ref, bound, valid in bounded:
            got = ops.read(fn, np.float32)
            if got is None or got.size != ref.size:
                failures.append("%s: out was not written" % cid)
                continue
            got = got.reshape(ref.shape)
            err = np.abs(got.astype(np.float64) - ref)
            print("%s: max(err / bound) = %.4f" % (cid, (err[valid != 0] / bound[valid != 0]).max()))
            if not np.isfinite(got).all() or (err > bound).any():
                failures.append("%s: %d of %d values outside the bound, largest error %.3g" % (cid, (err > bound).sum(), err.size, err.max()))
            if got[valid == 0].view(np.uint32).any():
                failures.append("%s: the row with valid == 0 is not zeros" % cid)
        _runner.require_ended_well()
        assert not failures, "%d checks failed:\n%s" % (len(failures), "\n".join(failures[:40]))
    finally:
        shutil.rmtree(str(work), ignore_errors=True)
