"""Every launch between the detector's heads and the recogniser's input ALONE and batched (cases, references and bounds:
tests/det_tail_ref.py; the program that runs them: tests/cpp/det_tail_check.cpp): decode_kernel, nms_kernel, landmark_decode_kernel,
crop_faces_kernel, align_faces_kernel, pack_results_kernel.  The other tests see these through batch-1 calls on a handful of candidates or
through a float32 mirror of the kernels; here
  * boxes, n_out, kept anchors, candidate sets and result records equal the reference exactly, frame by frame, at 255 / 256 / 257 candidates
    and on both sides of the NMS's two paths, in any candidate order, on reused scratch;
  * every landmark value and every aligned pixel lies inside a bound derived from the kernel's float32 operations around a float64 reference;
    max(err / bound) is printed per case;
  * crops equal oracle.crop_faces byte for byte in the batched form (n_boxes gating, padded strides, crops == nullptr, frames_shared);
  * no guard byte in front of or behind any buffer, and no byte of an input, has changed.
The DetGeom of every case is the production table (det_geometry in libfrt.so), compared with anchors derived on the Python side.
One harness process per group, each under its own timeout.  A process that ends on a HIP error or at its timeout ends the module: the
remaining parameters fail with its message and launch nothing.
Seen on an MI355X, 2026-10-20: landmarks max(err / bound) 0.3227 (mnet table), 0.4140 / 0.4263 (Slim table, either un-letterbox branch);
alignment max((err - 0.5) / bound) 0.0019 over all pixels of all faces (RATIOS_SEEN in tests/det_tail_ref.py).  No ratio exceeded 1 and no
bound was changed after measuring; the tests found no bug in the kernels.
decode_kernel zeroes the score of a lane past A before it compares, so the guard pattern behind the last frame's conf cannot become a candidate
whether or not `in_range` stands in `take`; what tells the two apart is a NEGATIVE threshold (every finite score is a candidate, and a lane
past A with its score of 0 would be one too): the decode_*_neg cases, count == A exactly."""
import shutil

import pytest

import det_tail_ref as R
from launch_harness import Runner, build

_runner = Runner()


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return build(tmp_path_factory.mktemp("det_tail_check"), "det_tail_check")


@pytest.mark.gpu
@pytest.mark.parametrize("group", list(R.GROUPS))
def test_det_tail_alone(group, harness, tmp_path):
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
