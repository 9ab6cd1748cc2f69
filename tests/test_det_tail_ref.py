"""The references and input makers of tests/det_tail_ref.py checked WITHOUT a GPU: the box reference against both existing oracles, the exact
candidate counts, the placement of the ties, the float64 landmark and alignment references against the float32 mirror (oracle/align.py), which
must lie inside the derived bounds, and the operation lists every group writes for the harness."""
import numpy as np
import pytest

import det_tail_ref as R
import slim_ref
from oracle import align


def test_geometries_take_both_unletterbox_branches():
    assert R.MNET.A == 3780 and R.SLIM.A == 888 and R.SLIMW.A == 888
    assert R.MNET.A % 64 and R.SLIM.A % 64
    assert R.MNET.branch_h and R.SLIMW.branch_h and not R.SLIM.branch_h
    assert len(R.oracle().anchors(R.MNET.in_w, R.MNET.in_h)) == R.MNET.A


def test_anchor_tables_agree():
    """the float64 anchors of the landmark reference narrow to slim_ref.anchors and, for mnet, to oracle.anchors"""
    for g in (R.MNET, R.SLIM):
        a64 = R.anchors64(g)
        assert np.array_equal(a64.astype(np.float32), slim_ref.anchors(g.in_w, g.in_h, g.table))
        ls = R.anchor_level_size(g)
        sizes = np.array([g.table["min_sizes"][k][l] for k, l in ls], np.float64)
        assert np.allclose(a64[:, 2] * g.in_w, sizes, rtol=1e-14, atol=0)
    assert np.array_equal(R.anchors64(R.MNET).astype(np.float32), R.oracle().anchors(R.MNET.in_w, R.MNET.in_h))


def test_batched_counts_and_references():
    """exact candidate counts (257, 0, 256, ...), slim_ref with the mnet table == oracle.postprocess on every frame (asserted inside ref_frame),
    at least min(K, 4, candidates) boxes kept"""
    loc, conf, refs = R.heads_and_refs("mnet", R.BATCH_COUNTS, 1, R.BATCH_KS)
    assert tuple((conf[..., 1] > np.float32(R.BBOX_THR)).sum(1)) == R.BATCH_COUNTS
    for K in R.BATCH_KS:
        for n, (boxes, kept, cand) in zip(R.BATCH_COUNTS, refs[K]):
            assert len(cand) == n and len(boxes) == len(kept) <= K
            assert len(boxes) >= min(K, 4, n)
    assert len(refs[300][7][0]) == 300  # the cap to max_faces after the NMS is reached
    assert 4 < len(refs[300][4][0]) < 255  # and in another frame the NMS runs out of candidates first
    for i, counts in enumerate(R.SEQ_COUNTS):
        R.heads_and_refs("mnet", counts, 10 + i, (R.SEQ_K,))
    for g in (R.SLIM, R.SLIMW):
        assert R.slim_kept_level3(g)


def test_decode_inputs():
    for g in (R.MNET, R.SLIM):
        conf, want = R._decode_inputs(g, R.BBOX_THR)
        assert len(want[0]) == 0 and len(want[1]) and want[1].min() >= (g.A // 64) * 64 and g.A - 1 in want[2]
        assert (conf[2, :, 1] == np.float32(R.BBOX_THR)).sum() >= 10 and np.isnan(conf[2, :, 1]).sum() == 10
        conf, want = R._decode_inputs(g, -1.0)
        assert len(want[0]) == g.A


@pytest.mark.parametrize("n", [256, 700])
def test_tie_placement(n):
    """tie_case() asserts the placement; here once more from its results: equal scores, different lane groups / strides in every order, and the
    reference picks the lower anchor of each group first"""
    loc, anch, score, orders, (boxes, kept, cand) = R.tie_case(n)
    unit = 64 if n == 256 else 256
    assert len(cand) == n and (n <= 256) == (unit == 64)
    for g, (lo, hi) in enumerate(R.TIE_RANKS[n]):
        assert score[lo] == score[hi] == np.float32(R.TIE_SCORES[g]) and anch[lo] < anch[hi]
        assert kept[2 * g] == anch[lo] and kept[2 * g + 1] == anch[hi]
        for o in orders.values():
            assert np.nonzero(o == lo)[0][0] // unit != np.nonzero(o == hi)[0][0] // unit
    assert sorted(orders["shuffle"].tolist()) == list(range(n)) and not np.array_equal(orders["shuffle"], orders["asc"])


def test_landmark_mirror_inside_bound():
    """oracle/align.py's float32 chain (the kernel's operation order) lies inside the bound derived for the float64 formula, mnet table"""
    g = R.MNET
    ldm, kept, nout = R.landmark_inputs(g)
    worst = 0.0
    for f in (0, 2):
        idx = kept[f, :nout[f]].astype(np.int64)
        val, bound = R.landmark_reference(g, ldm[f], idx)
        got = align.decode_landmarks(ldm[f], idx, g.in_h, g.in_w, g.frame_h, g.frame_w).reshape(-1, 10)
        ratio = np.abs(got.astype(np.float64) - val) / bound
        worst = max(worst, ratio.max())
        assert (ratio <= 1).all()
        assert bound.max() < 1e-3  # tighter than the mirror test's 1e-3 px
    print("landmark mirror: max(err / bound) = %.4f" % worst)
    for g in (R.SLIM, R.SLIMW):
        ldm, kept, nout = R.landmark_inputs(g)
        val, bound = R.landmark_reference(g, ldm[0], kept[0].astype(np.int64))
        assert np.isfinite(val).all() and (bound > 0).all() and bound.max() < 1e-3


def test_landmark_reference_detects_a_wrong_table():
    """the bound is tight enough to tell the tables apart: decoding Slim anchors with a size one step off moves values by far more than the bound"""
    g = R.SLIM
    ldm, kept, _ = R.landmark_inputs(g)
    idx = kept[0].astype(np.int64)
    val, bound = R.landmark_reference(g, ldm[0], idx)
    wrong = R.Geom("x", 4, 4, g.in_w, g.in_h, g.frame_w, g.frame_h, dict(steps=g.table["steps"], min_sizes=((10, 16, 20), (32, 48), (64, 96), (128, 192, 256))))
    val2, _ = R.landmark_reference(wrong, ldm[0], idx)
    assert (np.abs(val2 - val) > 100 * bound).any()


def test_alignment_mirror_inside_bound_and_matrix():
    """oracle.align.align_faces inside 0.5 + bound on every case, no pixel left out; the float64 matrix equals oracle.align.similarity_matrix"""
    frames = R.tight_frames()
    names = set()
    for rnd in R.align_rounds():
        for slot, face in zip(R.LIVE, rnd):
            frame = frames[slot // R.MAXF]
            with np.errstate(invalid="ignore"):  # (the NaN / inf cases)
                crops, valid = align.align_faces(frame, face.lm[None])
            fails = []
            ratio = R.check_aligned(face.name, face, frame, crops[0], valid[0], fails)
            assert not fails, fails
            ok, value, bound, M = R.align_reference(frame, face.lm)
            if ok:
                assert np.allclose(M, align.similarity_matrix(face.lm), rtol=1e-9, atol=1e-9)
                assert ratio <= 1
                print("%s: mirror max((err - 0.5) / bound) = %.4f, largest bound %.3g" % (face.name, ratio, bound.max()))
                assert bound.max() < 64, "a bound that decides nothing"
            names.add(face.kind)
    assert names == {"bound", "zeros", "copy", "invalid"}


def test_alignment_cases_cover_the_edges():
    frames = R.tight_frames()
    faces = {f.name: f for f in R.align_faces_list()}
    H, W = R.FH, R.FW
    for name, outside in (("edge_left", lambda sx, sy: sx < 0), ("edge_right", lambda sx, sy: sx > W), ("edge_top", lambda sx, sy: sy < 0), ("edge_bottom", lambda sx, sy: sy > H)):
        ok, value, _, M = R.align_reference(frames[0], faces[name].lm)
        A = np.vstack([M, [0, 0, 1]])
        inv = np.linalg.inv(A)
        corners = np.array([[0, 0, 1], [111, 0, 1], [0, 111, 1], [111, 111, 1]], np.float64) @ inv.T
        assert ok and any(outside(x, y) for x, y, _ in corners) and value.any(), name
    ok, value, _, _ = R.align_reference(frames[0], faces["outside"].lm)
    assert ok and not value.any()
    ok, _, _, M = R.align_reference(frames[0], faces["mirror"].lm)
    assert ok and np.linalg.det(M[:, :2]) > 0  # the least-squares similarity, never a reflection
    for name in ("identical_den0", "nan", "inf"):
        assert not R.align_reference(frames[0], faces[name].lm)[0]
    s = faces["den1e-3"].lm.astype(np.float64)
    assert 3e-4 < ((s - s.mean(0)) ** 2).sum() < 3e-3


def test_crop_cases():
    kinds = R.crop_conditions()
    assert {"up", "whole", "1x1", "empty", "negative", "far", "frame0", "frame2"} <= kinds, kinds
    assert R.FRAME_STRIDE > R.FH * R.ROW_STRIDE and R.ROW_STRIDE == 128 * 3 + 13
    frames = R.tight_frames()
    buf = R.padded_frames(frames, R.ROW_STRIDE, R.FRAME_STRIDE)
    assert np.array_equal(buf[2 * R.FRAME_STRIDE + 5 * R.ROW_STRIDE:][:R.FW * 3].reshape(-1, 3), frames[2, 5])
    assert not np.array_equal(frames[0], frames[1])


def test_pack_reference():
    boxes = np.zeros(8, R.BBOX_DTYPE)
    boxes["x1"] = np.arange(8) + 1
    boxes["score"] = 0.7
    out = R.pack_reference(boxes, [2, 1], np.array([1, 0, 1, 1, 5, 1, 1, 1]), np.arange(8) + 100, np.arange(8) * 0.1, 4)
    assert out["valid"].tolist() == [1, 0, 0, 0, 1, 0, 0, 0] and out["frame"].tolist() == [0, 0, 0, 0, 1, 1, 1, 1]
    assert out["match_idx"].tolist() == [100, -1, -1, -1, 104, -1, -1, -1]
    assert out["x1"].tolist() == [1, 2, 0, 0, 5, 0, 0, 0] and out["score"][1] == np.float32(0.7) and out["score"][2] == 0
    out = R.pack_reference(boxes, [2, 1], np.ones(8, np.int32), None, None, 4)
    assert (out["match_idx"] == -1).all() and (out["match_sim"] == 0).all()


@pytest.mark.parametrize("group", list(R.GROUPS))
def test_group_writes_its_operations(group, tmp_path):
    """every group builds (all of its input makers' assertions run) and names only operations the harness knows; without the harness's output
    its check reports every case as unfinished and raises nothing"""
    ops = R.Ops(tmp_path)
    check = R.GROUPS[group](ops)
    ops.write()
    known = {"case", "buf", "rbuf", "load", "geom", "dump_geom", "decode", "nms", "landmarks", "crop", "align", "pack", "dump", "end"}
    assert {ln.split()[0] for ln in ops.lines} <= known
    assert ops.lines.count("end") == len(ops.cases) > 0
    fails = check()
    assert len(fails) >= len(ops.cases)
