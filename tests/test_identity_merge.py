"""Merge of per-shard identity lists (frt_merge_topk_labels, include/frt.h "Top-k over IDENTITIES"): the C-ABI host merge against a NumPy
restatement of the definition - order the occupied entries by (higher similarity, lower global index), keep the first entry of every label,
report the first k.  CPU only: no device call.  Every comparison is exact."""
import ctypes

import numpy as np
import pytest


def reference_merge(lab, idx, sim):
    """[shards, n, k] x 3 -> [n, k] x 3 by the definition"""
    shards, n, k = idx.shape
    lo = np.full((n, k), -1, np.int32)
    io = np.full((n, k), -1, np.int32)
    so = np.full((n, k), -np.inf, np.float32)
    for q in range(n):
        l, i, s = lab[:, q].reshape(-1), idx[:, q].reshape(-1), sim[:, q].reshape(-1)
        live = i >= 0
        l, i, s = l[live], i[live], s[live]
        order = np.lexsort((i, -s))
        seen, o = set(), 0
        for e in order:
            if int(l[e]) in seen:
                continue
            seen.add(int(l[e]))
            lo[q, o], io[q, o], so[q, o] = l[e], i[e], s[e]
            o += 1
            if o == k:
                break
    return lo, io, so


def shard_lists(r, shards, n, k, n_labels, ties=True):
    """what a shard's identity search returns: sorted lists of DISTINCT labels with global indices, some with empty tails; labels are shared
    between the shards, similarities come from a small set so that ties across shards are common"""
    lab = np.full((shards, n, k), -1, np.int32)
    idx = np.full((shards, n, k), -1, np.int32)
    sim = np.full((shards, n, k), -np.inf, np.float32)
    for s in range(shards):
        for q in range(n):
            m = int(r.integers(0, min(k, n_labels) + 1))
            v = r.choice(np.arange(-8, 9, dtype=np.float32) / 8, size=m) if ties else r.standard_normal(m).astype(np.float32)
            i = r.choice(np.arange(s * 1000, (s + 1) * 1000), size=m, replace=False)
            l = r.choice(np.arange(n_labels), size=m, replace=False)
            order = np.lexsort((i, -v))
            lab[s, q, :m], idx[s, q, :m], sim[s, q, :m] = l[order], i[order], v[order]
    return lab, idx, sim


def assert_same(got, want):
    for g, w, name in zip(got, want, ("label", "idx", "sim")):
        assert g.dtype == w.dtype and np.array_equal(g, w), name


@pytest.mark.parametrize("k", [1, 4, 16])
@pytest.mark.parametrize("n_labels", [3, 20, 200])
def test_merge_matches_the_definition(frt, k, n_labels):
    """3 shards, 7 queries; 3 labels = fewer than k identities overall for k = 4 and 16, and every list has empty slots"""
    r = np.random.default_rng(1000 * k + n_labels)
    lab, idx, sim = shard_lists(r, 3, 7, k, n_labels)
    assert (idx < 0).any()
    got = frt.merge_topk_labels(lab, idx, sim)
    want = reference_merge(lab, idx, sim)
    assert_same(got, want)
    if n_labels < k:
        assert (got[0][:, n_labels:] == -1).all() and (got[1][:, n_labels:] == -1).all() and np.isneginf(got[2][:, n_labels:]).all()


def test_identity_in_every_shard_with_equal_similarity_takes_the_lowest_index(frt):
    k = 4
    lab = np.full((3, 2, k), -1, np.int32)
    idx = np.full((3, 2, k), -1, np.int32)
    sim = np.full((3, 2, k), -np.inf, np.float32)
    for s, base in enumerate((2000, 50, 1000)):  # the lowest global index sits in the MIDDLE shard
        lab[s, :, 0], idx[s, :, 0], sim[s, :, 0] = 9, base + 3, 0.75
        lab[s, :, 1], idx[s, :, 1], sim[s, :, 1] = 100 + s, base + 7, 0.5 - 0.125 * s
    # query 1: label 9 has a strictly better row in the last shard - the similarity decides before the index
    sim[2, 1, 0] = 0.875
    lo, io, so = frt.merge_topk_labels(lab, idx, sim)
    assert lo[0].tolist() == [9, 100, 101, 102] and io[0].tolist() == [53, 2007, 57, 1007]
    assert so[0].tolist() == [0.75, 0.5, 0.375, 0.25]
    assert lo[1].tolist() == [9, 100, 101, 102] and io[1].tolist() == [1003, 2007, 57, 1007] and so[1, 0] == np.float32(0.875)
    assert_same((lo, io, so), reference_merge(lab, idx, sim))


def test_empty_slots_and_fewer_identities_than_k(frt):
    k = 4
    lab = np.full((2, 3, k), -1, np.int32)
    idx = np.full((2, 3, k), -1, np.int32)
    sim = np.full((2, 3, k), -np.inf, np.float32)
    # query 0: nothing at all; query 1: one identity, twice; query 2: an empty slot IN FRONT of an occupied one is skipped, not a terminator
    lab[0, 1, 0], idx[0, 1, 0], sim[0, 1, 0] = 5, 10, 0.25
    lab[1, 1, 0], idx[1, 1, 0], sim[1, 1, 0] = 5, 1010, 0.5
    lab[0, 2, 1], idx[0, 2, 1], sim[0, 2, 1] = 1, 11, 0.125
    lab[1, 2, 2], idx[1, 2, 2], sim[1, 2, 2] = 2, 1011, 0.125
    lo, io, so = frt.merge_topk_labels(lab, idx, sim)
    assert (lo[0] == -1).all() and (io[0] == -1).all() and np.isneginf(so[0]).all()
    assert lo[1].tolist() == [5, -1, -1, -1] and io[1].tolist() == [1010, -1, -1, -1] and so[1, 0] == 0.5 and np.isneginf(so[1, 1:]).all()
    assert lo[2].tolist() == [1, 2, -1, -1] and io[2].tolist() == [11, 1011, -1, -1]
    assert_same((lo, io, so), reference_merge(lab, idx, sim))


@pytest.mark.parametrize("k", [1, 4, 16])
def test_distinct_labels_reduce_to_the_row_merge(frt, k):
    """every entry its own identity (label = global index): the lists of frt_merge_topk, bit for bit"""
    r = np.random.default_rng(77 + k)
    _, idx, sim = shard_lists(r, 3, 7, k, 64)
    lab = idx.copy()
    lo, io, so = frt.merge_topk_labels(lab, idx, sim)
    ri, rs = frt.merge_topk(idx, sim)
    assert np.array_equal(io, ri) and np.array_equal(so, rs) and np.array_equal(lo, ri)


def test_bad_arguments_are_invalid(frt):
    k = 2
    lab = np.zeros((1, 1, k), np.int32)
    idx = np.zeros((1, 1, k), np.int32)
    sim = np.zeros((1, 1, k), np.float32)
    out_l, out_i, out_s = np.zeros((1, k), np.int32), np.zeros((1, k), np.int32), np.zeros((1, k), np.float32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    f = frt.lib.frt_merge_topk_labels
    assert f(1, 1, k, p(lab), p(idx), p(sim), p(out_l), p(out_i), p(out_s)) == 0
    assert f(0, 1, k, p(lab), p(idx), p(sim), p(out_l), p(out_i), p(out_s)) == frt.FRT_ERR_INVALID
    assert f(1, -1, k, p(lab), p(idx), p(sim), p(out_l), p(out_i), p(out_s)) == frt.FRT_ERR_INVALID
    assert f(1, 1, 0, p(lab), p(idx), p(sim), p(out_l), p(out_i), p(out_s)) == frt.FRT_ERR_INVALID
    for hole in range(6):
        args = [p(lab), p(idx), p(sim), p(out_l), p(out_i), p(out_s)]
        args[hole] = None
        assert f(1, 1, k, *args) == frt.FRT_ERR_INVALID, hole
    # the device form checks its arguments before it touches a device
    assert frt.lib.frt_merge_topk_labels_dev(1, 1, k, None, None, None, None, None, None, None) == frt.FRT_ERR_INVALID
    assert frt.lib.frt_merge_topk_labels_dev(0, 1, k, p(lab), p(idx), p(sim), p(out_l), p(out_i), p(out_s), None) == frt.FRT_ERR_INVALID
