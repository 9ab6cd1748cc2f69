"""frt_matcher_cluster (include/frt.h), the part that needs no GPU: the numpy oracle of tests/cluster_ref.py on graphs
made by hand, and the two entry points as the header, the library and the Python binding declare them."""
import ctypes
import os

import numpy as np

import cluster_ref
from conftest import ROOT

CSRC = os.path.join(ROOT, "face-recognition-cpp-tensorrt_amd", "csrc")


def sims_of(n, edges, low=0.0):
    s = np.full((n, n), low, np.float32)
    for i, j, v in edges:
        s[i, j] = s[j, i] = v
    np.fill_diagonal(s, 1.0)  # a row is never joined to itself: the diagonal must not count
    return s


def test_a_chain_is_one_component_although_its_ends_are_far_apart():
    s = sims_of(5, [(0, 1, 0.7), (1, 2, 0.7), (2, 3, 0.7), (3, 4, 0.7)])
    assert s[0, 4] < 0.5
    labels, clusters, edges = cluster_ref.cluster_sims(s, 0.5)
    assert labels.dtype == np.int32 and labels.tolist() == [0] * 5 and (clusters, edges) == (1, 4)


def test_two_components_and_isolated_rows_take_their_smallest_row_as_label():
    s = sims_of(8, [(6, 2, 0.9), (2, 4, 0.6), (7, 1, 0.8), (6, 4, 0.55)])
    labels, clusters, edges = cluster_ref.cluster_sims(s, 0.5)
    assert labels.tolist() == [0, 1, 2, 3, 2, 5, 2, 1]
    assert (clusters, edges) == (5, 4)


def test_an_edge_at_equality_joins_and_the_next_float_above_does_not():
    t = np.float32(0.5)
    s = sims_of(3, [(0, 2, t)])
    assert cluster_ref.cluster_sims(s, t)[0].tolist() == [0, 1, 0]
    assert cluster_ref.cluster_sims(s, np.nextafter(t, np.float32(np.inf)))[0].tolist() == [0, 1, 2]


def test_a_nan_similarity_joins_nothing():
    s = sims_of(3, [(0, 1, np.nan), (1, 2, 0.9)])
    labels, clusters, edges = cluster_ref.cluster_sims(s, 0.5)
    assert labels.tolist() == [0, 1, 1] and (clusters, edges) == (2, 1)


def test_whole_array_union_find_equals_a_pointer_chasing_one_on_random_graphs():
    rng = np.random.Generator(np.random.PCG64(5))
    for n, m in ((1, 0), (40, 25), (300, 260), (300, 2000)):
        ei, ej = rng.integers(n, size=m), rng.integers(n, size=m)
        parent = list(range(n))

        def root(x):
            while parent[x] != x:
                x = parent[x]
            return x

        for a, b in zip(ei.tolist(), ej.tolist()):
            ra, rb = root(a), root(b)
            parent[max(ra, rb)] = min(ra, rb)
        assert cluster_ref.components(n, ei, ej).tolist() == [root(i) for i in range(n)]


def test_rows_form_and_blocked_pairs_agree_with_the_matrix_form():
    rng = np.random.Generator(np.random.PCG64(9))
    centres = rng.standard_normal((30, 48))
    rows = centres[rng.integers(30, size=200)] + 0.4 * rng.standard_normal((200, 48))
    rows = (rows / np.linalg.norm(rows, axis=1, keepdims=True)).astype(np.float32)
    want = cluster_ref.cluster_rows(rows, 0.5, np.float32)
    assert 1 < want[1] < 200 and want[2] > 0
    i, j, s = cluster_ref.high_pairs(rows, 0.3, block=64)
    assert (i < j).all() and cluster_ref.from_edges(200, i[s >= 0.5], j[s >= 0.5])[1:] == want[1:]
    assert np.array_equal(cluster_ref.from_edges(200, i[s >= 0.5], j[s >= 0.5])[0], want[0])
    some = np.array([3, 77, 199])
    pi, pj, ps = cluster_ref.high_pairs(rows, 0.3, block=64, lo_rows=some)
    touching = np.isin(i, some) | np.isin(j, some)
    assert sorted(zip(pi.tolist(), pj.tolist())) == sorted(zip(i[touching].tolist(), j[touching].tolist()))


def test_cluster_is_declared_exported_and_bound(frt):
    header = open(os.path.join(ROOT, "include", "frt.h")).read()
    for s, n_args in (("frt_matcher_cluster", 5), ("frt_matcher_cluster_dev", 5)):
        assert s + "(" in header
        assert hasattr(frt.lib, s), "libfrt.so does not export %s" % s
        assert s in frt.ABI and len(frt.ABI[s][1]) == n_args, "python binding misses %s" % s
        assert frt.ABI[s][0] is ctypes.c_int and frt.ABI[s][1][1] is ctypes.c_float  # (the threshold travels as a float)
    assert callable(frt.MatMul.cluster) and callable(frt.MatMul.cluster_dev)


def test_cluster_rejects_a_null_matcher(frt):
    assert frt.lib.frt_matcher_cluster(None, 0.5, None, 0, None) == frt.FRT_ERR_INVALID
    assert b"null argument" in frt.lib.frt_last_error()
    assert frt.lib.frt_matcher_cluster_dev(None, 0.5, None, None, None) == frt.FRT_ERR_INVALID


def test_kernel_file_is_part_of_the_library_build():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "kernels_cluster" in mk
    src = open(os.path.join(CSRC, "kernels_cluster.hip")).read()
    for k in ("cluster_rerank_union_kernel", "cluster_dense_union_kernel", "cluster_flatten_kernel", "__HIP_MEMORY_SCOPE_AGENT"):
        assert k in src
