"""Reference for frt_matcher_cluster (include/frt.h) in plain numpy: single-linkage clustering at a similarity
threshold = the connected components of the graph "sim(i, j) >= t" over the pairs i < j, every component labelled with its smallest row.
Nothing here knows how the device does it."""
import numpy as np


def components(n, ei, ej):
    """Union-find over the edges (ei[k], ej[k]) -> label[n] int32, label[i] = the smallest index of i's component.  Whole-array form: lab[x]
    always names a row of x's component that is <= x; every round hands the smaller label across every edge and then follows the labels to
    their end.  At the fixed point all rows of a component carry one label L with lab[L] == L, and the component's smallest row m has
    lab[m] <= m inside the component, i.e. lab[m] == m == L."""
    ei, ej = np.asarray(ei, np.int64), np.asarray(ej, np.int64)
    lab = np.arange(n, dtype=np.int64)
    while True:
        new = lab.copy()
        m = np.minimum(lab[ei], lab[ej])
        np.minimum.at(new, ei, m)
        np.minimum.at(new, ej, m)
        while not np.array_equal(new[new], new):
            new = new[new]
        if np.array_equal(new, lab):
            return lab.astype(np.int32)
        lab = new


def from_edges(n, ei, ej):
    """-> (labels, number of clusters, number of joined pairs)"""
    labels = components(n, ei, ej)
    return labels, int((labels == np.arange(n)).sum()), int(len(ei))


def cluster_sims(sims, t):
    """sims [n, n] (any float type; only the upper triangle is read).  A NaN similarity joins nothing, no row is joined to itself."""
    sims = np.asarray(sims)
    with np.errstate(invalid="ignore"):
        ei, ej = np.nonzero(np.triu(sims >= t, 1))
    return from_edges(sims.shape[0], ei, ej)


def cluster_rows(rows, t, dtype=np.float64):
    """rows [n, d]: the similarity is the dot product in `dtype`"""
    r = np.asarray(rows).astype(dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        return cluster_sims(r @ r.T, t)


def high_pairs(rows, floor, block=2048, lo_rows=None):
    """Blocked float32 sgemm over the upper triangle: every pair i < j with sim >= floor -> (i, j, sim) arrays (NaN pairs never qualify).
    lo_rows: only pairs whose row i is one of these (sorted) rows OR whose row j is - the pairs a few changed rows take part in."""
    r = np.ascontiguousarray(rows, np.float32)
    n = r.shape[0]
    out_i, out_j, out_s = [], [], []

    def take(a0, a_idx, b0, b1):
        with np.errstate(invalid="ignore", over="ignore"):
            s = r[a_idx] @ r[b0:b1].T
            ii, jj = np.nonzero(s >= floor)
        gi, gj = np.asarray(a_idx)[ii] if a0 is None else ii + a0, jj + b0
        out_i.append(gi)
        out_j.append(gj)
        out_s.append(s[ii, jj])

    if lo_rows is None:
        for a0 in range(0, n, block):
            for b0 in range(a0, n, block):
                take(a0, slice(a0, min(a0 + block, n)), b0, min(b0 + block, n))
    else:
        for b0 in range(0, n, block):
            take(None, np.asarray(lo_rows), b0, min(b0 + block, n))
    i, j, s = np.concatenate(out_i), np.concatenate(out_j), np.concatenate(out_s)
    if lo_rows is not None:  # (a, b) came out with a in lo_rows: order every pair, drop self pairs and the doubles among lo_rows
        keep = i != j
        i, j, s = i[keep], j[keep], s[keep]
        i, j = np.minimum(i, j), np.maximum(i, j)
        _, first = np.unique(i.astype(np.int64) * n + j, return_index=True)
        return i[first], j[first], s[first]
    keep = i < j
    return i[keep], j[keep], s[keep]
