"""Reference for frt_matcher_separation (include/frt.h) in plain numpy, written from the definition: for every row the
best OTHER row of its own label (genuine) and the best row of any other label (impostor) - largest similarity, lowest row among equal
values, a NaN similarity is no candidate, -inf / -1 without a candidate - plus the statistics and the threshold counts.  Nothing here knows
how the device does it."""
import numpy as np


def masked_argmax(sims, mask):
    """sims [q, n], mask [q, n] bool -> (sim [q] float32, row [q] int32): per query the first maximum over the candidates mask & ~isnan."""
    sims = np.asarray(sims)
    cand = np.asarray(mask) & ~np.isnan(sims)
    s = np.where(cand, sims, -np.inf)
    row = np.argmax(s, axis=1)  # the FIRST maximum
    q = np.arange(sims.shape[0])
    has = cand.any(axis=1)
    # a candidate whose similarity is -inf ties with the non-candidates in front of it: take the first CANDIDATE among the maxima
    best = s[q, row]
    first = np.argmax(cand & (s == best[:, None]), axis=1)
    row = np.where(has, first, -1).astype(np.int32)
    sim = np.where(has, best, -np.inf).astype(np.float32)
    return sim, row


def from_sims(sims, labels, query_rows=None):
    """sims [q, n]: query k is gallery row query_rows[k] (default: every row in order, q == n).  -> gen_sim, gen_row, imp_sim, imp_row [q]"""
    sims = np.asarray(sims)
    labels = np.asarray(labels)
    qr = np.arange(sims.shape[0]) if query_rows is None else np.asarray(query_rows)
    same = labels[qr][:, None] == labels[None, :]
    not_self = np.arange(sims.shape[1])[None, :] != qr[:, None]
    gen_sim, gen_row = masked_argmax(sims, same & not_self)
    imp_sim, imp_row = masked_argmax(sims, ~same)
    return gen_sim, gen_row, imp_sim, imp_row


def from_rows(rows, labels, dtype=np.float64):
    """rows [n, d]: the similarity is the dot product in `dtype`"""
    r = np.asarray(rows).astype(dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        return from_sims(r @ r.T, labels)


def stats(gen_sim, gen_row, imp_sim, imp_row):
    """-> [rows with a genuine candidate, rows with an impostor candidate, rows with both and imp_sim >= gen_sim]"""
    hg, hi = np.asarray(gen_row) >= 0, np.asarray(imp_row) >= 0
    return [int(hg.sum()), int(hi.sum()), int((hg & hi & (np.asarray(imp_sim) >= np.asarray(gen_sim))).sum())]


def counts(gen_sim, gen_row, imp_sim, imp_row, thresholds):
    """-> int64 [len(thresholds), 2]: rows with a genuine candidate and gen_sim < t | rows with an impostor candidate and imp_sim >= t"""
    hg, hi = np.asarray(gen_row) >= 0, np.asarray(imp_row) >= 0
    out = np.zeros((len(thresholds), 2), np.int64)
    for k, t in enumerate(np.asarray(thresholds, np.float32)):
        out[k, 0] = (hg & (np.asarray(gen_sim) < t)).sum()
        out[k, 1] = (hi & (np.asarray(imp_sim) >= t)).sum()
    return out
