"""tests/separation_ref.py, the numpy oracle of frt_matcher_separation, on matrices small enough to check by hand, and the three statements
that make the call the calibration of frt_matcher_cluster's threshold (include/frt.h), against tests/cluster_ref.py.  No device."""
import numpy as np

import cluster_ref
import separation_ref

NINF = -np.inf


def sym(n, entries, diag=1.0):
    s = np.zeros((n, n), np.float32)
    np.fill_diagonal(s, diag)
    for (i, j), v in entries.items():
        s[i, j] = s[j, i] = v
    return s


def test_tie_takes_the_lowest_row_on_both_sides():
    labels = [0, 0, 0, 1, 1, 2]
    s = sym(6, {(0, 1): 0.8, (0, 2): 0.8, (1, 2): 0.7, (0, 3): 0.25, (0, 4): 0.25, (0, 5): 0.25, (3, 4): 0.9, (1, 5): 0.1})
    gs, gr, is_, ir = separation_ref.from_sims(s, labels)
    assert gr.tolist() == [1, 0, 0, 4, 3, -1] and gs.tolist() == [np.float32(v) for v in (0.8, 0.8, 0.8, 0.9, 0.9, NINF)]
    assert ir[0] == 3 and is_[0] == np.float32(0.25)  # rows 3, 4, 5 tie at 0.25: the lowest wins
    assert ir[2] == 3 and is_[2] == 0.0  # all impostors of row 2 at 0: still the lowest row
    assert ir.tolist()[3:] == [0, 0, 0]
    assert gs.dtype == np.float32 and gr.dtype == np.int32 and is_.dtype == np.float32 and ir.dtype == np.int32


def test_nan_is_no_candidate_and_a_nan_row_has_none():
    labels = [0, 0, 1, 1, 2, 2]
    s = sym(6, {(0, 1): 0.8, (2, 3): 0.8, (4, 5): 0.6, (0, 2): 0.3, (1, 3): 0.2})
    s[5, :] = np.nan  # row 5 is a NaN row: every similarity with it is NaN, in both directions
    s[:, 5] = np.nan
    s[0, 1] = np.nan  # one NaN entry of an otherwise fine query: its only genuine candidate goes
    gs, gr, is_, ir = separation_ref.from_sims(s, labels)
    assert (gs[5], gr[5], is_[5], ir[5]) == (NINF, -1, NINF, -1)
    assert (gs[4], gr[4]) == (NINF, -1) and ir[4] == 0  # its only partner is the NaN row
    assert (gs[0], gr[0]) == (NINF, -1) and (gs[1], gr[1]) == (np.float32(0.8), 0)
    assert 5 not in gr.tolist() and 5 not in ir.tolist()
    assert separation_ref.stats(gs, gr, is_, ir) == [3, 5, 0]


def test_a_candidate_at_minus_infinity_still_wins():
    s = sym(6, {})
    s[0, 1] = NINF
    s[0, 2:] = NINF
    gs, gr, is_, ir = separation_ref.from_sims(s, [0, 0, 1, 1, 1, 1])
    assert (gs[0], gr[0], is_[0], ir[0]) == (NINF, 1, NINF, 2)


def test_singleton_and_single_identity_gallery():
    s = sym(6, {(0, 1): 0.9, (2, 3): 0.5, (2, 4): 0.6, (3, 4): 0.4, (0, 5): 0.35})
    gs, gr, is_, ir = separation_ref.from_sims(s, [0, 0, 1, 1, 1, 7])
    assert (gs[5], gr[5]) == (NINF, -1) and (is_[5], ir[5]) == (np.float32(0.35), 0)  # a person with one photo
    assert gr.tolist()[:5] == [1, 0, 4, 2, 2]
    assert separation_ref.stats(gs, gr, is_, ir) == [5, 6, 0]
    gs, gr, is_, ir = separation_ref.from_sims(s, [3] * 6)  # one identity: nobody has an impostor
    assert ir.tolist() == [-1] * 6 and np.all(is_ == NINF)
    assert gr.tolist() == [1, 0, 4, 2, 2, 0]
    assert separation_ref.stats(gs, gr, is_, ir) == [6, 0, 0]
    assert separation_ref.counts(gs, gr, is_, ir, [0.5]).tolist() == [[1, 0]]  # only row 5's 0.35 is below 0.5


def test_closer_to_another_person_counts_and_thresholds():
    labels = [0, 0, 1, 1, 2, 2]
    s = sym(6, {(0, 1): 0.4, (0, 2): 0.7, (2, 3): 0.7, (4, 5): 0.9, (1, 4): 0.4})
    gs, gr, is_, ir = separation_ref.from_sims(s, labels)
    # row 0: gen 0.4 < imp 0.7; row 1: gen 0.4 == imp 0.4 (>= counts); row 2: gen 0.7 == imp 0.7; row 4: imp 0.4 < gen 0.9
    assert gs.tolist() == [np.float32(v) for v in (0.4, 0.4, 0.7, 0.7, 0.9, 0.9)]
    assert is_.tolist() == [np.float32(v) for v in (0.7, 0.4, 0.7, 0.0, 0.4, 0.0)]
    assert separation_ref.stats(gs, gr, is_, ir) == [6, 6, 3]
    c = separation_ref.counts(gs, gr, is_, ir, [0.0, 0.4, 0.5, 0.7, 0.95])
    assert c.tolist() == [[0, 6], [0, 4], [2, 2], [2, 2], [6, 0]]  # gen_sim < t is strict, imp_sim >= t is not
    # query_rows: the same answers for a subset of the rows
    q = [4, 0]
    sub = separation_ref.from_sims(s[q], labels, q)
    assert [a.tolist() for a in sub] == [a[q].tolist() for a in (gs, gr, is_, ir)]


def persons(n, seed, D=512):
    """n rows, 1 to 6 per person: unit centre + 0.5 x unit noise, re-normalised, shuffled -> rows float32, person id per row"""
    rng = np.random.Generator(np.random.PCG64(seed))
    rows, person = [], []
    p = 0
    while len(rows) < n:
        c = rng.standard_normal(D)
        c /= np.linalg.norm(c)
        for _ in range(min(1 + p % 6, n - len(rows))):
            u = rng.standard_normal(D)
            r = c + 0.5 * u / np.linalg.norm(u)
            rows.append(r / np.linalg.norm(r))
            person.append(p)
        p += 1
    perm = rng.permutation(n)
    return np.ascontiguousarray(np.array(rows)[perm], np.float32), np.array(person, np.int32)[perm]


def test_the_three_cluster_consequences_on_a_persons_gallery():
    """t* = max imp_sim: above it no component of cluster() holds two labels and the singletons are the rows with gen_sim < t; at t* the
    arg-max pair shares a component.  One float32 similarity matrix feeds both oracles, so the statements hold exactly."""
    rows, labels = persons(300, 7)
    with np.errstate(invalid="ignore"):
        sims = rows @ rows.T
    sims = np.maximum(sims, sims.T)  # (bitwise symmetric, as the device's S is)
    gs, gr, is_, ir = separation_ref.from_sims(sims, labels)
    assert separation_ref.stats(gs, gr, is_, ir)[1] == 300 and (gr < 0).sum() > 0  # everybody has an impostor, some persons have one photo
    a = int(np.argmax(is_))
    t_star = is_[a]
    above = np.nextafter(t_star, np.float32(np.inf))
    comp, n_comp, _ = cluster_ref.cluster_sims(sims, above)
    for c in np.unique(comp):
        assert len(set(labels[comp == c].tolist())) == 1
    sizes = np.bincount(comp, minlength=300)[comp]
    assert np.array_equal(sizes == 1, gs < above)
    assert n_comp >= len(set(labels.tolist()))  # persons stay whole or split, never merge
    comp, _, _ = cluster_ref.cluster_sims(sims, t_star)
    assert comp[a] == comp[ir[a]] and labels[a] != labels[ir[a]]
    # a higher threshold, still above t*: the singleton statement keeps holding
    t = np.float32(0.8)
    assert t > t_star
    comp, _, _ = cluster_ref.cluster_sims(sims, t)
    assert np.array_equal(np.bincount(comp, minlength=300)[comp] == 1, gs < t)
