"""frt_matcher_separation (include/frt.h): leave-one-out genuine / impostor scores of a labelled gallery, on the device,
against the numpy oracle of tests/separation_ref.py.

Galleries are the persons of tests/test_gpu_cluster.py (the helper is copied, not imported): every row is its person's unit centre plus a
unit noise direction times SPREAD, re-normalised, 1 to 6 rows per person, shuffled; the label of a row is its person.  Wherever the device
is compared with `==` the oracle runs on the matcher's own bits - the full matrix frt_matcher_calculate downloads for queries = the stored
rows - so the comparison is exact whatever the summation order.  Against the blocked float32 sgemm oracle the bound is 1e-4: the worst-case
rounding of a 512-term fp32 dot product of unit vectors is 512 * 2^-24 = 3.1e-5 on each side.  Oracles and device results that several
tests need are computed once and kept unchanged."""
import numpy as np
import pytest

import separation_ref

pytestmark = pytest.mark.gpu

SPREAD = 0.5
MARGIN = 1e-4
N_SMALL = 1000
N_BIG = 32768 + 200                 # just above SCREEN_MIN_ROWS (frt_matcher.hpp); the last 128-row tile holds 72 rows
SPECIAL = (5, 20_000, N_BIG - 1)    # one person, placed by hand: first chunk, a middle one, the partial last tile
THRESHOLDS = np.array([0.1, 0.3, 0.5, 0.8, 0.95], np.float32)
_CACHE = {}


# ---------------------------------------------------------------------------------------------------------------- inputs and oracles
def person_rows(rng, counts, D):
    """-> rows [sum(counts), D] float64 (unit norm), person [sum(counts)]"""
    rows, person = [], []
    for p, m in enumerate(counts):
        c = rng.standard_normal(D)
        c /= np.linalg.norm(c)
        for _ in range(m):
            u = rng.standard_normal(D)
            u /= np.linalg.norm(u)
            r = c + SPREAD * u
            rows.append(r / np.linalg.norm(r))
            person.append(p)
    return np.array(rows), np.array(person)


def stored32(rows, fp16):
    """the values the matcher keeps, as float32 (fp16 storage widens exactly)"""
    r = np.ascontiguousarray(rows, np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        return r.astype(np.float16).astype(np.float32) if fp16 else r


def small_rows(D, seed=0):
    """N_SMALL rows, 1 to 6 per person, shuffled -> rows float32, labels int32"""
    key = ("small_rows", D, seed)
    if key not in _CACHE:
        rng = np.random.Generator(np.random.PCG64(3100 + D + seed))
        counts = []
        while sum(counts) < N_SMALL:
            counts.append(min(1 + len(counts) % 6, N_SMALL - sum(counts)))
        rows, person = person_rows(rng, counts, D)
        perm = rng.permutation(N_SMALL)
        _CACHE[key] = (np.ascontiguousarray(rows[perm], np.float32), person[perm].astype(np.int32))
    return _CACHE[key]


def planted_rows(D):
    """small_rows with an exact duplicate pair under one label, an exact duplicate pair under two labels, and (already there) singletons"""
    key = ("planted", D)
    if key not in _CACHE:
        rows, labels = small_rows(D)
        rows = rows.copy()
        n_of = np.bincount(labels)
        big = np.nonzero(n_of[labels] >= 3)[0]
        a = int(big[0])
        b = int(np.nonzero(labels == labels[a])[0][-1])
        c = int(big[np.nonzero(labels[big] != labels[a])[0][0]])
        d = int(big[np.nonzero((labels[big] != labels[a]) & (labels[big] != labels[c]))[0][-1]])
        assert a != b and labels[a] == labels[b] and labels[c] != labels[d] and len({a, b, c, d}) == 4
        rows[b] = rows[a]
        rows[d] = rows[c]
        assert (n_of == 1).any()
        _CACHE[key] = (rows, labels, (a, b, c, d))
    return _CACHE[key]


def big_rows():
    """A screened gallery: N_BIG x 512, 1 to 6 rows per person (M <= 6), shuffled over the whole gallery, one person of three at SPECIAL"""
    if "big_rows" not in _CACHE:
        rng = np.random.Generator(np.random.PCG64(5150))
        counts = []
        while sum(counts) < N_BIG - 3:
            counts.append(min(1 + len(counts) % 6, N_BIG - 3 - sum(counts)))
        body, body_person = person_rows(rng, counts, 512)
        sp, _ = person_rows(rng, [3], 512)
        rows = np.empty((N_BIG, 512), np.float32)
        labels = np.empty(N_BIG, np.int32)
        free = np.setdiff1d(np.arange(N_BIG), np.array(SPECIAL))
        free = free[rng.permutation(len(free))]
        rows[free], labels[free] = body, body_person
        rows[list(SPECIAL)], labels[list(SPECIAL)] = sp, len(counts)
        assert np.bincount(labels).max() <= 6
        _CACHE["big_rows"] = (rows, labels)
    return _CACHE["big_rows"]


def sgemm_oracle(rows, labels, block=1024):
    """Blocked float32 sgemm over ALL pairs -> (gen_max [n], imp_max [n]): the largest similarity among the other rows of the row's label
    (-inf without one) and among the rows of every other label."""
    r = np.ascontiguousarray(rows, np.float32)
    n = r.shape[0]
    order = np.argsort(labels, kind="stable")
    bounds = np.nonzero(np.diff(labels[order]))[0] + 1
    pi, pj = [], []
    for grp in np.split(order, bounds):  # every ordered pair (i, j) of one label, i == j included
        pi.append(np.repeat(grp, len(grp)))
        pj.append(np.tile(grp, len(grp)))
    pi, pj = np.concatenate(pi), np.concatenate(pj)
    by_i = np.argsort(pi, kind="stable")
    pi, pj = pi[by_i], pj[by_i]
    gen = np.full(n, -np.inf, np.float32)
    imp = np.empty(n, np.float32)
    for a0 in range(0, n, block):
        a1 = min(a0 + block, n)
        s = r[a0:a1] @ r.T
        lo, hi = np.searchsorted(pi, a0), np.searchsorted(pi, a1)
        qi, qj = pi[lo:hi], pj[lo:hi]
        other = qi != qj
        np.maximum.at(gen, qi[other], s[qi[other] - a0, qj[other]])
        s[qi - a0, qj] = -np.inf
        imp[a0:a1] = s.max(axis=1)
    return gen, imp


def big_oracle(fp16):
    key = ("big_oracle", fp16)
    if key not in _CACHE:
        rows, labels = big_rows()
        _CACHE[key] = sgemm_oracle(stored32(rows, fp16), labels)
    return _CACHE[key]


def load(frt, rows, labels, fp16=False, screening=True):
    mm = frt.MatMul(0)
    mm.setScreening(screening)
    mm.setStorage(fp16)
    mm.init(rows)
    mm.setStorage(False)
    if labels is not None:
        mm.set_labels(labels)
    return mm


def stat_list(frt, stats):
    return [stats[k] for k in frt.MatMul.SEPARATION_STATS]


def check_against_calculate(frt, mm, rows, labels, fp16, got, what=""):
    """got = mm.separation(THRESHOLDS): every output == the oracle on the bits frt_matcher_calculate returns for queries = the stored rows"""
    n = len(labels)
    sims = mm.calculate(stored32(rows, fp16))
    want = separation_ref.from_sims(sims, labels)
    gs, gr, is_, ir, counts, stats = got
    print("%s stats %s (oracle %s)" % (what, stat_list(frt, stats), separation_ref.stats(*want)))
    assert gs.dtype == np.float32 and gr.dtype == np.int32 and is_.dtype == np.float32 and ir.dtype == np.int32
    for name, g, w in zip(("gen_sim", "gen_row", "imp_sim", "imp_row"), (gs, gr, is_, ir), want):
        bad = np.nonzero(g != w)[0]
        assert bad.size == 0, "%s differs at rows %s: %s != %s" % (name, bad[:5], g[bad[:5]], w[bad[:5]])
    assert stat_list(frt, stats)[:3] == separation_ref.stats(*want)
    assert stats["screened_chunks"] + stats["exact_chunks"] == (n + 127) // 128
    assert counts.dtype == np.int64 and np.array_equal(counts, separation_ref.counts(*want, THRESHOLDS))
    return want


# ---------------------------------------------------------------------------------------------------------------- 1. bits, small
@pytest.mark.parametrize("fp16", [False, True], ids=["fp32", "fp16"])
@pytest.mark.parametrize("D", [64, 512])
def test_small_gallery_equals_the_oracle_on_the_matchers_bits(frt, D, fp16):
    rows, labels, (a, b, c, d) = planted_rows(D)
    mm = load(frt, rows, labels, fp16)
    got = mm.separation(THRESHOLDS)
    want = check_against_calculate(frt, mm, rows, labels, fp16, got)
    mm.close()
    gs, gr, is_, ir = want
    assert gr[a] == b and gr[b] == a and gs[a] == gs[b]  # the duplicates under one label find each other
    assert ir[c] == d and ir[d] == c and is_[c] == is_[d]  # and so do the duplicates under two
    assert (gr < 0).any() and got[5]["genuine_rows"] < N_SMALL and got[5]["impostor_rows"] == N_SMALL
    assert got[5]["closer_to_another"] >= 2 and got[5]["screened_chunks"] == 0


# ---------------------------------------------------------------------------------------------------------------- 2. large identity
@pytest.mark.parametrize("fp16", [False, True], ids=["fp32", "fp16"])
def test_one_label_of_300_rows_spread_over_all_chunks(frt, fp16):
    rows, labels = small_rows(512)
    labels = labels.copy()
    crowd = np.arange(0, 900, 3)
    labels[crowd] = labels.max() + 1
    assert len(crowd) == 300 and set((crowd // 128).tolist()) == set(range(8))
    mm = load(frt, rows, labels, fp16)
    assert mm.labels_info()[1] == 300  # M + 1 > 16: no screen for the impostor side either way
    got = mm.separation(THRESHOLDS)
    want = check_against_calculate(frt, mm, rows, labels, fp16, got)
    mm.close()
    assert got[5]["screened_chunks"] == 0
    assert (labels[want[1][crowd]] == labels[crowd[0]]).all() and (want[1][crowd] != crowd).all()


# ---------------------------------------------------------------------------------------------------------------- 3. screened
def screened_run(frt, fp16):
    """the screened gallery's device results, once per storage type"""
    key = ("screened_run", fp16)
    if key not in _CACHE:
        rows, labels = big_rows()
        mm = load(frt, rows, labels, fp16)
        assert mm.labels_info()[1] <= 6
        got = mm.separation(THRESHOLDS)
        qr = np.concatenate([np.array(SPECIAL), np.setdiff1d(np.arange(0, N_BIG, 64), np.array(SPECIAL))[:509]])
        assert len(qr) == 512 and len(set(qr.tolist())) == 512
        sims = mm.calculate(stored32(rows, fp16)[qr])
        mm.close()
        _CACHE[key] = (got, qr, separation_ref.from_sims(sims, labels, qr))
    return _CACHE[key]


@pytest.mark.parametrize("fp16", [False, True], ids=["fp32", "fp16"])
def test_screened_gallery_equals_the_oracles(frt, fp16):
    rows, labels = big_rows()
    (gs, gr, is_, ir, counts, stats), qr, want = screened_run(frt, fp16)
    chunks = (N_BIG + 127) // 128
    print("stats", stat_list(frt, stats))
    assert stats["screened_chunks"] > 0 and stats["screened_chunks"] + stats["exact_chunks"] == chunks
    # 512 query rows, exactly: the oracle on calculate's bits
    for name, g, w in zip(("gen_sim", "gen_row", "imp_sim", "imp_row"), (gs, gr, is_, ir), want):
        bad = np.nonzero(g[qr] != w)[0]
        assert bad.size == 0, "%s differs at rows %s: %s != %s" % (name, qr[bad[:5]], g[qr][bad[:5]], w[bad[:5]])
    assert set(gr[list(SPECIAL)].tolist()) <= set(SPECIAL) and (gr[list(SPECIAL)] != np.array(SPECIAL)).all()
    # all rows: the blocked float32 sgemm oracle
    gen_max, imp_max = big_oracle(fp16)
    r = stored32(rows, fp16)
    me = np.arange(N_BIG)
    has_gen = np.isfinite(gen_max)
    assert np.array_equal(gr >= 0, has_gen) and (ir >= 0).all()
    assert np.all(gs[~has_gen] == -np.inf)
    print("largest |sim - oracle|: genuine %.3g impostor %.3g" % (np.abs(gs[has_gen] - gen_max[has_gen]).max(), np.abs(is_ - imp_max).max()))
    assert np.abs(gs[has_gen] - gen_max[has_gen]).max() <= MARGIN and np.abs(is_ - imp_max).max() <= MARGIN
    g = me[has_gen]
    assert (labels[gr[g]] == labels[g]).all() and (gr[g] != g).all()
    assert (labels[ir] != labels).all() and (ir != me).all()
    # the returned row's own similarity (float32 dot of the two stored rows) against the oracle maximum
    assert np.abs(np.einsum("ij,ij->i", r[g], r[gr[g]]) - gen_max[g]).max() <= MARGIN
    assert np.abs(np.einsum("ij,ij->i", r, r[ir]) - imp_max).max() <= MARGIN
    want_all = (gs, gr, is_, ir)
    assert stat_list(frt, stats)[:3] == separation_ref.stats(*want_all) and np.array_equal(counts, separation_ref.counts(*want_all, THRESHOLDS))


# ---------------------------------------------------------------------------------------------------------------- 4. path independence
@pytest.mark.parametrize("fp16", [False, True], ids=["fp32", "fp16"])
def test_screening_off_returns_the_same_arrays(frt, fp16):
    rows, labels = big_rows()
    screened = screened_run(frt, fp16)[0]
    mm = load(frt, rows, labels, fp16, screening=False)
    exact = mm.separation(THRESHOLDS)
    mm.close()
    assert exact[5]["screened_chunks"] == 0 and exact[5]["exact_chunks"] == (N_BIG + 127) // 128
    for a, b in zip(exact[:5], screened[:5]):
        assert np.array_equal(a, b)
    assert stat_list(frt, exact[5])[:3] == stat_list(frt, screened[5])[:3]


# ---------------------------------------------------------------------------------------------------------------- 5. non-finite rows
@pytest.mark.parametrize("fp16", [False, True], ids=["fp32", "fp16"])
def test_a_nan_row_and_an_inf_row(frt, fp16):
    rows, labels = small_rows(512)
    rows = rows.copy()
    n_of = np.bincount(labels)
    nan_row = int(np.nonzero(n_of[labels] >= 3)[0][7])
    inf_row = int(np.nonzero((n_of[labels] >= 3) & (labels != labels[nan_row]))[0][11])
    rows[nan_row] = np.nan
    rows[inf_row, 0] = np.inf
    mm = load(frt, rows, labels, fp16)
    got = mm.separation(THRESHOLDS)
    gs, gr, is_, ir = got[:4]
    assert (gs[nan_row], gr[nan_row], is_[nan_row], ir[nan_row]) == (-np.inf, -1, -np.inf, -1)
    assert nan_row not in gr.tolist() and nan_row not in ir.tolist()
    assert not np.isnan(gs).any() and not np.isnan(is_).any()
    check_against_calculate(frt, mm, rows, labels, fp16, got)
    mm.close()


# ---------------------------------------------------------------------------------------------------------------- 6. the cluster consequences
def consequences(mm, labels, got):
    gs, gr, is_, ir = got[:4]
    a = int(np.argmax(is_))
    t_star = is_[a]
    above = np.nextafter(t_star, np.float32(np.inf))
    comp, _ = mm.cluster(above)
    order = np.argsort(comp, kind="stable")
    lo = np.minimum.reduceat(labels[order], np.nonzero(np.diff(comp[order], prepend=-1))[0])
    hi = np.maximum.reduceat(labels[order], np.nonzero(np.diff(comp[order], prepend=-1))[0])
    assert np.array_equal(lo, hi), "a component above t* holds two labels"
    assert np.array_equal(np.bincount(comp, minlength=len(comp))[comp] == 1, gs < above)
    comp, _ = mm.cluster(t_star)
    assert comp[a] == comp[ir[a]] and labels[a] != labels[ir[a]]


def margin_holds(gen_max, imp_max):
    """on a CPU oracle: apart from the two rows of the arg-max pair itself, no gen_sim / imp_sim lies within MARGIN of t* (and so of
    nextafter(t*), the two thresholds the test uses)"""
    t = imp_max.max()
    near_imp = np.abs(imp_max - t) <= MARGIN
    return near_imp.sum() <= 2 and not (np.abs(gen_max[np.isfinite(gen_max)] - t) <= MARGIN).any()


@pytest.mark.parametrize("fp16", [False, True], ids=["fp32", "fp16"])
@pytest.mark.parametrize("D", [64, 512])
def test_cluster_consequences_small(frt, D, fp16):
    """The gallery of test 1 before the duplicates are planted: with them t* is the 1.0 of the duplicate pair under two labels and the
    gen_sim of the pair under one label is a 1.0 as well, so no gallery holding both can keep the margin this test asserts first."""
    for seed in range(20):
        rows, labels = small_rows(D, seed)
        gs, gr, is_, ir = separation_ref.from_rows(stored32(rows, fp16), labels, np.float64)
        if margin_holds(gs, is_):
            break
    else:
        raise AssertionError("no seed keeps the margin")
    mm = load(frt, rows, labels, fp16)
    consequences(mm, labels, mm.separation())
    mm.close()


@pytest.mark.parametrize("fp16", [False, True], ids=["fp32", "fp16"])
def test_cluster_consequences_screened(frt, fp16):
    rows, labels = big_rows()
    assert margin_holds(*big_oracle(fp16))
    mm = load(frt, rows, labels, fp16)
    consequences(mm, labels, screened_run(frt, fp16)[0])
    mm.close()


# ---------------------------------------------------------------------------------------------------------------- 7. device form, surface
def test_device_form_on_a_side_stream_and_what_the_call_leaves_alone(frt):
    import torch
    rows, labels, _ = planted_rows(512)
    mm = load(frt, rows, labels)
    probe = rows[:37] + 0.01
    before = mm.topk_labels(probe, 3)
    host = mm.separation(THRESHOLDS)
    gen = mm.generation()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        gs = torch.full((N_SMALL,), -7.0, dtype=torch.float32, device="cuda")
        is_ = torch.full((N_SMALL,), -7.0, dtype=torch.float32, device="cuda")
        gr = torch.full((N_SMALL,), -7, dtype=torch.int32, device="cuda")
        ir = torch.full((N_SMALL,), -7, dtype=torch.int32, device="cuda")
        counts = torch.full((len(THRESHOLDS), 2), -7, dtype=torch.int64, device="cuda")
        stats = torch.full((5,), -7, dtype=torch.int64, device="cuda")
        mm.separation_dev(gs.data_ptr(), gr.data_ptr(), is_.data_ptr(), ir.data_ptr(), THRESHOLDS, counts.data_ptr(), stats.data_ptr(), side.cuda_stream)
    side.synchronize()
    for d, h in zip((gs, gr, is_, ir, counts), host[:5]):
        assert np.array_equal(d.cpu().numpy(), h)
    assert stats.cpu().numpy().tolist() == stat_list(frt, host[5])
    # every output is optional
    stats.fill_(-7)
    torch.cuda.synchronize()
    mm.separation_dev(0, 0, 0, 0, None, 0, stats.data_ptr())
    torch.cuda.synchronize()
    assert stats.cpu().numpy().tolist() == stat_list(frt, host[5])
    mm.separation_dev(0, 0, 0, 0)
    torch.cuda.synchronize()
    assert mm.generation() == gen and mm.labels_info() == (len(set(labels.tolist())), int(np.bincount(labels).max()))
    after = mm.topk_labels(probe, 3)
    for x, y in zip(before, after):
        assert np.array_equal(x, y)
    mm.close()


def test_error_paths_and_the_empty_gallery(frt):
    import torch
    rows, labels, _ = planted_rows(512)
    mm = load(frt, rows, None)
    stats = torch.full((5,), -7, dtype=torch.int64, device="cuda")
    with pytest.raises(frt.FrtError) as e:
        mm.separation()
    assert e.value.code == frt.FRT_ERR_INVALID and "labels" in str(e.value)
    with pytest.raises(frt.FrtError) as e:
        mm.separation_dev(0, 0, 0, 0, None, 0, stats.data_ptr())
    assert e.value.code == frt.FRT_ERR_INVALID
    mm.set_labels(labels)
    for bad in ([0.5, np.nan], [np.inf], np.zeros(65)):
        with pytest.raises(frt.FrtError) as e:
            mm.separation(bad)
        assert e.value.code == frt.FRT_ERR_INVALID
    assert mm.separation(np.zeros(64))[4].shape == (64, 2)
    mm.setRowOffset(128)
    with pytest.raises(frt.FrtError) as e:
        mm.separation()
    assert e.value.code == frt.FRT_ERR_INVALID and "row offset" in str(e.value)
    with pytest.raises(frt.FrtError) as e:
        mm.separation_dev(0, 0, 0, 0, None, 0, stats.data_ptr())
    assert e.value.code == frt.FRT_ERR_INVALID and "row offset" in str(e.value)
    torch.cuda.synchronize()
    assert (stats == -7).all()  # a refused call writes nothing
    mm.setRowOffset(0)
    mm.galleryBegin(0, 512)
    mm.galleryCommit()
    got = mm.separation(THRESHOLDS)
    assert all(a.shape == (0,) for a in got[:4]) and not got[4].any() and stat_list(frt, got[5]) == [0] * 5
    counts = torch.full((len(THRESHOLDS), 2), -7, dtype=torch.int64, device="cuda")
    mm.separation_dev(0, 0, 0, 0, THRESHOLDS, counts.data_ptr(), stats.data_ptr())
    torch.cuda.synchronize()
    assert stats.cpu().numpy().tolist() == [0] * 5 and not counts.cpu().numpy().any()
    mm.close()
