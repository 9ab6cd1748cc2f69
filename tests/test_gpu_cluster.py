"""frt_matcher_cluster (include/frt.h): single-linkage clustering of the gallery at a similarity threshold, on the
device, against the numpy oracle of tests/cluster_ref.py.

Galleries are persons: every row is its person's unit centre plus a unit noise direction times SPREAD, re-normalised, so two photos of one
person have a similarity near 1 / (1 + SPREAD^2) = 0.8 and photos of different persons one near 0.  Every comparison is exact (==): before
any GPU call each test asserts on the CPU that no pair's oracle similarity lies within MARGIN = 1e-4 of the threshold.  The worst-case
rounding of a 512-term fp32 dot product of unit vectors is 512 * 2^-24 = 3.1e-5, so inside that margin the float64 oracle, the blocked
float32 sgemm oracle and the device's fmaf chain all put every pair on the same side of t.  Pairs below FLOOR = 0.3 are never listed by the
sgemm oracle: they are 0.2 away from every threshold used here that is not derived from a listed pair.
The oracles are computed once per gallery and kept unchanged."""
import numpy as np
import pytest

import cluster_ref

pytestmark = pytest.mark.gpu

T = np.float32(0.5)
MARGIN = 1e-4
FLOOR = 0.3
SPREAD = 0.5
N_SMALL = 1000
N_BIG = 32768 + 200                 # just above SCREEN_MIN_ROWS (frt_matcher.hpp); the last 128-row tile holds 72 rows
SPECIAL = (5, 20_000, N_BIG - 1)    # one person, placed by hand: first chunk, a middle one, the partial last tile
CHAIN = (130, 9_000, 31_000)        # a - b - c in three different 128-row chunks: S(a, b), S(b, c) >= t > S(a, c)
# 385 tiles: chunks 0 .. 129 have at least FRT_MATCH_COARSE_WG = 256 tiles from their own on and scan from there (the triangular walk), the
# chunks behind them scan from tile 0.  N_BIG's 258 tiles leave that to chunks 0 .. 2 only.
N_TRI = 49_152 + 100
SPECIAL_TRI = (5, 30_000, N_TRI - 1)
CHAIN_TRI = (130, 20_000, 45_000)   # a in a chunk that scans from its own tile, c in one that scans from tile 0
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
    return r.astype(np.float16).astype(np.float32) if fp16 else r


def smallest_member(person):
    """true person ids -> the label the clustering gives a person whose rows form one component: its smallest row"""
    first = {}
    for r, p in enumerate(person.tolist()):
        first.setdefault(p, r)
    return np.array([first[p] for p in person.tolist()], np.int32)


def small_case(D, fp16):
    """N_SMALL rows, 1 to 6 per person, shuffled; the float64 oracle at T.  The first seed whose gallery keeps every pair MARGIN away from T."""
    key = ("small", D, fp16)
    if key not in _CACHE:
        for seed in range(100 + D, 200 + D):
            rng = np.random.Generator(np.random.PCG64(seed))
            counts = []
            while sum(counts) < N_SMALL:
                counts.append(min(1 + len(counts) % 6, N_SMALL - sum(counts)))
            rows, person = person_rows(rng, counts, D)
            perm = rng.permutation(N_SMALL)
            rows, person = np.ascontiguousarray(rows[perm], np.float32), person[perm]
            r64 = stored32(rows, fp16).astype(np.float64)
            s = (r64 @ r64.T)[np.triu_indices(N_SMALL, 1)]
            if np.abs(s - float(T)).min() > MARGIN:
                break
        else:
            raise AssertionError("no seed keeps the margin")
        _CACHE[key] = (rows, person, cluster_ref.cluster_rows(stored32(rows, fp16), T, np.float64))
    return _CACHE[key]


def big_rows(N_BIG=N_BIG, SPECIAL=SPECIAL, CHAIN=CHAIN):
    """A screened gallery: N_BIG x 512, 1 to 6 rows per person, shuffled over the whole gallery (members of a person lie in different
    chunks and tiles), one person at SPECIAL, the chain at CHAIN."""
    key = ("big_rows", N_BIG)
    if key not in _CACHE:
        rng = np.random.Generator(np.random.PCG64(2024 + N_BIG - 32_968))
        counts = []
        while sum(counts) < N_BIG - 6:
            counts.append(min(1 + len(counts) % 6, N_BIG - 6 - sum(counts)))
        body, body_person = person_rows(rng, counts, 512)
        sp, _ = person_rows(rng, [3], 512)
        e = np.linalg.qr(rng.standard_normal((512, 2)))[0].T
        chain = np.array([e[0], (e[0] + e[1]) / np.sqrt(2.0), e[1]])  # S(a, b) = S(b, c) = 0.707, S(a, c) = 0
        rows = np.empty((N_BIG, 512), np.float32)
        person = np.empty(N_BIG, np.int64)
        fixed = np.array(SPECIAL + CHAIN)
        free = np.setdiff1d(np.arange(N_BIG), fixed)
        free = free[rng.permutation(len(free))]
        rows[free], person[free] = body, body_person
        rows[list(SPECIAL)], person[list(SPECIAL)] = sp, len(counts)
        rows[list(CHAIN)], person[list(CHAIN)] = chain, len(counts) + 1
        _CACHE[key] = (rows, person)
    return _CACHE[key]


def tri_case():
    """the N_TRI gallery, fp32 storage -> rows, person, the oracle result at T"""
    if "tri" not in _CACHE:
        rows, person = big_rows(N_TRI, SPECIAL_TRI, CHAIN_TRI)
        i, j, s = cluster_ref.high_pairs(rows, FLOOR)
        assert np.abs(s - T).min() > MARGIN
        _CACHE["tri"] = (rows, person, cluster_ref.from_edges(N_TRI, i[s >= T], j[s >= T]))
    return _CACHE["tri"]


def big_case(fp16):
    """-> rows, person, (i, j, s) = every pair of the stored rows with a float32 sgemm similarity >= FLOOR, the oracle result at T"""
    key = ("big", fp16)
    if key not in _CACHE:
        rows, person = big_rows()
        i, j, s = cluster_ref.high_pairs(stored32(rows, fp16), FLOOR)
        assert np.abs(s - T).min() > MARGIN
        _CACHE[key] = (rows, person, (i, j, s), cluster_ref.from_edges(N_BIG, i[s >= T], j[s >= T]))
    return _CACHE[key]


def load(frt, rows, fp16=False, screening=True):
    mm = frt.MatMul(0)
    mm.setScreening(screening)
    mm.setStorage(fp16)
    mm.init(rows)
    mm.setStorage(False)
    return mm


def check(got, want, what=""):
    labels, stats = got
    print("%s clusters %d edges %d screened chunks %d dense chunks %d (oracle: %d clusters, %d edges)"
          % (what, stats["clusters"], stats["edges"], stats["screened_chunks"], stats["dense_chunks"], want[1], want[2]))
    assert labels.dtype == np.int32 and np.array_equal(labels, want[0])
    assert (stats["clusters"], stats["edges"]) == (want[1], want[2])
    assert stats["screened_chunks"] + stats["dense_chunks"] == (len(labels) + 127) // 128


# ---------------------------------------------------------------------------------------------------------------- 1. dense path
@pytest.mark.parametrize("fp16", [False, True], ids=["fp32", "fp16"])
@pytest.mark.parametrize("D", [64, 512])
def test_dense_path_equals_the_float64_oracle(frt, D, fp16):
    rows, person, want = small_case(D, fp16)
    if D == 512:  # (at 64 columns strangers can look alike; at 512 the components are the persons)
        assert np.array_equal(want[0], smallest_member(person))
    mm = load(frt, rows, fp16)
    got = mm.cluster(T)
    mm.close()
    check(got, want)
    assert got[1]["screened_chunks"] == 0


# ---------------------------------------------------------------------------------------------------------------- 2. + 3. screened path
@pytest.mark.parametrize("fp16", [False, True], ids=["fp32", "fp16"])
def test_screened_path_equals_the_sgemm_oracle_and_the_unscreened_run(frt, fp16):
    rows, person, _, want = big_case(fp16)
    assert np.array_equal(want[0], smallest_member(person))  # the persons, the hand-placed one and the chain come out whole
    assert want[0][list(SPECIAL)].tolist() == [5, 5, 5]
    mm = load(frt, rows, fp16)
    got = mm.cluster(T)
    check(got, want, "screened:")
    assert got[1]["screened_chunks"] > 0
    mm.setScreening(False)
    exact = mm.cluster(T)
    mm.close()
    check(exact, want, "screening off:")
    assert exact[1]["screened_chunks"] == 0 and np.array_equal(exact[0], got[0]) and exact[1]["edges"] == got[1]["edges"]


def test_single_linkage_chains_across_chunks(frt):
    rows, _, _, want = big_case(False)
    a, b, c = CHAIN
    r = rows.astype(np.float64)
    assert len({a // 128, b // 128, c // 128}) == 3
    assert r[a] @ r[b] >= T + MARGIN and r[b] @ r[c] >= T + MARGIN and r[a] @ r[c] < T - MARGIN
    assert want[0][[a, b, c]].tolist() == [a, a, a]
    mm = load(frt, rows)
    labels, stats = mm.cluster(T)
    mm.close()
    assert labels[[a, b, c]].tolist() == [a, a, a] and stats["screened_chunks"] > 0


def test_triangular_walk_equals_the_oracle_and_the_scan_from_tile_0(frt, monkeypatch):
    """Chunk c joins rows j > i only, so its coarse scan begins at tile c while at least FRT_MATCH_COARSE_WG tiles are left.
    The profiling brackets carry the rows each chunk's coarse scan covered: that is how the test sees which walk ran."""
    rows, person, want = tri_case()
    assert np.array_equal(want[0], smallest_member(person))
    a, b, c = CHAIN_TRI
    assert want[0][[a, b, c]].tolist() == [a, a, a] and want[0][list(SPECIAL_TRI)].tolist() == [5, 5, 5]
    chunks, tiles = (N_TRI + 127) // 128, (N_TRI + 127) // 128
    mm = load(frt, rows)

    def scanned_rows():
        frt.profile_enable(3)
        got = mm.cluster(T)
        names, _, work = frt.profile_collect()
        frt.profile_enable(0)
        per_chunk = [w / (2.0 * 512 * min(128, N_TRI - 128 * k)) for k, w in enumerate(w for n, w in zip(names, work) if n == "cluster_coarse")]
        return got, per_chunk

    got, covered = scanned_rows()
    check(got, want, "triangular:")
    assert got[1]["screened_chunks"] == chunks
    assert covered == [N_TRI - 128 * k if tiles - k >= 256 else N_TRI for k in range(chunks)] and covered[129] < N_TRI == covered[130]
    monkeypatch.setenv("FRT_CLUSTER_FULL_WALK", "1")
    full, covered = scanned_rows()
    monkeypatch.delenv("FRT_CLUSTER_FULL_WALK")
    check(full, want, "every chunk from tile 0:")
    assert covered == [N_TRI] * chunks
    mm.close()
    # fp16 storage scans the stored rows themselves from the chunk's tile on: against the exact dense pass over the same rows
    mm = load(frt, rows, fp16=True)
    screened = mm.cluster(T)
    mm.setScreening(False)
    dense = mm.cluster(T)
    mm.close()
    assert screened[1]["screened_chunks"] == chunks and dense[1]["dense_chunks"] == chunks
    assert np.array_equal(screened[0], dense[0]) and (screened[1]["clusters"], screened[1]["edges"]) == (dense[1]["clusters"], dense[1]["edges"])


# ---------------------------------------------------------------------------------------------------------------- 4. >= on the product's own bits
def lonely_pair(i, j, s):
    """a listed pair whose two rows take part in no other listed pair: at a threshold of its similarity it is joined or not by its own edge"""
    deg = np.bincount(np.concatenate([i, j]))
    for k in np.nonzero((deg[i] == 1) & (deg[j] == 1))[0].tolist():
        if np.abs(np.delete(s, k) - s[k]).min() > 3 * MARGIN:  # (the product's own value lies within MARGIN of the oracle's)
            return k
    raise AssertionError("no such pair")


@pytest.mark.parametrize("which", ["dense", "screened"])
def test_equality_joins_and_the_next_float_does_not(frt, which):
    if which == "dense":
        rows = small_case(512, False)[0]
        i, j, s = cluster_ref.high_pairs(rows, FLOOR)
    else:
        rows, _, (i, j, s), _ = big_case(False)
    n = len(rows)
    k = lonely_pair(i, j, s)
    a, b = int(i[k]), int(j[k])
    mm = load(frt, rows)
    own = np.float32(mm.calculate(rows[a:a + 1])[0, b])  # S(a, b) as the product computes it
    others = np.delete(s, k)
    assert abs(float(own) - float(s[k])) < MARGIN and np.abs(others - own).min() > MARGIN  # no OTHER pair within the margin of the threshold
    above = others > own
    ei, ej = np.delete(i, k)[above], np.delete(j, k)[above]
    joined = mm.cluster(own)
    apart = mm.cluster(np.nextafter(own, np.float32(np.inf)))
    mm.close()
    check(joined, cluster_ref.from_edges(n, np.append(ei, a), np.append(ej, b)), "t = s:")
    check(apart, cluster_ref.from_edges(n, ei, ej), "t = next float above s:")
    assert joined[0][b] == joined[0][a] == a and apart[0][a] == a and apart[0][b] == b
    assert (joined[1]["screened_chunks"] > 0) == (which == "screened")


# ---------------------------------------------------------------------------------------------------------------- 5. overflow -> dense, still exact
def test_an_overflowing_pair_list_falls_back_and_stays_exact(frt):
    """Capacity arithmetic (frt_matcher::ensure_queries, kernels_match.hip): 128 queries -> pair_cap = max(128 * 64, 8192) = 8192 pairs in 64
    sub-lists of 128, one per (sixteenth of the tiles, query mod 4), i.e. 32 queries share a sub-list.  The gallery below has 281 tiles, so
    the last sixteenth is tiles 263 .. 280, all of them near-copies of row 5.  A chunk of 128 near-copies lists, for each of its queries, every
    one of those tiles from its own on: chunk 258 puts 32 * 18 = 576 pairs into a sub-list of 128, and so does every chunk up to number 276
    (32 * (281 - c) > 128).  If pair_cap grows past 576 * 64 this gallery no longer overflows and the last assertion says so."""
    rows, _, (i, j, s), _ = big_case(False)
    rng = np.random.Generator(np.random.PCG64(77))
    noise = rng.standard_normal((3000, 512))
    extra = rows[5].astype(np.float64) + 0.02 * noise / np.linalg.norm(noise, axis=1, keepdims=True)
    extra = (extra / np.linalg.norm(extra, axis=1, keepdims=True)).astype(np.float32)
    allrows = np.concatenate([rows, extra])
    n = len(allrows)
    assert (n + 127) // 128 == 281
    ni, nj, ns = cluster_ref.high_pairs(allrows, FLOOR, lo_rows=np.arange(N_BIG, n))
    assert np.abs(ns - T).min() > MARGIN and (ns >= T).sum() >= 3000 * 2999 // 2
    ei, ej = np.concatenate([i[s >= T], ni[ns >= T]]), np.concatenate([j[s >= T], nj[ns >= T]])
    want = cluster_ref.from_edges(n, ei, ej)
    assert (want[0][N_BIG:] == 5).all()
    mm = load(frt, allrows)
    got = mm.cluster(T)
    mm.close()
    check(got, want)
    assert got[1]["dense_chunks"] > 0 and got[1]["screened_chunks"] > 0


# ---------------------------------------------------------------------------------------------------------------- 6. non-finite rows
@pytest.mark.parametrize("which", ["dense", "screened"])
def test_a_nan_row_and_an_inf_row_are_singletons(frt, which):
    if which == "dense":
        rows = small_case(512, False)[0].copy()
        bad = (17, 640)
        i, j, s = cluster_ref.high_pairs(small_case(512, False)[0], FLOOR)
    else:
        rows, _, (i, j, s), _ = big_case(False)
        rows = rows.copy()
        bad = (1000, 25_000)
    rows[bad[0]] = np.nan
    rows[bad[1]] = np.inf  # (against rows with entries of both signs every product sum holds +inf and -inf: NaN)
    n = len(rows)
    bi, bj, bs = cluster_ref.high_pairs(rows, FLOOR, lo_rows=np.array(bad))
    assert len(bi) == 0  # the oracle: no similarity of either row reaches any threshold
    keep = ~(np.isin(i, bad) | np.isin(j, bad)) & (s >= T)
    want = cluster_ref.from_edges(n, i[keep], j[keep])
    mm = load(frt, rows)
    got = mm.cluster(T)
    mm.close()
    check(got, want)
    assert got[0][list(bad)].tolist() == list(bad)
    # one non-finite row leaves the shadow without an error bound: every query lists every tile, the pair list of nearly every chunk
    # overflows, and what this case exercises is the dense fallback behind the screen
    assert got[1]["dense_chunks"] > (n + 127) // 128 // 2


# ---------------------------------------------------------------------------------------------------------------- 7. end to end
def test_cluster_install_then_templates_equal_the_true_labels_route(frt):
    rows, person, want = small_case(512, False)
    true = smallest_member(person)
    assert np.array_equal(want[0], true)
    mm = load(frt, rows)
    labels, stats = mm.cluster(T, install=True)
    assert np.array_equal(labels, true)
    assert mm.labels_info() == (stats["clusters"], int(np.bincount(true).max())) and stats["clusters"] == len(set(true.tolist()))
    dst = frt.MatMul(0)
    got = mm.buildTemplates(dst, want_templates=True)
    ref_mm = load(frt, rows)
    ref_mm.set_labels(true)
    ref_dst = frt.MatMul(0)
    ref = ref_mm.buildTemplates(ref_dst, want_templates=True)
    for g, r in zip(got, ref):
        assert g.dtype == r.dtype and np.array_equal(g.view(np.uint32 if g.dtype == np.float32 else g.dtype), r.view(np.uint32 if r.dtype == np.float32 else r.dtype))
    q = stored32(rows[::37] + 0.01, False)
    for a, b in ((mm, ref_mm), (dst, ref_dst)):
        for x, y in zip(a.topk_labels(q, 5), b.topk_labels(q, 5)):
            assert np.array_equal(x.view(np.int32), y.view(np.int32))
    for m in (mm, dst, ref_mm, ref_dst):
        m.close()


# ---------------------------------------------------------------------------------------------------------------- 8. device form, errors
def test_device_form_equals_the_host_form_and_generation_rules(frt):
    import torch
    rows, _, want = small_case(512, False)
    mm = load(frt, rows)
    host = mm.cluster(T)
    gen = mm.generation()
    labels = torch.full((N_SMALL,), -7, dtype=torch.int32, device="cuda")
    stats = torch.full((4,), -7, dtype=torch.int64, device="cuda")
    mm.cluster_dev(T, labels.data_ptr(), stats.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(labels.cpu().numpy(), host[0]) and stats.cpu().numpy().tolist() == [host[1][k] for k in frt.MatMul.CLUSTER_STATS]
    labels.fill_(-7)
    mm.cluster_dev(T, labels.data_ptr())  # the statistics are optional
    torch.cuda.synchronize()
    assert np.array_equal(labels.cpu().numpy(), host[0])
    check(host, want)
    assert mm.generation() == gen and mm.labels_info() == (0, 0)  # nothing installed, nothing moved
    mm.cluster(T, install=True)
    assert mm.generation() == gen + 1 and mm.labels_info()[0] == want[1]
    mm.close()


def test_error_paths(frt):
    rows = small_case(512, False)[0]
    mm = load(frt, rows)
    for bad in (np.nan, np.inf, -np.inf):
        with pytest.raises(frt.FrtError) as e:
            mm.cluster(bad)
        assert e.value.code == frt.FRT_ERR_INVALID and "finite" in str(e.value)
        with pytest.raises(frt.FrtError) as e:
            mm.cluster_dev(bad, 0)
        assert e.value.code == frt.FRT_ERR_INVALID
    import torch
    stats = torch.full((4,), -7, dtype=torch.int64, device="cuda")
    labels = torch.full((N_SMALL,), -7, dtype=torch.int32, device="cuda")
    mm.setRowOffset(128)
    with pytest.raises(frt.FrtError) as e:
        mm.cluster(T)
    assert e.value.code == frt.FRT_ERR_INVALID and "row offset" in str(e.value)
    with pytest.raises(frt.FrtError) as e:
        mm.cluster_dev(T, labels.data_ptr(), stats.data_ptr())
    assert e.value.code == frt.FRT_ERR_INVALID and "row offset" in str(e.value)
    torch.cuda.synchronize()
    assert (labels == -7).all() and (stats == -7).all()  # a refused call writes nothing
    mm.setRowOffset(0)
    with pytest.raises(frt.FrtError) as e:
        mm.cluster_dev(T, 0, stats.data_ptr())  # rows, but nowhere to put their labels
    assert e.value.code == frt.FRT_ERR_INVALID
    assert mm.cluster(T)[1]["clusters"] == small_case(512, False)[2][1]
    mm.galleryBegin(0, 512)
    mm.galleryCommit()
    labels, stats = mm.cluster(T, install=True)
    assert labels.shape == (0,) and stats == dict(clusters=0, edges=0, screened_chunks=0, dense_chunks=0)
    dstats = torch.full((4,), -7, dtype=torch.int64, device="cuda")
    mm.cluster_dev(T, 0, dstats.data_ptr())  # the device form on the empty gallery: no labels to write, the statistics zeroed
    torch.cuda.synchronize()
    assert dstats.cpu().numpy().tolist() == [0, 0, 0, 0]
    mm.cluster_dev(T, 0)
    mm.close()
    fresh = frt.MatMul(0)  # no gallery at all
    assert fresh.cluster(T)[1]["clusters"] == 0
    fresh.close()


# ---------------------------------------------------------------------------------------------------------------- 9. after edits
def test_cluster_after_edits_equals_a_fresh_load(frt):
    rows, _, _, _ = big_case(False)
    rng = np.random.Generator(np.random.PCG64(31))
    gone = np.unique(np.concatenate([[5, 129, N_BIG - 1], rng.integers(N_BIG, size=300)]))
    noise = rng.standard_normal((500, 512)).astype(np.float32)
    added = rows[rng.integers(N_BIG, size=500)] + 0.3 * noise / np.linalg.norm(noise, axis=1, keepdims=True)
    added = np.ascontiguousarray(added / np.linalg.norm(added, axis=1, keepdims=True), np.float32)
    mm = load(frt, rows)
    mm.galleryRemove(gone)
    mm.galleryAdd(added)
    edited = mm.cluster(T)
    mm.close()
    result = np.concatenate([np.delete(rows, gone, axis=0), added])
    fresh_mm = load(frt, result)
    fresh = fresh_mm.cluster(T)
    fresh_mm.close()
    assert len(edited[0]) == len(result) and np.array_equal(edited[0], fresh[0])
    assert (edited[1]["clusters"], edited[1]["edges"]) == (fresh[1]["clusters"], fresh[1]["edges"])
    assert edited[1]["screened_chunks"] > 0 and edited[1]["clusters"] < len(result)
