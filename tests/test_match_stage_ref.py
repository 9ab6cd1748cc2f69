"""The CPU-side conditions of the matcher's stage checks (tests/match_stage_ref.py): the layout restatements against a brute-force loop, the
premises of the exact classes, and the screening theorem on the reference's own shadow - before a GPU is involved.  No GPU."""
import numpy as np
import pytest

import match_stage_ref as R


@pytest.mark.parametrize("D", [64, 512])
def test_g16_layout_restatement_matches_the_documented_formula(D):
    rows = np.arange(128 * D, dtype=np.float32).reshape(128, D) % 2039
    flat = R.to_g16(rows[:100].astype(np.float16))
    for g in range(128):
        for k in range(D):
            assert flat[R.g16_index(g, k, D)] == (rows[g, k] if g < 100 else 0)
    assert np.array_equal(R.from_g16(flat, D)[:100], rows[:100])


def test_g8_layout_restatement_matches_the_documented_formula():
    rows = (np.arange(256 * 512).reshape(256, 512) * 7 % 251).astype(np.uint8)
    flat = R.to_g8(rows[:200])
    for g in (0, 1, 31, 32, 63, 97, 127, 128, 199, 200, 255):
        for k in range(512):
            assert flat[R.g8_offset(g, k)] == (rows[g, k] if g < 200 else 0x80)
    assert sorted(R.g8_offset(g, k) for g in range(128) for k in range(512)) == list(range(128 * 512))
    assert np.array_equal(R.from_g8(flat)[:200], rows[:200])


def test_shadow_reference_and_its_bounds():
    g = R.shadow_rows(R.N_SMALL, "a", False)
    b8, sc, q = R.shadow8_reference(g)
    assert b8[5, 3] == 255 and (np.delete(b8[5], 3) == 128).all() and sc[5] == np.float32(1) / np.float32(127)
    assert (b8[40] == 128).all() and sc[40] == 0
    assert b8[130].min() == 1 and b8[130].max() < 255                         # the largest element is negative
    v = g[200].astype(np.float64) * 128
    assert np.array_equal(v - np.floor(v), np.where(np.arange(512) == 7, 0, 0.5))  # every other element lands on .5
    assert (q[200] % 2 == 0)[np.arange(512) != 7].all()                     # ... and went to the even neighbour
    b = R.shadow8_bounds(g)                                                   # asserts that soundness follows from the derivation
    assert b["e_true"] <= b["e_lo"] <= b["e_hi"] <= b["e_true"] * 1.0001
    bad = R.shadow_rows(R.N_SMALL, "b", True)
    b8, sc, _ = R.shadow8_reference(bad)
    nf = ~np.isfinite(bad).all(1)
    assert nf.sum() == 3 and (b8[nf] == 128).all() and (sc[nf] == 0).all()


@pytest.mark.parametrize("kind,D", [("i8", 512), ("f16", 64), ("f16", 128), ("f16", 256), ("f16", 512)])
def test_coarse_class_a_premises(kind, D):
    R.coarse_a_conditions(kind, D)


@pytest.mark.parametrize("kind,D", [("i8", 512), ("f16", 512), ("f16", 64)])
def test_realistic_inputs_satisfy_the_screening_bound(kind, D):
    """|S~ - S| <= ||q|| (c_round max||g|| + 1.02 E) with S~ the exact similarity of the reference's own shadow and E, max||g|| the float64 values"""
    g, q, near = R.realistic()
    S = R.realistic_S(D)
    E = R.shadow8_bounds(g)["e_true"] if kind == "i8" else 0.0
    d = R.deltas(q[:, :D], kind == "i8", R.norm_bounds(g[:, :D])["gmax_true"], E)
    ratio = np.abs(R.shadow_exact_S(kind, D) - S) / d[:, None]
    print("%s D=%d: max(|S~ - S| / delta) = %.4f" % (kind, D, ratio.max()))
    assert ratio.max() <= 1
    if kind == "i8":   # the aligned rows: the true best row's coarse value is further below the four rows tied behind it than a bound with 0.5 E allows
        _, sc, q8 = R.shadow8_reference(g[[R.ADV_A] + list(R.ADV_B)])
        assert (np.abs(q8[:, 2:]) == 40).all() and S[R.ADV_Q].argmax() == R.ADV_A and sorted(np.argsort(-S[R.ADV_Q])[1:5]) == sorted(R.ADV_B)
        assert 0 < S[R.ADV_Q, R.ADV_A] - S[R.ADV_Q, R.ADV_B[0]] < 1e-4
        St = R.shadow_exact_S(kind, D)[R.ADV_Q]
        gap = St[R.ADV_B[0]] - St[R.ADV_A]
        half = R.deltas(q[R.ADV_Q:R.ADV_Q + 1], True, R.norm_bounds(g)["gmax_true"], 0.5 / R.F1_02 * E)[0]
        print("aligned rows: coarse gap %.5f, 2 delta %.5f, 2 delta with 0.5 E %.5f" % (gap, 2 * d[R.ADV_Q], 2 * half))
        assert 2 * half < gap <= 2 * d[R.ADV_Q]
    if D == 512:   # the near-ties are near-ties: 40 rows in 40 tiles within 1e-4 of the query's best similarity
        for i in range(R.NEAR_Q):
            assert len(set(near[i] // 128)) == R.NEAR_ROWS and (S[i, near[i]] >= S[i].max() - 1e-4).all()


@pytest.mark.parametrize("kind", ["i8", "f16"])
@pytest.mark.parametrize("k", [1, 4])
def test_chained_reference_lists_fit_the_pair_list(kind, k):
    """The selection of the reference alone (coarse entries of its own shadow, its own E) stays below pair_cap / 64 per sub-list, so a pass of
    the chained GPU case cannot come from the overflow fallback; and it lists every row at or above the k-th best."""
    g, q, _ = R.realistic()
    F, pair_cap = 33, 8192
    S = R.realistic_S(512)[:F]
    tm = R.block_max(R.shadow_exact_S(kind, 512)[:F]).astype(np.float32)
    E = R.shadow8_bounds(g)["e_hi"] if kind == "i8" else 0.0
    gmax = np.sqrt(R.norm_bounds(g)["n2_hi"])
    kth = R.kth_reference(tm.reshape(F, -1), k) if k > 1 else None
    ovf, counts, sets, _, _ = R.select_reference(tm, R.wg_maxima(tm), q[:F], gmax, E, kind == "i8", pair_cap, kth, strict=False)
    print("%s k=%d: %d pairs, largest sub-list %d of %d" % (kind, k, counts.sum(), counts.max(), pair_cap // 64))
    assert not ovf and counts.max() < pair_cap // R.SEL_SUB
    listed = {(qq, t * 4 + b) for s in sets for qq, t, m in s for b in range(4) if m >> b & 1}
    kbest = np.sort(S, axis=1)[:, -k]
    assert all((int(qq), int(r) // 32) in listed for qq, r in np.argwhere(S >= kbest[:, None]))


def test_kth_reference():
    for n_ent in R.KTH_ENT:
        for k in R.KTH_K:
            rows = R.kth_rows(n_ent, k)
            want = R.kth_reference(rows, k)
            assert want[4] == -np.inf and (n_ent >= k or (want == -np.inf).all())
            if n_ent >= 16:
                assert want[2] == 7.5
            # row 1: its largest entries are 10, 11, ... on the indices 5, 261, ... (= 5 mod 256: one thread's list), as many as n_ent has, 16 at the most;
            # all 16 of them exist from n_ent = 5 + 15 * 256 + 1 on (only 4 * 1031 here)
            on5 = np.arange(5, n_ent, 256)[:16]
            assert len(on5) == (16 if n_ent >= 5 + 15 * 256 + 1 else -(-(n_ent - 5) // 256) if n_ent > 5 else 0)
            top = np.argsort(-rows[1], kind="stable")[:len(on5)]
            assert sorted(top) == list(on5) and (top % 256 == 5).all()
            if len(on5) >= k:
                assert want[1] == 10.0 + len(on5) - k
            if n_ent > k:
                assert np.sort(rows[5])[::-1][k] == want[5]


@pytest.mark.parametrize("variant", R.SELECT_VARIANTS)
def test_selection_inputs_keep_clear_of_the_threshold(variant):
    d = R.select_inputs(variant)
    ovf, counts, sets, thr, slack = R.select_case_reference(d)   # asserts: no entry within the slack of thr
    sub_cap = d["pair_cap"] // R.SEL_SUB
    assert ovf == (variant == "overflow")
    if variant == "overflow":
        assert sorted(counts)[-2:] == [sub_cap, sub_cap + 1] or (sorted(counts)[-1] == sub_cap + 1 and sorted(counts)[-2] <= sub_cap)
        assert (counts > sub_cap).sum() == 1
    fin = np.isfinite(thr)
    e = d["tilemax"].astype(np.float64)
    for q in np.nonzero(fin)[0]:   # entries just inside and just outside: within 8 slack on both sides
        near = np.abs(e[q, d["tile_min"]:] - thr[q]) <= 8 * slack[q]
        assert (e[q, d["tile_min"]:][near] > thr[q]).any() and (e[q, d["tile_min"]:][near] < thr[q]).any(), (variant, q)
    if variant in ("nonfinite", "qnorm", "gmax"):
        every = {"nonfinite": (1, 2, 3), "qnorm": (3,), "gmax": range(5)}[variant]
        for q in every:
            assert sum(1 for s in sets for qq, t, m in s if qq == q and m == 15) == d["T"]
    if variant == "abs":
        assert all(t >= d["tile_min"] for s in sets for _, t, _ in s) and any((e[:, :d["tile_min"]] > thr[:, None, None]).ravel())
    segs = {(s % R.SEL_SEG) for s, members in enumerate(sets) if members}
    assert len(segs) == (R.SEL_SEG if variant != "abs" else R.SEL_SEG - 3) and {s // R.SEL_SEG for s, m in enumerate(sets) if m} == {0, 1, 2, 3}


def test_rerank_lists_exercise_what_they_claim():
    R.rerank_conditions()
