"""The restatement of the exact scan (tests/match_exact_ref.py) held to something outside itself, and the conditions its cases claim, asserted on
the references.  CPU only: no device call."""
import ctypes

import numpy as np
import pytest

import match_exact_ref as X
import match_stage_ref as R

F32 = np.float32


def _libm_fmaf():
    f = ctypes.CDLL("libm.so.6").fmaf
    f.restype = ctypes.c_float
    f.argtypes = [ctypes.c_float] * 3
    return lambda a, b, c: np.array([f(float(x), float(y), float(z)) for x, y, z in zip(a, b, c)], F32)


def _same_bits(a, b):
    return np.array_equal(np.asarray(a, F32).view(np.uint32), np.asarray(b, F32).view(np.uint32))


def test_fmaf32_is_libm_fmaf_on_random_triples():
    r = np.random.default_rng(20)
    n = 120000
    a = (r.standard_normal(n) * 2.0 ** r.integers(-20, 20, n)).astype(F32)
    b = (r.standard_normal(n) * 2.0 ** r.integers(-20, 20, n)).astype(F32)
    c = (r.standard_normal(n) * 2.0 ** r.integers(-40, 40, n)).astype(F32)
    # a third of them cancel almost completely, a third have an addend close to the product's last bits
    c[::3] = -(a[::3].astype(np.float64) * b[::3]).astype(F32)
    c[1::3] = ((a[1::3].astype(np.float64) * b[1::3]) * 2.0 ** r.integers(20, 30, len(c[1::3]))).astype(F32)
    want = _libm_fmaf()(a, b, c)
    assert _same_bits(X.fmaf32(a, b, c), want)
    assert _same_bits(X._fma_exact(a.astype(np.float64), b.astype(np.float64), c.astype(np.float64)), want)   # the slow path on its own


def planted_double_rounding():
    """a b = 64 (1 - 2^-46) (and its negative): next to c = +-(2^30 + 128 j) the exact sum lies 2^-40 beside an fp32 midpoint, the float64 sum on it"""
    a, b = F32(8 * (1 + 2.0 ** -23)), F32(8 * (1 - 2.0 ** -23))
    t = [(a, b, F32(2.0 ** 30)), (a, b, F32(2.0 ** 30 + 128)), (a, b, F32(-(2.0 ** 30) - 128)), (a, b, F32(-(2.0 ** 30) - 256)),
         (-a, b, F32(2.0 ** 30 + 128)), (-a, b, F32(2.0 ** 30 + 256)), (-a, b, F32(-(2.0 ** 30))), (-a, b, F32(-(2.0 ** 30) - 128)),
         (F32(1 + 2.0 ** -23), F32(1 - 2.0 ** -23), F32(2.0 ** 24 + 2)), (F32(1 + 2.0 ** -23), F32(1 - 2.0 ** -23), F32(2.0 ** 24))]
    return tuple(np.array(x, F32) for x in zip(*t))


def test_fmaf32_on_double_rounding_triples():
    a, b, c = planted_double_rounding()
    want = _libm_fmaf()(a, b, c)
    assert _same_bits(X.fmaf32(a, b, c), want)
    naive = X.fmaf32_naive(a, b, c)
    assert (naive.view(np.uint32) != want.view(np.uint32)).any(), "no planted triple makes the twice-rounded float64 sum wrong: the correction is not exercised"


def test_chain_is_exact_row_dot_statement_by_statement():
    g, q = X.chain_data(96, False)
    assert _same_bits(X.chain_S(q[:3], g[:5]), X.exact_row_dot_literal(q[:3], g[:5]))
    g, q = X.chain_data(32, True)
    assert _same_bits(X.chain_S(q[:3], g[:5]), X.exact_row_dot_literal(q[:3], g[:5]))


@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("D", [32, 96, 512])
def test_chain_within_gamma_of_float64_and_discriminating(D, half):
    g, q, S, s64, sabs = X.reference("C", D, half)
    assert np.abs(S.astype(np.float64) - s64).max() > 0
    assert (np.abs(S.astype(np.float64) - s64) <= X.gamma(D) * sabs).all()
    # the case can tell the chain from another order and from float64: some query's float64 winner is not the chain's winner ...
    win64, win = np.argmax(s64, axis=1), X.ranking(S, 1)[0][:, 0]
    assert (win64 != win).any(), "float64 and the chain agree on every winner"
    # ... and the plain order k = 0, 1, 2, ... gives other bits for some winner's similarity
    if D == 96:
        acc = np.zeros_like(S)
        gf = g.astype(F32)
        for k in range(D):
            acc = X.fmaf32(gf[None, :, k], q[:, None, k], acc)
        assert (acc[np.arange(len(q)), win].view(np.uint32) != S[np.arange(len(q)), win].view(np.uint32)).any()
        assert not np.array_equal(X.ranking(acc, 5)[0], X.ranking(S, 5)[0])


@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("D", [32, 96, 512])
def test_class_a_conditions(D, half):
    g, q, S, s64, _ = X.reference("A", D, half)
    N = len(g)
    p = list(X.PLANTED)
    live = ~np.isnan(s64[0])
    assert len({s64[0, i] for i in p}) == 1 and s64[0, 2] == s64[0, live].max() and (s64[0, live] == s64[0, 2]).sum() == len(p)
    # rows 2 and 5: one 32-row block, the two lane halves of the epilogue (row r of a block is held by half (r >> 2) & 1); 40: another wave;
    # 198: another tile, i.e. another workgroup; 393: tile 3, which workgroup 0 walks behind tile 0 at partial_blocks = 3
    assert 2 // 32 == 5 // 32 and (2 >> 2) & 1 == 0 and (5 >> 2) & 1 == 1 and 40 // 32 == 1 and 198 // 128 == 1 and 393 // 128 == 3 and 3 % 3 == 0
    assert X.ranking(S, 1)[0][0, 0] == 2 and X.ranking(S, 5)[0][0].tolist() == p and X.ranking(S, 5, 1000)[0][0].tolist() == [i + 1000 for i in p]
    assert len(set(X.ranking(S, 5)[1][0].view(np.uint32).tolist())) == 1
    # the NaN row never wins and is NaN in its full-matrix column; the all-zero query sees +0.0 everywhere and takes the first live index
    assert np.isnan(S[:, X.NAN_ROW]).all() and not np.isnan(np.delete(S, X.NAN_ROW, 1)).any() and not (X.ranking(S, 5)[0] == X.NAN_ROW).any()
    assert not np.delete(S[X.ZERO_Q], X.NAN_ROW).view(np.uint32).any() and X.ranking(S, 5)[0][X.ZERO_Q].tolist() == [0, 1, 2, 3, 4]
    # excluded: identity 2 owns rows 2, 5 and 198: without it row 40 wins; some queries exclude nothing
    lab = X.labels_of(N, "excl")
    ex = X.excluded_of(S, lab)
    assert lab[2] == lab[5] == lab[198] == ex[0] and lab[40] != ex[0] and X.ranking(S, 1, 0, lab, ex)[0][0, 0] == 40
    assert (ex == -1).any() and (ex[:32] == -1).any() and (X.ranking(S, 1, 0, lab, ex)[0][:, 0] != X.ranking(S, 1)[0][:, 0]).sum() >= (ex >= 0).sum() - 1
    # identities: % 7 - rows 40 and 198 carry taken labels, row 393 is third; 3 labels - two empty slots for every query
    l7, i7, _ = X.ranking(S, 5, 0, X.labels_of(N, "seven"), identities=True)
    assert i7[0, :3].tolist() == [2, 5, 393] and l7[0, :3].tolist() == [2, 5, 1] and all(len(set(r)) == 5 for r in l7.tolist())
    l3, i3, s3 = X.ranking(S, 5, 1000, X.labels_of(N, "three"), identities=True)
    assert i3[0, :3].tolist() == [1002, 1040, 1198] and (l3[:, 3:] == -1).all() and (i3[:, 3:] == -1).all() and np.isneginf(s3[:, 3:]).all() and (l3[:, :3] >= 0).all()


def test_ranking_agrees_with_the_stage_reference_and_the_merge_definition():
    import test_identity_merge
    g, q, S, _, _ = X.reference("A", 32, False)
    i, s = X.ranking(S[:8], 4, 7)
    wi, ws = R.exact_ranking(S[:8].astype(np.float64), 4, 7)
    assert np.array_equal(i, wi) and _same_bits(s, ws)
    # identities: the whole gallery as one shard's complete list, merged by the definition of the identity merge
    N = S.shape[1]
    lab = X.labels_of(N, "seven")
    S8 = np.delete(S[:8], X.NAN_ROW, 1)
    rows = np.delete(np.arange(N), X.NAN_ROW)
    order = np.argsort(-S8.astype(np.float64), axis=1, kind="stable")
    idx = rows[order][None].astype(np.int32)
    want = test_identity_merge.reference_merge(lab[idx], idx, np.take_along_axis(S8, order, 1)[None])
    got = X.ranking(S[:8], 5, 0, lab, identities=True)
    for a, b in zip(got, (w[:, :5] for w in want)):
        assert np.array_equal(a, b)


def test_small_galleries_run_out_of_rows():
    for N in (1, 2):
        g, q, S, _, _ = X.reference("C", 32, True, N)
        i, s = X.ranking(S, 3, 1000)
        assert (i[:, N:] == -1).all() and np.isneginf(s[:, N:]).all() and (i[:, :N] >= 1000).all()


def test_merge_lists_hold_what_they_claim():
    seen = {"tie": 0, "empty_slot": 0, "empty_query": 0, "few_labels": 0}
    for labelled in (False, True):
        for shards, n, k in X.MERGE_SHAPES:
            lab, idx, sim = X.merge_lists(shards, n, k, labelled)
            assert idx.shape == (shards, n, k)
            seen["empty_slot"] += int(((idx < 0).any(2) & (idx >= 0).any(2)).any())
            seen["empty_query"] += int((idx < 0).all((0, 2)).any())
            if shards > 1:
                for qq in range(n):
                    a, b = sim[0, qq][idx[0, qq] >= 0], sim[1:, qq][idx[1:, qq] >= 0]
                    seen["tie"] += int(np.isin(a, b).any())
            if labelled:
                want = X.merge_reference(lab, idx, sim)
                seen["few_labels"] += int(((want[0] < 0).any(1) & ((idx >= 0).sum((0, 2)) >= k)).any())
    assert all(v > 10 for v in seen.values()), seen


def test_case_lists_reach_every_instantiation():
    """(launcher, NQ by the launchers' selection, row type is every case's second axis): top-1 NQ 1 / 2 / 4, full NQ 1 / 4, EXCL NQ 1 / 4, EXCL + LAB
    NQ 1 / 4; partial_blocks 3, 4 and 6 and row_offset 1000 for every partial-writing launcher"""
    nq = lambda op, F: 1 if F <= 32 else (2 if op == "top1" and F <= 64 else 4)
    for D in (512, 96, 32):
        L = X.launches(D)
        have = {(op, nq(op, F)) for op, F, *_ in L}
        assert have >= {("top1", 1), ("top1", 2), ("top1", 4), ("full", 4), ("topk", 1), ("topk", 4), ("topk_labels", 1), ("topk_labels", 4), ("top1_excl", 1),
                        ("top1_excl", 4)}, D
    L = X.launches(512)
    assert ("full", 1) in {(op, nq(op, F)) for op, F, *_ in L}
    for op in ("top1", "topk", "topk_labels"):
        assert {pb for o, F, pb, *_ in L if o == op} >= {3, 4, 6} and {off for o, F, pb, off, *_ in L if o == op} == {0, 1000}, op
    assert {F for op, F, *_ in L if op == "top1"} == {1, 32, 33, 64, 65, 130}
    assert {k for op, F, pb, off, k, _ in L if op == "topk"} == {1, 5}
    assert any(op == "topk" and k == 3 for op, F, pb, off, k, _ in X.small_launches(2))
