"""Top-k over identities (frt_matcher_set_labels / topk_labels / gallery_add_labeled / frt_merge_topk_labels_dev; include/frt.h "Top-k over
IDENTITIES").  The expected lists are a NumPy function of the product's own calculate() matrix - which tests/test_gpu_match.py holds against
the oracle - and the labels: order the rows by (higher similarity, lower index), keep the first row of every label, report the first k.
Every comparison of labels, indices and similarity bits is ==."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SCREEN_MIN = 32768  # a gallery screens from here on (frt.h)


# ---------------------------------------------------------------------------------------------------------------- helpers
def expected(C, labels, k, row_offset=0):
    """the definition, on a similarity matrix [F, N] and labels [N] -> (label, idx, sim), each [F, k]"""
    F, N = C.shape
    lo = np.full((F, k), -1, np.int32)
    io = np.full((F, k), -1, np.int32)
    so = np.full((F, k), -np.inf, np.float32)
    rows = np.arange(N)
    for q in range(F):
        order = np.lexsort((rows, -C[q]))
        _, first = np.unique(labels[order], return_index=True)  # first position of every label in the row order
        sel = order[np.sort(first)[:k]]
        lo[q, :len(sel)], io[q, :len(sel)], so[q, :len(sel)] = labels[sel], sel + row_offset, C[q, sel]
    return lo, io, so


def same(got, want):
    for g, w, name in zip(got, want, ("label", "idx", "sim")):
        assert g.dtype == w.dtype and g.shape == w.shape, name
        assert np.array_equal(g, w), (name, np.argwhere(g != w)[:5], g[g != w][:5], w[g != w][:5])


def check(mm, q, labels, k, row_offset=0):
    want = expected(mm.calculate(q), labels, k, row_offset)
    got = mm.topk_labels(q, k)
    same(got, want)
    return got


@pytest.fixture(scope="module")
def mm(frt):
    m = frt.MatMul(0)
    yield m
    m.close()


@pytest.fixture(scope="module")
def fresh(frt):
    m = frt.MatMul(0)
    yield m
    m.close()


_SMALL = {}


def small(synth):
    """300 rows x 512: two full 128-row tiles and a ragged one; labels row % 75, so the four rows of an identity lie in different tiles
    (0 / 75 / 150 / 225).  Planted: row 200 duplicates row 10 under ANOTHER label (10 and 50: the tie goes to row 10, and row 200 is the best
    row of label 50), row 160 duplicates row 10 under the SAME label (160 % 75 == 10: one identity, its lower row reported)."""
    if not _SMALL:
        g = synth.make_gallery(300, seed=31)
        g[200] = g[10]
        g[160] = g[10]
        _SMALL["g"], _SMALL["labels"] = g, (np.arange(300) % 75).astype(np.int32)
    return _SMALL["g"], _SMALL["labels"]


def small_queries(synth, g, F):
    """query 0 IS an enrolled row (the planted one), then near-copies of rows of several tiles, then random directions"""
    near = synth.make_queries(g, [0, 127, 128, 255, 256, 299][:max(0, min(6, F - 1))], noise=0.05, seed=F)
    rnd = np.random.Generator(np.random.PCG64(900 + F)).standard_normal((F - 1 - len(near), g.shape[1])).astype(np.float32)
    return np.ascontiguousarray(np.concatenate([g[10:11], near, rnd]), np.float32)


def load(mm, rows, labels, fp16=False, screening=True):
    mm.setRowOffset(0)
    mm.setScreening(screening)
    mm.setStorage(fp16)
    mm.init(rows)
    mm.setStorage(False)
    if labels is not None:
        mm.set_labels(labels)


# ---------------------------------------------------------------------------------------------------------------- exact path
def exact_path(frt, synth, mm, F, k, fp16):
    g, labels = small(synth)
    q = small_queries(synth, g, F)
    load(mm, g, labels, fp16)
    assert mm.labels_info() == (75, 4)
    lab, idx, sim = check(mm, q, labels, k)
    # the planted rows: the enrolled query finds itself at the LOWEST of its three copies, and label 50's best row is the copy at 200
    assert (lab[0, 0], idx[0, 0]) == (10, 10)
    if k >= 3:
        assert (lab[0, 1], idx[0, 1]) == (50, 200) and sim[0, 1] == sim[0, 0]
    # entry 0 is the top-1 answer, bit for bit
    i1, s1 = mm.top1(q)
    assert np.array_equal(idx[:, 0], i1) and np.array_equal(sim[:, 0], s1)
    # no identity twice
    for row in lab:
        assert len(set(row.tolist())) == k


@pytest.mark.parametrize("k", [1, 3, 16])
@pytest.mark.parametrize("F", [5, 40])
def test_exact_path_matches_the_definition(frt, synth, mm, F, k):
    exact_path(frt, synth, mm, F, k, False)


def test_fp16_stored_gallery_matches_the_definition(frt, synth, mm):
    """the similarities are then those of the fp16-rounded rows - calculate() returns the same ones"""
    exact_path(frt, synth, mm, 40, 16, True)
    exact_path(frt, synth, mm, 5, 3, True)


def test_fewer_identities_than_k(frt, synth, mm):
    g, _ = small(synth)
    labels = (np.arange(300) >= 130).astype(np.int32) * 7  # two labels, 0 and 7
    q = small_queries(synth, g, 5)
    load(mm, g, labels)
    assert mm.labels_info() == (2, 170)
    lab, idx, sim = check(mm, q, labels, 3)
    assert (lab[:, 2] == -1).all() and (idx[:, 2] == -1).all() and np.isneginf(sim[:, 2]).all()
    assert (np.sort(lab[:, :2], axis=1) == [0, 7]).all()


@pytest.mark.parametrize("F", [5, 40])
def test_distinct_labels_reduce_to_the_row_topk(frt, synth, mm, F):
    g, _ = small(synth)
    q = small_queries(synth, g, F)
    labels = np.arange(300, dtype=np.int32)
    load(mm, g, labels)
    for k in (1, 5, 16):
        lab, idx, sim = mm.topk_labels(q, k)
        ri, rs = mm.topk(q, k)
        assert np.array_equal(idx, ri) and np.array_equal(sim, rs) and np.array_equal(lab, ri)


def test_labels_are_replaced_cleared_and_dropped_by_a_reload(frt, synth, mm):
    g, labels = small(synth)
    q = small_queries(synth, g, 5)
    load(mm, g, labels)
    gen = mm.generation()
    other = (np.arange(300) // 4).astype(np.int32)
    mm.set_labels(other)
    assert mm.generation() != gen and mm.labels_info() == (75, 4)
    check(mm, q, other, 3)
    gen = mm.generation()
    mm.set_labels(None)
    assert mm.generation() != gen and mm.labels_info() == (0, 0)
    with pytest.raises(frt.FrtError) as e:
        mm.topk_labels(q, 3)
    assert e.value.code == frt.FRT_ERR_INVALID
    mm.set_labels(labels)
    mm.init(g)  # a reload replaces the gallery: no labels
    assert mm.labels_info() == (0, 0)
    ri, rs = mm.topk(q, 3)  # ... and the row search is what it was
    mm.set_labels(np.arange(300, dtype=np.int32))
    assert np.array_equal(mm.topk_labels(q, 3)[1], ri)


# ---------------------------------------------------------------------------------------------------------------- screened path
_CLUSTERS = {}


def clustered(synth, n, d, m):
    """n rows in identities of m rows: row = base + 0.03 * noise (normalised), so that the best m rows of a matching query are ONE person -
    the case a threshold that counts rows gets wrong.  The members of identity i are the rows i, i + n0 / m, i + 2 n0 / m ... (n0 = 32 768):
    thousands of rows, i.e. dozens of tiles, apart.  Rows from n0 on (the ragged tail) are identities of one row each."""
    key = (n, d, m)
    if key not in _CLUSTERS:
        n0 = SCREEN_MIN
        ids = n0 // m
        base = synth.make_gallery(ids + (n - n0), d=d, seed=50 + m)
        which = np.concatenate([np.arange(n0) % ids, ids + np.arange(n - n0)])
        r = np.random.Generator(np.random.PCG64([d, m]))
        rows = base[which] + np.float32(0.03) * r.standard_normal((n, d)).astype(np.float32)
        rows /= np.sqrt((rows.astype(np.float64) ** 2).sum(1, keepdims=True)).astype(np.float32)
        _CLUSTERS[key] = (np.ascontiguousarray(rows, np.float32), which.astype(np.int32), base)
    return _CLUSTERS[key]


def cluster_queries(synth, rows, base, d, F):
    """an enrolled row, near-copies of identity centres (every member of the identity scores high), random directions"""
    ids = [5, 4000, SCREEN_MIN // 8 - 1][:F - 1]
    near = synth.make_queries(base, ids, noise=0.02, seed=d + F)
    rnd = np.random.Generator(np.random.PCG64(70 + F)).standard_normal((F - 1 - len(near), d)).astype(np.float32)
    rnd /= np.sqrt((rnd ** 2).sum(1, keepdims=True))
    return np.ascontiguousarray(np.concatenate([rows[12345:12346], near, rnd]), np.float32)


@pytest.mark.parametrize("m", [4, 8], ids=["M4_screened", "M8_exact_passes"])
@pytest.mark.parametrize("n,d,F", [(SCREEN_MIN, 512, 3), (SCREEN_MIN + 77, 128, 40)], ids=["int8_shadow", "fp16_shadow_ragged"])
def test_screened_gallery_is_bit_identical_with_screening_on_and_off(frt, synth, mm, n, d, F, m):
    """k = 4: with M = 4 the bound (k - 1) M + 1 = 13 fits the selection kernel's 16 and the call screens; with M = 8 it is 25 and the call
    takes the exact passes.  Either way: the definition, bit for bit."""
    k = 4
    rows, labels, base = clustered(synth, n, d, m)
    q = cluster_queries(synth, rows, base, d, F)
    load(mm, rows, labels, screening=True)
    assert mm.labels_info() == (SCREEN_MIN // m + n - SCREEN_MIN, m)
    assert mm.scanBytes() == n * d * (1 if d == 512 else 2)  # the gallery does screen
    C = mm.calculate(q)
    want = expected(C, labels, k)
    # the case at stake: for a matching query the best m ROWS are one identity
    order = np.argsort(-C[1], kind="stable")[:m]
    assert len(set(labels[order].tolist())) == 1
    on = mm.topk_labels(q, k)
    same(on, want)
    mm.setScreening(False)
    off = mm.topk_labels(q, k)
    mm.setScreening(True)
    same(off, want)
    i1, s1 = mm.top1(q)
    assert np.array_equal(on[1][:, 0], i1) and np.array_equal(on[2][:, 0], s1)


# ---------------------------------------------------------------------------------------------------------------- device forms, shards
def test_dev_form_with_fp16_queries_on_a_side_stream(frt, synth, mm):
    import torch
    g, labels = small(synth)
    F, k = 40, 3
    q = small_queries(synth, g, F)
    load(mm, g, labels)
    dq16 = torch.from_numpy(q).cuda().to(torch.float16)
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        dl = torch.full((F, k), -7, dtype=torch.int32, device="cuda")
        di = torch.full((F, k), -7, dtype=torch.int32, device="cuda")
        ds = torch.zeros(F, k, device="cuda")
        mm.topk_labels_dev(dq16.data_ptr(), F, k, dl.data_ptr(), di.data_ptr(), ds.data_ptr(), st.cuda_stream, fp16=True)
    st.synchronize()
    q16 = q.astype(np.float16).astype(np.float32)
    want = mm.topk_labels(q16, k)
    same((dl.cpu().numpy(), di.cpu().numpy(), ds.cpu().numpy()), want)
    same(want, expected(mm.calculate(q16), labels, k))


def test_row_offset_makes_the_indices_global(frt, synth, mm):
    g, labels = small(synth)
    q = small_queries(synth, g, 5)
    load(mm, g, labels)
    local = mm.topk_labels(q, 16)
    mm.setRowOffset(100_000)
    try:
        lab, idx, sim = check(mm, q, labels, 16, row_offset=100_000)
    finally:
        mm.setRowOffset(0)
    assert np.array_equal(lab, local[0]) and np.array_equal(idx, local[1] + 100_000) and np.array_equal(sim, local[2])


@pytest.mark.parametrize("k", [3, 16])
def test_two_shards_merged_on_the_device_equal_the_whole_gallery(frt, synth, mm, fresh, k):
    """labels row % 75 with the cut at row 150: every identity has two rows in either shard"""
    import torch
    g, labels = small(synth)
    F = 40
    q = small_queries(synth, g, F)
    load(mm, g, labels)
    whole = mm.topk_labels(q, k)
    dq = torch.from_numpy(q).cuda()
    ll = torch.zeros(2, F, k, dtype=torch.int32, device="cuda")
    li = torch.zeros(2, F, k, dtype=torch.int32, device="cuda")
    ls = torch.zeros(2, F, k, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    for r, (b, e) in enumerate(((0, 150), (150, 300))):
        load(fresh, g[b:e], labels[b:e])
        fresh.setRowOffset(b)
        fresh.topk_labels_dev(dq.data_ptr(), F, k, ll[r].data_ptr(), li[r].data_ptr(), ls[r].data_ptr(), s)
        torch.cuda.synchronize()
    fresh.setRowOffset(0)
    ol = torch.zeros(F, k, dtype=torch.int32, device="cuda")
    oi = torch.zeros(F, k, dtype=torch.int32, device="cuda")
    os_ = torch.zeros(F, k, device="cuda")
    frt.merge_topk_labels_dev(2, F, k, ll.data_ptr(), li.data_ptr(), ls.data_ptr(), ol.data_ptr(), oi.data_ptr(), os_.data_ptr(), s)
    torch.cuda.synchronize()
    same((ol.cpu().numpy(), oi.cpu().numpy(), os_.cpu().numpy()), whole)
    # and the host merge of the same lists
    same(frt.merge_topk_labels(ll.cpu().numpy(), li.cpu().numpy(), ls.cpu().numpy()), whole)


# ---------------------------------------------------------------------------------------------------------------- edits
def edited_equals_fresh(frt, mm, fresh, rows, labels, q, k=4):
    """the edited matcher against a fresh one on (rows, labels), and both against the definition; labels_info never under-states"""
    assert mm.m == len(rows)
    load(fresh, rows, labels)
    got = mm.topk_labels(q, k)
    same(got, fresh.topk_labels(q, k))
    same(got, expected(mm.calculate(q), labels, k))
    assert mm.scanBytes() == fresh.scanBytes()
    counts = np.unique(labels, return_counts=True)[1]
    n_id, m_max = mm.labels_info()
    assert n_id == len(counts) and m_max >= counts.max()
    return n_id, m_max, int(counts.max())


def test_edits_across_the_screening_threshold_equal_a_fresh_matcher(frt, synth, mm, fresh):
    rows_all, labels_all, base = clustered(synth, SCREEN_MIN, 512, 4)
    n0 = SCREEN_MIN - 2
    rows, labels = rows_all[:n0].copy(), labels_all[:n0].copy()
    q = np.concatenate([cluster_queries(synth, rows_all, base, 512, 3), synth.make_queries(base, [77, 8000], noise=0.02, seed=9)])
    load(mm, rows, labels)
    mm.galleryReserve(33_000)
    assert mm.scanBytes() == n0 * 512 * 4  # below the threshold: the exact scan
    _, m_max, true_max = edited_equals_fresh(frt, mm, fresh, rows, labels, q)
    assert m_max == true_max == 4
    # + 5 rows: the two that were cut off, a FIFTH row for identity 77, two rows of a new identity -> 32 771 rows: screens now
    new = np.concatenate([rows_all[n0:], synth.make_queries(base, [77], noise=0.02, seed=10), synth.make_gallery(2, seed=11)])
    new_labels = np.concatenate([labels_all[n0:], [77, 9000, 9000]]).astype(np.int32)
    before = mm.editStats()
    gen = mm.generation()
    assert mm.gallery_add_labeled(new, new_labels) == n0
    assert mm.generation() != gen
    assert mm.editStats()["reallocations"] == before["reallocations"]  # inside the reserved capacity
    rows, labels = np.concatenate([rows, new]), np.concatenate([labels, new_labels])
    assert mm.scanBytes() == len(rows) * 512
    n_id, m_max, true_max = edited_equals_fresh(frt, mm, fresh, rows, labels, q)
    assert m_max == true_max == 5 and n_id == SCREEN_MIN // 4 + 1
    # - the whole identity 77 (five rows, in five tiles): 32 766 rows, below the threshold again
    gone = np.flatnonzero(labels == 77)
    assert len(gone) == 5
    mm.galleryRemove(gone[::-1])
    keep = np.ones(len(rows), bool)
    keep[gone] = False
    rows, labels = rows[keep], labels[keep]
    assert mm.scanBytes() == len(rows) * 512 * 4
    n_id, m_max, true_max = edited_equals_fresh(frt, mm, fresh, rows, labels, q)
    assert n_id == SCREEN_MIN // 4 and true_max == 4 and m_max in (4, 5)  # may over-state after a remove, never under-states
    # - one row of another identity (the best row of query 0's own identity: its next best row takes over)
    lab0 = mm.topk_labels(q[:1], 1)
    mm.galleryRemove([int(lab0[1][0, 0])])
    keep = np.ones(len(rows), bool)
    keep[int(lab0[1][0, 0])] = False
    rows, labels = rows[keep], labels[keep]
    edited_equals_fresh(frt, mm, fresh, rows, labels, q)
    assert mm.topk_labels(q[:1], 1)[0][0, 0] == lab0[0][0, 0]
    # and back up across the threshold with a reallocation-free labelled add from the device
    import torch
    more = synth.make_gallery(4, seed=12)
    more_labels = np.array([3, 9001, 9001, 9002], np.int32)
    d_more = torch.from_numpy(more).cuda()
    torch.cuda.synchronize()
    mm.gallery_add_labeled_dev(d_more.data_ptr(), more_labels)
    rows, labels = np.concatenate([rows, more]), np.concatenate([labels, more_labels])
    assert len(rows) >= SCREEN_MIN and mm.scanBytes() == len(rows) * 512
    edited_equals_fresh(frt, mm, fresh, rows, labels, q)


def test_an_empty_gallery_takes_either_add(frt, synth, mm):
    g, labels = small(synth)
    q = small_queries(synth, g, 5)
    mm.setStorage(False)
    mm.galleryBegin(0, 512)
    mm.galleryCommit()
    mm.gallery_add_labeled(g[:200], labels[:200])
    mm.gallery_add_labeled(g[200:], labels[200:])
    assert mm.labels_info() == (75, 4)
    check(mm, q, labels, 3)
    mm.galleryRemove(np.arange(300))
    with pytest.raises(frt.FrtError) as e:
        mm.topk_labels(q, 3)
    assert e.value.code == frt.FRT_ERR_EMPTY
    mm.galleryAdd(g[:10])  # the plain add on the emptied gallery: unlabelled from here on
    assert mm.labels_info() == (0, 0)
    mm.galleryAdd(g[10:20])


# ---------------------------------------------------------------------------------------------------------------- errors
def test_error_paths(frt, synth, mm):
    g, labels = small(synth)
    q = small_queries(synth, g, 5)
    load(mm, g, None)

    def invalid(fn, *a):
        with pytest.raises(frt.FrtError) as e:
            fn(*a)
        assert e.value.code == frt.FRT_ERR_INVALID, a

    invalid(mm.topk_labels, q, 3)                                  # unlabelled gallery
    invalid(mm.gallery_add_labeled, g[:2], labels[:2])             # the labelled add on an unlabelled gallery with rows
    bad = labels.copy()
    bad[17] = -1
    invalid(mm.set_labels, bad)                                    # negative label
    invalid(mm.set_labels, labels[:299])                           # wrong n
    assert mm.labels_info() == (0, 0) and mm.m == 300              # nothing changed
    mm.set_labels(labels)
    invalid(mm.set_labels, bad)
    invalid(mm.set_labels, np.concatenate([labels, labels[:1]]))
    invalid(mm.galleryAdd, g[:2])                                  # the plain add on a labelled gallery
    invalid(mm.gallery_add_labeled, g[:2], np.array([3, -2], np.int32))
    invalid(mm.topk_labels, q, 0)
    invalid(mm.topk_labels, q, 17)
    assert mm.labels_info() == (75, 4) and mm.m == 300             # nothing changed
    check(mm, q, labels, 3)
