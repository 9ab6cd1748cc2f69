"""Live gallery edits (frt_matcher_gallery_reserve / add / add_dev / remove): after any sequence of edits a matcher answers exactly as a
FRESH matcher that was init'ed with the resulting row list in the same storage mode - indices, similarities and the first-maximum tie rule,
bit for bit (np.array_equal, no tolerance).  Against the NumPy oracle the comparison is the one of tests/test_gpu_match.py (planted
answers; 1e-5 on similarities of unit rows for NumPy's different summation order)."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

PKG = os.path.join(ROOT, "face-recognition-cpp-tensorrt_amd")
SCREEN_MIN = 32768  # a fresh init screens from here on (frt.h)


# ---------------------------------------------------------------------------------------------------------------- helpers
@pytest.fixture(scope="module")
def pair(frt):
    """(edited, fresh): two matchers; the second one only ever sees frt_matcher_init."""
    a, b = frt.MatMul(0), frt.MatMul(0)
    yield a, b
    a.close()
    b.close()


_BASE = {}


def base_rows(synth, d):
    if d not in _BASE:
        _BASE[d] = synth.make_gallery(110_000, d=d, seed=21)
    return _BASE[d]


def stored(rows, fp16):
    """The values the similarities are defined on (frt_matcher_set_storage)."""
    return rows.astype(np.float16).astype(np.float32) if fp16 else rows


def start(frt, mm, rows, fp16, d, reserve=0):
    """A matcher holding ``rows`` through the ordinary load (an empty one: begin + commit with zero rows, which fixes the width)."""
    mm.setScreening(True)
    mm.setStorage(fp16)
    if reserve:
        mm.galleryReserve(reserve)
    if len(rows):
        mm.init(rows)
    else:
        mm.galleryBegin(0, d)
        mm.galleryCommit()
    assert mm.m == len(rows) and mm.k == d


def same_answers(frt, mm, fresh, rows, q, fp16, k=5):
    """edited vs fresh on ``rows``: top1, topk, calculate, calculate_top1, scan bytes - bit for bit."""
    assert mm.m == len(rows) == int(frt.lib.frt_matcher_num_rows(mm._h))
    if len(rows) == 0:
        with pytest.raises(frt.FrtError) as e:
            mm.top1(q)
        assert e.value.code == frt.FRT_ERR_EMPTY
        return None
    fresh.setScreening(True)
    fresh.setStorage(fp16)
    fresh.init(rows)
    i1, s1 = mm.top1(q)
    i2, s2 = fresh.top1(q)
    assert np.array_equal(i1, i2), (i1, i2)
    assert np.array_equal(s1, s2)
    ki1, ks1 = mm.topk(q, k)
    ki2, ks2 = fresh.topk(q, k)
    assert np.array_equal(ki1, ki2) and np.array_equal(ks1, ks2)
    assert np.array_equal(ki1[:, 0], i1) and np.array_equal(ks1[:, 0], s1)
    c1, c2 = mm.calculate(q), fresh.calculate(q)
    assert c1.shape == (len(q), len(rows)) and np.array_equal(c1, c2)
    _, ci, cs = mm.calculate_top1(q, materialize=False)
    assert np.array_equal(ci, i1) and np.array_equal(cs, s1)
    assert np.array_equal(c1.argmax(1).astype(np.int32), i1) and np.array_equal(c1.max(1), s1)  # the first-maximum rule on the materialised rows
    assert mm.scanBytes() == fresh.scanBytes()  # screens exactly when a fresh matcher does, and says what a call reads
    return i1, s1


def delta(after, before):
    return {k: after[k] - before[k] for k in after}


# ---------------------------------------------------------------------------------------------------------------- add
@pytest.mark.parametrize("d", [512, 128])
@pytest.mark.parametrize("fp16", [False, True], ids=["fp32", "fp16"])
@pytest.mark.parametrize("n", [1, 3, 127, 128, 129, 5000])
@pytest.mark.parametrize("n0", [0, 100, 32_700, 40_077, 100_000])
def test_add_equals_fresh_init(frt, synth, pair, n0, n, fp16, d):
    from oracle import match
    mm, fresh = pair
    base = base_rows(synth, d)[:n0]
    new = synth.make_gallery(n, d=d, seed=1000 + n)
    dup_old = n0 > 7 and n >= 2
    if dup_old:
        new[n - 1] = base[7]       # a new row that duplicates an old one loses to the old index
    if n >= 3:
        new[1] = new[0]            # two identical new rows resolve to the lower one
    start(frt, mm, base, fp16, d)
    gen0 = mm.generation()
    assert mm.galleryAdd(new) == n0
    assert mm.generation() != gen0
    rows = np.concatenate([base, new])
    want = [n0, n0, 7 if dup_old else n0 + n - 1]
    q = [new[0], new[1] if n >= 3 else new[0], new[n - 1]]
    old = [0, n0 // 2, n0 - 1] if n0 else []
    edge = (n0 + 2 + 127) // 128 * 128  # new rows either side of a 128-row tile edge (not the duplicates at new[0], new[1], new[n - 1])
    if n0 + 2 <= edge - 1 and edge <= n0 + n - 2:
        old += [edge - 1, edge]
    q = np.concatenate([np.stack(q), synth.make_queries(rows, old, noise=0.01) if old else np.zeros((0, d), np.float32),
                        np.random.Generator(np.random.PCG64(n0 + n)).standard_normal((8, d)).astype(np.float32)])
    want += old
    i, s = same_answers(frt, mm, fresh, rows, q, fp16)
    assert i[:len(want)].tolist() == want
    oi, osim = match.top1(q[:len(want)], stored(rows, fp16))
    # (the duplicates' similarities are bit-identical on the device, so the index is decided there; NumPy may see either of two equal rows)
    assert np.abs(osim - s[:len(want)]).max() < 1e-5
    assert all(int(a) == b or np.array_equal(rows[int(a)], rows[b]) for a, b in zip(oi, want))
    # the same through the exact scan
    mm.setScreening(False)
    i0, s0 = mm.top1(q)
    mm.setScreening(True)
    assert np.array_equal(i0, i) and np.array_equal(s0, s)


@pytest.mark.parametrize("fp16", [False, True], ids=["fp32", "fp16"])
def test_add_from_device_memory(frt, synth, pair, fp16):
    """galleryAddDev: the rows are already on the device (the embedder's output)."""
    import torch
    mm, fresh = pair
    base = base_rows(synth, 512)[:40_077]
    new = synth.make_gallery(200, seed=5)
    start(frt, mm, base, fp16, 512)
    t = torch.from_numpy(new).cuda()
    torch.cuda.synchronize()
    before = mm.editStats()
    assert mm.galleryAddDev(t.data_ptr(), 200) == 40_077
    assert delta(mm.editStats(), before)["rows_uploaded"] == 200
    rows = np.concatenate([base, new])
    q = synth.make_queries(rows, [40_077, 40_276, 5, 40_076], noise=0.01)
    i, _ = same_answers(frt, mm, fresh, rows, q, fp16)
    assert i.tolist() == [40_077, 40_276, 5, 40_076]


def test_add_of_a_non_finite_row_keeps_answers_exact(frt, synth, pair):
    """A non-finite new row poisons the screening bounds the way it does at build time: the other queries still get the fresh answers."""
    mm, fresh = pair
    base = base_rows(synth, 512)[:40_077]
    new = synth.make_gallery(3, seed=6)
    new[1, 17] = np.inf
    start(frt, mm, base, False, 512)
    mm.galleryAdd(new)
    rows = np.concatenate([base, new])
    q = synth.make_queries(rows, [3, 40_077, 40_079, 20_000], noise=0.01)
    q[:, 17] = 0  # (inf * 0 would be NaN either way; keep the expected similarities finite except for the poisoned row)
    fresh.setStorage(False)
    fresh.init(rows)
    i1, s1 = mm.top1(q)
    i2, s2 = fresh.top1(q)
    assert np.array_equal(i1, i2) and np.array_equal(s1, s2, equal_nan=True)


# ---------------------------------------------------------------------------------------------------------------- remove
def remove_cases(n):
    r = np.random.Generator(np.random.PCG64(n))
    return {
        "first": [0],
        "middle": [n // 2],
        "last": [n - 1],
        "tile_edge": [127, 128, 16_383, 16_384],
        "scattered_1pct": r.choice(n, n // 100, replace=False).tolist(),
        "block_10000": list(range(12_345, 22_345)),
        "below_threshold": list(range(1_000, 1_000 + n - SCREEN_MIN + 5)),
        "unsorted_with_duplicates": [n - 1, 5, 300, 5, n - 1, 299],
    }


@pytest.mark.parametrize("d", [512, 128])
@pytest.mark.parametrize("fp16", [False, True], ids=["fp32", "fp16"])
@pytest.mark.parametrize("case", ["first", "middle", "last", "tile_edge", "scattered_1pct", "block_10000", "below_threshold", "unsorted_with_duplicates"])
def test_remove_equals_fresh_init(frt, synth, pair, case, fp16, d):
    from oracle import match
    mm, fresh = pair
    n = 40_077
    base = base_rows(synth, d)[:n]
    holes = remove_cases(n)[case]
    start(frt, mm, base, fp16, d)
    gen0, before = mm.generation(), mm.editStats()
    mm.galleryRemove(holes)
    assert mm.generation() != gen0
    keep = np.ones(n, bool)
    keep[holes] = False
    rows = base[keep]
    new_index = np.cumsum(keep) - 1
    # rows in front of, between and behind the holes, found at their new places
    probe = sorted({i for h in (min(holes), max(holes)) for i in (h - 1, h + 1, h + 130) if 0 <= i < n and keep[i]} | {n - 2 if keep[n - 2] else n - 3, 1})
    q = np.concatenate([synth.make_queries(base, probe, noise=0.01), np.random.Generator(np.random.PCG64(7)).standard_normal((8, d)).astype(np.float32)])
    i, s = same_answers(frt, mm, fresh, rows, q, fp16)
    assert i[:len(probe)].tolist() == [int(new_index[p]) for p in probe]
    oi, osim = match.top1(q[:len(probe)], stored(rows, fp16))
    assert np.array_equal(oi, i[:len(probe)]) and np.abs(osim - s[:len(probe)]).max() < 1e-5
    # incrementality (derived): nothing uploaded, only rows behind the first hole move, the shadow is rebuilt from its tile on
    st, r0, cnt = delta(mm.editStats(), before), min(holes), len(set(holes))
    assert st["rows_uploaded"] == 0 and st["reallocations"] == 0
    assert st["rows_moved"] <= n - r0 - cnt
    assert st["shadow_rows_rebuilt"] <= n - 128 * (r0 // 128)
    mm.setScreening(False)
    i0, s0 = mm.top1(q)
    mm.setScreening(True)
    assert np.array_equal(i0, i) and np.array_equal(s0, s)


@pytest.mark.parametrize("fp16", [False, True], ids=["fp32", "fp16"])
def test_remove_the_lower_duplicate_and_then_every_row(frt, synth, pair, fp16):
    mm, fresh = pair
    n = 33_000
    base = base_rows(synth, 512)[:n].copy()
    base[30_000] = base[200]
    start(frt, mm, base, fp16, 512)
    q = base[[200]]
    assert mm.top1(q)[0].tolist() == [200]
    mm.galleryRemove([200, 10])                      # the lower duplicate goes (and a row in front of it): the higher one, shifted by two, answers
    rows = np.delete(base, [200, 10], axis=0)
    i, _ = same_answers(frt, mm, fresh, rows, np.concatenate([q, synth.make_queries(rows, [0, 32_997])]), fp16)
    assert i.tolist() == [29_998, 0, 32_997]
    gen = mm.generation()
    mm.galleryRemove(np.arange(len(rows)))          # every row: an empty gallery, FRT_ERR_EMPTY as after init with zero rows
    assert mm.generation() != gen
    same_answers(frt, mm, fresh, rows[:0], q, fp16)
    mm.galleryAdd(base[:3])                          # and it can be filled again
    i, _ = same_answers(frt, mm, fresh, base[:3], base[[2, 0]], fp16)
    assert i.tolist() == [2, 0]


# ---------------------------------------------------------------------------------------------------------------- sequences
@pytest.mark.parametrize("fp16", [False, True], ids=["fp32", "fp16"])
def test_interleaved_adds_and_removes_follow_the_row_list_model(frt, synth, pair, fp16):
    """30 seeded random edits around the screening threshold, checked against the NumPy row list after every step."""
    from oracle import match
    mm, fresh = pair
    r = np.random.Generator(np.random.PCG64(2024))
    pool = base_rows(synth, 512)
    rows = pool[:32_700].copy()
    used = 32_700
    start(frt, mm, rows, fp16, 512)
    crossed = set()
    for step in range(30):
        if r.random() < 0.5 or len(rows) < 1000:
            n = int(r.choice([1, 2, 50, 130, 400]))
            new = pool[used:used + n]
            used += n
            if r.random() < 0.3:
                new = new.copy()
                new[0] = rows[int(r.integers(0, len(rows)))]  # a duplicate of an existing row
            assert mm.galleryAdd(new) == len(rows)
            rows = np.concatenate([rows, new])
        else:
            n = int(r.choice([1, 3, 100, 450]))
            holes = r.choice(len(rows), n, replace=False)
            mm.galleryRemove(holes)
            rows = np.delete(rows, holes, axis=0)
        crossed.add(len(rows) >= SCREEN_MIN)
        probe = r.integers(0, len(rows), 6)
        q = np.concatenate([synth.make_queries(rows, probe, noise=0.01, seed=step), r.standard_normal((6, 512)).astype(np.float32)])
        i, s = same_answers(frt, mm, fresh, rows, q, fp16)
        oi, osim = match.top1(q[:6], stored(rows, fp16))
        assert np.abs(osim - s[:6]).max() < 1e-5
        assert all(int(a) == int(b) or np.array_equal(rows[int(a)], rows[int(b)]) for a, b in zip(oi, i[:6]))
    assert crossed == {True, False}  # the sequence went over the threshold and back
    mm.setScreening(False)
    fresh.setScreening(False)
    try:
        q = np.concatenate([synth.make_queries(rows, [0, len(rows) - 1]), r.standard_normal((6, 512)).astype(np.float32)])
        i1, s1 = mm.top1(q)
        i2, s2 = fresh.top1(q)
        assert np.array_equal(i1, i2) and np.array_equal(s1, s2) and i1[:2].tolist() == [0, len(rows) - 1]
        assert mm.scanBytes() == fresh.scanBytes()
    finally:
        mm.setScreening(True)
        fresh.setScreening(True)


# ---------------------------------------------------------------------------------------------------------------- incrementality
@pytest.mark.parametrize("fp16", [False, True], ids=["fp32", "fp16"])
def test_adds_inside_the_reserved_capacity_are_incremental(frt, synth, fp16):
    """From edit_stats (derived, not measured): an add inside the capacity uploads its rows and nothing else; the add that runs out of
    capacity reallocates exactly once and the contents are still right."""
    mm, fresh = frt.MatMul(0), frt.MatMul(0)
    try:
        base = base_rows(synth, 512)
        n0 = 40_077
        start(frt, mm, base[:n0], fp16, 512, reserve=41_000)
        n_now = n0
        for n in (1, 3, 127, 128, 129, 300):  # 688 rows: inside 41 000
            before = mm.editStats()
            mm.galleryAdd(base[n_now:n_now + n])
            n_now += n
            st = delta(mm.editStats(), before)
            assert st["rows_uploaded"] == n and st["rows_moved"] == 0 and st["reallocations"] == 0 and st["shadow_rows_rebuilt"] <= n + 127, st
        q = synth.make_queries(base, [0, n0 - 1, n0, n_now - 1], noise=0.01)
        i, _ = same_answers(frt, mm, fresh, base[:n_now], q, fp16)
        assert i.tolist() == [0, n0 - 1, n0, n_now - 1]
        # reserve never shrinks and changes nothing
        gen = mm.generation()
        mm.galleryReserve(10)
        mm.galleryReserve(41_000)
        assert mm.generation() == gen
        # past the capacity: one reallocation
        before = mm.editStats()
        mm.galleryAdd(base[n_now:n_now + 500])
        n_now += 500
        st = delta(mm.editStats(), before)
        assert st["reallocations"] == 1 and st["rows_uploaded"] == 500 and st["rows_moved"] == 0, st
        q = synth.make_queries(base, [0, 40_000, n_now - 500, n_now - 1], noise=0.01)
        i, _ = same_answers(frt, mm, fresh, base[:n_now], q, fp16)
        assert i.tolist() == [0, 40_000, n_now - 500, n_now - 1]
        # the new capacity is geometric: the next adds fit again
        before = mm.editStats()
        mm.galleryAdd(base[n_now:n_now + 500])
        assert delta(mm.editStats(), before)["reallocations"] == 0
        # a reserve beyond the capacity of a live gallery moves it once, answers unchanged
        before = mm.editStats()
        mm.galleryReserve(100_000)
        assert delta(mm.editStats(), before)["reallocations"] == 1
        i, _ = same_answers(frt, mm, fresh, base[:n_now + 500], q, fp16)
        assert i.tolist() == [0, 40_000, n_now - 500, n_now - 1]
    finally:
        mm.close()
        fresh.close()


# ---------------------------------------------------------------------------------------------------------------- errors
def test_rejected_edits_change_nothing(frt, synth, pair):
    import ctypes
    mm, fresh = pair
    base = base_rows(synth, 512)[:5000]
    start(frt, mm, base, False, 512)
    q = synth.make_queries(base, [0, 4999, 77])
    want = mm.top1(q)
    gen = mm.generation()
    stats = mm.editStats()
    for bad in ([5000], [-1], [3, 4, 5000], [2, -7]):
        with pytest.raises(frt.FrtError) as e:
            mm.galleryRemove(bad)
        assert e.value.code == frt.FRT_ERR_INVALID
    assert frt.lib.frt_matcher_gallery_add(mm._h, None, 1) == frt.FRT_ERR_INVALID
    assert frt.lib.frt_matcher_gallery_add_dev(mm._h, None, 1) == frt.FRT_ERR_INVALID
    assert frt.lib.frt_matcher_gallery_add(mm._h, base.ctypes.data_as(ctypes.c_void_p), -1) == frt.FRT_ERR_INVALID
    assert frt.lib.frt_matcher_gallery_remove(mm._h, None, 1) == frt.FRT_ERR_INVALID
    mm.setRowOffset(1000)  # a shard is not edited (the offset itself moves the generation)
    gen_off = mm.generation()
    for call in (lambda: mm.galleryAdd(base[:1]), lambda: mm.galleryRemove([0]), lambda: mm.galleryReserve(9000)):
        with pytest.raises(frt.FrtError) as e:
            call()
        assert e.value.code == frt.FRT_ERR_INVALID
    assert mm.generation() == gen_off
    mm.setRowOffset(0)
    assert mm.m == 5000 and mm.editStats() == stats
    got = mm.top1(q)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    # nothing to do is not an edit either
    g2 = mm.generation()
    mm.galleryRemove([])
    mm.galleryAdd(base[:0])
    assert mm.generation() == g2
    # every successful edit moves the generation
    seen = {g2}
    for edit in (lambda: mm.galleryAdd(base[:2]), lambda: mm.galleryRemove([1]), lambda: mm.galleryRemove([0, 4999])):
        edit()
        assert mm.generation() not in seen
        seen.add(mm.generation())
    # a matcher that has never seen a gallery does not know its width
    m0 = frt.MatMul(0)
    try:
        assert frt.lib.frt_matcher_gallery_add(m0._h, base.ctypes.data_as(ctypes.c_void_p), 1) == frt.FRT_ERR_INVALID
    finally:
        m0.close()
    assert gen != mm.generation()


def test_edit_during_an_open_streamed_load_acts_on_the_live_gallery(frt, synth, pair):
    mm, fresh = pair
    base = base_rows(synth, 512)
    start(frt, mm, base[:1000], False, 512)
    mm.galleryBegin(50, 512)
    mm.galleryAppend(base[2000:2040])
    mm.galleryAdd(base[1000:1010])       # the live gallery: 1010 rows
    mm.galleryRemove([0])
    live = base[1:1010]
    i, _ = same_answers(frt, mm, fresh, live, synth.make_queries(live, [0, 1008]), False)
    assert i.tolist() == [0, 1008]
    mm.galleryCommit()                   # the load replaces it, as always
    i, _ = same_answers(frt, mm, fresh, base[2000:2040], synth.make_queries(base[2000:2040], [39]), False)
    assert i.tolist() == [39]


# ---------------------------------------------------------------------------------------------------------------- 1M rows
def test_one_million_gallery_edits_by_properties(frt, synth):
    """BASELINE size, in the style of test_one_million_gallery_properties: reserve, init, add 64, remove two - by planted answers and
    edit_stats (no fresh 2 GB matcher beside it)."""
    N = 1_000_000
    mm = frt.MatMul(0)
    try:
        g = synth.make_gallery(N)
        mm.galleryReserve(N + 128)
        mm.init(g)
        new = synth.make_gallery(64, seed=99)
        before = mm.editStats()
        assert mm.galleryAdd(new) == N
        st = delta(mm.editStats(), before)
        assert st == dict(rows_uploaded=64, rows_moved=0, shadow_rows_rebuilt=st["shadow_rows_rebuilt"], reallocations=0) and st["shadow_rows_rebuilt"] <= 64 + 127
        assert mm.scanBytes() == (N + 64) * 512
        qn = synth.make_queries(new, np.arange(64), noise=0.01)
        i, s = mm.top1(qn)
        assert np.array_equal(i, N + np.arange(64)) and s.min() > 0.97
        plant = np.array([0, 4, 6, 499_999, 500_001, 999_999])
        qp = synth.make_queries(g, plant, noise=0.01)
        assert np.array_equal(mm.top1(qp)[0], plant)
        before = mm.editStats()
        mm.galleryRemove([500_000, 5])
        st = delta(mm.editStats(), before)
        assert st["rows_uploaded"] == 0 and st["reallocations"] == 0
        assert 0 < st["rows_moved"] <= (N + 64) - 5 - 2 and st["shadow_rows_rebuilt"] <= N + 64
        i, s = mm.top1(np.concatenate([qp, qn]))
        assert i[:6].tolist() == [0, 4, 5, 499_998, 499_999, 999_997] and np.array_equal(i[6:], 999_998 + np.arange(64)) and s.min() > 0.97
        # exact scan and top-k agree with the screened answers
        mm.setScreening(False)
        i0, s0 = mm.top1(np.concatenate([qp, qn]))
        mm.setScreening(True)
        assert np.array_equal(i0, i) and np.array_equal(s0, s)
        ki, ks = mm.topk(qn[:4], 3)
        assert np.array_equal(ki[:, 0], i[6:10]) and np.array_equal(ks[:, 0], s[6:10])
        osim = (qn.astype(np.float64) * new).sum(1)  # NumPy on the planted rows themselves (no second 2 GB row list on the host)
        assert np.abs(osim - s[6:]).max() < 1e-5
    finally:
        mm.close()


# ---------------------------------------------------------------------------------------------------------------- pipeline
@pytest.fixture(scope="module")
def stack(frt, synth, blobs):
    dpath, _ = blobs("det")
    rpath, _ = blobs("ir")
    B, K, H, W = 4, 4, 640, 640
    det = frt.RetinaFace(dpath, W, H, (3, H, W), B, K, 0.4, 0.6)
    frames = synth.make_frames(B, H, W)

    def make(n_gallery):
        rec = frt.ArcFaceIR50(rpath, W, H, maxBatchSize=B * K, maxFacesPerScene=K)
        if n_gallery:
            rec.setGallery(synth.make_gallery(n_gallery, seed=31))
            rec.initMatMul()
        else:
            rec.matmul.galleryBegin(0, 512)
            rec.matmul.galleryCommit()
        return frt.Pipeline(det, rec, B), rec

    yield make, frames, B, K
    det.close()


def fields_equal(a, b):
    return all(np.array_equal(a[k], b[k]) for k in a.dtype.names)


def run_submit(frt, pipe, frames, K, tickets=3):
    """the same frames as several tickets in flight at once -> the records / embeddings of every ticket"""
    outs = []
    for _ in range(tickets):
        res = np.zeros(len(frames) * K, frt.RESULT_DTYPE)
        emb = np.zeros((len(frames) * K, 512), np.float32)
        outs.append((pipe.submit(frames, res, emb), res, emb))
    for t, _, _ in outs:
        pipe.wait(t)
    for _, res, emb in outs[1:]:
        assert fields_equal(res, outs[0][1]) and np.array_equal(emb, outs[0][2])
    return outs[0][1], outs[0][2]


@pytest.mark.parametrize("n_gallery", [40_000, 0], ids=["gallery40000", "empty"])
@pytest.mark.parametrize("mode", ["run", "run_graph", "submit"])
@pytest.mark.parametrize("dev", [False, True], ids=["host_rows", "device_rows"])
def test_pipeline_sees_an_edit_on_its_next_call(frt, synth, stack, n_gallery, mode, dev):
    make, frames, B, K = stack
    pipe, rec = make(n_gallery)
    fresh = frt.MatMul(0)
    try:
        pipe.set_graph(mode != "run")
        go = (lambda: run_submit(frt, pipe, frames, K)) if mode == "submit" else (lambda: pipe.run(frames))
        go()
        res1, emb1 = go()  # (graph mode: the second call replays)
        v = res1["valid"] == 1
        assert v[:K].sum() >= 1 and v.sum() > v[:K].sum()
        if n_gallery:
            assert (res1["match_idx"][v] >= 0).all() and (res1["match_idx"][v] < n_gallery).all()
        else:
            assert (res1["match_idx"] == -1).all()
        # enrol frame 0's faces
        mine = np.nonzero(v[:K])[0]
        enrol = np.ascontiguousarray(emb1[mine])
        if dev:
            import torch
            t = torch.from_numpy(enrol).cuda()
            torch.cuda.synchronize()
            first = rec.matmul.galleryAddDev(t.data_ptr(), len(mine))
        else:
            first = rec.matmul.galleryAdd(enrol)
        assert first == n_gallery
        res2, emb2 = go()
        assert np.array_equal(emb2, emb1) and np.array_equal(res2["valid"], res1["valid"])
        rows = np.concatenate([synth.make_gallery(n_gallery, seed=31), enrol]) if n_gallery else enrol
        fresh.init(rows)
        fi, fs = fresh.top1(emb2[v])
        assert np.array_equal(res2["match_idx"][v], fi) and np.array_equal(res2["match_sim"][v], fs)
        assert res2["match_idx"][mine].tolist() == [n_gallery + j for j in range(len(mine))]  # those faces now report the new rows
        if n_gallery:
            others = v.copy()
            others[:K] = False
            far = others & (res2["match_idx"] < n_gallery)
            assert np.array_equal(res2["match_idx"][far], res1["match_idx"][far]) and np.array_equal(res2["match_sim"][far], res1["match_sim"][far])
        res2b, _ = go()
        assert fields_equal(res2b, res2)
        # and remove them again: the first run's records come back
        rec.matmul.galleryRemove(np.arange(first, first + len(mine)))
        res3, emb3 = go()
        assert fields_equal(res3, res1) and np.array_equal(emb3, emb1)
    finally:
        fresh.close()
        pipe.close()
        rec.close()


# ---------------------------------------------------------------------------------------------------------------- shell
def test_shell_enrols_and_removes_classes_without_a_reload(frt, synth, blobs, tmp_path):
    """tests/cpp/enrol_demo.cpp: enrolEmbedding / removeClass / featureMatching / getOutputs through include/frt/arcface.h, against the
    NumPy model of the (name, row) list."""
    from oracle import match
    rpath, _ = blobs("ir")
    exe = str(tmp_path / "enrol_demo")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "enrol_demo.cpp"), "-o", exe, os.path.join(PKG, "libfrt.so"), "-Wl,-rpath," + PKG,
                           "-Wl,-rpath,/opt/rocm/lib"])
    N = 500
    face = synth.make_frame(11, 112, 112)
    boxes = np.zeros(1, frt.BBOX_DTYPE)
    boxes[0] = (0, 0, 112, 112, 1.0)
    rec = frt.ArcFaceIR50(rpath, 640, 480, (3, 112, 112), 512, 1, 4, 0.65)
    emb = rec.forward(face, boxes).copy()
    rec.close()
    gal = synth.make_gallery(N)
    (tmp_path / "face.bin").write_bytes(face.tobytes())
    (tmp_path / "gal.bin").write_bytes(gal.tobytes())
    (tmp_path / "emb.bin").write_bytes(emb[0].tobytes())
    out = subprocess.run([exe, rpath, str(tmp_path / "face.bin"), str(tmp_path / "gal.bin"), str(N), str(tmp_path / "emb.bin")],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = [l.split() for l in out.stdout.splitlines() if l.startswith("step")]
    # the model: a list of (name, row)
    model, want = [], []

    def snap(ret):
        names = [n for n, _ in model]
        i, s = match.top1(emb, np.stack([r for _, r in model]))
        want.append((len(model), names[int(i[0])], float(s[0]), ret))

    def remove(name):
        k = sum(n == name for n, _ in model)
        model[:] = [(n, r) for n, r in model if n != name]
        return k

    model.append(("first", gal[0]));                                   snap(0)
    model[:] = [("u%d" % i, gal[i]) for i in range(N)];                snap(0)
    model.append(("alice", emb[0]));                                   snap(0)
    model.append(("bob", emb[0]));                                     snap(0)
    snap(remove("alice"))
    snap(remove("u0") + remove("nobody"))
    model.extend([("carol", emb[0]), ("carol", gal[1])]);              snap(0)
    snap(remove("bob") + remove("carol"))
    assert len(lines) == len(want) == 8
    for k, (l, w) in enumerate(zip(lines, want)):
        assert int(l[1]) == k and int(l[2]) == w[0] and l[3] == w[1] and abs(float(l[4]) - w[2]) < 1e-5 and int(l[5]) == w[3], (l, w)
    assert [w[1] for w in want[2:7]] == ["alice", "alice", "bob", "bob", "bob"]


def test_python_shell_keeps_names_in_step(frt, synth, blobs):
    rpath, _ = blobs("ir")
    rec = frt.ArcFaceIR50(rpath, 640, 480, (3, 112, 112), 512, 1, 4, 0.65)
    try:
        face = synth.make_frame(11, 112, 112)
        boxes = np.zeros(1, frt.BBOX_DTYPE)
        boxes[0] = (0, 0, 112, 112, 1.0)
        emb = rec.forward(face, boxes).copy()
        assert rec.enrolEmbedding("first", synth.make_gallery(1)[0]) == 0   # never loaded: becomes row 0
        assert rec.matchTop1()[0] == ["first"]
        gal = synth.make_gallery(300)
        rec.setGallery(gal, ["u%d" % i for i in range(300)])
        rec.initMatMul()
        assert rec.enrolEmbedding(["alice", "bob"], np.stack([emb[0], emb[0]])) == 300 and rec.classCount == 302
        assert rec.matchTop1()[0] == ["alice"]
        assert rec.removeClass("alice") == 1 and rec.removeClass("u7") == 1 and rec.removeClass("nobody") == 0
        names, sims = rec.matchTop1()
        assert names == ["bob"] and sims[0] > 0.9999 and rec.classCount == 300 == rec.matmul.m
        full = rec.featureMatching()
        assert full.shape == (1, 300) and rec.getOutputs(full)[0] == ["bob"]
    finally:
        rec.close()
