"""tests/tiled_ref.py against its own definitions: the plan's coverage properties and count formula, the cut's padding, the map of the
overview and of padded tiles, and the vectorised greedy merge against the brute-force O(n^2) restatement.  No GPU, no library."""
import math

import numpy as np
import pytest

import tiled_ref as tr

AXES = [(L, T, V) for T in (7, 96, 160) for V in sorted({0, 1, T // 4, T - 1}) for L in list(range(1, 3 * T + 3, max(1, T // 7))) + [T, T + 1, 2 * T - V, 2 * T - V + 1]]


def test_axis_covers_every_pixel_stays_inside_and_counts_by_the_formula():
    for L, T, V in AXES:
        o = tr.axis_origins(L, T, V)
        S = T - V
        assert len(o) == (1 if L <= T else math.ceil((L - T) / S) + 1), (L, T, V)
        assert o[0] == 0 and o == sorted(o)
        covered = np.zeros(L, bool)
        for a in o:
            covered[a:a + T] = True
        assert covered.all(), (L, T, V)
        if L >= T:
            assert all(a + T <= L for a in o), (L, T, V)      # never padded: the last tile is pulled inward
            assert o[-1] == L - T
        assert all(b - a <= S for a, b in zip(o, o[1:])), (L, T, V)  # neighbours share at least V pixels
        assert len(set(o)) == len(o)


def test_plan_is_the_row_major_product_with_the_overview_last():
    for rows, cols, ov in ((200, 410, True), (60, 300, False), (96, 160, True), (97, 161, False), (1, 1, True)):
        t = tr.plan(rows, cols, 96, 160, 32, 32, ov)
        ro, co = tr.axis_origins(rows, 96, 32), tr.axis_origins(cols, 160, 32)
        grid = t[:len(ro) * len(co)]
        assert len(t) == len(ro) * len(co) + ov
        assert [(int(a), int(b)) for a, b in zip(grid["row0"], grid["col0"])] == [(r, c) for r in ro for c in co]
        assert (grid["kind"] == 0).all() and (grid["rows"] == np.minimum(96, rows - grid["row0"])).all() and (grid["cols"] == np.minimum(160, cols - grid["col0"])).all()
        if ov:
            assert tuple(t[-1]) == (0, 0, rows, cols, 1)
    assert [tuple(x) for x in tr.plan(97, 161, 96, 160, 32, 32, False)] == [(0, 0, 96, 160, 0), (0, 1, 96, 160, 0), (1, 0, 96, 160, 0), (1, 1, 96, 160, 0)]


def test_cut_pads_with_128_and_hands_the_overview_to_the_resize():
    rng = np.random.Generator(np.random.PCG64(5))
    img = rng.integers(0, 256, (60, 300, 3), dtype=np.uint8)
    t = tr.plan(60, 300, 96, 160, 32, 32, True)
    got = tr.cut(img, t, 96, 160, resize=lambda im, w, h: np.full((h, w, 3), 7, np.uint8))
    assert got.shape == (4, 96, 160, 3) and (got[3] == 7).all()
    for i in range(3):
        assert np.array_equal(got[i, :60], img[:, t[i]["col0"]:t[i]["col0"] + 160]) and (got[i, 60:] == 128).all()


def boxes_of(rows):
    """rows: per tile a list of (x1, y1, x2, y2, score)"""
    slots = max(1, max(len(r) for r in rows))
    b = np.zeros((len(rows), slots), tr.BBOX_DTYPE)
    for t, r in enumerate(rows):
        for s, v in enumerate(r):
            b[t, s] = v
    return b, np.array([len(r) for r in rows], np.int32)


def test_map_cut_test_padding_and_overview():
    tiles = tr.plan(200, 410, 96, 160, 32, 32, True)  # 3 x 4 grid (row origins 0 64 104, column origins 0 128 250 = 410 - 160 ... ) + overview
    assert list(tr.axis_origins(200, 96, 32)) == [0, 64, 104] and list(tr.axis_origins(410, 160, 32)) == [0, 128, 250]
    rows = [[] for _ in tiles]
    rows[0] = [(0, 0, 10, 10, .9), (5, 5, 95, 20, .8), (5, 5, 20, 159, .7)]  # the photo's corner: not cut; bottom edge, right edge: cut
    rows[4] = [(0, 3, 9, 9, .6), (3, 0, 9, 9, .5), (1, 1, 94, 158, .4)]       # tile (64, 128): top and left edges cut; one clear of all edges
    rows[8] = [(50, 50, 95, 159, .3)]                                        # tile (104, 250), the last of both axes: the photo's border, not cut
    rows[9] = [(0, 0, 95, 159, .2), (10, 20, 10, 20, .1)]                    # overview
    b, n = boxes_of(rows)
    c, n_cut = tr.candidates(b, n, tiles, 200, 410, 96, 160, False)
    assert n_cut == 4 and len(c) == 9
    by_src = {x[0]: x[1:5] for x in c}
    assert by_src[4 * 3 + 2] == (65, 129, 158, 286) and by_src[8 * 3] == (154, 300, 199, 409)
    assert by_src[9 * 3] == (0, 0, 199, 409) and by_src[9 * 3 + 1] == (10 * 200 // 96, 20 * 410 // 160, max(11 * 200 // 96 - 1, 10 * 200 // 96), 21 * 410 // 160 - 1)
    c, _ = tr.candidates(b, n, tiles, 200, 410, 96, 160, True)
    assert sorted(x[0] for x in c) == [0, 14, 24, 27, 28]
    # a padded tile (photo 60 x 300): wholly in padding -> dropped, straddling -> clipped; the padded edge is no cut edge
    tiles = tr.plan(60, 300, 96, 160, 32, 32, False)
    b, n = boxes_of([[(70, 5, 90, 30, .9), (50, 5, 95, 30, .8)], [], []])
    c, n_cut = tr.candidates(b, n, tiles, 60, 300, 96, 160, True)
    assert n_cut == 0 and [x[:5] for x in c] == [(1, 50, 5, 59, 30)]
    # NaN is never a candidate; n_boxes beyond the slots means all slots
    b, n = boxes_of([[(1, 1, 5, 5, np.nan), (1, 1, 5, 5, .5)], [], []])
    n[0] = 9
    assert [x[0] for x in tr.candidates(b, n, tiles, 60, 300, 96, 160, False)[0]] == [1]


def random_case(rng, n_tiles_side, slots, photo=(200, 410), tile=(96, 160), ties=False):
    tiles = tr.plan(photo[0], photo[1], tile[0], tile[1], 32, 32, True)
    b = np.zeros((len(tiles), slots), tr.BBOX_DTYPE)
    n = rng.integers(0, slots + 1, len(tiles)).astype(np.int32)
    x1 = rng.integers(0, tile[0] - 8, b.shape)
    y1 = rng.integers(0, tile[1] - 8, b.shape)
    b["x1"], b["y1"] = x1, y1
    b["x2"] = np.minimum(x1 + rng.integers(4, 60, b.shape), tile[0] - 1)
    b["y2"] = np.minimum(y1 + rng.integers(4, 60, b.shape), tile[1] - 1)
    b["score"] = rng.integers(1, 6, b.shape) / 8.0 if ties else rng.random(b.shape, np.float32)
    return b, n, tiles


@pytest.mark.parametrize("metric", [0, 1])
def test_greedy_merge_equals_the_brute_force_restatement(metric):
    rng = np.random.Generator(np.random.PCG64(11 + metric))
    total = 0
    for k in range(12):
        b, n, tiles = random_case(rng, 3, 6, ties=k % 3 == 0)
        for drop_cut in (False, True):
            for max_out in (256, 5):
                args = (b, n, tiles, 200, 410, 96, 160, metric, drop_cut, 0.3 + 0.05 * (k % 4), max_out)
                st = {}
                out, src, cnt = tr.merge(*args, stats=st)
                bout, bsrc, bcnt = tr.merge_brute(*args)
                assert cnt == bcnt and np.array_equal(src, bsrc) and out.tobytes() == bout.tobytes()
                assert (src[cnt:] == -1).all() and not out[cnt:].tobytes().strip(b"\0") and cnt <= min(max_out, st["candidates"])
                sc = out["score"][:cnt]
                assert (sc[:-1] >= sc[1:]).all()
                total += st["candidates"] - cnt
    assert total > 100  # (the lists do suppress)


def test_overlap_is_float32_and_the_threshold_is_inclusive():
    a, b = (0, 0, 0, 9, 9, np.float32(.9)), (1, 0, 5, 9, 14, np.float32(.8))  # inter 50, union 150: 1/3, rounded to float32
    assert tr.overlap(a, b, 0) == np.float32(50) / np.float32(150) and tr.overlap(a, b, 0).dtype == np.float32
    assert tr.overlap(a, b, 1) == np.float32(0.5)
    # areas 64 and 32, inter 32: IoU 32 / 64 = 0.5 exactly, over the smaller area 1.0 exactly
    a, b = (0, 0, 0, 7, 7, np.float32(.9)), (1, 0, 0, 3, 7, np.float32(.8))
    assert tr.overlap(a, b, 0) == 0.5 and tr.overlap(a, b, 1) == 1.0
    tiles = tr.plan(96, 160, 96, 160, 0, 0, False)
    bx, n = boxes_of([[a[1:], b[1:]]])
    assert tr.merge(bx, n, tiles, 96, 160, 96, 160, 0, False, 0.5, 8)[2] == 1
    assert tr.merge(bx, n, tiles, 96, 160, 96, 160, 0, False, np.nextafter(np.float32(0.5), np.float32(1)), 8)[2] == 2
