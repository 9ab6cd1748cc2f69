"""Large photos by tiles on the GPU (frt_cut_tiles, frt_merge_boxes, frt_detector_find_faces_tiled): everything is compared for exact
equality - ints, score bits, source indices, bytes.  The reference is never the code under test: it is tests/tiled_ref.py (numpy) around the
EXISTING findFaceBatch / findFaceLandmarks / resizeFrame, whose own tests stand.

Detector: the synthetic `det` blob, frame = input = 96 x 160, max_batch 4, max_faces 8, nms 0.4, bbox threshold 0.02."""
import numpy as np
import pytest

import tiled_ref as tr

pytestmark = pytest.mark.gpu
T_R, T_C, BATCH, SLOTS, NMS, BBOX = 96, 160, 4, 8, 0.4, 0.02


def make_det(frt, blobs, kind="det", frame=(T_R, T_C)):
    path, _ = blobs(kind)
    return frt.RetinaFace(path, frame[1], frame[0], (3, T_R, T_C), BATCH, SLOTS, NMS, BBOX)


def same(got, want):
    """(out, src, n) of the library against the reference's, whole arrays: the zeros and -1 behind the count included"""
    assert got[2] == want[2], (got[2], want[2])
    assert np.array_equal(got[1], want[1]), (got[1][:got[2]], want[1][:want[2]])
    assert got[0].tobytes() == want[0].tobytes()


# ------------------------------------------------------------------------------------------------------------------- 1. cut alone
@pytest.mark.parametrize("rows,cols,tile,strided", [(200, 410, (96, 160), True), (60, 300, (96, 160), False), (96, 160, (96, 160), False),
                                                    (97, 161, (96, 160), False), (200, 410, (96, 161), False)])
@pytest.mark.parametrize("overview", [False, True])
def test_cut_alone(frt, synth, rows, cols, tile, strided, overview):
    img = synth.make_frames(1, rows, cols)[0]
    if strided:  # row_stride = cols * 3 + 5
        wide = np.full((rows, cols * 3 + 5), 77, np.uint8)
        wide[:, :cols * 3] = img.reshape(rows, -1)
        view = wide[:, :cols * 3].reshape(rows, cols, 3)
        assert view.strides[0] == cols * 3 + 5
    else:
        view = img
    tiles = tr.plan(rows, cols, tile[0], tile[1], 32, 32, overview)
    if (rows, cols) == (97, 161):
        assert [(int(t["row0"]), int(t["col0"])) for t in tiles[:4]] == [(0, 0), (0, 1), (1, 0), (1, 1)]
    want = tr.cut(img, tiles, tile[0], tile[1], resize=frt.resizeFrame)
    got = frt.cutTiles(view, tiles, tile[0], tile[1])
    assert got.shape == want.shape and got.tobytes() == want.tobytes()
    assert np.array_equal(frt.tilePlan(rows, cols, tile[0], tile[1], 32, overview), tiles)


# ------------------------------------------------------------------------------------------------------------------- 2. merge alone
def both(frt, boxes, n_boxes, tiles, photo, metric, drop_cut, thr, max_out, tile=(T_R, T_C), stats=None):
    want = tr.merge(boxes, n_boxes, tiles, photo[0], photo[1], tile[0], tile[1], metric, drop_cut, thr, max_out, stats=stats)
    got = frt.mergeBoxes(boxes, n_boxes, tiles, photo[0], photo[1], tile[0], tile[1], metric, drop_cut, thr, max_out, full=True)
    same(got, want)
    return want


def random_boxes(rng, n_tiles, slots, ties=False, full=False, size=60, least=4):
    b = np.zeros((n_tiles, slots), tr.BBOX_DTYPE)
    n = np.full(n_tiles, slots, np.int32) if full else rng.integers(0, slots + 1, n_tiles).astype(np.int32)
    x1 = rng.integers(0, T_R - 8, b.shape)
    y1 = rng.integers(0, T_C - 8, b.shape)
    b["x1"], b["y1"] = x1, y1
    b["x2"] = np.minimum(x1 + rng.integers(least, size, b.shape), T_R - 1)
    b["y2"] = np.minimum(y1 + rng.integers(least, size, b.shape), T_C - 1)
    b["score"] = rng.integers(1, 6, b.shape) / 8.0 if ties else rng.random(b.shape, np.float32)
    return b, n


def boxes_of(rows, slots=None):
    slots = slots or max(1, max(len(r) for r in rows))
    b = np.zeros((len(rows), slots), tr.BBOX_DTYPE)
    for t, r in enumerate(rows):
        for s, v in enumerate(r):
            b[t, s] = v
    return b, np.array([len(r) for r in rows], np.int32)


@pytest.mark.parametrize("metric", [0, 1])
def test_merge_random_lists_and_ties(frt, metric):
    """3 tiles x 8 slots (a 60 x 300 photo's plan, the tiles padded below), then equal scores across tiles and slots: tile / slot order decides"""
    rng = np.random.Generator(np.random.PCG64(21 + metric))
    tiles = tr.plan(60, 300, T_R, T_C, 32, 32, False)
    assert len(tiles) == 3
    suppressed = 0
    for k in range(6):
        b, n = random_boxes(rng, 3, 8, ties=k >= 3, size=90, least=40)
        for drop_cut in (False, True):
            st = {}
            want = both(frt, b, n, tiles, (60, 300), metric, drop_cut, 0.3, 256, stats=st)
            suppressed += st["candidates"] - want[2]
    print("suppressed in all", suppressed)
    assert suppressed > 10
    # every score equal, every box the same place in the photo: the first tile's first slot wins
    tiles = tr.plan(200, 410, T_R, T_C, 32, 32, False)
    b, n = boxes_of([[(70 - int(t["row0"]), 135 - int(t["col0"]), 85 - int(t["row0"]), 150 - int(t["col0"]), .5)] * 2 if t["row0"] <= 64 and 0 < t["col0"] <= 128 else []
                     for t in tiles], slots=2)
    want = both(frt, b, n, tiles, (200, 410), metric, False, 0.4, 16)
    assert want[2] == 1 and want[1][0] == 1 * 2 + 0


@pytest.mark.parametrize("metric", [0, 1])
def test_merge_threshold_is_inclusive_and_max_out_caps(frt, metric):
    tiles = tr.plan(T_R, T_C, T_R, T_C, 0, 0, False)
    # areas 64 and 32, intersection 32: IoU = 32 / 64 and inter / smaller = 32 / 32, both exact in float32
    b, n = boxes_of([[(0, 0, 7, 7, .9), (0, 0, 3, 7, .8)]])
    thr = 0.5 if metric == 0 else 1.0
    assert both(frt, b, n, tiles, (T_R, T_C), metric, False, thr, 8)[2] == 1
    assert both(frt, b, n, tiles, (T_R, T_C), metric, False, float(np.nextafter(np.float32(thr), np.float32(2))), 8)[2] == 2
    # survivors > max_out
    rng = np.random.Generator(np.random.PCG64(3))
    tiles = tr.plan(200, 410, T_R, T_C, 32, 32, True)
    b, n = random_boxes(rng, len(tiles), 8, full=True, size=20)
    assert both(frt, b, n, tiles, (200, 410), metric, False, 0.4, 256)[2] > 30
    for max_out in (1, 7, 30):
        assert both(frt, b, n, tiles, (200, 410), metric, False, 0.4, max_out)[2] == max_out


def test_merge_empty_tiles_nan_and_the_map(frt):
    tiles = tr.plan(200, 410, T_R, T_C, 32, 32, True)
    rng = np.random.Generator(np.random.PCG64(4))
    b, n = random_boxes(rng, len(tiles), 8, full=True)
    # all tiles empty: zeros, -1, n_out 0 (the boxes behind the counts are never read as candidates)
    want = both(frt, b, np.zeros(len(tiles), np.int32), tiles, (200, 410), 1, True, 0.4, 16)
    assert want[2] == 0 and (want[1] == -1).all() and not want[0].tobytes().strip(b"\0")
    n[::2] = 0  # some tiles empty
    assert both(frt, b, n, tiles, (200, 410), 0, False, 0.4, 64)[2] > 0
    # a NaN score is never a candidate, even as the only box; -0 and +0 are one score
    b2, n2 = boxes_of([[(1, 1, 9, 9, np.nan), (20, 20, 30, 30, -0.0)], [(40, 2, 50, 12, 0.0)]] + [[]] * (len(tiles) - 2))
    want = both(frt, b2, n2, tiles, (200, 410), 0, False, 0.4, 16)
    assert want[1][:want[2]].tolist() == [1, 2]
    # the four cut edges on an inner tile, and the same edges on the photo's border (not cut)
    rows = [[] for _ in tiles]
    rows[4] = [(0, 30, 9, 40, .9), (30, 0, 40, 9, .8), (80, 30, 95, 40, .7), (30, 150, 40, 159, .6), (20, 60, 30, 70, .5)]  # tile (64, 128): inner
    rows[0] = [(0, 30, 9, 40, .45), (30, 0, 40, 9, .4)]                                                                    # top / left border
    rows[8] = [(80, 30, 95, 40, .35), (30, 150, 40, 159, .3)]                                                              # bottom / right border
    b3, n3 = boxes_of(rows)
    st = {}
    want = both(frt, b3, n3, tiles, (200, 410), 1, True, 0.4, 16, stats=st)
    assert st["cut"] == 4 and sorted(want[1][:want[2]].tolist()) == [0, 1, 4 * 5 + 4, 8 * 5, 8 * 5 + 1]
    assert both(frt, b3, n3, tiles, (200, 410), 1, False, 0.4, 16)[2] == 9
    # a padded tile: one box wholly in the padding (dropped), one straddling it (clipped)
    tp = tr.plan(60, 300, T_R, T_C, 32, 32, False)
    b4, n4 = boxes_of([[(70, 5, 90, 30, .9), (50, 5, 95, 30, .8)], [], []])
    want = both(frt, b4, n4, tp, (60, 300), 0, True, 0.4, 4)
    assert want[2] == 1 and tuple(want[0][0])[:4] == (50, 5, 59, 30)
    # the overview's map on a photo that is no multiple of the tile
    to = tr.plan(211, 397, T_R, T_C, 32, 32, True)
    rows = [[] for _ in to]
    rows[-1] = [(0, 0, 95, 159, .9), (10, 20, 10, 20, .8), (95, 159, 95, 159, .7), (33, 77, 60, 120, .6)]
    b5, n5 = boxes_of(rows)
    want = both(frt, b5, n5, to, (211, 397), 0, False, 0.99, 8)
    assert tuple(want[0][0])[:4] == (0, 0, 210, 396) and want[2] == 4


CLOUD = {}


def cloud(n_tiles, slots):
    """n_tiles x slots full slots on a square photo (300 pixels, 600 for the largest), tiles at random origins (a multi-scale scheme of the
    caller's own) -> boxes, n_boxes, tiles, the photo's side"""
    if (n_tiles, slots) not in CLOUD:
        rng = np.random.Generator(np.random.PCG64(n_tiles * 31 + slots))
        side = 600 if n_tiles * slots > 2000 else 300
        tiles = np.zeros(n_tiles, tr.TILE_DTYPE)
        tiles["row0"] = rng.integers(0, side - T_R + 1, n_tiles)
        tiles["col0"] = rng.integers(0, side - T_C + 1, n_tiles)
        tiles["rows"], tiles["cols"] = T_R, T_C
        b, n = random_boxes(rng, n_tiles, slots, full=True, size=40)
        CLOUD[(n_tiles, slots)] = (b, n, tiles, side)
    return CLOUD[(n_tiles, slots)]


@pytest.mark.parametrize("n_tiles,slots", [(255, 1), (32, 8), (257, 1), (205, 5), (2048, 8)])
def test_merge_sizes_around_the_block_edges(frt, n_tiles, slots):
    """255 / 256 / 257 / 1025 / 16384 candidates: below, at and above one rank block, several mask words, the most there may be"""
    b, n, tiles, side = cloud(n_tiles, slots)
    assert n_tiles * slots in (255, 256, 257, 1025, 16384)
    metric = n_tiles % 2
    st = {}
    want = both(frt, b, n, tiles, (side, side), metric, False, 0.4, 16384, stats=st)
    assert st["candidates"] == n_tiles * slots and want[2] < st["candidates"]


def test_merge_leaves_no_state_behind(frt):
    """a small call after a larger one: same buffers, nothing stale"""
    b, n, tiles, side = cloud(205, 5)
    big = frt.mergeBoxes(b, n, tiles, side, side, T_R, T_C, 1, False, 0.4, 1024, full=True)
    sb, sn, st, sside = cloud(32, 8)
    both(frt, sb, sn, st, (sside, sside), 1, False, 0.4, 1024)
    assert big[2] > 100
    same(frt.mergeBoxes(b, n, tiles, side, side, T_R, T_C, 1, False, 0.4, 1024, full=True), big)


# ------------------------------------------------------------------------------------------------------------------- 3. end to end
@pytest.fixture(scope="module")
def det(frt, blobs):
    d = make_det(frt, blobs)
    yield d
    d.close()


def tile_boxes(frt, detector, photo, frame=(T_R, T_C), landmarks=False):
    """The loop a user writes today: numpy cut (overview included, it is the last tile), findFaceBatch per chunk of max_batch tiles
    -> (tiles, boxes [n][SLOTS], n_boxes, chunks[, landmarks [n][SLOTS][5][2]])."""
    tiles = tr.plan(photo.shape[0], photo.shape[1], frame[0], frame[1], 32, 32, True)
    frames = tr.cut(photo, tiles, frame[0], frame[1], resize=frt.resizeFrame)
    boxes = np.zeros((len(tiles), SLOTS), tr.BBOX_DTYPE)
    n = np.zeros(len(tiles), np.int32)
    ldm = np.zeros((len(tiles), SLOTS, 5, 2), np.float32)
    chunks = 0
    for first in range(0, len(tiles), BATCH):
        chunks += 1
        if landmarks:
            found = []
            for f in frames[first:first + BATCH]:
                bx, lm = detector.findFaceLandmarks(f)
                ldm[first + len(found), :len(bx)] = lm
                found.append(bx)
        else:
            found = detector.findFaceBatch(frames[first:first + BATCH])
        for i, bx in enumerate(found):
            boxes[first + i, :len(bx)] = bx
            n[first + i] = len(bx)
    return (tiles, boxes, n, chunks) + ((ldm,) if landmarks else ())


@pytest.fixture(scope="module")
def photo_ref(frt, synth, det):
    out = {}
    for shape in ((200, 410), (60, 300)):
        photo = synth.make_frames(1, *shape)[0]
        out[shape] = (photo,) + tile_boxes(frt, det, photo)
    return out


def expect(ref, shape, overview, metric, drop_cut, max_out=128, thr=NMS, stats=None):
    photo, tiles, boxes, n, chunks = ref[shape]
    k = len(tiles) - (0 if overview else 1)
    return tr.merge(boxes[:k], n[:k], tiles[:k], shape[0], shape[1], T_R, T_C, metric, drop_cut, np.float32(thr), max_out, stats=stats)


def found(detector, photo, max_out=128, **kw):
    boxes, src = detector.findFaceTiled(photo, overlap=32, max_out=max_out, sources=True, **kw)
    out = np.zeros(max_out, tr.BBOX_DTYPE)
    s = np.full(max_out, -1, np.int32)
    out[:len(boxes)], s[:len(src)] = boxes, src
    return out, s, len(boxes)


@pytest.mark.parametrize("overview", [False, True])
@pytest.mark.parametrize("drop_cut", [False, True])
@pytest.mark.parametrize("metric", [0, 1])
def test_end_to_end_equals_the_loop_a_user_writes(det, photo_ref, metric, drop_cut, overview):
    photo, tiles, boxes, n, chunks = photo_ref[(200, 410)]
    st = {}
    want = expect(photo_ref, (200, 410), overview, metric, drop_cut, stats=st)
    print("reference: tiles %d chunks %d candidates %d cut %d cross-tile suppressions %d kept %d" % (len(tiles), chunks, st["candidates"], st["cut"], st["cross_tile"], want[2]))
    assert len(tiles) == 10 and chunks >= 3 and st["cross_tile"] >= 1 and st["cut"] >= 1  # asserted ON THE REFERENCE
    same(found(det, photo, overview=overview, metric=metric, drop_cut=drop_cut), want)


def test_end_to_end_on_a_padded_photo_and_the_defaults(det, photo_ref):
    photo = photo_ref[(60, 300)][0]
    st = {}
    want = expect(photo_ref, (60, 300), True, 1, True, stats=st)
    print("reference: candidates %d cut %d cross-tile suppressions %d kept %d" % (st["candidates"], st["cut"], st["cross_tile"], want[2]))
    assert st["cross_tile"] >= 1 and st["cut"] >= 1
    same(found(det, photo, overview=True, metric=1, drop_cut=True), want)
    # a threshold of the caller's, and max_out below the survivors
    same(found(det, photo, overview=True, metric=0, drop_cut=False, threshold=0.25), expect(photo_ref, (60, 300), True, 0, False, thr=0.25))
    same(found(det, photo, max_out=3, overview=True, metric=0, drop_cut=False), expect(photo_ref, (60, 300), True, 0, False, max_out=3))
    # the defaults: overlap a quarter of the tile, overview, metric 1, cut boxes dropped, the detector's threshold
    big = photo_ref[(200, 410)][0]
    assert det.findFaceTiled(big).tobytes() == det.findFaceTiled(big, overlap=(T_R // 4, T_C // 4), overview=True, metric=1, drop_cut=True, threshold=NMS).tobytes()


# ------------------------------------------------------------------------------------------------------------------- 4. one tile
def test_one_tile_is_find_face(det, synth):
    for seed in (0, 1, 2):
        photo = synth.make_frames(seed + 1, T_R, T_C)[seed]
        want = det.findFace(photo)
        got, src = det.findFaceTiled(photo, overlap=32, overview=False, metric=0, drop_cut=False, sources=True)
        assert len(want) > 0 and got.tobytes() == want.tobytes() and src.tolist() == list(range(len(want)))


# ------------------------------------------------------------------------------------------------------------------- 5. letterboxed detector
def test_letterboxed_detector(frt, blobs, synth):
    """frame 128 x 192 on the 96 x 160 input: the tile is the FRAME, the detector's own letterbox stays in play"""
    d = make_det(frt, blobs, frame=(128, 192))
    photo = synth.make_frames(1, 200, 410)[0]
    tiles, boxes, n, chunks = tile_boxes(frt, d, photo, frame=(128, 192))
    assert n.sum() > 8
    for metric, drop_cut in ((0, False), (1, True)):
        want = tr.merge(boxes, n, tiles, 200, 410, 128, 192, metric, drop_cut, np.float32(NMS), 128)
        same(found(d, photo, overview=True, metric=metric, drop_cut=drop_cut), want)
    d.close()


# ------------------------------------------------------------------------------------------------------------------- 6. landmarks
def test_landmarks_follow_their_boxes(frt, blobs, synth, det):
    d = make_det(frt, blobs, kind="det_ldm")
    photo = synth.make_frames(1, 200, 410)[0]
    tiles, boxes, n, chunks, ldm = tile_boxes(frt, d, photo, landmarks=True)
    # a threshold that keeps nearly every candidate: boxes of the grid tiles AND of the overview survive, so both maps are checked
    want = tr.merge(boxes, n, tiles, 200, 410, T_R, T_C, 0, False, np.float32(0.99), 96)
    got, lm, src = d.findFaceTiled(photo, overlap=32, overview=True, metric=0, drop_cut=False, threshold=0.99, max_out=96, landmarks=True, sources=True)
    assert len(got) == want[2] and got.tobytes() == want[0][:want[2]].tobytes() and np.array_equal(src, want[1][:want[2]])
    assert (tiles[src // SLOTS]["kind"] == 1).any() and (tiles[src // SLOTS]["kind"] == 0).any()
    assert lm.tobytes() == tr.map_landmarks(ldm, src, tiles, SLOTS, 200, 410, T_R, T_C).tobytes()
    d.close()
    with pytest.raises(frt.FrtError) as e:  # the trimmed blob has no LandmarkHead
        det.findFaceTiled(photo, landmarks=True)
    assert e.value.code == frt.FRT_ERR_FORMAT


# ------------------------------------------------------------------------------------------------------------------- 7. state across calls
def test_state_across_calls(frt, blobs, synth, photo_ref):
    """three photos of different sizes in turn, then findFace and findFaceBatch on plain frames: a fresh detector's answers"""
    fresh = make_det(frt, blobs)
    frames = synth.make_frames(BATCH, T_R, T_C)
    want_one, want_batch = fresh.findFace(frames[0]), fresh.findFaceBatch(frames)
    fresh.close()
    used = make_det(frt, blobs)
    small = synth.make_frames(1, 50, 70)[0]
    first = found(used, photo_ref[(200, 410)][0], overview=True, metric=1, drop_cut=True)
    same(first, expect(photo_ref, (200, 410), True, 1, True))
    assert found(used, small, overview=True, metric=1, drop_cut=True)[2] >= 0
    same(found(used, photo_ref[(60, 300)][0], overview=False, metric=0, drop_cut=False), expect(photo_ref, (60, 300), False, 0, False))
    same(found(used, photo_ref[(200, 410)][0], overview=True, metric=1, drop_cut=True), first)
    assert used.findFace(frames[0]).tobytes() == want_one.tobytes()
    got = used.findFaceBatch(frames)
    assert len(got) == len(want_batch) and all(a.tobytes() == b.tobytes() for a, b in zip(got, want_batch))
    used.close()
