"""Large photos by tiles (include/frt.h, "Large photos by tiles"), restated in numpy: the plan, the cut, the map into photo coordinates and
the greedy merge.  This is the contract the device code (kernels_tiles.hip) is held to, integer for integer and bit for bit; nothing here
calls the library.  x is the row, y the column, corners inclusive."""
import numpy as np

BBOX_DTYPE = np.dtype([("x1", "<i4"), ("y1", "<i4"), ("x2", "<i4"), ("y2", "<i4"), ("score", "<f4")])
TILE_DTYPE = np.dtype([("row0", "<i4"), ("col0", "<i4"), ("rows", "<i4"), ("cols", "<i4"), ("kind", "<i4")])
MAX_TILES, MAX_CANDIDATES, MAX_OUT = 4096, 16384, 16384


def axis_origins(L, T, V):
    """Origins of the tiles along an axis of length L: tile T, overlap V, stride T - V; the last tile is pulled inward."""
    assert L >= 1 and T >= 1 and 0 <= V < T
    if L <= T:
        return [0]
    S = T - V
    n = -(-(L - T) // S) + 1
    return [min(i * S, L - T) for i in range(n)]


def plan(rows, cols, tile_rows, tile_cols, overlap_rows, overlap_cols, overview):
    tiles = [(r, c, min(tile_rows, rows - r), min(tile_cols, cols - c), 0)
             for r in axis_origins(rows, tile_rows, overlap_rows) for c in axis_origins(cols, tile_cols, overlap_cols)]
    if overview:
        tiles.append((0, 0, rows, cols, 1))
    return np.array(tiles, TILE_DTYPE)


def cut(img, tiles, tile_rows, tile_cols, resize=None):
    """-> u8 [n][tile_rows][tile_cols][3].  resize(img, width, height) makes the overview (the library's resizeFrame, whose own tests stand)."""
    out = np.full((len(tiles), tile_rows, tile_cols, 3), 128, np.uint8)
    for i, t in enumerate(tiles):
        if t["kind"] == 1:
            out[i] = resize(img, tile_cols, tile_rows)
            continue
        part = img[t["row0"]:t["row0"] + tile_rows, t["col0"]:t["col0"] + tile_cols]
        out[i, :part.shape[0], :part.shape[1]] = part
    return out


def _tdiv(a, b):
    """C's integer division (towards zero) of Python ints, b > 0."""
    return a // b if a >= 0 else -((-a) // b)


def _clip(v, hi):
    return max(0, min(int(v), hi))


def candidates(boxes, n_boxes, tiles, photo_rows, photo_cols, tile_rows, tile_cols, drop_cut):
    """-> (list of (src, x1, y1, x2, y2, score) in photo coordinates, in source order; the number of candidates the cut test marks)."""
    slots = boxes.shape[1]
    cands, n_cut = [], 0
    for t, tl in enumerate(tiles):
        row0, col0 = int(tl["row0"]), int(tl["col0"])
        for s in range(min(max(int(n_boxes[t]), 0), slots)):
            b = boxes[t, s]
            if np.isnan(b["score"]):
                continue
            x1, y1, x2, y2 = int(b["x1"]), int(b["y1"]), int(b["x2"]), int(b["y2"])
            if tl["kind"] == 0:
                is_cut = (x1 == 0 and row0 > 0) or (y1 == 0 and col0 > 0) or (x2 == tile_rows - 1 and row0 + tile_rows < photo_rows) or \
                    (y2 == tile_cols - 1 and col0 + tile_cols < photo_cols)
                n_cut += bool(is_cut)
                if drop_cut and is_cut:
                    continue
                x1, x2, y1, y2 = x1 + row0, x2 + row0, y1 + col0, y2 + col0
                if x1 >= photo_rows or y1 >= photo_cols:
                    continue
            else:
                x1, x2 = _tdiv(x1 * photo_rows, tile_rows), _tdiv((x2 + 1) * photo_rows, tile_rows) - 1
                y1, y2 = _tdiv(y1 * photo_cols, tile_cols), _tdiv((y2 + 1) * photo_cols, tile_cols) - 1
                x2, y2 = max(x2, x1), max(y2, y1)
            cands.append((t * slots + s, _clip(x1, photo_rows - 1), _clip(y1, photo_cols - 1), _clip(x2, photo_rows - 1), _clip(y2, photo_cols - 1),
                          np.float32(b["score"])))
    return cands, n_cut


def _area(x1, y1, x2, y2):
    return np.float32((x2 - x1 + 1) * (y2 - y1 + 1))  # the exact integer product, rounded once


def overlap(a, b, metric):
    """float32, operation for operation nms_kernel's ovr (kernels_post.hip); metric 1 divides by the smaller area instead of the union."""
    f = np.float32
    xx1, yy1 = f(max(a[1], b[1])), f(max(a[2], b[2]))
    xx2, yy2 = f(min(a[3], b[3])), f(min(a[4], b[4]))
    w = max(f(f(xx2 - xx1) + f(1)), f(0))
    h = max(f(f(yy2 - yy1) + f(1)), f(0))
    inter = f(w * h)
    aa, ab = _area(*a[1:5]), _area(*b[1:5])
    with np.errstate(divide="ignore", invalid="ignore"):
        if metric == 0:
            return f(inter / f(f(aa + ab) - inter))
        return f(inter / min(aa, ab))


def _ordered(cands):
    """score descending, then source index (tile, then slot) ascending; -0 and +0 are one score"""
    return sorted(cands, key=lambda c: (-float(c[5]), c[0]))


def _emit(kept, max_out):
    out = np.zeros(max_out, BBOX_DTYPE)
    src = np.full(max_out, -1, np.int32)
    for i, c in enumerate(kept):
        out[i] = (c[1], c[2], c[3], c[4], c[5])
        src[i] = c[0]
    return out, src, len(kept)


def merge(boxes, n_boxes, tiles, photo_rows, photo_cols, tile_rows, tile_cols, metric, drop_cut, threshold, max_out, stats=None):
    """The greedy merge -> (out [max_out], src [max_out], n), the overlaps of one winner against all live candidates as float32 arrays.
    stats (a dict) receives: candidates, cut (marked by the cut test, dropped or not), cross_tile (suppressions whose winner lies in
    another tile than the loser)."""
    slots = boxes.shape[1]
    cands, n_cut = candidates(boxes, n_boxes, tiles, photo_rows, photo_cols, tile_rows, tile_cols, drop_cut)
    order = _ordered(cands)
    src = np.array([c[0] for c in order], np.int64)
    x1, y1, x2, y2 = (np.array([c[k] for c in order], np.int64) for k in (1, 2, 3, 4))
    area = ((x2 - x1 + 1) * (y2 - y1 + 1)).astype(np.float32)
    live = np.ones(len(order), bool)
    thr = np.float32(threshold)
    kept, cross = [], 0
    for i in range(len(order)):
        if len(kept) == max_out:
            break
        if not live[i]:
            continue
        kept.append(order[i])
        live[i] = False
        j = np.nonzero(live)[0]
        w = np.minimum(x2[i], x2[j]).astype(np.float32) - np.maximum(x1[i], x1[j]).astype(np.float32) + np.float32(1)
        h = np.minimum(y2[i], y2[j]).astype(np.float32) - np.maximum(y1[i], y1[j]).astype(np.float32) + np.float32(1)
        inter = np.maximum(w, np.float32(0)) * np.maximum(h, np.float32(0))
        with np.errstate(divide="ignore", invalid="ignore"):
            ovr = inter / ((area[i] + area[j]) - inter) if metric == 0 else inter / np.minimum(area[i], area[j])
        assert ovr.dtype == np.float32
        dead = j[ovr >= thr]
        cross += int(((src[dead] // slots) != (src[i] // slots)).sum())
        live[dead] = False
    if stats is not None:
        stats.update(candidates=len(cands), cut=n_cut, cross_tile=int(cross))
    return _emit(kept, max_out)


def merge_brute(boxes, n_boxes, tiles, photo_rows, photo_cols, tile_rows, tile_cols, metric, drop_cut, threshold, max_out):
    """The same result from the definition turned round: in sorted order a candidate is kept exactly when no KEPT earlier one overlaps it at
    the threshold or above; all n x n overlaps are computed first."""
    cands, _ = candidates(boxes, n_boxes, tiles, photo_rows, photo_cols, tile_rows, tile_cols, drop_cut)
    order = _ordered(cands)
    n = len(order)
    thr = np.float32(threshold)
    hit = np.zeros((n, n), bool)
    for i in range(n):
        for j in range(n):
            hit[i, j] = i != j and overlap(order[min(i, j)], order[max(i, j)], metric) >= thr
    is_kept = np.zeros(n, bool)
    for j in range(n):
        is_kept[j] = not (hit[:j, j] & is_kept[:j]).any()
    return _emit([order[j] for j in range(n) if is_kept[j]][:max_out], max_out)


def map_landmarks(ldm, src, tiles, slots, photo_rows, photo_cols, tile_rows, tile_cols):
    """ldm [n_tiles][slots][5][2] (x = column, y = row, tile coordinates) at the source indices src -> [len(src)][5][2] in photo coordinates."""
    out = np.zeros((len(src), 5, 2), np.float32)
    f = np.float32
    for i, sidx in enumerate(src):
        tl = tiles[sidx // slots]
        p = ldm[sidx // slots, sidx % slots].astype(np.float32)
        if tl["kind"] == 0:
            out[i, :, 0] = p[:, 0] + f(tl["col0"])
            out[i, :, 1] = p[:, 1] + f(tl["row0"])
        else:
            out[i, :, 0] = (p[:, 0] * f(photo_cols)) / f(tile_cols)
            out[i, :, 1] = (p[:, 1] * f(photo_rows)) / f(tile_rows)
    return out
