"""Recognising a large photo by tiles (include/frt.h, "Recognising a large photo by tiles"), restated in numpy: the gate, the stable
compaction and pass_count - and the loop a user writes today around the EXISTING findFaceTiled / forward / forwardAligned / MatMul.top1,
whose own tests stand.  Nothing here calls the code under test (frt_select_faces, frt_pipeline_run_photo_tiled)."""
import numpy as np

BBOX_DTYPE = np.dtype([("x1", "<i4"), ("y1", "<i4"), ("x2", "<i4"), ("y2", "<i4"), ("score", "<f4")])
RESULT_DTYPE = np.dtype([("x1", "<i4"), ("y1", "<i4"), ("x2", "<i4"), ("y2", "<i4"), ("score", "<f4"), ("frame", "<i4"),
                         ("match_idx", "<i4"), ("match_sim", "<f4"), ("valid", "<i4")])
MAX_OUT = 16384


def gate(boxes, min_face):
    """kept iff min(x2 - x1, y2 - y1) >= min_face: the crop's ROI extents, far corner excluded; min_face <= 0 keeps everything"""
    b = np.asarray(boxes, BBOX_DTYPE)
    if min_face <= 0:
        return np.ones(len(b), bool)
    return np.minimum(b["x2"].astype(np.int64) - b["x1"], b["y2"].astype(np.int64) - b["y1"]) >= min_face


def pass_count(n_kept, cap, max_batch):
    """faces of recogniser pass j, j < ceil(cap / max_batch)"""
    return np.array([min(max(n_kept - j * max_batch, 0), max_batch) for j in range(-(-cap // max_batch))], np.int32)


def select(boxes, src=None, landmarks=None, min_face=0, max_batch=128):
    """-> dict of the whole arrays (length n = len(boxes)): the kept entries dense and in order, zeros / -1 behind n_kept"""
    b = np.asarray(boxes, BBOX_DTYPE).reshape(-1)
    n = len(b)
    assert 0 <= n <= MAX_OUT and max_batch >= 1
    keep = np.flatnonzero(gate(b, min_face))
    k = len(keep)
    out = dict(boxes=np.zeros(n, BBOX_DTYPE), src=None, landmarks=None, keep_pos=np.full(n, -1, np.int32), n_kept=k,
               pass_count=pass_count(k, n, max_batch))
    out["boxes"][:k] = b[keep]
    out["keep_pos"][:k] = keep
    if src is not None:
        out["src"] = np.full(n, -1, np.int32)
        out["src"][:k] = np.asarray(src, np.int32)[keep]
    if landmarks is not None:
        out["landmarks"] = np.zeros((n, 5, 2), np.float32)
        out["landmarks"][:k] = np.asarray(landmarks, np.float32).reshape(n, 5, 2)[keep]
    return out


def same_selection(got, want):
    assert got["n_kept"] == want["n_kept"], (got["n_kept"], want["n_kept"])
    for key in ("boxes", "src", "landmarks", "keep_pos", "pass_count"):
        if want[key] is None:
            assert got[key] is None, key
        else:
            assert got[key].shape == want[key].shape and got[key].tobytes() == want[key].tobytes(), key


def loop(frt, det, rec, photo, min_face=0, max_out=256, align=False, match=True, **tiled):
    """The loop of the header's semantics on existing entry points -> dict(results [max_out] as the pack kernel leaves them, src [max_out],
    landmarks [max_out][5][2] or None, embeds [n][512], crops [n][112][112][3], n, merged = the list before the gate)."""
    photo = np.ascontiguousarray(photo, np.uint8)
    if align:
        boxes, ldm, src = det.findFaceTiled(photo, max_out=max_out, landmarks=True, sources=True, **tiled)
    else:
        boxes, src = det.findFaceTiled(photo, max_out=max_out, sources=True, **tiled)
        ldm = None
    keep = np.flatnonzero(gate(boxes, min_face))
    kb = np.ascontiguousarray(boxes[keep])
    n = len(kb)
    embeds = np.zeros((n, 512), np.float32)
    crops = np.zeros((n, 112, 112, 3), np.uint8)
    valid = np.ones(n, np.int32)
    if n:
        import ctypes
        p = lambda a: ctypes.c_void_p(a.ctypes.data)
        if align:
            kl = np.ascontiguousarray(ldm[keep]).reshape(-1, 10)
            rc = frt.lib.frt_embedder_forward_aligned(rec._h, p(photo), photo.shape[0], photo.shape[1], photo.strides[0], p(kl), n, p(embeds), p(crops))
        else:
            rc = frt.lib.frt_embedder_forward(rec._h, p(photo), photo.shape[0], photo.shape[1], photo.strides[0], p(kb), n, p(embeds), p(crops))
        assert rc in (frt.FRT_OK, frt.FRT_ERR_EMPTY_ROI), frt.lib.frt_last_error()
        valid = (np.abs(embeds).sum(1) > 0).astype(np.int32)  # an empty ROI: an all-zero embedding (every other one has norm 1)
    res = np.zeros(max_out, RESULT_DTYPE)
    res["match_idx"] = -1
    for c in ("x1", "y1", "x2", "y2", "score"):
        res[c][:n] = kb[c]
    res["valid"][:n] = valid
    if match and n and rec.matmul.m > 0:
        idx, sim = rec.matmul.top1(embeds)
        ok = valid != 0
        res["match_idx"][:n][ok] = idx[ok]
        res["match_sim"][:n][ok] = sim[ok]
    s = np.full(max_out, -1, np.int32)
    s[:n] = src[keep]
    lm = None
    if align:
        lm = np.zeros((max_out, 5, 2), np.float32)
        lm[:n] = ldm[keep]
    return dict(results=res, src=s, landmarks=lm, embeds=embeds, crops=crops, n=n, merged=boxes, merged_src=src)
