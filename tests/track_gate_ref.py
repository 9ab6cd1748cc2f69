"""The tracker's gate (include/frt.h, "Gate"), restated in numpy: G1 presence, G2 the peek, G3 follow or embed, G4 the records, and the
recogniser's work list with its pass counts.  This is the contract track_gate_kernel (kernels_track.hip) is held to, record for record and
entry for entry; nothing here calls the library.  The peek is not written a second time: it IS step 2 of track_ref.Tracker.update, run on a
throwaway copy of the stream's slots."""
import numpy as np

import track_ref as tk
from tiled_ref import overlap

BBOX_DTYPE = np.dtype([("x1", "<i4"), ("y1", "<i4"), ("x2", "<i4"), ("y2", "<i4"), ("score", "<f4")])  # == frt_bbox
GATE_DTYPE = np.dtype([("decision", "<i4"), ("slot", "<i4"), ("ovr", "<f4"), ("why", "<i4")])            # == frt_track_gate
assert GATE_DTYPE.itemsize == 16
ABSENT, EMBED, FOLLOW = 0, 1, 2
NO_TRACK, UNCONFIRMED, FEW_EMBEDS, LOW_OVERLAP, REFRESH = 1, 2, 4, 8, 16
ABSENT_RECORD = np.array((ABSENT, -1, 0.0, 0), GATE_DTYPE)
LIST_FILL = -1  # what the list holds behind its n_embed entries


def check_options(refresh, min_embeds, skip_iou):
    """True where the library accepts the options (a NaN fails the comparison)"""
    return bool(refresh >= 1 and min_embeds >= 1 and np.float32(skip_iou) > 0 and np.float32(skip_iou) <= 1)


def present_mask(boxes, n_boxes=None):
    """G1: boxes [max_faces] of one frame, n_boxes its count or None"""
    p = boxes["score"] > 0
    if n_boxes is not None:
        p &= np.arange(len(boxes)) < int(n_boxes)
    return p


def peek(slots, boxes, present, iou_threshold):
    """G2: slots STATE_DTYPE [max_tracks] at entry -> (peek int [max_faces], ovr float32 [max_faces]).  The association is the update's: a
    twin tracker that holds a copy of the slots takes one update of the present boxes, valid 0 everywhere, and never expires anything
    (max_missed 2^30), so a birth can only land in a slot that was free at entry; a detection whose record names a slot live at entry was
    matched by step 2."""
    T, MF = len(slots), len(boxes)
    twin = tk.Tracker(1, T, MF, 4, iou_threshold=iou_threshold, max_missed=2 ** 30, min_hits=1)
    twin.slots[0] = slots
    res = np.zeros(MF, tk.RESULT_DTYPE)
    for k in ("x1", "y1", "x2", "y2"):
        res[k] = boxes[k]
    res["score"] = np.where(present, boxes["score"], np.float32(0))
    tracks, _ = twin.update(res, np.zeros((MF, 4), np.float32))
    out, ovr = np.full(MF, -1), np.zeros(MF, np.float32)
    for d in range(MF):
        t = int(tracks[0, d]["slot"])
        if present[d] and t >= 0 and slots[t]["live"] != 0:
            out[d], ovr[d] = t, np.float32(overlap(tk._box(boxes[d]), tk._box(slots[t]), 0))
    return out, ovr


def gate_frame(slots, boxes, n_boxes, iou_threshold, min_hits, refresh, min_embeds, skip_iou):
    """G1 - G4 of one frame -> GATE_DTYPE [max_faces]"""
    assert check_options(refresh, min_embeds, skip_iou)
    MF = len(boxes)
    present = present_mask(boxes, n_boxes)
    pk, ovr = peek(slots, boxes, present, iou_threshold)
    out = np.empty(MF, GATE_DTYPE)
    out[:] = ABSENT_RECORD
    for d in np.nonzero(present)[0]:
        t = int(pk[d])
        if t < 0:
            out[d] = (EMBED, -1, 0.0, NO_TRACK)
            continue
        hits, ne = int(slots[t]["hits"]), int(slots[t]["n_embeds"])
        why = 0
        if hits < min_hits:
            why |= UNCONFIRMED
        if ne < min_embeds:
            why |= FEW_EMBEDS
        if not ovr[d] >= np.float32(skip_iou):
            why |= LOW_OVERLAP
        if (hits + 1) % refresh == 0:
            why |= REFRESH
        out[d] = (EMBED if why else FOLLOW, t, ovr[d], why)
    return out


def work_list(gate, max_batch):
    """gate GATE_DTYPE [n_frames, max_faces] -> (list int32 [n_frames * max_faces], n_embed, pass_count int32 [ceil(F / max_batch)])"""
    flat = gate.reshape(-1)
    F = flat.size
    idx = np.nonzero(flat["decision"] == EMBED)[0].astype(np.int32)
    lst = np.full(F, LIST_FILL, np.int32)
    lst[:len(idx)] = idx
    passes = -(-F // max_batch)
    pc = np.clip(len(idx) - np.arange(passes, dtype=np.int64) * max_batch, 0, max_batch).astype(np.int32)
    return lst, len(idx), pc


def gate(slots_by_frame, boxes, n_boxes, iou_threshold, min_hits, refresh, min_embeds, skip_iou, max_batch):
    """One call: slots_by_frame STATE_DTYPE [n_frames, max_tracks] - the slots AT ENTRY of each frame's stream -, boxes BBOX_DTYPE
    [n_frames, max_faces], n_boxes [n_frames] or None -> (gate records, list, n_embed, pass_count)"""
    boxes = np.asarray(boxes)
    n = boxes.shape[0]
    rec = np.stack([gate_frame(slots_by_frame[f], boxes[f], None if n_boxes is None else n_boxes[f], iou_threshold, min_hits, refresh, min_embeds,
                               skip_iou) for f in range(n)])
    return (rec,) + work_list(rec, max_batch)
