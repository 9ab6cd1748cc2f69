"""Scripted scenes for the sighting book, shared by tests/test_sightings_ref.py (hand-written expectations against the numpy restatement)
and tests/test_gpu_sightings.py (the library against the restatement, byte for byte, after every step).  A script is a list of steps on
the 3 streams x 4 tracks x 3 faces, dim 8 shape: ("update", {stream: [det, ...]}) - the call's frames in the dict's order -, ("close", stream),
("drain", max_out) or ("reset", stream).  Nothing here calls the library."""
import numpy as np

import sightings_ref as sr
import track_ref as tk
from quality_ref import QUALITY_DTYPE

SHAPE = dict(n_streams=3, max_tracks=4, max_faces=3, dim=8)
A, B, C = (10, 10, 50, 50), (100, 100, 140, 140), (200, 10, 240, 50)   # three faces that never overlap


def det(box, sharpness=10.0, size=40, qscore=None, flags=0, valid=1, present=None, score=0.9):
    return dict(box=box, sharpness=sharpness, size=size, qscore=score if qscore is None else qscore, flags=flags, valid=valid,
                present=valid if present is None else present, score=score)


def arrays(frames, max_faces, dim, keep_crops, rng):
    """[[det, ...] per frame] -> results, embeds, quality, crops (or None) of one call; embeddings, crops and the quality fields the book only
    copies are random"""
    n = len(frames)
    res = np.zeros((n, max_faces), tk.RESULT_DTYPE)
    qual = np.zeros((n, max_faces), QUALITY_DTYPE)
    emb = rng.standard_normal((n, max_faces, dim)).astype(np.float32)
    crops = rng.integers(0, 256, (n, max_faces) + sr.CROP, dtype=np.uint8) if keep_crops else None
    res["match_idx"] = -1
    for f, dets in enumerate(frames):
        for d, x in enumerate(dets):
            r, q = res[f, d], qual[f, d]
            r["x1"], r["y1"], r["x2"], r["y2"] = x["box"]
            r["score"], r["frame"], r["valid"] = x["score"], f, x["valid"]
            if x["present"]:
                q["present"], q["flags"], q["sharpness"], q["size"], q["score"] = 1, x["flags"], x["sharpness"], x["size"], x["qscore"]
                q["luma_var"], q["mean"] = rng.random() * 100, rng.random() * 255
    return res.reshape(-1), emb.reshape(-1, dim), qual.reshape(-1), crops.reshape((-1,) + sr.CROP) if keep_crops else None


class RefRig:
    """track_ref.Tracker with a sightings_ref.Book behind it"""

    def __init__(self, capacity, rank=0, min_hits=1, keep_crops=True, max_missed=1, track_min_hits=2, shape=SHAPE):
        self.tracker = tk.Tracker(iou_threshold=0.3, max_missed=max_missed, min_hits=track_min_hits, **shape)
        self.book = sr.Book(capacity=capacity, rank=rank, min_hits=min_hits, keep_crops=keep_crops, **shape)

    def update(self, res, emb, qual, crops, ids, templates="own"):
        """templates: "own" - the restated tracker's, rounded to float32 -, None, or the array to hand to the book"""
        tracks, tpl = self.tracker.update(res, emb, ids)
        if isinstance(templates, str):
            templates = tpl.astype(np.float32)
        slots, ticks = sr.tracker_state(self.tracker, ids)
        self.book.update(slots, ticks, res, tracks, emb, qual, templates, crops, ids)
        return tracks


def run_ref(script, seed=0, **rig):
    """a script on the restatement alone -> (rig, [what each "drain" step returned], [(results, embeds, quality, crops) of each update])"""
    r = RefRig(**rig)
    rng = np.random.default_rng(seed)
    drained, inputs = [], []
    for step in script:
        if step[0] == "update":
            ids = list(step[1])
            inputs.append(arrays([step[1][s] for s in ids], SHAPE["max_faces"], SHAPE["dim"], r.book.keep_crops, rng))
            r.update(*inputs[-1], ids)
        elif step[0] == "close":
            r.book.close(step[1])
        elif step[0] == "drain":
            drained.append(r.book.drain(step[1]))
        elif step[0] == "reset":
            r.tracker.reset(step[1])
    return r, drained, inputs


def one_stream(*frames):
    """updates of stream 0 alone, one per argument"""
    return [("update", {0: list(f)}) for f in frames]


# ---- the scenes.  max_missed is given with each (RefRig's default 1: a track coasts one update and expires on the second)
BIRTH_TO_EXPIRY = one_stream([det(A, 5.0)], [det(A, 9.0)], [det(A, 7.0)], [], []) + [("drain", 8)]
REPLACED = one_stream([det(A)], [det(B)]) + [("drain", 8)]                                     # max_missed 0
DISCARD = one_stream([det(A)], []) + [("drain", 8)]                                            # max_missed 0, book min_hits 2
OVERFLOW = one_stream([det(A), det(B), det(C)], []) + [("drain", 8)]                           # max_missed 0, capacity 2
THREE_RANKS = one_stream([det(A, 9.0, 30, 0.5)], [det(A, 5.0, 50, 0.7)], [det(A, 7.0, 40, 0.9)]) + [("close", 0), ("drain", 8)]
FLAGGED = one_stream([det(A, 100.0, flags=2)], [det(A, 1.0)], [det(A, 50.0, flags=2)]) + [("close", 0), ("drain", 8)]
TIE = one_stream([det(A, 5.0)], [det(A, 5.0)]) + [("close", 0), ("drain", 8)]
NAN_SCORE = one_stream([det(A, qscore=0.5)], [det(A, qscore=float("nan"))], [det(A, qscore=0.25)]) + [("close", 0), ("drain", 8)]   # rank 2
CLOSE_CONTINUES = one_stream([det(A)], [det(A)]) + [("close", 0)] + one_stream([det(A)]) + [("close", -1), ("drain", 8)]
# all three streams, an invalid and an unscored face, then the sparse calls: stream 2 alone, streams 2 and 0 in reversed order
SPARSE = [("update", {0: [det(A), det(B)], 1: [det(A, valid=0)], 2: [det(C, present=0), det(A, 3.0)]}),
          ("update", {0: [det(A, 20.0), det(B, 1.0)], 1: [det(A)], 2: [det(A, 4.0), det(C)]}),
          ("update", {2: [det(A, 2.0)]}),
          ("update", {2: [det(A, 8.0), det(B)], 0: [det(B, 30.0)]}),
          ("update", {2: [], 0: []}),
          ("drain", 1),
          ("update", {2: [det(C)], 0: [], 1: []}),
          ("update", {0: [], 1: [], 2: []}),
          ("reset", 1), ("update", {1: [det(B)]}), ("close", 1),
          ("drain", 8), ("close", -1), ("drain", 8)]
# close(s) before the tracker's reset, and a reset without it: the next update of that stream ends the stale entry with ticks from before the reset
CLOSE_BEFORE_RESET = [("update", {0: [det(A), det(B)], 1: [det(A)]}), ("update", {1: [det(A)], 0: [det(A), det(B)]}), ("close", 0), ("reset", 0),
                      ("update", {0: [det(A)], 1: [det(A)]}), ("drain", 8), ("close", -1), ("drain", 8)]
RESET_WITHOUT_CLOSE = [("update", {0: [det(A), det(B)], 1: [det(A)]}), ("update", {1: [det(A)], 0: [det(A), det(B)]}), ("reset", 0),
                       ("update", {0: [det(C)], 1: [det(A)]}), ("drain", 8), ("reset", -1), ("update", {0: [], 1: [], 2: []}), ("drain", 8)]

SCENES = {  # name -> (script, rig)
    "birth_to_expiry": (BIRTH_TO_EXPIRY, dict(capacity=4)),
    "replaced": (REPLACED, dict(capacity=4, max_missed=0)),
    "discard": (DISCARD, dict(capacity=4, max_missed=0, min_hits=2)),
    "overflow": (OVERFLOW, dict(capacity=2, max_missed=0)),
    "rank_sharpness": (THREE_RANKS, dict(capacity=4, rank=0)),
    "rank_size": (THREE_RANKS, dict(capacity=4, rank=1)),
    "rank_score": (THREE_RANKS, dict(capacity=4, rank=2)),
    "flagged": (FLAGGED, dict(capacity=4)),
    "tie": (TIE, dict(capacity=4)),
    "nan_score": (NAN_SCORE, dict(capacity=4, rank=2)),
    "close_continues": (CLOSE_CONTINUES, dict(capacity=4)),
    "sparse": (SPARSE, dict(capacity=3)),
    "close_before_reset": (CLOSE_BEFORE_RESET, dict(capacity=8)),
    "reset_without_close": (RESET_WITHOUT_CLOSE, dict(capacity=8)),
    "sparse_no_crops": (SPARSE, dict(capacity=3, keep_crops=False, rank=1)),
}
