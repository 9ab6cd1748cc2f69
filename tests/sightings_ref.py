"""The sighting book (include/frt.h, "Sightings"), restated in numpy: S1 close, S2 observe, S3 best shot, close and drain.  This is the
contract the device code (kernels_sightings.hip) is held to - every record and every payload row for equality; nothing here calls the
library.  The tracker under the book is track_ref.Tracker (or the library's own, read back), the quality records are quality_ref's."""
import numpy as np

from quality_ref import QUALITY_DTYPE
from track_ref import RESULT_DTYPE, TRACK_DTYPE

SIGHTING_DTYPE = np.dtype([("stream", "<i4"), ("track_id", "<i4"), ("first_tick", "<i4"), ("last_tick", "<i4"), ("close_tick", "<i4"),
                           ("reason", "<i4"), ("hits", "<i4"), ("n_embeds", "<i4"), ("confirmed", "<i4"), ("match_idx", "<i4"), ("match_sim", "<f4"),
                           ("n_shots", "<i4"), ("best_tick", "<i4"), ("x1", "<i4"), ("y1", "<i4"), ("x2", "<i4"), ("y2", "<i4"), ("score", "<f4"),
                           ("best_sharpness", "<f4"), ("best_luma_var", "<f4"), ("best_mean", "<f4"), ("best_flags", "<u4"), ("best_size", "<i4"),
                           ("reserved", "<i4")])  # == frt_sighting; x1 .. score: best_box
assert SIGHTING_DTYPE.itemsize == 96
RANK_SHARPNESS, RANK_SIZE, RANK_SCORE = 0, 1, 2
EXPIRED, REPLACED, CLOSED = 1, 2, 3
CROP = (112, 112, 3)
METRIC = {RANK_SHARPNESS: "sharpness", RANK_SIZE: "size", RANK_SCORE: "score"}


def tracker_state(tracker, stream_ids):
    """what a book update reads of a track_ref.Tracker AFTER its update of the same frames: (slots [n_frames, max_tracks], ticks [n_frames])"""
    ids = list(stream_ids)
    return tracker.slots[ids].copy(), tracker.tick[ids] - 1


class Book:
    def __init__(self, n_streams, max_tracks, max_faces, dim, capacity, rank=RANK_SHARPNESS, min_hits=1, keep_crops=True):
        assert 1 <= capacity <= 65536 and rank in METRIC and min_hits >= 1
        self.n_streams, self.max_tracks, self.max_faces, self.dim = n_streams, max_tracks, max_faces, dim
        self.capacity, self.rank, self.min_hits, self.keep_crops = capacity, rank, min_hits, bool(keep_crops)
        self.rec = np.zeros((n_streams, max_tracks), SIGHTING_DTYPE)             # a free entry is all zero
        self.emb = np.zeros((n_streams, max_tracks, dim), np.float32)
        self.tpl = np.zeros((n_streams, max_tracks, dim), np.float32)
        self.crops = np.zeros((n_streams, max_tracks) + CROP, np.uint8) if keep_crops else None
        self.key = np.zeros((n_streams, max_tracks), "<f4" if rank != RANK_SIZE else "<i4")   # the metric the best shot was taken with
        self.queue = []                                                           # (record, best_embed, template, crop or None), oldest first
        self.overflowed = self.discarded = self.closed = 0

    def is_open(self, s, t):
        return self.rec[s, t]["close_tick"] == -1

    def _end(self, s, t, reason, close_tick):
        """S1 for an entry known to end"""
        e = self.rec[s, t].copy()
        self.closed += 1
        if e["hits"] < self.min_hits:
            self.discarded += 1
        elif len(self.queue) < self.capacity:
            e["reason"], e["close_tick"] = reason, close_tick
            self.queue.append((e, self.emb[s, t].copy(), self.tpl[s, t].copy(), self.crops[s, t].copy() if self.keep_crops else None))
        else:
            self.overflowed += 1
        self.rec[s, t] = np.zeros((), SIGHTING_DTYPE)
        self.emb[s, t] = 0
        self.tpl[s, t] = 0
        self.key[s, t] = 0
        if self.keep_crops:
            self.crops[s, t] = 0

    def update(self, slots, ticks, results, tracks, embeds, quality, templates=None, crops=None, stream_ids=None):
        """slots STATE_DTYPE [n_frames, max_tracks] and ticks [n_frames]: the tracker's state of each frame's stream after ITS update of these
        frames and the tick that update used (tracker_state); the rest as frt_sightings_update takes them."""
        MF, T, D = self.max_faces, self.max_tracks, self.dim
        results = np.asarray(results, RESULT_DTYPE).reshape(-1, MF)
        n_frames = results.shape[0]
        tracks = np.asarray(tracks, TRACK_DTYPE).reshape(n_frames, MF)
        quality = np.asarray(quality, QUALITY_DTYPE).reshape(n_frames, MF)
        embeds = np.asarray(embeds, np.float32).reshape(n_frames, MF, D)
        templates = None if templates is None else np.asarray(templates, np.float32).reshape(n_frames, MF, D)
        assert (crops is not None) == self.keep_crops
        crops = None if crops is None else np.asarray(crops, np.uint8).reshape((n_frames, MF) + CROP)
        ids = list(range(n_frames)) if stream_ids is None else [int(s) for s in stream_ids]
        assert len(ids) == n_frames == len(set(ids)) and 0 <= min(ids) and max(ids) < self.n_streams
        for f, s in enumerate(ids):
            tick = int(ticks[f])
            for t in range(T):                                                    # S1
                st = slots[f][t]
                if self.is_open(s, t) and not (st["live"] != 0 and st["id"] == self.rec[s, t]["track_id"]):
                    self._end(s, t, EXPIRED if st["live"] == 0 else REPLACED, tick)
            for d in range(MF):
                tr = tracks[f, d]
                if tr["track_id"] < 0:
                    continue
                t = int(tr["slot"])
                e = self.rec[s, t]
                if not self.is_open(s, t):                                        # S2
                    e["stream"], e["track_id"], e["first_tick"] = s, tr["track_id"], tick - int(tr["age"]) + 1
                    e["close_tick"], e["best_tick"] = -1, -1
                e["last_tick"] = tick
                for k in ("hits", "n_embeds", "confirmed", "match_idx", "match_sim"):
                    e[k] = tr[k]
                if templates is not None:
                    self.tpl[s, t] = templates[f, d]
                r, q = results[f, d], quality[f, d]
                if r["valid"] == 0 or q["present"] == 0:                          # S3
                    continue
                e["n_shots"] += 1
                metric = self.key.dtype.type(q[METRIC[self.rank]])
                passes, best_passes = int(q["flags"] == 0), int(e["best_flags"] == 0)
                with np.errstate(invalid="ignore"):
                    greater = bool(metric > self.key[s, t])                       # a NaN on either side: False
                if e["best_tick"] < 0 or passes > best_passes or (passes == best_passes and greater):
                    e["best_tick"] = tick
                    for k in ("x1", "y1", "x2", "y2", "score"):
                        e[k] = r[k]
                    e["best_sharpness"], e["best_luma_var"], e["best_mean"] = q["sharpness"], q["luma_var"], q["mean"]
                    e["best_flags"], e["best_size"] = q["flags"], q["size"]
                    self.key[s, t] = metric
                    self.emb[s, t] = embeds[f, d]
                    if self.keep_crops:
                        self.crops[s, t] = crops[f, d]

    def close(self, stream=-1):
        for s in range(self.n_streams) if stream < 0 else [stream]:
            for t in range(self.max_tracks):
                if self.is_open(s, t):
                    self._end(s, t, CLOSED, int(self.rec[s, t]["last_tick"]))

    def drain(self, max_out):
        """-> (records [n], best embeddings [n, dim], templates [n, dim], crops [n, 112, 112, 3] or None, counters)"""
        counters = dict(queued=len(self.queue), overflowed=self.overflowed, discarded=self.discarded, closed=self.closed)
        out, self.queue = self.queue[:max_out], self.queue[max_out:]
        rec = np.array([o[0] for o in out], SIGHTING_DTYPE).reshape(-1)
        emb = np.array([o[1] for o in out], np.float32).reshape(-1, self.dim)
        tpl = np.array([o[2] for o in out], np.float32).reshape(-1, self.dim)
        crops = np.array([o[3] for o in out], np.uint8).reshape((-1,) + CROP) if self.keep_crops else None
        return rec, emb, tpl, crops, counters

    def open(self, stream):
        return self.rec[stream].copy(), self.emb[stream].copy(), self.tpl[stream].copy(), self.crops[stream].copy() if self.keep_crops else None
