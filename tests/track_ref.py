"""The face tracker (include/frt.h, "Face tracker"), restated in numpy: association, expiry, births, the running sums, templates and the
scatter of identities.  This is the contract the device code (kernels_track.hip) is held to - integers for equality, the fp32 sums bit for
bit; nothing here calls the library.  The overlap is tiled_ref.overlap, metric 0: the float32 IoU of the detector's own NMS."""
import numpy as np

from tiled_ref import overlap

RESULT_DTYPE = np.dtype([("x1", "<i4"), ("y1", "<i4"), ("x2", "<i4"), ("y2", "<i4"), ("score", "<f4"), ("frame", "<i4"),
                         ("match_idx", "<i4"), ("match_sim", "<f4"), ("valid", "<i4")])  # == frt_face_result
TRACK_DTYPE = np.dtype([("track_id", "<i4"), ("slot", "<i4"), ("age", "<i4"), ("hits", "<i4"), ("n_embeds", "<i4"), ("confirmed", "<i4"),
                        ("match_idx", "<i4"), ("match_sim", "<f4")])  # == frt_track_result
STATE_DTYPE = np.dtype([("live", "<i4"), ("id", "<i4"), ("x1", "<i4"), ("y1", "<i4"), ("x2", "<i4"), ("y2", "<i4"), ("score", "<f4"),
                        ("born", "<i4"), ("hits", "<i4"), ("missed", "<i4"), ("n_embeds", "<i4"), ("match_idx", "<i4"),
                        ("match_sim", "<f4")])  # == frt_track_state
assert TRACK_DTYPE.itemsize == 32 and STATE_DTYPE.itemsize == 52
BOX = ("x1", "y1", "x2", "y2", "score")
ABSENT = np.array((-1, -1, 0, 0, 0, 0, -1, 0.0), TRACK_DTYPE)


def _box(rec):
    """the tuple tiled_ref.overlap reads: (source, x1, y1, x2, y2)"""
    return (0, int(rec["x1"]), int(rec["y1"]), int(rec["x2"]), int(rec["y2"]))


def template64(sums):
    """float64 sum / ||sum|| of fp32 sums [..., dim]; zeros where the norm is zero"""
    s = np.asarray(sums, np.float64)
    n = np.sqrt((s * s).sum(-1, keepdims=True))
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(n > 0, s / n, 0.0)


class Tracker:
    def __init__(self, n_streams, max_tracks, max_faces, dim, iou_threshold=0.3, max_missed=5, min_hits=3, decay=1.0):
        assert 1 <= n_streams <= 1024 and 1 <= max_tracks <= 64 and 1 <= max_faces <= 64 and 4 <= dim <= 2048 and dim % 4 == 0
        self.n_streams, self.max_tracks, self.max_faces, self.dim = n_streams, max_tracks, max_faces, dim
        self.thr, self.decay = np.float32(iou_threshold), np.float32(decay)
        assert 0 < self.thr <= 1 and max_missed >= 0 and min_hits >= 1 and 0 < self.decay <= 1
        self.max_missed, self.min_hits = int(max_missed), int(min_hits)
        self.slots = np.zeros((n_streams, max_tracks), STATE_DTYPE)
        self.sums = np.zeros((n_streams, max_tracks, dim), np.float32)
        self.next_id = np.zeros(n_streams, np.int32)
        self.tick = np.zeros(n_streams, np.int32)
        self.dropped = np.zeros(n_streams, np.int32)

    def check_ids(self, n_frames, stream_ids):
        """-> the ids of a call, or None where the library answers FRT_ERR_INVALID / FRT_ERR_CAPACITY"""
        if not 1 <= n_frames <= 256:
            return None
        ids = list(range(n_frames)) if stream_ids is None else [int(s) for s in stream_ids]
        if len(ids) != n_frames or len(set(ids)) != n_frames or min(ids) < 0 or max(ids) >= self.n_streams:
            return None
        return ids

    def update(self, results, embeds, stream_ids=None, top1=None):
        """results RESULT_DTYPE [n_frames * max_faces], embeds fp32 [n_frames * max_faces, dim] -> (tracks TRACK_DTYPE [n_frames, max_faces],
        templates float64 [n_frames, max_faces, dim]: template64 of the fp32 sums).  top1: None (no matcher, or one without rows), or a function
        templates fp32 [n_frames * max_faces, dim] -> (idx, sim), whose answers apply_identity scatters."""
        MF, T, D = self.max_faces, self.max_tracks, self.dim
        results = np.asarray(results).reshape(-1, MF)
        n_frames = results.shape[0]
        embeds = np.asarray(embeds, np.float32).reshape(n_frames, MF, D)
        ids = self.check_ids(n_frames, stream_ids)
        assert ids is not None, "a call the library refuses"
        tracks = np.empty((n_frames, MF), TRACK_DTYPE)
        tracks[:] = ABSENT
        templates = np.zeros((n_frames, MF, D), np.float64)
        for f, s in enumerate(ids):
            st, tick = self.slots[s], int(self.tick[s])
            live_entry = st["live"] != 0
            taken = np.zeros(T, bool)
            det_slot = np.full(MF, -1)
            present = results[f]["score"] > 0                                     # 1
            for d in np.nonzero(present)[0]:                                      # 2
                best, best_t = None, -1
                for t in range(T):
                    if live_entry[t] and not taken[t]:
                        o = overlap(_box(results[f, d]), _box(st[t]), 0)
                        if o >= self.thr and (best_t < 0 or o > best):
                            best, best_t = o, t
                if best_t >= 0:
                    for k in BOX:
                        st[best_t][k] = results[f, d][k]
                    st[best_t]["hits"] += 1
                    st[best_t]["missed"] = 0
                    taken[best_t] = True
                    det_slot[d] = best_t
            for t in range(T):                                                    # 3
                if live_entry[t] and not taken[t]:
                    st[t]["missed"] += 1
                    if st[t]["missed"] > self.max_missed:
                        st[t] = np.zeros((), STATE_DTYPE)
                        self.sums[s, t] = 0
            for d in np.nonzero(present)[0]:                                      # 4
                if det_slot[d] >= 0:
                    continue
                free = np.nonzero(st["live"] == 0)[0]
                if len(free) == 0:
                    self.dropped[s] += 1
                    continue
                t = free[0]
                st[t] = np.zeros((), STATE_DTYPE)
                for k in BOX:
                    st[t][k] = results[f, d][k]
                st[t]["live"], st[t]["id"], st[t]["born"], st[t]["hits"], st[t]["match_idx"] = 1, self.next_id[s], tick, 1, -1
                self.next_id[s] += 1
                self.sums[s, t] = 0
                det_slot[d] = t
            for d in range(MF):
                t = det_slot[d]
                if t < 0:
                    continue
                if results[f, d]["valid"] != 0:                                   # 5: two roundings, fp32 both
                    self.sums[s, t] = (self.decay * self.sums[s, t]).astype(np.float32) + embeds[f, d]
                    st[t]["n_embeds"] += 1
                if st[t]["n_embeds"] > 0:                                         # 6
                    templates[f, d] = template64(self.sums[s, t])
                tracks[f, d] = (st[t]["id"], t, tick - st[t]["born"] + 1, st[t]["hits"], st[t]["n_embeds"], st[t]["hits"] >= self.min_hits, -1, 0.0)
            self.tick[s] += 1                                                     # 8
        if top1 is not None:                                                      # 7
            idx, sim = top1(templates.reshape(-1, D).astype(np.float32))
            self.apply_identity(tracks, ids, idx, sim)
        return tracks, templates

    def apply_identity(self, tracks, stream_ids, idx, sim):
        """step 7: (idx, sim) [n_frames * max_faces] of the template rows -> the tracked records with n_embeds > 0 and their slots, in place"""
        ids = list(range(tracks.shape[0])) if stream_ids is None else list(stream_ids)
        idx, sim = np.asarray(idx).reshape(tracks.shape), np.asarray(sim, np.float32).reshape(tracks.shape)
        for f, s in enumerate(ids):
            for d in range(self.max_faces):
                r = tracks[f, d]
                if r["slot"] >= 0 and r["n_embeds"] > 0:
                    r["match_idx"] = self.slots[s, r["slot"]]["match_idx"] = idx[f, d]
                    r["match_sim"] = self.slots[s, r["slot"]]["match_sim"] = sim[f, d]

    def reset(self, stream=-1):
        for s in range(self.n_streams) if stream < 0 else [stream]:
            self.slots[s] = np.zeros((), STATE_DTYPE)
            self.sums[s] = 0
            self.tick[s] = self.dropped[s] = 0

    def counters(self, stream):
        return np.array([self.next_id[stream], self.tick[stream], self.dropped[stream]], np.int32)
