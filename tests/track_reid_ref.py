"""The tracker's appearance term (include/frt.h "Face tracker", the "Appearance" block), restated in numpy on top of tests/track_ref.py: the
reduction dot2r, the similarity S with its DEFINED bit, steps 2a (the veto) and 2b (the re-attach), and the association records.  This is the
contract the device code (kernels_track.hip: track_similarity_kernel, track_update_kernel<true>) is held to - integers for equality, the fp32
S, overlaps and sums bit for bit; nothing here calls the library.  With both settings off an update is track_ref.Tracker's."""
import numpy as np

import track_ref as tk
from track_ref import BOX, STATE_DTYPE, TRACK_DTYPE, ABSENT, _box, overlap, template64

ASSOC_DTYPE = np.dtype([("how", "<i4"), ("gap", "<i4"), ("ovr", "<f4"), ("sim", "<f4")])  # == frt_track_assoc
assert ASSOC_DTYPE.itemsize == 16
HOW_ABSENT, HOW_IOU, HOW_APPEARANCE, HOW_BIRTH, HOW_UNTRACKED = range(5)
REID_OFF, MIN_SIM_OFF = np.float32(2.0), np.float32(-2.0)
_PERM = [np.arange(64) ^ off for off in (32, 16, 8, 4, 2, 1)]


def dot2r(x, y):
    """the header's reduction over the last axis of fp32 x, y [..., dim] -> fp32 [...]: pad to [G, 64, 4] with zeros, one chain per lane of
    fl(acc + fl(x * y)) over g then j, then the six butterfly steps v + v[lane ^ off]; lane 0's value"""
    x, y = np.broadcast_arrays(np.asarray(x, np.float32), np.asarray(y, np.float32))
    dim = x.shape[-1]
    G = -(-dim // 256)
    pad = [(0, 0)] * (x.ndim - 1) + [(0, G * 256 - dim)]
    x = np.pad(x, pad).reshape(x.shape[:-1] + (G, 64, 4))
    y = np.pad(y, pad).reshape(x.shape)
    acc = np.zeros(x.shape[:-3] + (64,), np.float32)
    with np.errstate(all="ignore"):
        for g in range(G):
            for j in range(4):
                acc = acc + x[..., g, :, j] * y[..., g, :, j]      # float32 arrays: each operation rounds once
        for perm in _PERM:
            acc = acc + acc[..., perm]
    assert acc.dtype == np.float32
    return acc[..., 0]


def check_appearance(reid_threshold, iou_min_sim):
    """what frt_tracker_set_appearance accepts (a NaN fails every comparison)"""
    r, m = np.float32(reid_threshold), np.float32(iou_min_sim)
    return bool(((r > 0) & (r <= 1)) | (r == REID_OFF)) and bool(((m >= -1) & (m <= 1)) | (m == MIN_SIM_OFF))


class Tracker(tk.Tracker):
    def __init__(self, *args, reid_threshold=None, iou_min_sim=None, **kw):
        super().__init__(*args, **kw)
        self.vetoes = 0
        self.set_appearance(reid_threshold, iou_min_sim)

    def set_appearance(self, reid_threshold=None, iou_min_sim=None):
        """None: off"""
        r = REID_OFF if reid_threshold is None else np.float32(reid_threshold)
        m = MIN_SIM_OFF if iou_min_sim is None else np.float32(iou_min_sim)
        assert check_appearance(r, m), "a call the library refuses"
        self.reid, self.min_sim = r, m

    def similarity(self, results_f, embeds_f, stream):
        """one frame: S fp32 [max_faces, max_tracks] and its DEFINED bits, from the stream's state as it is now (at entry)"""
        st, sums = self.slots[stream], self.sums[stream]
        with np.errstate(all="ignore"):
            n2 = dot2r(sums, sums)                                                     # [T]
            S = dot2r(embeds_f[:, None, :], sums[None, :, :]) / np.sqrt(n2)[None, :]   # [MF, T]: fl(dot / fl(sqrt))
            det_ok = (results_f["score"] > 0) & (results_f["valid"] != 0)
            trk_ok = (st["live"] != 0) & (st["n_embeds"] > 0) & (n2 > 0)
        assert S.dtype == np.float32
        return S, det_ok[:, None] & trk_ok[None, :]

    def update(self, results, embeds, stream_ids=None, top1=None, want_assoc=False):
        """track_ref.Tracker.update with steps 2a / 2b -> (tracks, templates[, assoc ASSOC_DTYPE [n_frames, max_faces]])"""
        MF, T, D = self.max_faces, self.max_tracks, self.dim
        results = np.asarray(results).reshape(-1, MF)
        n_frames = results.shape[0]
        embeds = np.asarray(embeds, np.float32).reshape(n_frames, MF, D)
        ids = self.check_ids(n_frames, stream_ids)
        assert ids is not None, "a call the library refuses"
        veto_on, reid_on = self.min_sim != MIN_SIM_OFF, self.reid != REID_OFF
        tracks = np.empty((n_frames, MF), TRACK_DTYPE)
        tracks[:] = ABSENT
        assoc = np.zeros((n_frames, MF), ASSOC_DTYPE)
        templates = np.zeros((n_frames, MF, D), np.float64)
        for f, s in enumerate(ids):
            st, tick = self.slots[s], int(self.tick[s])
            S, defined = self.similarity(results[f], embeds[f], s)
            live_entry = st["live"] != 0
            taken = np.zeros(T, bool)
            det_slot = np.full(MF, -1)
            present = results[f]["score"] > 0                                     # 1

            def match(d, t, how, ovr):
                assoc[f, d] = (how, st[t]["missed"], ovr, S[d, t] if defined[d, t] else 0.0)
                for k in BOX:
                    st[t][k] = results[f, d][k]
                st[t]["hits"] += 1
                st[t]["missed"] = 0
                taken[t] = True
                det_slot[d] = t

            for d in np.nonzero(present)[0]:                                      # 2a
                best, best_t = None, -1
                for t in range(T):
                    if live_entry[t] and not taken[t]:
                        o = overlap(_box(results[f, d]), _box(st[t]), 0)
                        if veto_on and defined[d, t] and S[d, t] < self.min_sim:
                            self.vetoes += int(o >= self.thr)                     # (a count for the tests: the pair would have been a candidate)
                            continue
                        if o >= self.thr and (best_t < 0 or o > best):
                            best, best_t = o, t
                if best_t >= 0:
                    match(d, best_t, HOW_IOU, best)
            for d in np.nonzero(present)[0] if reid_on else []:                   # 2b
                if det_slot[d] >= 0 or results[f, d]["valid"] == 0:
                    continue
                best, best_t = None, -1
                for t in range(T):
                    if live_entry[t] and not taken[t] and defined[d, t] and S[d, t] >= self.reid and (best_t < 0 or S[d, t] > best):
                        best, best_t = S[d, t], t
                if best_t >= 0:
                    match(d, best_t, HOW_APPEARANCE, overlap(_box(results[f, d]), _box(st[best_t]), 0))
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
                    assoc[f, d]["how"] = HOW_UNTRACKED
                    continue
                t = free[0]
                st[t] = np.zeros((), STATE_DTYPE)
                for k in BOX:
                    st[t][k] = results[f, d][k]
                st[t]["live"], st[t]["id"], st[t]["born"], st[t]["hits"], st[t]["match_idx"] = 1, self.next_id[s], tick, 1, -1
                self.next_id[s] += 1
                self.sums[s, t] = 0
                det_slot[d] = t
                assoc[f, d]["how"] = HOW_BIRTH
            for d in range(MF):
                t = det_slot[d]
                if t < 0:
                    continue
                if results[f, d]["valid"] != 0:                                   # 5: two roundings, fp32 both
                    with np.errstate(all="ignore"):
                        self.sums[s, t] = (self.decay * self.sums[s, t]).astype(np.float32) + embeds[f, d]
                    st[t]["n_embeds"] += 1
                if st[t]["n_embeds"] > 0:                                         # 6
                    templates[f, d] = template64(self.sums[s, t])
                tracks[f, d] = (st[t]["id"], t, tick - st[t]["born"] + 1, st[t]["hits"], st[t]["n_embeds"], st[t]["hits"] >= self.min_hits, -1, 0.0)
            self.tick[s] += 1                                                     # 8
        if top1 is not None:                                                      # 7
            idx, sim = top1(templates.reshape(-1, D).astype(np.float32))
            self.apply_identity(tracks, ids, idx, sim)
        return (tracks, templates, assoc) if want_assoc else (tracks, templates)


# ---- inputs the CPU and the GPU tests share
def frame(max_faces, *dets):
    """dets: (x1, y1, x2, y2[, score[, valid]]) -> RESULT_DTYPE [max_faces] as the pipeline writes them: unused slots zero but match_idx -1"""
    r = np.zeros(max_faces, tk.RESULT_DTYPE)
    r["match_idx"] = -1
    for i, d in enumerate(dets):
        d = tuple(d) + (0.9, 1)[len(d) - 4:]
        r[i] = (d[0], d[1], d[2], d[3], d[4], 0, -1, 0.0, d[5])
    return r


def identities(rng, n, dim):
    """n unit rows [n, dim], fp32: orthogonal axes (with signs) while dim allows, so that two identities never look alike at dim 8 either"""
    if n <= dim:
        v = np.zeros((n, dim), np.float32)
        v[np.arange(n), rng.permutation(dim)[:n]] = rng.choice(np.float32([-1, 1]), n)
        return v
    v = rng.standard_normal((n, dim)).astype(np.float32)
    return v / np.linalg.norm(v, axis=1, keepdims=True).astype(np.float32)


def noisy(rng, v, noise=0.3):
    """v + noise * (a random unit vector), re-normalised in fp32: cosine about 1 / sqrt(1 + noise^2) with v"""
    g = rng.standard_normal(v.shape).astype(np.float32)
    e = v + np.float32(noise) * g / np.float32(np.linalg.norm(g))
    return (e / np.float32(np.linalg.norm(e))).astype(np.float32)


def pool_boxes(n, size=40, step=50, shift=12):
    """n box positions: a grid of disjoint squares, every third one a copy of its predecessor shifted by `shift` pixels (IoU about 0.5)"""
    out = []
    for i in range(n):
        if i % 3 == 2:
            x, y = out[-1][0] + shift, out[-1][1]
        else:
            x, y = step * 2 * (i % 8), step * 2 * (i // 8)
        out.append((x, y, x + size, y + size))
    return out


def soak(seed, n_streams, max_faces, dim, updates, n_ids=6, n_pos=5, p_valid=0.9, p_stream=0.9):
    """a seeded sequence of calls: per update a random subset of the streams in random order; per frame up to max_faces detections, each an
    identity (distinct within the frame) at a position of the pool (distinct within the frame), score-descending; the embedding is the
    identity plus noise.  Identities hop between positions, so a face leaves its track's box (a re-attach when appearance is on) and
    lands on another track's (a veto) -> [(ids, results [n * max_faces], embeds [n * max_faces, dim])]"""
    rng = np.random.default_rng(seed)
    who = [identities(rng, n_ids, dim) for _ in range(n_streams)]
    pool = pool_boxes(n_pos)
    calls = []
    for _ in range(updates):
        ids = [s for s in rng.permutation(n_streams) if rng.random() < p_stream] or [0]
        res, emb = [], np.zeros((len(ids), max_faces, dim), np.float32)
        for i, s in enumerate(ids):
            n = int(rng.integers(0, min(max_faces, n_ids, n_pos) + 1))
            faces, places = rng.permutation(n_ids)[:n], rng.permutation(n_pos)[:n]
            dets = []
            for d in range(n):
                dets.append(pool[places[d]] + (float(np.float32(0.95 - 0.9 * d / max_faces)), int(rng.random() < p_valid)))
                emb[i, d] = noisy(rng, who[s][faces[d]])
            res.append(frame(max_faces, *dets))
        calls.append(([int(s) for s in ids], np.concatenate(res), emb.reshape(-1, dim)))
    return calls
