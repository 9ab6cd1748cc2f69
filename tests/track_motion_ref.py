"""The tracker's motion term (include/frt.h "Face tracker", the "Motion" block), restated in Python ints on top of tests/track_reid_ref.py,
so appearance and motion combine: the velocity array, the predicted box M1, the velocity update M2, expiry and births M3, and a gate
restatement that takes its association from this file's own update, the way tests/track_gate_ref.py takes it from track_ref's.  This is the
contract the device code (kernels_track.hip: track_update_kernel<.., true>, track_gate_kernel<true>) is held to - integers for equality, the
fp32 overlaps and sums bit for bit; nothing here calls the library.  With gain 0 an update is track_reid_ref.Tracker's, answer for answer."""
import numpy as np

import track_gate_ref as gr
import track_reid_ref as rr
from track_ref import BOX, STATE_DTYPE, TRACK_DTYPE, ABSENT, _box, overlap, template64
from track_reid_ref import ASSOC_DTYPE, HOW_IOU, HOW_APPEARANCE, HOW_BIRTH, HOW_UNTRACKED, REID_OFF, MIN_SIM_OFF

I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1
SHIFT_MAX, DC_MAX = 2 ** 30, 2 ** 22


def tdiv(a, b):
    """sign(a) * (|a| / b) for b > 0: truncation toward zero, C's division - not numpy's flooring //"""
    a, b = int(a), int(b)
    assert b > 0
    return a // b if a >= 0 else -((-a) // b)


def clamp(v, lo, hi):
    return lo if v < lo else hi if v > hi else v


def check_gain(gain):
    """what frt_tracker_set_motion accepts"""
    return 0 <= int(gain) <= 256


def shift(v, missed):
    """M1: the shift of one axis, for a velocity v (1/256 pixel per update) and the track's `missed`"""
    return clamp(tdiv(int(v) * (int(missed) + 1), 256), -SHIFT_MAX, SHIFT_MAX)


def predicted(slot, vel):
    """M1: slot STATE_DTYPE (), vel (vx, vy) -> (x1, y1, x2, y2) Python ints, each clamped to the int32 range"""
    sx, sy = shift(vel[0], slot["missed"]), shift(vel[1], slot["missed"])
    return (clamp(int(slot["x1"]) + sx, I32_MIN, I32_MAX), clamp(int(slot["y1"]) + sy, I32_MIN, I32_MAX),
            clamp(int(slot["x2"]) + sx, I32_MIN, I32_MAX), clamp(int(slot["y2"]) + sy, I32_MIN, I32_MAX))


def matched_velocity(v, det, trk, gain):
    """M2, one track: v (vx, vy) at entry, det / trk records with x1 .. y2 (trk: the last MEASURED box, hits and missed at entry) -> (vx, vy)"""
    g = int(trk["missed"]) + 1
    out = []
    for lo, hi, v0 in (("x1", "x2", int(v[0])), ("y1", "y2", int(v[1]))):
        dc = clamp((int(det[lo]) + int(det[hi])) - (int(trk[lo]) + int(trk[hi])), -DC_MAX, DC_MAX)
        raw = tdiv(dc * 128, g)
        out.append(raw if int(trk["hits"]) == 1 else v0 + tdiv((raw - v0) * int(gain), 256))
    return tuple(out)


class Tracker(rr.Tracker):
    def __init__(self, *args, motion_gain=0, **kw):
        super().__init__(*args, **kw)
        self.gain = 0
        self.vel = None  # int32 [n_streams, max_tracks, 2], allocated by the first call that needs it
        self.set_motion(motion_gain)

    def set_motion(self, gain):
        assert check_gain(gain), "a call the library refuses"
        if self.gain == 0 and gain > 0 and self.vel is not None:
            self.vel[:] = 0                                                      # off -> on zeroes; on -> on keeps; on -> off leaves alone
        self.gain = int(gain)

    def _ensure_vel(self):
        if self.vel is None:
            self.vel = np.zeros((self.n_streams, self.max_tracks, 2), np.int32)

    def reset(self, stream=-1):
        super().reset(stream)
        if self.vel is not None:
            for s in range(self.n_streams) if stream < 0 else [stream]:
                self.vel[s] = 0

    def motion(self, stream):
        """frt_tracker_motion -> (vel int32 [max_tracks, 2], pred BBOX_DTYPE [max_tracks]: M1's box for the NEXT update, zero for a free slot)"""
        assert self.gain > 0, "a call the library refuses"
        self._ensure_vel()
        pred = np.zeros(self.max_tracks, gr.BBOX_DTYPE)
        for t in range(self.max_tracks):
            st = self.slots[stream, t]
            if st["live"] != 0:
                pred[t] = predicted(st, self.vel[stream, t]) + (st["score"],)
        return self.vel[stream].copy(), pred

    def update(self, results, embeds, stream_ids=None, top1=None, want_assoc=False):
        """track_reid_ref.Tracker.update with M1 - M3 -> (tracks, templates[, assoc])"""
        if self.gain == 0:
            return super().update(results, embeds, stream_ids, top1, want_assoc)
        self._ensure_vel()
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
            st, vel, tick = self.slots[s], self.vel[s], int(self.tick[s])
            S, defined = self.similarity(results[f], embeds[f], s)
            live_entry = st["live"] != 0
            pred = [(0,) + predicted(st[t], vel[t]) if live_entry[t] else None for t in range(T)]   # M1: from the state at entry, once
            taken = np.zeros(T, bool)
            det_slot = np.full(MF, -1)
            present = results[f]["score"] > 0                                     # 1

            def match(d, t, how, ovr):
                assoc[f, d] = (how, st[t]["missed"], ovr, S[d, t] if defined[d, t] else 0.0)
                vel[t] = matched_velocity(vel[t], results[f, d], st[t], self.gain)   # M2, before the box is overwritten
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
                        o = overlap(_box(results[f, d]), pred[t], 0)
                        if veto_on and defined[d, t] and S[d, t] < self.min_sim:
                            self.vetoes += int(o >= self.thr)
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
                    match(d, best_t, HOW_APPEARANCE, overlap(_box(results[f, d]), pred[best_t], 0))
            for t in range(T):                                                    # 3
                if live_entry[t] and not taken[t]:
                    st[t]["missed"] += 1
                    if st[t]["missed"] > self.max_missed:
                        st[t] = np.zeros((), STATE_DTYPE)
                        self.sums[s, t] = 0
                        vel[t] = 0                                                # M3
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
                vel[t] = 0                                                        # M3
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


# ---- the gate with motion (include/frt.h "Motion", M4): reads the velocities, writes none
def peek(slots, vel, gain, boxes, present, iou_threshold):
    """G2 with the predicted boxes: slots STATE_DTYPE [max_tracks] and vel [max_tracks, 2] at entry -> (peek int [max_faces], ovr float32
    [max_faces]).  The association is this file's update on a twin - appearance off, valid 0 everywhere, nothing ever expires -; the ovr is the
    overlap with M1's box of the slot at entry.  gain 0: track_gate_ref.peek."""
    if gain == 0:
        return gr.peek(slots, boxes, present, iou_threshold)
    T, MF = len(slots), len(boxes)
    twin = Tracker(1, T, MF, 4, iou_threshold=iou_threshold, max_missed=2 ** 30, min_hits=1, motion_gain=gain)
    twin._ensure_vel()
    twin.slots[0], twin.vel[0] = slots, vel
    res = np.zeros(MF, rr.tk.RESULT_DTYPE)
    for k in ("x1", "y1", "x2", "y2"):
        res[k] = boxes[k]
    res["score"] = np.where(present, boxes["score"], np.float32(0))
    tracks, _ = twin.update(res, np.zeros((MF, 4), np.float32))
    out, ovr = np.full(MF, -1), np.zeros(MF, np.float32)
    for d in range(MF):
        t = int(tracks[0, d]["slot"])
        if present[d] and t >= 0 and slots[t]["live"] != 0:
            out[d], ovr[d] = t, np.float32(overlap(_box(boxes[d]), (0,) + predicted(slots[t], vel[t]), 0))
    return out, ovr


def gate_frame(slots, vel, gain, boxes, n_boxes, iou_threshold, min_hits, refresh, min_embeds, skip_iou):
    """G1 - G4 of one frame -> GATE_DTYPE [max_faces]; G3's skip_iou comparison is against the predicted box's overlap"""
    assert gr.check_options(refresh, min_embeds, skip_iou)
    MF = len(boxes)
    present = gr.present_mask(boxes, n_boxes)
    pk, ovr = peek(slots, vel, gain, boxes, present, iou_threshold)
    out = np.empty(MF, gr.GATE_DTYPE)
    out[:] = gr.ABSENT_RECORD
    for d in np.nonzero(present)[0]:
        t = int(pk[d])
        if t < 0:
            out[d] = (gr.EMBED, -1, 0.0, gr.NO_TRACK)
            continue
        hits, ne = int(slots[t]["hits"]), int(slots[t]["n_embeds"])
        why = 0
        if hits < min_hits:
            why |= gr.UNCONFIRMED
        if ne < min_embeds:
            why |= gr.FEW_EMBEDS
        if not ovr[d] >= np.float32(skip_iou):
            why |= gr.LOW_OVERLAP
        if (hits + 1) % refresh == 0:
            why |= gr.REFRESH
        out[d] = (gr.EMBED if why else gr.FOLLOW, t, ovr[d], why)
    return out


def gate(slots_by_frame, vel_by_frame, gain, boxes, n_boxes, iou_threshold, min_hits, refresh, min_embeds, skip_iou, max_batch):
    """One call: slots_by_frame [n_frames, max_tracks] and vel_by_frame [n_frames, max_tracks, 2] (ignored at gain 0) - the state AT ENTRY of
    each frame's stream -, boxes BBOX_DTYPE [n_frames, max_faces], n_boxes [n_frames] or None -> (gate records, list, n_embed, pass_count)"""
    boxes = np.asarray(boxes)
    n = boxes.shape[0]
    rec = np.stack([gate_frame(slots_by_frame[f], None if gain == 0 else vel_by_frame[f], gain, boxes[f], None if n_boxes is None else n_boxes[f],
                               iou_threshold, min_hits, refresh, min_embeds, skip_iou) for f in range(n)])
    return (rec,) + gr.work_list(rec, max_batch)


def tracker_gate(trk, boxes, stream_ids, n_boxes, refresh, min_embeds, skip_iou, max_batch):
    """the gate of a Tracker of this file as it stands: boxes BBOX_DTYPE [n_frames, max_faces] of the streams stream_ids (None: 0, 1, ..)"""
    boxes = np.asarray(boxes).reshape(-1, trk.max_faces)
    ids = trk.check_ids(boxes.shape[0], stream_ids)
    assert ids is not None, "a call the library refuses"
    if trk.gain > 0:
        trk._ensure_vel()
    return gate(trk.slots[ids], None if trk.gain == 0 else trk.vel[ids], trk.gain, boxes, n_boxes, float(trk.thr), trk.min_hits, refresh, min_embeds,
                skip_iou, max_batch)
