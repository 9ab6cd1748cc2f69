"""The tracker's motion term on the GPU (frt_tracker_set_motion / frt_tracker_motion, and every route that honours the setting) against
tests/track_motion_ref.py, the restatement of include/frt.h "Motion" in Python ints.  The reference is never the code under test.
Everything is compared for equality: records, frt_track_assoc, gate records, slots, velocities and predicted boxes by their bytes, the sums
by their bits; the templates within the bound derived in tests/test_gpu_track.py.  An update that asks for the association records takes
track_update_kernel<true, ..>, one that does not (appearance off) track_update_kernel<false, ..>: the walks alternate between the two."""
import threading

import numpy as np
import pytest

import track_gate_ref as gr
import track_motion_ref as mr
import track_ref as tk
import track_reid_ref as rr
from test_gpu_track import check_templates, frame, walk_frames
from test_gpu_track_gate import to_boxes
from test_track_motion_ref import COASTING, SCENES, box

pytestmark = pytest.mark.gpu


class Pair:
    """a device tracker and its restatement, fed the same calls"""

    def __init__(self, frt, n_streams, max_tracks, max_faces, dim, seed=0, **opt):
        self.frt = frt
        self.dev = frt.Tracker(n_streams, max_tracks, max_faces, dim, **opt)
        ref_opt = dict(opt)
        gain = ref_opt.pop("motion_gain", None)
        self.ref = mr.Tracker(n_streams, max_tracks, max_faces, dim, motion_gain=gain or 0, **ref_opt)
        self.rng = np.random.default_rng(seed)
        self.n_streams, self.max_tracks, self.max_faces, self.dim = n_streams, max_tracks, max_faces, dim

    def set_motion(self, gain):
        self.dev.setMotion(gain)
        self.ref.set_motion(gain)
        assert self.dev.getMotion() == gain

    def reset(self, stream=-1):
        self.dev.reset(stream)
        self.ref.reset(stream)

    def embeds(self, n_frames):
        e = self.rng.standard_normal((n_frames * self.max_faces, self.dim)).astype(np.float32)
        return e / np.linalg.norm(e, axis=1, keepdims=True).astype(np.float32)

    def update(self, results, embeds=None, ids=None, want_assoc=True):
        results = np.concatenate(results) if isinstance(results, (list, tuple)) else results
        n = len(results) // self.max_faces
        embeds = self.embeds(n) if embeds is None else embeds
        got = self.dev.update(results, embeds, ids, None, want_assoc=want_assoc)
        want = self.ref.update(results, embeds, ids, want_assoc=want_assoc)
        assert got[0].shape == want[0].shape and got[0].tobytes() == want[0].tobytes(), (got[0], want[0])
        check_templates(got[1], want[1], self.dim)
        if want_assoc:
            assert got[2].tobytes() == want[2].tobytes(), (got[2], want[2])
        return got

    def check_state(self, streams=None):
        for s in range(self.n_streams) if streams is None else streams:
            slots, cnt, sums = self.dev.tracks(s, want_sums=True)
            assert slots.tobytes() == self.ref.slots[s].tobytes(), (s, slots, self.ref.slots[s])
            assert [cnt["next_id"], cnt["tick"], cnt["dropped"]] == self.ref.counters(s).tolist(), s
            assert sums.tobytes() == self.ref.sums[s].tobytes(), s
            if self.ref.gain > 0:
                vel, pred = self.dev.motion(s)
                want_vel, want_pred = self.ref.motion(s)
                assert vel.dtype == np.int32 and vel.tobytes() == want_vel.tobytes(), (s, vel, want_vel)
                assert pred.tobytes() == want_pred.tobytes(), (s, pred, want_pred)

    def gate(self, results, ids, refresh, min_embeds, skip_iou, max_batch, n_boxes=None):
        """Tracker.gate against the restatement; the state and the velocities are compared before and after -> the reference's answer"""
        boxes = to_boxes(np.concatenate(results).reshape(len(results), self.max_faces))
        self.check_state(ids)
        got = self.dev.gate(boxes, refresh, min_embeds, skip_iou, ids, n_boxes, max_batch)
        self.check_state(ids)                                                          # the gate writes nothing (the ref's gate cannot)
        want = mr.tracker_gate(self.ref, boxes, ids, n_boxes, refresh, min_embeds, skip_iou, max_batch)
        assert got[0].shape == want[0].shape and got[0].tobytes() == want[0].tobytes(), (got[0], want[0])
        assert got[1].tolist() == want[1].tolist() and got[2] == want[2] and got[3].tolist() == want[3].tolist()
        return want

    def close(self):
        self.dev.close()


def drift_frames(rng, n_streams, max_faces, updates, faces=5, p_seen=0.75):
    """faces with integer positions and their own integer velocities of both signs (they bounce off the frame and cross), each seen with
    probability p_seen and jittered by a pixel -> per update a list of per-stream RESULT_DTYPE [max_faces], score-descending"""
    pos = rng.integers(20, 400, (n_streams, faces, 2))
    vel = rng.integers(-14, 15, (n_streams, faces, 2))
    size = rng.integers(24, 64, (n_streams, faces))
    out = []
    for _ in range(updates):
        pos += vel
        vel[(pos < 0) | (pos > 440)] *= -1
        per_stream = []
        for s in range(n_streams):
            dets = []
            for f in range(faces):
                if rng.random() < p_seen:
                    x, y = int(pos[s, f, 0]) + int(rng.integers(-1, 2)), int(pos[s, f, 1]) + int(rng.integers(-1, 2))
                    dets.append((x, y, x + int(size[s, f]), y + int(size[s, f]), float(np.float32(rng.uniform(0.1, 1.0))), int(rng.random() >= 0.1)))
            dets.sort(key=lambda d: -d[4])
            per_stream.append(frame(max_faces, *dets[:max_faces]))
        out.append(per_stream)
    return out


def test_off_is_the_parent(frt):
    """a tracker that never set motion, one that set gain 0, and one that went on -> off (with the velocity array allocated in between): all
    three give the bytes of track_ref on the random walk of tests/test_gpu_track.py"""
    opt = dict(max_missed=2, iou_threshold=0.25, decay=0.75)
    never, zero, onoff = (frt.Tracker(8, 8, 5, 64, **opt) for _ in range(3))
    zero.setMotion(0)
    onoff.setMotion(64)
    assert not onoff.motion(3)[0].any()
    onoff.setMotion(0)
    ref = tk.Tracker(8, 8, 5, 64, **opt)
    rng = np.random.default_rng(108)
    for k, per_stream in enumerate(walk_frames(rng, 8, 5, 30)):
        ids = [int(s) for s in rng.permutation(8)[:rng.integers(1, 9)]]
        res = np.concatenate([per_stream[s] for s in ids])
        e = rng.standard_normal((len(res), 64)).astype(np.float32)
        want, want_tpl = ref.update(res, e, ids)
        for t in (never, zero, onoff):
            got, tpl = t.update(res, e, ids)
            assert got.tobytes() == want.tobytes()
            check_templates(tpl, want_tpl, 64)
    for t in (never, zero, onoff):
        for s in range(8):
            slots, cnt, sums = t.tracks(s, want_sums=True)
            assert slots.tobytes() == ref.slots[s].tobytes() and sums.tobytes() == ref.sums[s].tobytes()
            assert [cnt["next_id"], cnt["tick"], cnt["dropped"]] == ref.counters(s).tolist()
        with pytest.raises(frt.FrtError):
            t.motion(0)
        t.close()


@pytest.mark.parametrize("max_tracks,max_faces", [(1, 1), (1, 2), (2, 1), (2, 2)])
def test_scripted_scenes(frt, max_tracks, max_faces):
    """the hand-computed scenes of tests/test_track_motion_ref.py on the device; the state is compared after every update"""
    for name, (opt, frames) in SCENES.items():
        p = Pair(frt, 1, max_tracks, max_faces, 4, **opt)
        ids = []
        for k, dets in enumerate(frames):
            got = p.update([frame(max_faces, *dets[:max_faces])], want_assoc=k % 2 == 0)
            ids.append(int(got[0][0, 0]["track_id"]))
            if len(frames) < 100 or k % 50 == 0 or k >= len(frames) - 2:
                p.check_state()
        if name == "acceleration":
            assert ids == [0] * 6, ids
        if name == "coasting":
            assert ids == [0, 0, 0, -1, -1, -1, -1, 0], ids
        if name == "shift clamp":
            assert ids[-1] == 0 and p.dev.motion(0)[0][0].tolist() == [mr.tdiv(2 ** 29, 601), 0]   # raw = 2^22 * 128 / 601, gain 256
        p.close()


def test_the_two_scenes_of_the_issue_with_motion_off_on_the_device(frt):
    for name, want in (("acceleration", [0, 0, 0, 1, 2, 3]), ("coasting", [0, 0, 0, -1, -1, -1, -1, 1])):
        p = Pair(frt, 1, 4, 1, 4)
        assert [int(p.update([frame(1, *dets)])[0][0, 0]["track_id"]) for dets in SCENES[name][1]] == want
        p.check_state()
        p.close()


@pytest.mark.parametrize("n_streams,max_tracks,max_faces,dim,gain,max_missed", [(8, 1, 1, 4, 1, 0), (8, 8, 5, 64, 64, 5), (8, 33, 5, 512, 255, 5),
                                                                                 (2, 64, 64, 256, 256, 0), (8, 4, 5, 64, 256, 5)])
def test_random_walk_with_motion_on(frt, n_streams, max_tracks, max_faces, dim, gain, max_missed):
    """drifting faces with dropouts; a random subset of the streams per call in random order; frt_tracker_motion after every call"""
    rng = np.random.default_rng(500 + max_tracks)
    p = Pair(frt, n_streams, max_tracks, max_faces, dim, seed=600 + max_tracks, max_missed=max_missed, iou_threshold=0.3, motion_gain=gain, decay=0.75)
    gaps, signs = 0, set()
    for k, per_stream in enumerate(drift_frames(rng, n_streams, max_faces, 30)):
        ids = [int(s) for s in rng.permutation(n_streams)[:rng.integers(1, n_streams + 1)]]
        got = p.update([per_stream[s] for s in ids], ids=ids, want_assoc=k % 2 == 0)
        if k % 2 == 0:
            gaps += int((got[2]["gap"] > 0).sum())
        p.check_state(ids)
        signs.update(np.sign(p.ref.vel).reshape(-1).tolist())
    p.check_state()
    assert signs == {-1, 0, 1} and p.ref.next_id.max() > 1                           # velocities of both signs were held along the way
    if max_tracks >= 8:
        assert (p.ref.slots["hits"] >= 3).any()
    if max_missed and max_tracks >= 8:
        assert gaps > 0                                                               # a coasting track was matched at its predicted place
    p.close()


def test_a_full_wave_of_detections_and_tracks_each_with_its_own_velocity(frt):
    rng = np.random.default_rng(17)
    p = Pair(frt, 1, 64, 64, 8, seed=18, iou_threshold=0.3, motion_gain=192)
    v = [(int(rng.integers(-9, 10)), int(rng.integers(-9, 10))) for _ in range(64)]
    assert len(set(v)) > 32

    def grid(step, order=range(64)):
        return [(120 * (j // 8) + step * v[j][0], 120 * (j % 8) + step * v[j][1], 120 * (j // 8) + step * v[j][0] + 40,
                 120 * (j % 8) + step * v[j][1] + 40, 1.0 - i / 100.0) for i, j in enumerate(order)]

    got = p.update([frame(64, *grid(0))])
    assert got[0][0]["slot"].tolist() == list(range(64))
    p.update([frame(64, *grid(1))], want_assoc=False)
    p.check_state()
    assert p.ref.vel[0].tolist() == [[256 * a, 256 * b] for a, b in v]
    perm = rng.permutation(64)
    got = p.update([frame(64, *grid(2, perm))])
    assert got[0][0]["slot"].tolist() == perm.tolist() and (got[2][0]["ovr"] == 1).all()   # every detection sits on its track's predicted box
    p.update([frame(64, *grid(4, perm[:40]))])                                              # 24 tracks coast; the others jump two steps
    p.update([frame(64, *grid(5))], want_assoc=False)
    p.check_state()
    p.close()


def test_appearance_and_motion_together(frt):
    """a 2b re-attach updates the velocity by M2 and reports the predicted box's overlap; then the seeded soak of the appearance tests with
    every setting on"""
    e = np.zeros((1, 4), np.float32)
    e[0, 1] = 1
    p = Pair(frt, 1, 2, 1, 4, reid_threshold=0.5, motion_gain=256)
    for x in (0, 10, 20):
        p.update([frame(1, box(x))], e)
    got = p.update([frame(1, box(70))], e)
    a = got[2][0, 0]
    assert int(a["how"]) == frt.TRACK_ASSOC_APPEARANCE and a["ovr"] == tk.overlap((0,) + box(70)[:4], (0,) + box(30)[:4], 0) and a["sim"] == 1
    p.check_state()
    assert p.dev.motion(0)[0][0].tolist() == [50 * 256, 0]
    p.close()
    q = Pair(frt, 3, 6, 4, 8, reid_threshold=0.6, iou_min_sim=0.3, motion_gain=128, max_missed=3)
    hows = set()
    for k, (ids, res, emb) in enumerate(rr.soak(23, 3, 4, 8, 30)):
        got = q.update(res, emb, ids, want_assoc=k % 3 != 2)
        if k % 3 != 2:
            hows.update(got[2]["how"].reshape(-1).tolist())
        q.check_state(ids)
    assert {rr.HOW_IOU, rr.HOW_APPEARANCE, rr.HOW_BIRTH} <= hows
    q.close()


@pytest.mark.parametrize("n_streams,max_tracks,max_faces,gain,max_missed", [(8, 1, 1, 256, 5), (8, 8, 5, 64, 5), (8, 33, 5, 255, 0), (2, 64, 64, 1, 5)])
def test_the_gate_on_the_walks(frt, n_streams, max_tracks, max_faces, gain, max_missed):
    """appearance off: the gate's peek equals the association of the update that follows, on every call"""
    rng = np.random.default_rng(700 + max_tracks)
    p = Pair(frt, n_streams, max_tracks, max_faces, 4, seed=800 + max_tracks, max_missed=max_missed, iou_threshold=0.3, min_hits=2, motion_gain=gain)
    decisions = set()
    for k, per_stream in enumerate(drift_frames(rng, n_streams, max_faces, 24)):
        ids = [int(s) for s in rng.permutation(n_streams)[:rng.integers(1, n_streams + 1)]]
        results = [per_stream[s] for s in ids]
        counts = np.array([(r["score"] > 0).sum() for r in results], np.int32)
        g = p.gate(results, ids, int(rng.integers(1, 6)), int(rng.integers(1, 3)), float(np.float32(rng.uniform(0.3, 0.9))),
                   int(rng.integers(1, 2 * max_faces + 2)), None if k % 3 else counts)[0]
        got = p.update(results, ids=ids)
        trk, assoc = got[0], got[2]
        present, by_overlap = g["decision"] != gr.ABSENT, assoc["how"] == frt.TRACK_ASSOC_IOU
        assert (present == (assoc["how"] != frt.TRACK_ASSOC_ABSENT)).all()
        assert (g["slot"][present & by_overlap] == trk["slot"][present & by_overlap]).all() and (g["slot"][present & ~by_overlap] == -1).all()
        assert (g["ovr"][present & by_overlap].view(np.uint32) == assoc["ovr"][present & by_overlap].view(np.uint32)).all()
        decisions.update(g["decision"].reshape(-1).tolist())
    if max_tracks >= 8:
        assert {gr.EMBED, gr.FOLLOW} <= decisions
    p.close()


def test_the_gate_follows_a_coasting_return_only_with_motion(frt):
    for gain, want in ((256, (gr.FOLLOW, 0, 1.0, 0)), (None, (gr.EMBED, -1, 0.0, gr.NO_TRACK))):
        p = Pair(frt, 1, 2, 1, 4, min_hits=2, motion_gain=gain)
        for dets in COASTING[:-1]:
            p.update([frame(1, *dets)])
        g, lst, n, pc = p.gate([frame(1, *COASTING[-1])], None, 1000, 1, 0.9, 4)
        assert g[0, 0].tolist() == want and n == (0 if gain else 1)
        p.close()


def test_the_full_list_of_256_frames_of_64_faces_with_motion_on(frt):
    """every stream's faces move by the stream's own velocity; two tracks per stream: 512 faces are followed at skip_iou 0.9 because they
    sit on their tracks' predicted boxes, and none would be against the measured ones"""
    p = Pair(frt, 256, 2, 64, 4, seed=5, min_hits=1, iou_threshold=0.2, motion_gain=256)
    rng = np.random.default_rng(6)
    ids = [int(s) for s in rng.permutation(256)]
    v = rng.integers(-6, 7, (256, 2))
    v[:, 0] = rng.integers(3, 7, 256) * rng.choice([-1, 1], 256)                      # 3 px off the measured box is below skip_iou 0.9: 1558 / 1804

    def frames(step):
        return [frame(64, *[(60 * (i // 8) + step * int(v[s, 0]), 60 * (i % 8) + step * int(v[s, 1]), 60 * (i // 8) + step * int(v[s, 0]) + 40,
                             60 * (i % 8) + step * int(v[s, 1]) + 40, 1.0 - i / 100.0) for i in range(64)]) for s in ids]

    g, lst, n, pc = p.gate(frames(0), ids, 7, 1, 0.9, 128)
    assert n == 16384 and lst.tolist() == list(range(16384)) and pc.tolist() == [128] * 128
    p.update(frames(0), ids=ids, want_assoc=False)
    p.update(frames(1), ids=ids, want_assoc=False)
    g, lst, n, pc = p.gate(frames(2), ids, 7, 1, 0.9, 100)
    assert n == 16384 - 512 and (g["decision"] == gr.FOLLOW).sum() == 512 and (g["ovr"][g["decision"] == gr.FOLLOW] == 1).all() and (lst[n:] == -1).all()
    p.set_motion(0)
    assert p.gate(frames(2), ids, 7, 1, 0.9, 100)[2] == 16384
    p.close()


def test_reset_and_the_switch_between_calls(frt):
    p = Pair(frt, 2, 2, 1, 4)
    both = [0, 1]
    for x in (0, 10):
        p.update([frame(1, box(x)), frame(1, box(2 * x, 50))], ids=both)
    p.set_motion(64)                                                                  # live tracks with hits 2: the EMA branch from (0, 0)
    p.update([frame(1, box(20)), frame(1, box(40, 50))], ids=both)
    p.check_state()
    assert p.dev.motion(0)[0][0].tolist() == [640, 0] and p.dev.motion(1)[0][0].tolist() == [1280, 0]
    p.set_motion(256)                                                                 # on -> on keeps
    p.check_state()
    p.set_motion(0)
    p.update([frame(1, box(30)), frame(1, box(60, 50))], ids=both)                    # off: the array is neither read nor written
    p.check_state()
    p.set_motion(256)                                                                 # off -> on zeroes
    p.check_state()
    assert not p.dev.motion(0)[0].any() and not p.dev.motion(1)[0].any()
    p.update([frame(1, box(40)), frame(1, box(80, 50))], ids=both)
    p.check_state()
    p.reset(1)                                                                        # one stream: its velocities go, the other's stay
    p.check_state()
    assert p.dev.motion(0)[0][0].tolist() == [2560, 0] and not p.dev.motion(1)[0].any()
    p.update([frame(1, box(50)), frame(1, box(100, 50))], ids=both)
    p.reset()
    p.check_state()
    with pytest.raises(frt.FrtError):
        p.dev.setMotion(257)
    assert p.dev.getMotion() == 256
    p.close()


# ----------------------------------------------------------------------------------------------------------------- the pipeline
H, W, MF, PER, REC_BATCH = 96, 160, 8, 2, 4
TRACKER = dict(iou_threshold=0.3, max_missed=5, min_hits=2, decay=1.0)
OPTS = dict(refresh=1000, min_embeds=1, skip_iou=0.5)
ROLL, CALLS = 8, 6   # pixels per call
# n_embed per call of the rolled scene with motion off and on, from the restatement's gate on the CPU over the records Pipeline.run returns
# for these frames (tracks confirmed from the third call on).  The two differ, which is all the scene is for: the synthetic weights'
# boxes jitter from call to call rather than translate with the roll, so a velocity learned from them predicts no better than the
# measured box does - here it follows fewer faces.  What the setting does for boxes that do move is in the scripted scenes above.
N_EMBED = {0: [16, 16, 7, 7, 8, 9], 256: [16, 16, 12, 9, 10, 12]}


@pytest.fixture(scope="module")
def objs(frt, blobs, synth):
    dpath, _ = blobs("det")
    rpath, _ = blobs("ir")
    det = frt.RetinaFace(dpath, W, H, (3, H, W), 4, MF, 0.4, 0.02)
    rec = frt.ArcFaceIR50(rpath, W, H, maxBatchSize=REC_BATCH, maxFacesPerScene=MF)
    pipe = frt.Pipeline(det, rec, 4, match=False)
    yield pipe, synth.make_frames(PER, H, W)
    for o in (pipe, rec, det):
        o.close()


def twin_state_equals(tracked, twin):
    for s in range(PER):
        slots, cnt, sums = tracked.tracks(s, want_sums=True)
        assert slots.tobytes() == twin.slots[s].tobytes() and sums.tobytes() == twin.sums[s].tobytes(), s
        assert [cnt["next_id"], cnt["tick"], cnt["dropped"]] == twin.counters(s).tolist()
        if twin.gain:
            vel, pred = tracked.motion(s)
            assert vel.tobytes() == twin.motion(s)[0].tobytes() and pred.tobytes() == twin.motion(s)[1].tobytes(), s


@pytest.mark.parametrize("gain", [0, 256])
def test_run_tracked_honours_the_setting(frt, objs, gain):
    """the frames rolled ROLL px per call; the twin restatement is fed the pipeline's own records and embeddings"""
    pipe, first = objs
    tracked = frt.Tracker(PER, 16, MF, motion_gain=gain, **TRACKER)
    twin = mr.Tracker(PER, 16, MF, 512, motion_gain=gain, **TRACKER)
    lived = None
    for c in range(CALLS):
        res, emb, trk, tpl = pipe.runTracked(tracked, np.roll(first, ROLL * c, axis=2))
        want, want_tpl = twin.update(res, emb)
        assert trk.tobytes() == want.tobytes(), c
        check_templates(tpl, want_tpl, 512)
        twin_state_equals(tracked, twin)
        now = set(int(i) for i in trk["track_id"].reshape(-1) if i >= 0)
        lived = now if lived is None else lived & now
    assert lived, "no track lived through the calls"
    if gain:
        assert twin.vel.any()
    tracked.close()


@pytest.mark.parametrize("gain", [0, 256])
def test_run_tracked_gated_n_embed_matches_the_restatement_off_and_on(frt, objs, gain):
    """off and on differ on this scene, and NOT in motion's favour (see N_EMBED): the test is about equality with the restatement"""
    pipe, first = objs
    tracked = frt.Tracker(PER, 16, MF, motion_gain=gain, **TRACKER)
    twin = mr.Tracker(PER, 16, MF, 512, motion_gain=gain, **TRACKER)
    counts = []
    for c in range(CALLS):
        res, emb, trk, tpl, ne, gate = pipe.runTrackedGated(tracked, np.roll(first, ROLL * c, axis=2), want_gate=True, **OPTS)
        want_gate, _, want_ne, _ = mr.tracker_gate(twin, to_boxes(res), None, None, max_batch=REC_BATCH, **OPTS)
        assert gate.tobytes() == want_gate.tobytes() and ne == want_ne, (c, ne, want_ne)
        want, want_tpl = twin.update(res, emb)
        assert trk.tobytes() == want.tobytes(), c
        twin_state_equals(tracked, twin)
        counts.append(ne)
    print("n_embed per call, gain %d:" % gain, counts)
    assert counts == N_EMBED[gain], counts
    tracked.close()


def test_an_update_beside_another_threads_submits(frt, objs):
    pipe, first = objs
    want_res = np.zeros(PER * MF, frt.RESULT_DTYPE)
    pipe.wait(pipe.submit(first, want_res))
    errors, done, started = [], [], threading.Event()
    N = 60  # bound by a call count, not by time

    def worker():
        try:
            for _ in range(N):
                r = np.zeros(PER * MF, frt.RESULT_DTYPE)
                pipe.wait(pipe.submit(first, r))
                done.append(r.tobytes() == want_res.tobytes())
                started.set()
        except Exception as ex:  # noqa: BLE001
            errors.append(ex)
        started.set()

    th = threading.Thread(target=worker)
    th.start()
    assert started.wait(60)
    rng = np.random.default_rng(31)
    p = Pair(frt, 4, 8, 5, 64, seed=32, motion_gain=200, iou_threshold=0.3)
    for k, per_stream in enumerate(drift_frames(rng, 4, 5, 20)):
        ids = [int(s) for s in rng.permutation(4)[:rng.integers(1, 5)]]
        p.update([per_stream[s] for s in ids], ids=ids, want_assoc=k % 2 == 0)
        if k == 10:
            p.set_motion(0), p.set_motion(200)                                        # the zeroing, synchronous behind the last update
        p.check_state(ids)
    th.join()
    assert not errors and len(done) == N and all(done)
    p.close()
