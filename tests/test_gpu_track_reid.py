"""The tracker's appearance term on the GPU (track_similarity_kernel and track_update_kernel<true> behind frt_tracker_update_assoc,
frt_tracker_update and frt_pipeline_run_tracked) against tests/track_reid_ref.py, the numpy restatement fed the same calls.  After every update
the records, the association records (the `sim` and `ovr` bits included), and every stream's slots, counters and sums are compared by their
bytes; the templates go through test_gpu_track.py's bound, which holds unchanged: a template is still sum / ||sum|| of a bit-exact sum.  The
reference is never the code under test.  Inputs are finite (but for the one NaN case) and every product is normal or zero.

Why S can be held to the bit: dot2r fixes the order and the rounding of every operation (tests/test_track_reid_ref.py checks the numpy form
against a plain loop of the definition), and the fp32 division and square root are correctly rounded on both sides."""
import numpy as np
import pytest

import track_ref as tk
import track_reid_cases as cases
import track_reid_ref as rr
from test_gpu_track import template_bound
from test_track_reid_ref import SOAK, SOAK_OPT, SOAK_TRACKS

pytestmark = pytest.mark.gpu
SHAPES = [(8, 4, 3), (260, 4, 3), (512, 64, 3), (1024, 4, 64)]          # dim (260: a partial group), max_tracks, max_faces


def check_templates(got, want64, dim, nan_rows=None):
    """test_gpu_track.check_templates, but for the rows of tracks whose sum holds a NaN (the NaN case alone): track_ref's float64 template
    does not define those (its `norm > 0` is false for a NaN norm, the device divides by it), so they are only required to be NaN"""
    assert got.dtype == np.float32 and got.shape == want64.shape
    keep = np.ones(got.shape[:-1], bool) if nan_rows is None else ~nan_rows
    assert np.isnan(got[~keep]).all()
    got, want64 = got[keep], want64[keep]
    err = np.abs(got.astype(np.float64) - want64)
    assert (err <= template_bound(dim) * np.abs(want64) + 2.0 ** -149).all(), float((err / np.maximum(np.abs(want64), 1e-300)).max() * 2.0 ** 24)
    assert not got[want64 == 0].any()


class Pair:
    """a device tracker and the restatement fed the same calls; every update compares everything"""

    def __init__(self, frt, n_streams, max_tracks, max_faces, dim, reid_threshold=None, iou_min_sim=None, ref=None, **opt):
        self.dev = frt.Tracker(n_streams, max_tracks, max_faces, dim, reid_threshold=reid_threshold, iou_min_sim=iou_min_sim, **opt)
        self.ref = ref or rr.Tracker(n_streams, max_tracks, max_faces, dim, reid_threshold=reid_threshold, iou_min_sim=iou_min_sim, **opt)
        self.n_streams, self.dim = n_streams, dim

    def update(self, results, embeds, ids=None, want_assoc=True):
        results = np.concatenate(results) if isinstance(results, (list, tuple)) else results
        if want_assoc:
            got, tpl, assoc = self.dev.update(results, embeds, ids, want_assoc=True)
        else:
            (got, tpl), assoc = self.dev.update(results, embeds, ids), None
        if isinstance(self.ref, rr.Tracker):
            want, want_tpl, want_assoc_rec = self.ref.update(results, embeds, ids, want_assoc=True)
        else:
            (want, want_tpl), want_assoc_rec = self.ref.update(results, embeds, ids), None
        assert got.shape == want.shape and got.tobytes() == want.tobytes(), (got, want)
        if assoc is not None and want_assoc_rec is not None:
            assert assoc.shape == want_assoc_rec.shape and assoc.tobytes() == want_assoc_rec.tobytes(), (assoc, want_assoc_rec)
        stream = np.asarray(range(len(want)) if ids is None else ids)[:, None]
        nan_rows = (want["slot"] >= 0) & np.isnan(self.ref.sums[stream, np.maximum(want["slot"], 0)]).any(-1)
        check_templates(tpl, want_tpl, self.dim, nan_rows)
        self.check_state()
        return got, assoc

    def check_state(self):
        for s in range(self.n_streams):
            slots, cnt, sums = self.dev.tracks(s, want_sums=True)
            assert slots.tobytes() == self.ref.slots[s].tobytes(), (s, slots, self.ref.slots[s])
            assert [cnt["next_id"], cnt["tick"], cnt["dropped"]] == self.ref.counters(s).tolist(), s
            assert sums.tobytes() == self.ref.sums[s].tobytes(), s

    def set_appearance(self, reid, min_sim):
        self.dev.setAppearance(reid, min_sim)
        self.ref.set_appearance(reid, min_sim)

    def slots(self, s):
        return self.dev.tracks(s)[0]

    def sums(self, s):
        return self.dev.tracks(s, want_sums=True)[2]

    def close(self):
        self.dev.close()


def test_off_is_the_tracker_without_appearance(frt):
    """never set, and set to the off values: the plain update's records, templates and state are track_ref.Tracker's (which knows no
    appearance), and the association records of the same calls are the restatement's"""
    for setting in ("never set", "set to the off values"):
        for want_assoc in (False, True):
            ref = rr.Tracker(3, 4, 3, 260, max_missed=3) if want_assoc else tk.Tracker(3, 4, 3, 260, max_missed=3)
            p = Pair(frt, 3, 4, 3, 260, ref=ref, max_missed=3)
            if setting != "never set":
                p.dev.setAppearance(0.5, 0.2)
                p.dev.setAppearance(None, None)
            for ids, res, e in rr.soak(5, 3, 3, 260, 25):
                _, assoc = p.update(res, e, ids, want_assoc=want_assoc)
                assert assoc is None or not (assoc["how"] == rr.HOW_APPEARANCE).any()
            assert p.ref.next_id.sum() > 10
            p.close()


@pytest.mark.parametrize("dim,max_tracks,max_faces", SHAPES)
def test_reattach_after_a_jump(frt, dim, max_tracks, max_faces):
    """appearance on: the same id, how 2, gap 2; off: a new id.  (Fails on a library without the appearance term.)"""
    mk = lambda *a, **kw: Pair(frt, *a, **kw)
    cases.reattach_after_a_jump(mk, dim, max_tracks, max_faces, on=True)
    cases.reattach_after_a_jump(mk, dim, max_tracks, max_faces, on=False)
    for on in (True, False):
        cases.coast_past_max_missed_then_return(mk, dim, max_tracks, max_faces, on)


@pytest.mark.parametrize("dim,max_tracks,max_faces", SHAPES)
def test_veto_tie_and_order(frt, dim, max_tracks, max_faces):
    mk = lambda *a, **kw: Pair(frt, *a, **kw)
    cases.veto(mk, dim, max_tracks, max_faces, reid=True)
    cases.veto(mk, dim, max_tracks, max_faces, reid=False)
    cases.tie_goes_to_the_lowest_slot(mk, dim, max_tracks, max_faces)
    cases.detections_go_in_slot_order(mk, dim, max_tracks, max_faces)


@pytest.mark.parametrize("dim,max_tracks,max_faces", SHAPES)
def test_undefined_pairs_neither_veto_nor_match(frt, dim, max_tracks, max_faces):
    cases.undefined_pairs_neither_veto_nor_match(lambda *a, **kw: Pair(frt, *a, **kw), dim, max_tracks, max_faces)


def test_permuted_batch_and_a_stream_left_out(frt):
    cases.permuted_batch_and_a_stream_left_out(lambda *a, **kw: Pair(frt, *a, **kw), 260, 4, 3, rr.soak(6, 3, 3, 260, 25))


@pytest.mark.parametrize("decay", [1.0, 0.75])
def test_soak(frt, decay):
    """200 updates over 3 streams, thresholds 0.3 / 0.5 / 0.2: the calls whose coverage tests/test_track_reid_ref.py asserts for this seed"""
    p = Pair(frt, SOAK["n_streams"], SOAK_TRACKS, SOAK["max_faces"], SOAK["dim"], decay=decay, **SOAK_OPT)
    how = np.zeros(5, int)
    for ids, res, e in rr.soak(**SOAK):
        _, assoc = p.update(res, e, ids)
        how += np.bincount(assoc["how"].reshape(-1), minlength=5)
    assert (how >= 10).all() and p.ref.vetoes >= 10, (how, p.ref.vetoes)
    p.close()


def test_a_full_wave_of_detections_and_tracks(frt):
    """64 detections on 64 slots at dim 1024, 40 identities hopping between 48 positions: every lane of wave 0 takes part in 2a, 2b and the
    births, and the similarity kernel's workgroups stride all 64 slots"""
    p = Pair(frt, 2, 64, 64, 1024, iou_threshold=0.3, reid_threshold=0.5, iou_min_sim=0.2, max_missed=2)
    how = np.zeros(5, int)
    for ids, res, e in rr.soak(21, 2, 64, 1024, 8, n_ids=40, n_pos=48):
        _, assoc = p.update(res, e, ids)
        how += np.bincount(assoc["how"].reshape(-1), minlength=5)
    assert how[rr.HOW_IOU] > 0 and how[rr.HOW_APPEARANCE] > 5 and how[rr.HOW_BIRTH] > 20 and p.ref.vetoes > 0, (how, p.ref.vetoes)
    p.close()


def test_through_the_pipeline(frt, synth, blobs):
    """Pipeline.runTracked with appearance on, two streams, four calls (the scene drifts, and jumps far in the third): results / embeds are
    Pipeline.run's bit for bit, the tracks are the restatement's for those device results and embeddings"""
    H, W, MF, PER = 96, 160, 8, 2
    dpath, _ = blobs("det")
    rpath, _ = blobs("ir")
    det = frt.RetinaFace(dpath, W, H, (3, H, W), 4, MF, 0.4, 0.02)
    rec = frt.ArcFaceIR50(rpath, W, H, maxBatchSize=4, maxFacesPerScene=MF)
    pipe = frt.Pipeline(det, rec, 4, match=False)
    first = synth.make_frames(PER, H, W)
    opt = dict(reid_threshold=0.5, iou_min_sim=0.2, max_missed=2)
    tracked, ref = frt.Tracker(PER, 16, MF, **opt), rr.Tracker(PER, 16, MF, 512, **opt)
    faces, how = 0, np.zeros(5, int)
    for c, shift in enumerate((0, 2, 60, 62)):
        frames = np.roll(first, shift, axis=2)
        want_res, want_emb = pipe.run(frames)
        res, emb, trk, tpl = pipe.runTracked(tracked, frames)
        assert res.tobytes() == want_res.tobytes() and emb.tobytes() == want_emb.tobytes()
        want_trk, want_tpl, want_assoc = ref.update(want_res, want_emb, want_assoc=True)
        assert trk.tobytes() == want_trk.tobytes()
        how += np.bincount(want_assoc["how"].reshape(-1), minlength=5)
        check_templates(tpl, want_tpl, 512)
        faces += int((res["valid"] != 0).sum())
        for s in range(PER):
            slots, cnt, sums = tracked.tracks(s, want_sums=True)
            assert slots.tobytes() == ref.slots[s].tobytes() and sums.tobytes() == ref.sums[s].tobytes()
            assert [cnt["next_id"], cnt["tick"], cnt["dropped"]] == ref.counters(s).tolist()
    assert faces >= 8 and how[rr.HOW_IOU] > 0 and how[rr.HOW_APPEARANCE] > 0 and ref.vetoes > 0, (faces, how.tolist(), ref.vetoes)
    for o in (tracked, pipe, rec, det):
        o.close()
