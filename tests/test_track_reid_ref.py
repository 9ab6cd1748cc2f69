"""tests/track_reid_ref.py, the numpy restatement of the tracker's appearance term (include/frt.h "Appearance"): equal to track_ref.Tracker
with both settings off, dot2r against a plain loop of its definition, the scripted scenarios with the outcomes the header states, and the soak's
coverage for the seed the GPU test runs.  Nothing here needs the library."""
import numpy as np
import pytest

import track_ref as tk
import track_reid_cases as cases
import track_reid_ref as rr

SOAK = dict(seed=11, n_streams=3, max_faces=3, dim=260, updates=200)      # tests/test_gpu_track_reid.py runs the same calls
SOAK_OPT = dict(iou_threshold=0.3, reid_threshold=0.5, iou_min_sim=0.2, max_missed=3)
SOAK_TRACKS = 4


class Ref:
    """the restatement behind the interface of track_reid_cases"""

    def __init__(self, *shape, **opt):
        self.t = rr.Tracker(*shape, **opt)

    def update(self, results, embeds, ids=None):
        results = np.concatenate(results) if isinstance(results, (list, tuple)) else results
        trk, _, assoc = self.t.update(results, embeds, ids, want_assoc=True)
        return trk, assoc

    def set_appearance(self, reid, min_sim):
        self.t.set_appearance(reid, min_sim)

    def slots(self, s):
        return self.t.slots[s]

    def sums(self, s):
        return self.t.sums[s]

    def close(self):
        pass


def dot2r_loop(x, y):
    """the definition, one float32 operation at a time"""
    dim, G = len(x), -(-len(x) // 256)
    v = []
    for lane in range(64):
        acc = np.float32(0)
        for g in range(G):
            for j in range(4):
                k = 256 * g + 4 * lane + j
                if k < dim:
                    acc = np.float32(acc + np.float32(x[k] * y[k]))
        v.append(acc)
    for off in (32, 16, 8, 4, 2, 1):
        v = [np.float32(v[lane] + v[lane ^ off]) for lane in range(64)]
    assert all(a.tobytes() == v[0].tobytes() for a in v)                 # all lanes hold the same bits
    return v[0]


@pytest.mark.parametrize("dim", [4, 8, 260, 512, 2048])
def test_dot2r_is_the_plain_loop_of_its_definition(dim):
    rng = np.random.default_rng(dim)
    x, y = rng.standard_normal((2, 3, dim)).astype(np.float32)
    got = rr.dot2r(x, y)
    assert got.dtype == np.float32 and got.shape == (3,)
    for i in range(3):
        assert got[i].tobytes() == dot2r_loop(x[i], y[i]).tobytes()
    assert rr.dot2r(x[0], x[0]).tobytes() == dot2r_loop(x[0], x[0]).tobytes()


def test_with_both_settings_off_the_restatement_is_track_ref():
    for setting in ("never set", "set to the off values"):
        a, b = tk.Tracker(3, 4, 3, 64, max_missed=3), rr.Tracker(3, 4, 3, 64, max_missed=3)
        if setting != "never set":
            b.set_appearance(0.5, 0.2)
            b.set_appearance(None, None)
        for ids, res, e in rr.soak(5, 3, 3, 64, 60):
            ta, pa = a.update(res, e, ids)
            tb, pb, assoc = b.update(res, e, ids, want_assoc=True)
            assert ta.tobytes() == tb.tobytes() and pa.tobytes() == pb.tobytes()
            assert not (assoc["how"] == rr.HOW_APPEARANCE).any() and ((assoc["how"] == rr.HOW_ABSENT) == ~(res["score"] > 0).reshape(tb.shape)).all()
            assert ((assoc["how"] == rr.HOW_UNTRACKED) == ((tb["track_id"] < 0) & (res["score"] > 0).reshape(tb.shape))).all()
        assert a.slots.tobytes() == b.slots.tobytes() and a.sums.tobytes() == b.sums.tobytes() and b.vetoes == 0
        assert (a.next_id == b.next_id).all() and (a.tick == b.tick).all() and (a.dropped == b.dropped).all() and a.next_id.sum() > 20


def test_setting_ranges():
    for ok in ((0.5, 0.2), (1.0, -1.0), (1e-6, 1.0), (2.0, -2.0), (2.0, 0.0), (0.3, -2.0)):
        assert rr.check_appearance(*ok), ok
    nan = float("nan")
    for bad in ((0.0, 0.2), (-0.5, 0.2), (1.5, 0.2), (nan, 0.2), (0.5, -1.5), (0.5, 1.5), (0.5, nan), (0.5, 2.0), (-2.0, 0.2), (3.0, -2.0)):
        assert not rr.check_appearance(*bad), bad


@pytest.mark.parametrize("dim,max_tracks,max_faces", [(8, 4, 3), (260, 4, 3)])
def test_scripted_scenarios(dim, max_tracks, max_faces):
    for on in (True, False):
        cases.reattach_after_a_jump(Ref, dim, max_tracks, max_faces, on)
        cases.coast_past_max_missed_then_return(Ref, dim, max_tracks, max_faces, on)
        cases.veto(Ref, dim, max_tracks, max_faces, reid=on)
    cases.tie_goes_to_the_lowest_slot(Ref, dim, max_tracks, max_faces)
    cases.detections_go_in_slot_order(Ref, dim, max_tracks, max_faces)
    cases.undefined_pairs_neither_veto_nor_match(Ref, dim, max_tracks, max_faces)
    cases.permuted_batch_and_a_stream_left_out(Ref, dim, max_tracks, max_faces, rr.soak(6, 3, max_faces, dim, 25))


def test_without_the_veto_the_look_alike_swap_happens():
    """the veto scenario with both settings off: overlap hands track 0 the other person's face - what iou_min_sim is there to refuse"""
    a, b = cases.unit_rows(8)[:2]
    t = Ref(1, 4, 3, 8)
    t.update([rr.frame(3, cases.A, cases.B)], cases.emb(3, 8, a, b))
    trk, assoc = t.update([rr.frame(3, cases.A)], cases.emb(3, 8, b))
    assert trk[0, 0]["track_id"] == 0 and assoc[0, 0]["how"] == rr.HOW_IOU and assoc[0, 0]["sim"] == 0      # S(b, a) = 0: reported, not acted on
    assert t.sums(0)[0].tobytes() == (a + b).tobytes()                                                         # a template over two persons


@pytest.mark.parametrize("decay", [1.0, 0.75])
def test_soak_coverage(decay):
    """the sequence the GPU test runs reaches every `how` value, the veto and the re-attach at least ten times each"""
    t = rr.Tracker(SOAK["n_streams"], SOAK_TRACKS, SOAK["max_faces"], SOAK["dim"], decay=decay, **SOAK_OPT)
    how = np.zeros(5, int)
    gaps = set()
    for ids, res, e in rr.soak(**SOAK):
        _, _, assoc = t.update(res, e, ids, want_assoc=True)
        how += np.bincount(assoc["how"].reshape(-1), minlength=5)
        gaps.update(assoc["gap"][assoc["how"] == rr.HOW_APPEARANCE].tolist())
    assert (how >= 10).all(), how.tolist()
    assert t.vetoes >= 10 and how[rr.HOW_APPEARANCE] >= 10, (t.vetoes, how.tolist())
    assert len(gaps) >= 3 and t.dropped.sum() == how[rr.HOW_UNTRACKED] and t.tick.sum() > 400, (gaps, t.tick)
