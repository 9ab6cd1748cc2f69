"""Cases, inputs, references and derived bounds for the launches between the detector's heads and the recogniser's input, run ONE AT A TIME
(tests/cpp/det_tail_check.cpp): decode_kernel, nms_kernel, landmark_decode_kernel, pack_results_kernel (kernels_post.hip), crop_faces_kernel and
align_faces_kernel (kernels_image.hip).  A generator and a reference, not a test: tests/test_det_tail_ref.py (no GPU) and
tests/test_gpu_det_tail.py use it.  Every group below writes a list of operations for the harness (class Ops) and returns a function that reads
what the harness wrote back and returns failure messages.

The DetGeom of every case is made by the library's own det_geometry() (the harness's `geom` op) and dumped; this side derives the anchors from
oracle.anchors (mnet) and slim_ref.anchors (either table) and compares A and every table field of the dump with them.

Geometries (in_w x in_h, frame_w x frame_h):
    mnet   320 x 288, 640 x 480   A = 3 780 = 59 * 64 + 4     scale_h 0.6  >  scale_w 0.5
    slim   160 x 96,  100 x 200   A = 888  = 13 * 64 + 56     scale_h 0.48 <  scale_w 1.6: the other un-letterbox branch
    slimw  160 x 96,  200 x 100   A = 888                     scale_h 0.96 >  scale_w 0.8: a frame 200 wide and 100 high takes the SAME branch as
                                                              mnet, so the frame of `slim` is 100 wide and 200 high; both are run.

u = 2^-24 throughout.  The analyses below are written to first order; WIDE = 1 + 2^-10 covers the u |computed| against u |exact| terms, and
align_reference() adds the products of two errors (E_s E_d, E_a E_ms, E_ia E_ux, ...) and divides by den - E_den, n2 - E_n2 explicitly.

Boxes.  Reference: oracle.postprocess (mnet) / slim_ref.postprocess (Slim table), frame by frame; x1, y1, x2, y2 and the score bits are compared
exactly.  oracle.postprocess does not return the kept anchors: they come from slim_ref.postprocess run with the mnet table, after asserting that
its boxes equal the oracle's byte for byte and that the candidate anchors equal the oracle's.  make_heads() keeps |loc| <= 2, so every decoded
float is finite (exp(0.4) at most): the int conversion of a non-finite value is undefined in the reference.

Landmark decode (landmark_reference).  The formula in the comment above landmark_decode_kernel, in float64, the anchor table a parameter:
    X = (acx + p * 0.1 * asx) * in_w,  acx = (j + 0.5) step / in_w,  asx = min_size / in_w           (Y alike with i, in_h)
    scale_h > scale_w:  x = X / scale_w,  y = (Y - (in_h - scale_w frame_h) / 2) / scale_w;   otherwise  x = (X - (in_w - scale_h frame_w) / 2) / scale_h,  y = Y / scale_h
with scale_w = in_w / frame_w, scale_h = in_h / frame_h exact.  The kernel's float32 operations: asx and acx one division each ((j + 0.5) * step
is exact: step is a power of two), p * 0.1f (the constant u, the product u), * asx (u, and asx's own u): T = |p 0.1 asx| carries 4 u; the sum
acx + .. one rounding, * in_w one:
    E_X = u (in_w (acx + 4 T) + 2 |X|)
A division by the float32 scale (u for the scale, u for the quotient):  E_x = E_X / scale + 2 u |x|.  The pad: scale * frame (2 u on P = scale
frame), the subtraction from in (u |in - P|), the halving exact:  E_pad = (2 u P + u |in - P|) / 2;  Y - pad one rounding:
    E_y = (E_Y + E_pad + u |Y - pad|) / scale + 2 u |y|.
Bound = WIDE * E.  (A contracted multiply-add only removes a rounding.)  At these shapes the bound is 2e-5 .. 4e-4 px.

Alignment (align_reference).  float64: means, centred sums sa, sb, den, a = sa / den, b = sb / den, t = md - [a -b; b a] ms, n2 = a^2 + b^2,
ia = a / n2, ib = b / n2, source = [ia ib; -ib ia] (dst - t), bilinear value with zero border BEFORE rounding to u8.  The template is the
kernel's float32 constants (public ArcFace values), the landmarks the float32 inputs, both exact in float64.  Forward error of the kernel's
float32 operations, first order, S1 = sum |lm|:
    mean        four additions and * 0.2f (constant u, product u)          E_ms = 0.8 u S1 + 2 u |ms|            (E_md alike, for the template)
    centred     s_k = lm_k - ms                                            E_sk = E_ms + u |s_k|                 (E_dk alike)
    sa, sb      products, pair sums, five accumulations; Pa = sum |sx dx| + |sy dy|
                                                                           E_sa = sum (E_s |d| + E_d |s|) + 7 u Pa   (E_sb with Pb alike)
    den                                                                    E_den = sum 2 E_s |s| + 7 u den
    a = sa/den                                                             E_a = E_sa / den + |a| E_den / den + u |a|     (E_b alike)
    tx = mdx - (a msx - b msy)                                             E_tx = E_md + E_a |msx| + |a| E_msx + E_b |msy| + |b| E_msy
                                                                                  + 2 u (|a msx| + |b msy|) + u |tx|      (E_ty alike)
    n2                                                                     E_n2 = 2 |a| E_a + 2 |b| E_b + 2 u n2
    ia = a/n2                                                              E_ia = E_a / n2 + |ia| E_n2 / n2 + u |ia|      (E_ib alike)
    ux = ox - tx                                                           E_ux = E_tx + u |ux|                           (E_uy alike)
    sx = ia ux + ib uy                                                     E_sx = E_ia |ux| + |ia| E_ux + E_ib |uy| + |ib| E_uy + 2 u (|ia ux| + |ib uy|)
and E_sy the same with the roles of ia and ib exchanged.  The bilinear interpolant with zero border is continuous, and inside one cell its
slope in x is at most the larger of the cell's two horizontal tap differences (Lx; Ly alike), so moving the coordinate by (E_sx, E_sy) changes
it by at most E_sx Lx + E_sy Ly with Lx, Ly the maxima over the cells [floor(s - E), floor(s + E)] the move can touch (E >= 1: 255).  The
interpolation itself: wx = sx - floor(sx) and the tap differences are exact; top, bot two roundings each on values <= 255, bot - top, its
product with wy, the last sum and val + 0.5 one each:  E_I = 11 u 256.  The kernel's u8 is floor(val^ + 0.5), within 0.5 of val^:
    |got_u8 - value64| <= 0.5 + bound,   bound = WIDE (E_sx Lx + E_sy Ly) + E_I          every pixel and channel, none left out.
`ok` of the reference is den > 1e-6 and sa^2 + sb^2 > 1e-12 in float64; every case keeps both a factor 100 away from the constants or is
non-finite.  In align_faces_kernel a NaN or an infinite coordinate makes den NaN (inf - inf in the centring), and den > 1e-6f is then false;
five identical points give den = 0: all three set ok = false BEFORE the `if (ok)` block that holds every read of a frame byte.
chw is compared with ((crop[..., ::-1] - 127.5) * 0.0078125) of the device's own crops bit for bit: exact in float32 (a half-integer below 2^8
times a power of two).

Crops: oracle.crop_faces byte for byte; validity by the rule of frt_kernels.h (slot below n_boxes of its frame, ROI non-empty and inside the frame).
pack_results: the rule of the kernel's comment, restated in pack_reference().
"""
import collections
import functools
import os
import sys

import numpy as np

import slim_ref
from launch_harness import Ops as _Ops, bit_diff as _bit_diff, fbits, rng as _rng

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

U = 2.0 ** -24
WIDE = 1 + 2.0 ** -10
E_INTERP = 11 * U * 256
FILL32 = 0x5A5A5A5A
CC_STRIDE = 32
NMS_THR, BBOX_THR = 0.4, 0.6
f32 = np.float32

BBOX_DTYPE = slim_ref.BBOX_DTYPE
CAND_DTYPE = np.dtype([("x1", "<i4"), ("y1", "<i4"), ("x2", "<i4"), ("y2", "<i4"), ("score", "<f4"), ("anchor", "<i4")])
RESULT_DTYPE = np.dtype([("x1", "<i4"), ("y1", "<i4"), ("x2", "<i4"), ("y2", "<i4"), ("score", "<f4"), ("frame", "<i4"), ("match_idx", "<i4"),
                         ("match_sim", "<f4"), ("valid", "<i4")])
GEOM_DTYPE = np.dtype([("in_w", "<i4"), ("in_h", "<i4"), ("frame_w", "<i4"), ("frame_h", "<i4"), ("levels", "<i4"), ("fw", "<i4", 4), ("fh", "<i4", 4),
                       ("base", "<i4", 4), ("nsz", "<i4", 4), ("min_size", "<i4", (4, 3)), ("step", "<f4", 4), ("A", "<i4"), ("scale_w", "<f4"),
                       ("scale_h", "<f4"), ("nms_thr", "<f4"), ("bbox_thr", "<f4"), ("max_faces", "<i4")])
assert CAND_DTYPE.itemsize == 24 and RESULT_DTYPE.itemsize == 36 and GEOM_DTYPE.itemsize == 172

# The largest figures printed by tests/test_gpu_det_tail.py on an MI355X, 2026-10-20 (the assertion is ratio <= 1, whatever stands here).
# Landmarks: max(err / bound) per table.  Alignment: max((err - 0.5) / bound) over all pixels of all faces - it stays near 0 because a u8 lies
# within 0.5 of the float64 value unless that value sits next to a rounding boundary; the largest bound of a face is 0.13 - 1.5 grey levels
# (mirror 4.9, den1e-3 13.4).  The device gave the figures of the float32 mirror (oracle/align.py) on every case.
RATIOS_SEEN = {"landmarks": {"mnet": 0.3227, "slim": 0.4140, "slimw": 0.4263}, "alignment": {"largest, rot-0.90_s1": 0.0019}}


class Geom(collections.namedtuple("Geom", "name family levels in_w in_h frame_w frame_h table")):
    @property
    def A(self):
        return slim_ref.anchor_count(self.in_w, self.in_h, self.table)

    @property
    def branch_h(self):
        """the kernel's test scale_h > scale_w (float32, as DetGeom holds them)"""
        return bool(f32(self.in_h) / f32(self.frame_h) > f32(self.in_w) / f32(self.frame_w))


MNET = Geom("mnet", 1, 3, 320, 288, 640, 480, slim_ref.MNET)
SLIM = Geom("slim", 4, 4, 160, 96, 100, 200, slim_ref.SLIM)
SLIMW = Geom("slimw", 4, 4, 160, 96, 200, 100, slim_ref.SLIM)


def oracle():
    import oracle as o
    o.lib()
    return o


class Ops(_Ops):
    def load(self, name, arr, tag):
        fn = "%s.%s.%s.in" % (self.cid, name, tag)
        np.ascontiguousarray(arr).tofile(os.path.join(self.dir, fn))
        self.lines.append("load %s %s" % (name, fn))

    def geom(self, g, K, nms=NMS_THR, thr=BBOX_THR):
        """sets the DetGeom of the following launches and dumps it; returns the dump's file name"""
        self.op("geom", g.family, g.levels, g.in_w, g.in_h, g.frame_w, g.frame_h, fbits(nms), fbits(thr), K)
        fn = "%s.geom.out" % self.cid
        self.lines.append("dump_geom " + fn)
        return fn


def check_geom(ops, fn, g, K, nms=NMS_THR, thr=BBOX_THR):
    """[] or messages: the dumped production DetGeom against anchors derived here (oracle.anchors, slim_ref.anchors / feature_maps)"""
    raw = ops.read(fn, np.uint8)
    if raw is None or raw.size != GEOM_DTYPE.itemsize:
        return ["%s was not written" % fn]
    d = raw.view(GEOM_DTYPE)[0]
    fails = []
    anc = slim_ref.anchors(g.in_w, g.in_h, g.table)
    if int(d["A"]) != len(anc):
        fails.append("%s: A = %d, slim_ref.anchors has %d" % (fn, d["A"], len(anc)))
    if g.family == 1 and int(d["A"]) != len(oracle().anchors(g.in_w, g.in_h)):
        fails.append("%s: A = %d, oracle.anchors has %d" % (fn, d["A"], len(oracle().anchors(g.in_w, g.in_h))))
    fm = slim_ref.feature_maps(g.in_w, g.in_h, g.table)
    base = 0
    for k in range(g.levels):
        ms = g.table["min_sizes"][k]
        want = (fm[k][1], fm[k][0], base, len(ms), float(g.table["steps"][k]))
        got = (int(d["fw"][k]), int(d["fh"][k]), int(d["base"][k]), int(d["nsz"][k]), float(d["step"][k]))
        if got != want or tuple(d["min_size"][k][:len(ms)]) != tuple(ms):
            fails.append("%s: level %d is %r sizes %r, expected %r sizes %r" % (fn, k, got, tuple(d["min_size"][k]), want, ms))
        base += fm[k][0] * fm[k][1] * len(ms)
    want = (g.in_w, g.in_h, g.frame_w, g.frame_h, g.levels, K, fbits(nms), fbits(thr), fbits(f32(g.in_w) / f32(g.frame_w)), fbits(f32(g.in_h) / f32(g.frame_h)))
    got = (int(d["in_w"]), int(d["in_h"]), int(d["frame_w"]), int(d["frame_h"]), int(d["levels"]), int(d["max_faces"]), fbits(d["nms_thr"]), fbits(d["bbox_thr"]),
           fbits(d["scale_w"]), fbits(d["scale_h"]))
    if got != want:
        fails.append("%s: scalars %r, expected %r" % (fn, got, want))
    return fails


def _guards(ops, fails):
    res = ops.results()
    for cid in ops.cases:
        if cid not in res:
            fails.append("%s: the harness did not finish the case" % cid)
        elif res[cid]:
            fails.append("%s: %d guard bytes / inputs changed" % (cid, res[cid]))


# ------------------------------------------------------------------------------------------------ heads and the box reference
def make_heads(g, counts, seed, thr=BBOX_THR, top=()):
    """loc [B][A][4], conf [B][A][2] with EXACTLY counts[f] scores above thr in frame f (asserted), all distinct; the other scores lie below thr
    or exactly on it, and column 0 (never a score) is above it everywhere.  |loc| <= 2: every decoded float is finite (the int conversion of a
    non-finite value is undefined in the reference).  top: (frame, anchor) pairs that receive the highest scores of their frame."""
    rng = _rng("heads", g.name, seed, counts)
    A, B = g.A, len(counts)
    loc = np.clip(rng.normal(0, 0.5, (B, A, 4)), -2, 2).astype(f32)
    conf = np.empty((B, A, 2), f32)
    conf[..., 0] = 0.99
    conf[..., 1] = rng.uniform(0.0, thr - 0.01, (B, A)).astype(f32)
    for f, n in enumerate(counts):
        perm = rng.permutation(A)
        tops = np.array([a for ff, a in top if ff == f], np.int64)
        assert len(tops) <= n
        perm = np.concatenate([tops, perm[~np.isin(perm, tops)]])
        s = (thr + 0.01 + (0.97 - thr) * (np.arange(n)[::-1] + 0.5) / max(n, 1)).astype(f32)  # descending
        conf[f, perm[:n], 1] = np.concatenate([s[:len(tops)], rng.permutation(s[len(tops):])])
        conf[f, perm[n:n + 5], 1] = f32(thr)  # exactly on the threshold: not a candidate
        assert len(np.unique(conf[f, perm[:n], 1])) == n
    assert tuple(int(v) for v in (conf[..., 1] > f32(thr)).sum(1)) == tuple(counts)
    assert np.isfinite(loc).all() and np.abs(loc).max() <= 2
    return loc, conf


def ref_frame(g, loc, conf, K, nms=NMS_THR, thr=BBOX_THR):
    """(boxes, kept anchors, candidate anchors) of one frame"""
    boxes, kept = slim_ref.postprocess(loc, conf, g.in_w, g.in_h, g.frame_w, g.frame_h, nms, thr, K, table=g.table, return_kept=True)
    cand = np.nonzero(conf[:, 1] > f32(thr))[0]
    if g.family == 1:
        ob, _, cidx = oracle().postprocess(loc, conf, g.in_w, g.in_h, g.frame_w, g.frame_h, nms, thr, K, return_candidates=True)
        assert np.array_equal(cidx, cand), "the oracle's candidates differ from conf > thr"
        assert ob.tobytes() == boxes.tobytes(), "slim_ref.postprocess with the mnet table differs from oracle.postprocess"
        boxes = ob
    return boxes, np.asarray(kept, np.int32), cand


@functools.lru_cache(maxsize=None)
def heads_and_refs(gname, counts, seed, Ks, top=()):
    g = GEOMS[gname]
    loc, conf = make_heads(g, counts, seed, top=top)
    refs = {K: [ref_frame(g, loc[f], conf[f], K) for f in range(len(counts))] for K in Ks}
    for K in Ks:
        for n, (boxes, _, cand) in zip(counts, refs[K]):
            assert len(cand) == n
            assert len(boxes) >= min(K, 4, n), "the reference keeps %d boxes of %d candidates at K = %d" % (len(boxes), n, K)
    return loc, conf, refs


GEOMS = {g.name: g for g in (MNET, SLIM, SLIMW)}


def _post_bufs(ops, g, B, K, loc, conf, count=None):
    ops.rbuf("conf", conf)
    ops.rbuf("loc", loc)
    ops.buf("cand", B * g.A * 24)
    ops.buf("count", B * CC_STRIDE * 4, np.zeros(B * CC_STRIDE, np.int32) if count is None else count)
    ops.buf("dead", B * g.A)
    ops.buf("out", B * K * 20)
    ops.buf("nout", B * 4)
    ops.buf("kept", B * K * 4)


def _post_dumps(ops, tag=""):
    return {n: ops.dump(n, tag) for n in ("out", "nout", "kept", "count")}


def _cmp_post(tag, ops, files, B, K, refs, fresh, fails, check_count=True):
    out, nout, kept, count = (ops.read(files[n], t) for n, t in (("out", np.uint8), ("nout", np.int32), ("kept", np.uint32), ("count", np.int32)))
    if out is None or nout is None or kept is None or count is None:
        fails.append("%s: outputs were not written" % tag)
        return
    out = out.view(BBOX_DTYPE).reshape(B, K)
    kept = kept.reshape(B, K)
    for f, (boxes, rk, cand) in enumerate(refs):
        n = len(boxes)
        where = "%s frame %d (%d candidates)" % (tag, f, len(cand))
        if int(nout[f]) != n:
            fails.append("%s: n_out %d, reference %d" % (where, nout[f], n))
            continue
        if out[f, :n].tobytes() != boxes.tobytes():
            bad = [i for i in range(n) if out[f, i].tobytes() != boxes[i].tobytes()]
            fails.append("%s: %d of %d boxes differ, first slot %d: %r, reference %r" % (where, len(bad), n, bad[0], out[f, bad[0]], boxes[bad[0]]))
        if np.frombuffer(out[f, n:].tobytes(), np.uint8).any():
            fails.append("%s: a slot >= n_out is not all-zero" % where)
        if not np.array_equal(kept[f, :n].astype(np.int64), rk.astype(np.int64)):
            fails.append("%s: kept anchors %r, reference %r" % (where, kept[f, :n][:8], rk[:8]))
        if fresh and (kept[f, n:] != FILL32).any():
            fails.append("%s: kept_anchor was written at a slot >= n_out" % where)
    if check_count and count.any():
        fails.append("%s: cand_count is not back at zero: %r" % (tag, np.nonzero(count)[0][:8]))


# ------------------------------------------------------------------------------------------------ decode alone
def _decode_inputs(g, thr):
    """conf [3][A][2] and the expected candidate anchors per frame"""
    rng = _rng("decode", g.name, thr)
    A = g.A
    conf = np.empty((3, A, 2), f32)
    conf[..., 0] = 0.99
    if thr < 0:  # every finite score is above a negative threshold: count == A unless a lane past A is counted too
        conf[..., 1] = rng.uniform(0.01, 0.9, (3, A)).astype(f32)
        conf[1, rng.permutation(A)[:7], 1] = np.nan
    else:
        conf[..., 1] = rng.uniform(0.0, thr - 0.01, (3, A)).astype(f32)  # frame 0: no candidate
        last = (A // 64) * 64  # frame 1: candidates in the last, partial wave of the frame only
        assert 0 < A - last < 64
        conf[1, last + 1:A:2, 1] = rng.uniform(thr + 0.01, 0.99, len(range(last + 1, A, 2))).astype(f32)
        conf[1, A - 1, 1] = 0.97
        p = rng.permutation(A)  # frame 2, the last: a mixture; the guard pattern (1.5e16) lies directly behind it
        conf[2, p[:90], 1] = rng.uniform(thr + 0.01, 0.99, 90).astype(f32)
        conf[2, p[90:100], 1] = f32(thr)  # exactly on the threshold: not taken
        conf[2, p[100:110], 1] = np.nan  # not taken
        conf[2, p[110:114], 1] = np.inf  # taken
        conf[2, p[114:118], 1] = -np.inf
        conf[2, A - 1, 1] = 0.98
        conf[2, A - 2, 1] = f32(thr)
    with np.errstate(invalid="ignore"):
        want = [np.nonzero(conf[f, :, 1] > f32(thr))[0] for f in range(3)]
    if thr >= 0:
        assert len(want[0]) == 0 and want[1].min() >= (A // 64) * 64 and np.isinf(conf[2, want[2], 1]).sum() == 4
    else:
        assert [len(w) for w in want] == [A, A - 7, A]
    return conf, want


def group_decode(ops):
    plan = []
    for g in (MNET, SLIM):
        for thr in (BBOX_THR, -1.0):
            ops.case("decode_%s_%s" % (g.name, "neg" if thr < 0 else "pos"))
            conf, want = _decode_inputs(g, thr)
            ops.rbuf("conf", conf)
            ops.buf("cand", 3 * g.A * 24)
            count0 = np.full(3 * CC_STRIDE, FILL32, np.uint32)
            count0[::CC_STRIDE] = 0
            ops.buf("count", count0.nbytes, count0)
            gf = ops.geom(g, 4, thr=thr)
            ops.op("decode", "conf", 3, "cand", "count")
            plan.append((ops.cid, g, thr, conf, want, gf, ops.dump("cand"), ops.dump("count")))
            ops.end()

    def check():
        fails = []
        _guards(ops, fails)
        for cid, g, thr, conf, want, gf, fc, fn in plan:
            fails += check_geom(ops, gf, g, 4, thr=thr)
            cand, count = ops.read(fc, np.uint8), ops.read(fn, np.uint32)
            if cand is None or count is None:
                fails.append("%s: outputs were not written" % cid)
                continue
            cand = cand.view(CAND_DTYPE).reshape(3, g.A)
            other = np.ones(len(count), bool)
            other[::CC_STRIDE] = False
            if (count[other] != FILL32).any():
                fails.append("%s: a counter word of no frame was written" % cid)
            for f in range(3):
                n = int(count[f * CC_STRIDE])
                if n != len(want[f]):
                    fails.append("%s frame %d: cand_count %d, expected %d" % (cid, f, n, len(want[f])))
                    n = min(max(n, 0), g.A)
                got = cand[f, :n]
                gs = sorted(zip(got["anchor"].tolist(), got["score"].view(np.uint32).tolist()))
                ws = sorted(zip(want[f].tolist(), conf[f, want[f], 1].view(np.uint32).tolist()))
                if gs != ws:
                    fails.append("%s frame %d: the candidate set differs (%d entries, expected %d)" % (cid, f, len(gs), len(ws)))
                if any(got[k].any() for k in ("x1", "y1", "x2", "y2")):
                    fails.append("%s frame %d: a box field of a written candidate is not 0" % (cid, f))
                if (np.frombuffer(cand[f, n:].tobytes(), np.uint8) != 0x5A).any():
                    fails.append("%s frame %d: a cand entry past the count was written" % (cid, f))
        return fails

    return check


# ------------------------------------------------------------------------------------------------ decode + nms
BATCH_COUNTS = (257, 0, 256, 1000, 255, 1, 300, 3780)
BATCH_KS = (1, 4, 300)


def _batched(ops, g, counts, seed, Ks, plan, top=()):
    loc, conf, refs = heads_and_refs(g.name, counts, seed, Ks, top)
    B = len(counts)
    for K in Ks:
        ops.case("post_%s_K%d" % (g.name, K))
        _post_bufs(ops, g, B, K, loc, conf)
        gf = ops.geom(g, K)
        ops.op("decode", "conf", B, "cand", "count")
        ops.op("nms", "cand", "loc", "count", B, "dead", "out", "nout", "kept")
        plan.append((ops.cid, g, B, K, refs[K], gf, _post_dumps(ops)))
        ops.end()


def _batched_check(ops, plan):
    def check():
        fails = []
        _guards(ops, fails)
        for cid, g, B, K, refs, gf, files in plan:
            fails += check_geom(ops, gf, g, K)
            _cmp_post(cid, ops, files, B, K, refs, True, fails)
        return fails
    return check


def group_batched(ops):
    plan = []
    _batched(ops, MNET, BATCH_COUNTS, 1, BATCH_KS, plan)
    return _batched_check(ops, plan)


def slim_top(g):
    """level 3 of the Slim table (three sizes per cell) gets the best score of each frame: its last anchor (size index 2) and its first (0)"""
    fh, fw = slim_ref.feature_maps(g.in_w, g.in_h, g.table)[3]
    return ((0, g.A - 1), (1, g.A - fh * fw * 3))


def slim_kept_level3(g):
    _, _, refs = heads_and_refs(g.name, (40, 300), 2, (4,), slim_top(g))
    base3 = g.A - slim_ref.feature_maps(g.in_w, g.in_h, g.table)[3][0] * slim_ref.feature_maps(g.in_w, g.in_h, g.table)[3][1] * 3
    return all((kept >= base3).any() for _, kept, _ in refs[4])


def group_slim(ops):
    plan = []
    for g in (SLIM, SLIMW):
        assert slim_kept_level3(g), "no kept anchor in level 3 (three sizes per cell)"
        _batched(ops, g, (40, 300), 2, (4,), plan, slim_top(g))
    return _batched_check(ops, plan)


SEQ_COUNTS = ((1000, 300), (300, 200), (200, 1000))
SEQ_K = 300


def group_sequence(ops):
    """three calls on the same buffers, nothing re-initialised in between: a fast-path frame after a general-path one meets stale dead[] and cand[]"""
    g, B, K = MNET, 2, SEQ_K
    calls = [heads_and_refs(g.name, c, 10 + i, (K,)) for i, c in enumerate(SEQ_COUNTS)]
    ops.case("post_sequence")
    _post_bufs(ops, g, B, K, calls[0][0], calls[0][1])
    gf = ops.geom(g, K)
    files = []
    for i, (loc, conf, _) in enumerate(calls):
        if i:
            ops.load("conf", conf, "call%d" % i)
            ops.load("loc", loc, "call%d" % i)
        ops.op("decode", "conf", B, "cand", "count")
        ops.op("nms", "cand", "loc", "count", B, "dead", "out", "nout", "kept")
        files.append(_post_dumps(ops, ".call%d" % i))
    ops.end()

    def check():
        fails = []
        _guards(ops, fails)
        fails += check_geom(ops, gf, g, K)
        for i, (_, _, refs) in enumerate(calls):
            _cmp_post("post_sequence call %d" % (i + 1), ops, files[i], B, K, refs[K], i == 0, fails)
        return fails

    return check


# ------------------------------------------------------------------------------------------------ nms alone on an injected list
TIE_K = 16
TIE_RANKS = {256: ((3, 70), (20, 130), (63, 64), (40, 150)), 700: ((5, 261), (100, 400), (17, 529), (250, 450))}
TIE_SCORES = (0.99, 0.98, 0.97, 0.96)


@functools.lru_cache(maxsize=None)
def tie_case(n):
    """(loc [A][4], anchors ascending [n], scores [n], the three orders {name: permutation of range(n)}, reference of the frame).  Four groups
    of two equal scores, the highest of the list; a group's members are TIE_RANKS[n] in the ascending list: different 64-lane groups (n = 256:
    position // 64) resp. different 256-strides (n = 700: position // 256).  Asserted here: that holds in all three orders, and the reference
    keeps the eight members first, the lower anchor of each group in front of the higher - so no member is suppressed before it is picked."""
    g = MNET
    unit = 64 if n <= 256 else 256
    for seed in range(64):
        rng = _rng("ties", n, seed)
        anch = np.sort(rng.permutation(g.A)[:n]).astype(np.int32)
        loc = np.clip(rng.normal(0, 0.5, (g.A, 4)), -2, 2).astype(f32)
        score = (0.61 + 0.3 * (rng.permutation(n) + 0.5) / n).astype(f32)
        members = []
        for (lo, hi), s in zip(TIE_RANKS[n], TIE_SCORES):
            score[[lo, hi]] = f32(s)
            loc[anch[[lo, hi]]] = 0
            members += [int(anch[lo]), int(anch[hi])]
        orders = {"asc": np.arange(n), "desc": np.arange(n)[::-1].copy(), "shuffle": rng.permutation(n)}
        conf = np.zeros((g.A, 2), f32)
        conf[anch, 1] = score
        spread = all(np.nonzero(o == lo)[0][0] // unit != np.nonzero(o == hi)[0][0] // unit for o in orders.values() for lo, hi in TIE_RANKS[n])
        ref = ref_frame(g, loc, conf, TIE_K) if spread else None
        if spread and ref[1][:8].tolist() == members:
            assert len(ref[2]) == n and len(np.unique(score)) == n - 4
            return loc, anch, score, orders, ref
    raise AssertionError("no seed places the ties of n = %d as required" % n)


def group_nms_orders(ops):
    g, K = MNET, TIE_K
    plan = []
    for n in (256, 700):
        loc, anch, score, orders, ref = tie_case(n)
        for oname, o in orders.items():
            ops.case("nms_n%d_%s" % (n, oname))
            cand = np.zeros(n, CAND_DTYPE)
            cand["anchor"], cand["score"] = anch[o], score[o]
            count = np.full(CC_STRIDE, FILL32, np.uint32)
            count[0] = n
            ops.rbuf("loc", loc)
            ops.buf("cand", g.A * 24, cand)
            ops.buf("count", count.nbytes, count)
            ops.buf("dead", g.A)
            ops.buf("out", K * 20)
            ops.buf("nout", 4)
            ops.buf("kept", K * 4)
            gf = ops.geom(g, K)
            ops.op("nms", "cand", "loc", "count", 1, "dead", "out", "nout", "kept")
            plan.append((ops.cid, n, ref, gf, _post_dumps(ops)))
            ops.end()

    def check():
        fails = []
        _guards(ops, fails)
        first = {}
        for cid, n, ref, gf, files in plan:
            fails += check_geom(ops, gf, g, K)
            count = ops.read(files["count"], np.uint32)
            if count is None:
                fails.append("%s: outputs were not written" % cid)
                continue
            if count[0] != 0 or (count[1:] != FILL32).any():
                fails.append("%s: counter words afterwards %r" % (cid, count[:4]))
            _cmp_post(cid, ops, files, 1, K, [ref], True, fails, check_count=False)
            got = b"".join(ops.read(files[k], np.uint8).tobytes() for k in ("out", "nout", "kept"))
            if first.setdefault(n, got) != got:
                fails.append("%s: the bytes differ from the ascending order's" % cid)
        return fails

    return check


# ------------------------------------------------------------------------------------------------ landmark decode
LDM_K = 12


def anchors64(g):
    """[A][4] (acx, acy, asx, asy) in float64, not narrowed; order level, row, column, size (slim_ref.anchors' enumeration)"""
    out = []
    for (fh, fw), step, ms in zip(slim_ref.feature_maps(g.in_w, g.in_h, g.table), g.table["steps"], g.table["min_sizes"]):
        i, j, l = np.meshgrid(np.arange(fh), np.arange(fw), np.arange(len(ms)), indexing="ij")
        msz = np.array(ms, np.float64)[l]
        out.append(np.stack([(j + 0.5) * float(step) / g.in_w, (i + 0.5) * float(step) / g.in_h, msz / g.in_w, msz / g.in_h], -1).reshape(-1, 4))
    return np.concatenate(out)


def anchor_level_size(g):
    """[A][2]: level and size index of every anchor"""
    out = []
    for k, ((fh, fw), ms) in enumerate(zip(slim_ref.feature_maps(g.in_w, g.in_h, g.table), g.table["min_sizes"])):
        out.append(np.stack([np.full(fh * fw * len(ms), k), np.tile(np.arange(len(ms)), fh * fw)], -1))
    return np.concatenate(out)


def landmark_reference(g, ldm, idx):
    """ldm [A][10] float32, idx [n] anchors -> (values [n][10] float64 (x0, y0, ...), bounds [n][10]); derivation: the module docstring"""
    anc = anchors64(g)[idx]
    p = ldm[idx].astype(np.float64).reshape(-1, 5, 2)
    val = np.empty_like(p)
    err = np.empty_like(p)
    sw, sh = g.in_w / g.frame_w, g.in_h / g.frame_h
    assert (sh > sw) == g.branch_h
    for c, (dim, frame) in enumerate(((g.in_w, g.frame_w), (g.in_h, g.frame_h))):
        ac, asz = anc[:, None, c], anc[:, None, 2 + c]
        T = np.abs(p[..., c] * 0.1 * asz)
        X = (ac + p[..., c] * 0.1 * asz) * dim
        EX = U * (dim * (ac + 4 * T) + 2 * np.abs(X))
        scale = sw if g.branch_h else sh
        if (c == 1) == g.branch_h:  # the padded axis: y when the frame was fitted by its width, x otherwise
            P = scale * frame
            pad = (dim - P) / 2
            Epad = (2 * U * P + U * abs(dim - P)) / 2
            val[..., c] = (X - pad) / scale
            err[..., c] = (EX + Epad + U * np.abs(X - pad)) / scale + 2 * U * np.abs(val[..., c])
        else:
            val[..., c] = X / scale
            err[..., c] = EX / scale + 2 * U * np.abs(val[..., c])
    return val.reshape(-1, 10), (WIDE * err).reshape(-1, 10)


def landmark_inputs(g):
    """(ldm [3][A][10] ~ N(0, 3), kept [3][K] with the fill pattern in the unused slots, n_out): frame 0 holds every (level, size) pair, the
    first and the last anchor (asserted)"""
    rng = _rng("ldm", g.name)
    A, K = g.A, LDM_K
    ldm = rng.normal(0, 3, (3, A, 10)).astype(f32)
    ls = anchor_level_size(g)
    pairs = sorted(set(map(tuple, ls.tolist())))
    k0 = [int(rng.choice(np.nonzero((ls == p).all(1))[0])) for p in pairs]
    k0 = ([0, A - 1] + k0 + rng.permutation(A)[:K].tolist())[:K]
    assert len(pairs) + 2 <= K and set(map(tuple, ls[k0].tolist())) == set(pairs)
    kept = np.full((3, K), FILL32, np.uint32)
    kept[0] = k0
    kept[2, :2] = rng.permutation(A)[:2]
    return ldm, kept, np.array([K, 0, 2], np.int32)


def group_landmarks(ops):
    plan = []
    for g in (MNET, SLIM, SLIMW):
        ops.case("ldm_" + g.name)
        ldm, kept, nout = landmark_inputs(g)
        ops.rbuf("ldm", ldm)
        ops.rbuf("kept", kept)
        ops.rbuf("nout", nout)
        ops.buf("out", 3 * LDM_K * 40)
        gf = ops.geom(g, LDM_K)
        ops.op("landmarks", "ldm", "kept", "nout", 3, "out")
        plan.append((ops.cid, g, ldm, kept, nout, gf, ops.dump("out")))
        ops.end()

    def check():
        fails = []
        _guards(ops, fails)
        for cid, g, ldm, kept, nout, gf, fo in plan:
            fails += check_geom(ops, gf, g, LDM_K)
            out = ops.read(fo, f32)
            if out is None:
                fails.append("%s: out was not written" % cid)
                continue
            out = out.reshape(3, LDM_K, 10)
            worst = 0.0
            for f in range(3):
                n = int(nout[f])
                if out[f, n:].view(np.uint32).any():
                    fails.append("%s frame %d: a slot >= n_out is not exactly 0" % (cid, f))
                if n:
                    val, bound = landmark_reference(g, ldm[f], kept[f, :n].astype(np.int64))
                    ratio = np.abs(out[f, :n].astype(np.float64) - val) / bound
                    worst = max(worst, float(ratio.max()))
                    if not (ratio <= 1).all():
                        i = np.unravel_index(int(np.argmax(~(ratio <= 1))), ratio.shape)
                        fails.append("%s frame %d slot %d value %d: %r, reference %r, bound %.3g" % (cid, f, i[0], i[1], out[f, i[0], i[1]], val[i], bound[i]))
            print("%s: landmark max(err / bound) = %.4f" % (cid, worst))
        return fails

    return check


# ------------------------------------------------------------------------------------------------ frames of the two cutters
FH, FW, NFR, MAXF = 96, 128, 3, 4
ROW_STRIDE = FW * 3 + 13
FRAME_STRIDE = 99 * ROW_STRIDE + 7
N_BOXES = np.array([4, 0, 2], np.int32)
LIVE = (0, 1, 2, 3, 8, 9)  # the face slots below n_boxes of their frame


@functools.lru_cache(maxsize=None)
def tight_frames(n=NFR, H=FH, W=FW):
    """n different u8 BGR frames: smooth waves plus a little noise (neighbouring pixels differ by a few levels, every pixel is distinct context)"""
    rng = _rng("frames", n, H, W)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    out = np.empty((n, H, W, 3), np.uint8)
    for f in range(n):
        for c in range(3):
            v = 128 + 70 * np.sin(xx / (7 + c) + f) * np.cos(yy / (9 - c) - f) + 30 * np.sin((xx + 2 * yy) / 23 + c) + rng.integers(-5, 6, (H, W))
            out[f, ..., c] = np.clip(v, 0, 255)
    out.setflags(write=False)
    return out


def padded_frames(frames, row_stride, frame_stride):
    """the frames at the given strides, the bytes between rows and frames random"""
    n, H, W, _ = frames.shape
    buf = _rng("padding", n, H, W).integers(0, 256, (n - 1) * frame_stride + H * row_stride, dtype=np.uint8)
    for f in range(n):
        for y in range(H):
            o = f * frame_stride + y * row_stride
            buf[o:o + W * 3] = frames[f, y].reshape(-1)
    return buf


def normalised(crops):
    """u8 BGR [F][h][w][3] -> float32 planar RGB [F][3][h][w]: (x - 127.5) * 0.0078125, exact in float32"""
    return np.ascontiguousarray(((crops[..., ::-1].astype(f32) - f32(127.5)) * f32(0.0078125)).transpose(0, 3, 1, 2))


def _cmp_cut(cid, ops, files, valid_want, fails, crops_given=True):
    """valid and chw of a cutter's run against the device's own crops; returns (crops or None, chw)"""
    chw, valid = ops.read(files["chw"], f32), ops.read(files["valid"], np.int32)
    crops = ops.read(files["crops"], np.uint8) if crops_given else None
    if chw is None or valid is None or (crops_given and crops is None):
        fails.append("%s: outputs were not written" % cid)
        return None, None
    F = len(valid_want)
    chw = chw.reshape(F, 3, 112, 112)
    if not np.array_equal(valid, valid_want):
        fails.append("%s: valid %r, expected %r" % (cid, valid, valid_want))
    if crops_given:
        crops = crops.reshape(F, 112, 112, 3)
        want = np.where(np.asarray(valid_want, bool)[:, None, None, None], normalised(crops), f32(0))
        fails += _bit_diff(cid + " chw against its own crops", chw, want)
        if crops[np.asarray(valid_want) == 0].any():
            fails.append("%s: the crop of a slot with valid 0 is not zero" % cid)
    return crops, chw


# ------------------------------------------------------------------------------------------------ crop alone
def box(x1, y1, x2, y2):
    return (x1, y1, x2, y2, 0.9)


GATED_BOXES = [box(3, 4, 60, 70), box(0, 0, 96, 128), box(10, 10, 40, 40), box(50, 60, 51, 61)]  # usable, every one
CROP_ROUNDS = {
    # x = row, y = column, far corner excluded.  Frame 0: slots 0-3, frame 1: gated, frame 2: slots 0-1 live, 2-3 gated.
    "a": [box(10, 20, 31, 45), box(7, 9, 7, 30), box(-1, 5, 40, 60), box(5, 5, 97, 60)] + GATED_BOXES + [box(0, 0, FH, FW), box(5, 7, 6, 8)] + GATED_BOXES[:2],
    "b": [box(0, 0, FH, FW), box(95, 127, 96, 128), box(20, 30, 20, 31), box(5, 5, 60, 129)] + GATED_BOXES + [box(40, 3, 57, 22), box(5, -1, 60, 60)] + GATED_BOXES[2:],
}


def crop_valid(boxes, n_boxes, maxf, H, W):
    """the rule of frt_kernels.h: slot below n_boxes of its frame, ROI non-empty and inside the frame"""
    out = np.zeros(len(boxes), np.int32)
    for f, b in enumerate(boxes):
        live = n_boxes is None or f % maxf < n_boxes[f // maxf]
        out[f] = int(live and b["x2"] > b["x1"] and b["y2"] > b["y1"] and b["x1"] >= 0 and b["y1"] >= 0 and b["x2"] <= H and b["y2"] <= W)
    return out


def crop_reference(frames, boxes, valid, shared):
    out = np.zeros((len(boxes), 112, 112, 3), np.uint8)
    for f in np.nonzero(valid)[0]:
        out[f] = oracle().crop_faces(frames[0 if shared else f // MAXF], boxes[f:f + 1])[0]
    return out


def group_crop(ops):
    frames = tight_frames()
    fbuf = padded_frames(frames, ROW_STRIDE, FRAME_STRIDE)
    plan = []
    F = NFR * MAXF

    for rname, bl in CROP_ROUNDS.items():
        boxes = np.array(bl, BBOX_DTYPE)
        for variant in ("batched", "nocrops", "shared"):
            ops.case("crop_%s_%s" % (rname, variant))
            ops.rbuf("frames", fbuf)
            ops.rbuf("boxes", boxes)
            ops.rbuf("nboxes", N_BOXES)
            shared = variant == "shared"
            crops = variant != "nocrops"
            if crops:
                ops.buf("crops", F * 112 * 112 * 3)
            ops.buf("chw", F * 112 * 112 * 12)
            ops.buf("valid", F * 4)
            ops.op("crop", "frames", NFR, FH, FW, ROW_STRIDE, FRAME_STRIDE, "boxes", "nboxes", MAXF, F, int(shared), 112, 112, "crops" if crops else "-", "chw", "valid")
            files = {"crops": ops.dump("crops") if crops else None, "chw": ops.dump("chw"), "valid": ops.dump("valid")}
            valid = crop_valid(boxes, N_BOXES, MAXF, FH, FW)
            plan.append((ops.cid, rname, variant, files, valid, crop_reference(frames, boxes, valid, shared) if crops else None))
            ops.end()
    # the copy-size ROI: a 160 x 160 frame, one slot, no gating
    big = tight_frames(1, 160, 160)
    ops.case("crop_copy")
    ops.rbuf("frames", big.reshape(-1))
    cbox = np.array([box(23, 31, 135, 143)], BBOX_DTYPE)
    ops.rbuf("boxes", cbox)
    ops.buf("crops", 112 * 112 * 3)
    ops.buf("chw", 112 * 112 * 12)
    ops.buf("valid", 4)
    ops.op("crop", "frames", 1, 160, 160, 480, 160 * 480, "boxes", "-", 1, 1, 0, 112, 112, "crops", "chw", "valid")
    files = {"crops": ops.dump("crops"), "chw": ops.dump("chw"), "valid": ops.dump("valid")}
    copy_want = oracle().crop_faces(big[0], cbox)
    assert np.array_equal(copy_want[0], big[0, 23:135, 31:143])
    plan.append((ops.cid, "copy", "batched", files, np.ones(1, np.int32), copy_want))
    ops.end()

    def check():
        fails = []
        _guards(ops, fails)
        chw_of = {}
        for cid, rname, variant, files, valid, want in plan:
            crops, chw = _cmp_cut(cid, ops, files, valid, fails, crops_given=want is not None)
            if chw is None:
                continue
            if want is not None:
                fails += _bit_diff(cid + " crops", crops, want)
            if variant == "batched":
                chw_of[rname] = chw
            elif variant == "nocrops":
                fails += _bit_diff(cid + " chw against the run with crops", chw, chw_of[rname])
        return fails

    return check


def crop_conditions():
    """what the crop cases must contain (tests/test_det_tail_ref.py)"""
    kinds = set()
    for bl in CROP_ROUNDS.values():
        boxes = np.array(bl, BBOX_DTYPE)
        valid = crop_valid(boxes, N_BOXES, MAXF, FH, FW)
        assert crop_valid(boxes, None, MAXF, FH, FW)[[4, 5, 6, 7, 10, 11]].all(), "a gated slot holds a box that would not be valid"
        assert not valid[[4, 5, 6, 7, 10, 11]].any()
        for f in LIVE:
            b = boxes[f]
            rh, rw = b["x2"] - b["x1"], b["y2"] - b["y1"]
            if valid[f]:
                kinds.add("whole" if (rh, rw) == (FH, FW) else "1x1" if (rh, rw) == (1, 1) else "up" if rh < 112 and rw < 112 else "other")
                kinds.add("frame%d" % (f // MAXF))
            else:
                kinds.add("empty" if rh <= 0 or rw <= 0 else "negative" if min(b["x1"], b["y1"]) < 0 else "far")
    return kinds


# ------------------------------------------------------------------------------------------------ alignment
def template64():
    from oracle import align
    return align.ARC_TEMPLATE.astype(np.float64).reshape(5, 2)


def align_reference(frame, lm):
    """frame u8 [H][W][3], lm float32 [5][2] -> (ok, value64 [112][112][3], bound [112][112][3], M [2][3]); derivation: the module docstring"""
    H, W = frame.shape[:2]
    lm32 = np.asarray(lm, f32).reshape(5, 2)
    zero = np.zeros((112, 112, 3))
    if not np.isfinite(lm32).all():
        return False, zero, zero, None
    s, d = lm32.astype(np.float64), template64()
    ms, md = s.mean(0), d.mean(0)
    sc, dc = s - ms, d - md
    sa = float((sc * dc).sum())
    sb = float((sc[:, 0] * dc[:, 1] - sc[:, 1] * dc[:, 0]).sum())
    den = float((sc ** 2).sum())
    mag = sa * sa + sb * sb
    assert not (1e-8 < den < 1e-4) and not (1e-14 < mag < 1e-10), "a case too close to the kernel's constants"
    if not (den > 1e-6 and mag > 1e-12):
        return False, zero, zero, None
    a, b = sa / den, sb / den
    t = md - np.array([a * ms[0] - b * ms[1], b * ms[0] + a * ms[1]])
    n2 = a * a + b * b
    ia, ib = a / n2, b / n2
    oy, ox = np.mgrid[0:112, 0:112].astype(np.float64)
    ux, uy = ox - t[0], oy - t[1]
    sx, sy = ia * ux + ib * uy, -ib * ux + ia * uy
    # forward error of the float32 chain
    E_ms = 0.8 * U * np.abs(s).sum(0) + 2 * U * np.abs(ms)
    E_md = 0.8 * U * np.abs(d).sum(0) + 2 * U * np.abs(md)
    E_s, E_d = E_ms + U * np.abs(sc), E_md + U * np.abs(dc)  # [5][2]
    asc, adc = np.abs(sc), np.abs(dc)
    E_sa = (E_s * adc + E_d * asc + E_s * E_d).sum() + 7 * U * (asc * adc).sum()
    E_sb = (E_s * adc[:, ::-1] + E_d[:, ::-1] * asc + E_s * E_d[:, ::-1]).sum() + 7 * U * (asc * adc[:, ::-1]).sum()
    E_den = (2 * E_s * asc + E_s ** 2).sum() + 7 * U * den
    assert E_den < 0.1 * den
    E_a = (E_sa + abs(a) * E_den) / (den - E_den) + U * abs(a)
    E_b = (E_sb + abs(b) * E_den) / (den - E_den) + U * abs(b)
    big = abs(a * ms[0]) + abs(b * ms[1]), abs(b * ms[0]) + abs(a * ms[1])
    E_t = [E_md[0] + E_a * abs(ms[0]) + abs(a) * E_ms[0] + E_b * abs(ms[1]) + abs(b) * E_ms[1] + E_a * E_ms[0] + E_b * E_ms[1] + 2 * U * big[0] + U * abs(t[0]),
           E_md[1] + E_b * abs(ms[0]) + abs(b) * E_ms[0] + E_a * abs(ms[1]) + abs(a) * E_ms[1] + E_b * E_ms[0] + E_a * E_ms[1] + 2 * U * big[1] + U * abs(t[1])]
    E_n2 = 2 * abs(a) * E_a + 2 * abs(b) * E_b + E_a ** 2 + E_b ** 2 + 2 * U * n2
    assert E_n2 < 0.1 * n2
    E_ia = (E_a + abs(ia) * E_n2) / (n2 - E_n2) + U * abs(ia)
    E_ib = (E_b + abs(ib) * E_n2) / (n2 - E_n2) + U * abs(ib)
    E_ux, E_uy = E_t[0] + U * np.abs(ux), E_t[1] + U * np.abs(uy)
    E_sx = WIDE * (E_ia * np.abs(ux) + abs(ia) * E_ux + E_ib * np.abs(uy) + abs(ib) * E_uy + E_ia * E_ux + E_ib * E_uy + 2 * U * (np.abs(ia * ux) + np.abs(ib * uy)))
    E_sy = WIDE * (E_ib * np.abs(ux) + abs(ib) * E_ux + E_ia * np.abs(uy) + abs(ia) * E_uy + E_ib * E_ux + E_ia * E_uy + 2 * U * (np.abs(ib * ux) + np.abs(ia * uy)))
    img = frame.astype(np.float64)

    def tap(yy, xx):
        inside = (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)
        return np.where(inside[..., None], img[np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)], 0.0)

    def cell(v):  # floor as an index; far outside every tap is zero, so the clip changes nothing
        return np.clip(np.floor(v), -4, max(H, W) + 4).astype(np.int64)

    x0, y0 = cell(sx), cell(sy)
    wx = np.where((x0 > -4) & (x0 < max(H, W) + 4), sx - x0, 0.0)[..., None]
    wy = np.where((y0 > -4) & (y0 < max(H, W) + 4), sy - y0, 0.0)[..., None]
    top = tap(y0, x0) + wx * (tap(y0, x0 + 1) - tap(y0, x0))
    bot = tap(y0 + 1, x0) + wx * (tap(y0 + 1, x0 + 1) - tap(y0 + 1, x0))
    value = top + wy * (bot - top)
    Lx, Ly = np.zeros_like(value), np.zeros_like(value)
    for cy in (cell(sy - E_sy), cell(sy + E_sy)):
        for cx in (cell(sx - E_sx), cell(sx + E_sx)):
            t00, t01, t10, t11 = tap(cy, cx), tap(cy, cx + 1), tap(cy + 1, cx), tap(cy + 1, cx + 1)
            Lx = np.maximum(Lx, np.maximum(np.abs(t01 - t00), np.abs(t11 - t10)))
            Ly = np.maximum(Ly, np.maximum(np.abs(t10 - t00), np.abs(t11 - t01)))
    Lx = np.where((E_sx >= 1)[..., None], 255.0, Lx)
    Ly = np.where((E_sy >= 1)[..., None], 255.0, Ly)
    bound = E_sx[..., None] * Lx + E_sy[..., None] * Ly + E_INTERP
    return True, value, bound, np.array([[a, -b, t[0]], [b, a, t[1]]])


AlignFace = collections.namedtuple("AlignFace", "name lm kind")  # kind: "bound", "zeros" (valid 1, all zero), "copy" (dx, dy), "invalid"


@functools.lru_cache(maxsize=None)
def align_faces_list():
    """the faces of the alignment cases, in the order they fill the live slots (six per launch)"""
    rng = _rng("align faces")
    tc = template64() - template64().mean(0)

    def pose(name, rot, scale, cx, cy, kind="bound", mirror=False, noise=1.0):
        p = tc * [-1, 1] if mirror else tc
        R = np.array([[np.cos(rot), -np.sin(rot)], [np.sin(rot), np.cos(rot)]])
        return AlignFace(name, (scale * p @ R.T + [cx, cy] + noise * rng.normal(0, 1, (5, 2))).astype(f32), kind)

    faces = [pose("rot%.2f_s%g" % (r, s), r, s, 64, 48) for r in (0.0, np.pi / 2, np.pi, -0.9) for s in (0.25, 1, 3)]
    faces += [pose("edge_left", 0.2, 0.5, 0, 48), pose("edge_right", -0.3, 0.5, 128, 48), pose("edge_top", 0.1, 0.5, 64, 0), pose("edge_bottom", 2.0, 0.5, 64, 96),
              pose("outside", 0.3, 0.5, -300, -300, kind="zeros"), pose("mirror", 0.4, 0.6, 60, 50, mirror=True)]
    faces.append(AlignFace("copy", (template64() + [9, -5]).astype(f32), "copy"))
    same = np.tile(np.array([[40.25, 33.5]], f32), (5, 1))
    nan, inf = same + rng.normal(0, 9, (5, 2)).astype(f32), same + rng.normal(0, 9, (5, 2)).astype(f32)
    nan[2, 1], inf[3, 0] = np.nan, np.inf
    faces += [AlignFace("identical_den0", same, "invalid"), AlignFace("nan", nan, "invalid"), AlignFace("inf", inf, "invalid")]
    # den ~ 1e-3, the valid side of den > 1e-6 (its other side is den = 0 above): the template shrunk to a spot 0.02 px across
    tiny = (np.array([40.0, 33.0]) + tc * np.sqrt(1e-3 / (tc ** 2).sum())).astype(f32)
    faces.append(AlignFace("den1e-3", tiny, "bound"))
    faces.append(pose("plain", 0.0, 1.0, 60, 45, noise=0.0))
    assert len(faces) % len(LIVE) == 0
    return tuple(faces)


def align_rounds():
    faces = align_faces_list()
    return [faces[i:i + len(LIVE)] for i in range(0, len(faces), len(LIVE))]


def align_slots(rnd):
    """landmarks [12][10] of one launch: the round's faces in the live slots, usable landmarks (a shifted template) in the gated ones"""
    lm = np.tile((template64() + [8, -10]).astype(f32).reshape(1, 10), (NFR * MAXF, 1))
    for slot, face in zip(LIVE, rnd):
        lm[slot] = face.lm.reshape(10)
    return lm


def check_aligned(name, face, frame, crop, valid, fails):
    """one face of the device (or of the mirror oracle) against the float64 reference; returns max((err - 0.5) / bound) or None"""
    ok, value, bound, _ = align_reference(frame, face.lm)
    if bool(valid) != ok or (face.kind == "invalid") == ok:
        fails.append("%s: valid %d, reference %d" % (name, valid, ok))
        return None
    if not ok:
        if crop.any():
            fails.append("%s: the crop of an invalid face is not zero" % name)
        return None
    err = np.abs(crop.astype(np.float64) - value)
    ratio = (err - 0.5) / bound
    if not (ratio <= 1).all():
        i = np.unravel_index(int(np.argmax(~(ratio <= 1))), ratio.shape)
        fails.append("%s: %d values outside 0.5 + bound, first at %r: %d, reference %.6f, bound %.3g" % (name, (~(ratio <= 1)).sum(), i, crop[i], value[i], bound[i]))
    if face.kind == "zeros" and (crop.any() or value.any()):
        fails.append("%s: a source quad wholly outside the frame gave non-zero pixels" % name)
    if face.kind == "copy":
        H, W = frame.shape[:2]
        want = np.zeros((112, 112, 3), np.uint8)  # crop[oy][ox] = frame[oy - 5][ox + 9] where that lies in the frame
        rows, cols = min(112, H + 5), min(112, W - 9)
        want[5:rows, :cols] = frame[:rows - 5, 9:9 + cols]
        if not np.array_equal(crop, want):
            fails.append("%s: the integer-shifted template is not a plain copy (%d bytes differ)" % (name, (crop != want).sum()))
    return float(ratio.max())


def group_align(ops):
    frames = tight_frames()
    fbuf = padded_frames(frames, ROW_STRIDE, FRAME_STRIDE)
    F = NFR * MAXF
    plan = []
    for r, rnd in enumerate(align_rounds()):
        for variant in (("batched", "nocrops") if r == 0 else ("batched",)):
            ops.case("align_r%d_%s" % (r, variant))
            ops.rbuf("frames", fbuf)
            ops.rbuf("lm", align_slots(rnd))
            ops.rbuf("nboxes", N_BOXES)
            crops = variant == "batched"
            if crops:
                ops.buf("crops", F * 112 * 112 * 3)
            ops.buf("chw", F * 112 * 112 * 12)
            ops.buf("valid", F * 4)
            ops.op("align", "frames", NFR, FH, FW, ROW_STRIDE, FRAME_STRIDE, "lm", "nboxes", MAXF, F, 0, "crops" if crops else "-", "chw", "valid")
            files = {"crops": ops.dump("crops") if crops else None, "chw": ops.dump("chw"), "valid": ops.dump("valid")}
            plan.append((ops.cid, r, rnd, variant, files))
            ops.end()

    def check():
        fails = []
        _guards(ops, fails)
        chw0 = None
        worst = 0.0
        for cid, r, rnd, variant, files in plan:
            want_valid = np.zeros(F, np.int32)
            for slot, face in zip(LIVE, rnd):
                want_valid[slot] = int(align_reference(frames[slot // MAXF], face.lm)[0])
            crops, chw = _cmp_cut(cid, ops, files, want_valid, fails, crops_given=variant == "batched")
            if chw is None:
                continue
            if variant == "nocrops":
                fails += _bit_diff(cid + " chw against the run with crops", chw, chw0)
                continue
            if r == 0:
                chw0 = chw
            valid = ops.read(files["valid"], np.int32)
            for slot, face in zip(LIVE, rnd):
                ratio = check_aligned("%s slot %d (%s)" % (cid, slot, face.name), face, frames[slot // MAXF], crops[slot], valid[slot], fails)
                if ratio is not None:
                    print("%s %s: alignment max((err - 0.5) / bound) = %.4f" % (cid, face.name, ratio))
                    worst = max(worst, ratio)
        print("alignment: largest max((err - 0.5) / bound) = %.4f" % worst)
        return fails

    return check


# ------------------------------------------------------------------------------------------------ pack_results
def pack_reference(boxes, n_boxes, valid, idx, sim, maxf):
    """the rule of pack_results_kernel's comment: an unused slot (at or past n_boxes of its frame) is all zeros but for the frame, match -1"""
    out = np.zeros(len(boxes), RESULT_DTYPE)
    for f in range(len(boxes)):
        frame = f // maxf
        used = f % maxf < n_boxes[frame]
        ok = bool(used and valid[f] != 0)
        if used:
            for k in BBOX_DTYPE.names:
                out[f][k] = boxes[f][k]
        out[f]["frame"] = frame
        out[f]["valid"] = int(ok)
        out[f]["match_idx"] = idx[f] if ok and idx is not None else -1
        out[f]["match_sim"] = sim[f] if ok and sim is not None else 0.0
    return out


def group_pack(ops):
    rng = _rng("pack")
    F = 12
    boxes = np.zeros(F, BBOX_DTYPE)
    for k in ("x1", "y1", "x2", "y2"):
        boxes[k] = rng.integers(1, 500, F)
    boxes["score"] = rng.uniform(0.6, 1, F).astype(f32)
    valid = np.array([1, 0, 7, -3, 1, 1, 0, 1, 0, 1, 1, 1], np.int32)  # 0 inside the used range (slots 1, 8), any non-zero counts as valid
    idx = rng.integers(0, 10 ** 6, F).astype(np.int32)
    sim = rng.uniform(-1, 1, F).astype(f32)
    plan = []
    for variant in ("matched", "null"):
        ops.case("pack_" + variant)
        for name, arr in (("boxes", boxes), ("nboxes", N_BOXES), ("valid", valid), ("idx", idx), ("sim", sim)):
            ops.rbuf(name, arr)
        ops.buf("out", F * 36)
        m = variant == "matched"
        ops.op("pack", "boxes", "nboxes", "valid", "idx" if m else "-", "sim" if m else "-", MAXF, F, "out")
        plan.append((ops.cid, ops.dump("out"), pack_reference(boxes, N_BOXES, valid, idx if m else None, sim if m else None, MAXF)))
        ops.end()

    def check():
        fails = []
        _guards(ops, fails)
        for cid, fo, want in plan:
            got = ops.read(fo, np.uint8)
            if got is None or got.tobytes() != want.tobytes():
                fails.append("%s: records differ from the rule: %r, expected %r" % (cid, None if got is None else got.view(RESULT_DTYPE), want))
        return fails

    return check


GROUPS = collections.OrderedDict([
    ("decode", group_decode), ("decode_nms_batched", group_batched), ("three_calls", group_sequence), ("nms_orders", group_nms_orders),
    ("slim_batched", group_slim), ("landmarks", group_landmarks), ("crop", group_crop), ("align", group_align), ("pack_results", group_pack),
])
