"""Cases, inputs, float64 references and derived bounds for the stages of the matcher's screened search run ONE AT A TIME
(tests/cpp/match_stage_check.cpp).  A generator and a reference, not a test: tests/test_match_stage_ref.py (no GPU) and
tests/test_gpu_match_stages.py use it.  Every group below writes a list of operations for the harness (class Ops) and returns a function that
reads what the harness wrote back and returns failure messages.

The two layouts are restated from the formulas csrc/frt_kernels.h documents (g16_index, and the int8 offset at ScreenScratch::g8), not read off
the kernels at run time: g16_index() / g8_offset() below are the formulas, to_g16() / to_g8() the same permutation as one transpose
(test_match_stage_ref.py checks one against the other by brute force).  The int8 formula was not found documented: the header comment was written
together with this module, from the layout comment in kernels_match.hip and the quantiser's own expression, so the restatement is not
independent of gallery_to_i8_kernel.  What ties it down is that TWO kernels must agree with it: the shadow cases compare the quantiser's bytes at
these offsets, and the class A coarse cases feed match_coarse_i8_kernel bytes placed by to_g8() here, never by the quantiser.

u = 2^-24 throughout.

Stage 1, shadow build.  int8 (D = 512): m = max|v|, inv = 127 / m, scale = m / 127, byte = rint(v * inv) + 128 are single fp32 operations, each
correctly rounded and with nothing to contract: numpy float32 gives the same bits, compared bit for bit (a non-finite row: bytes 128, scale 0;
pad rows 0x80, scale 0).  max_err2 / max_norm2 are fp32 sums the compiler may contract:
  * d_i = v_i - scale * q_i is computed with at most two roundings, |d^_i - d_i| <= u (|scale q_i| + |d^_i|), so | ||d^|| - ||d|| | <=
    slack = u (||v|| + 2 ||d||)  (|scale q_i| <= |v_i| + |d_i|);
  * no value of a 512-term sum of squares passes more than 1 (the square) + 8 (a lane's terms) + 6 (the shuffle tree) = 15 roundings, and the
    1.0001 factor is one more: the squared result is off by a relative SUM = 16 u at most (contraction only removes roundings).
  So  sqrt(max_err2) lies in [max_r (||d_r|| - slack_r) sqrt(1.0001 (1 - SUM)),  max_r (||d_r|| + slack_r) sqrt(1.0001 (1 + SUM))]  and max_norm2 in
  [max ||v||^2 (1 - SUM), max ||v||^2 (1 + SUM)].  The upper ends are the tightness checks.  Soundness - sqrt(max_err2) >= the float64 max over rows
  of ||row - scale q8|| - is asserted as the issue states it; shadow8_bounds() also asserts that the lower end of the interval is above that
  maximum, i.e. that for these rows soundness follows from the derivation (the 1.0001 factor outweighs slack and SUM).
fp16 shadow: every half at g16_index equals np.float16(v) bit for bit, pad rows zero, max_norm2 as above (row_norm_max_kernel: 4 terms per
loop trip, D / 256 trips, 6 shuffle levels: <= 15 roundings as well).

Stage 2, coarse scan, N = 128 * 515 - 51.  Class A (exact): queries are integers in [-2, 2].  int8: the harness is fed g8 bytes and scales written
here at the documented offsets; the accumulator is an integer of magnitude <= 2 * 127 * 512 < 2^24, exact in fp32 in any order, and the entry is
fp32(acc) * scale with ONE rounding (a multiplication in front of fmaxf: nothing to contract) - numpy float32 gives the same bits.  Scales: 128
distinct values (1 + odd / 512) * 2^e, e over 11 octaves, permuted per tile so that the largest scale of block b sits at row b % 32 of it; pad rows
of the last tile hold 127 * sign(query) with scale 1, i.e. the largest products of all, if they were counted.  fp16: rows are (the same integers)
* 2^-6, every partial sum a multiple of 2^-6 below 2^11: exact.  coarse_a_conditions() asserts on the reference that the winning row moves through
all 32 positions (both k halves of the accumulator layout) and that dropping any one of the 32 k-steps changes block maxima.
Class B (realistic): |tilemax - max over the block's live rows of float64 S| <= delta = ||q|| (c_round gmax_norm + 1.02 gerr), c_round = 0.7e-3
(int8) / 1.2e-3 (fp16), gmax_norm and gerr being what the DEVICE's shadow build produced, delta recomputed here in float64 from the fp32 constants.
(|max a - max b| <= max |a - b|.)  wgmax[w][q] = the maximum of workgroup w's entries, bit for bit.  Ratios seen on an MI355X (max err / delta):
RATIOS_SEEN below, printed, not asserted (the assertion is ratio <= 1):
    int8 shadow   D = 512  F = 33: 0.7070   F = 130: 0.7070   (gerr 0.0247037, gmax_norm 3; the maximum is query 9 against the rows built to align
                           their quantisation error with it - adversarial_rows(); the same gallery without them: 0.0596 / 0.1066)
    fp16 shadow   D = 64   F = 33: 0.0661   F = 130: 0.0795   (gmax_norm 1.24882)
                  D = 128  F = 33: 0.0640   F = 130: 0.0640   (gmax_norm 1.59887)
                  D = 256  F = 33: 0.0690   F = 130: 0.0690   (gmax_norm 2.19284)
                  D = 512  F = 33: 0.0723   F = 130: 0.0723   (gmax_norm 3)
    chained       int8 F = 33, k = 1 and 4: 0.7070 (349 / 4892 pairs listed, largest sub-list 13 / 102 of 128)
                  fp16 F = 33, k = 1 and 4: 0.0723 (349 / 486 pairs listed, largest sub-list 13 / 14 of 128)
    shadow build  sqrt(max_err2) = 0.0883064052 = 1.0000500 x the float64 error norm 0.0883019887 (up to 1.0000592 allowed), for the whole build and
                  for the row-range form; max_norm2 163.779831 in [163.779675, 163.779987]

Stage 3, k-th entry: the k-th largest entry with duplicates counted separately; NaN and -inf entries never count; fewer than k -> -inf.

Stage 4, pair selection.  thr = m - 2 delta (top-1 / top-k) or t - delta (absolute) is computed on the device in fp32 with a free summation
order of ||q||^2: a term passes 1 + D / 256 + 6 + 2 <= 11 roundings (5.5 u on the norm), the root 1, c_round gmax + 1.02 gerr 3, the product 1:
10.5 u; SLACK_REL = 16 u = 2^-20 relative on delta is used, plus u |thr| for the final subtraction.  select_reference() computes thr in float64 and
asserts that no entry of the inputs lies within  slack = k_delta delta SLACK_REL + u |thr|  of it; entries are planted 4 slack inside and outside.
Pairs are compared per sub-list as sets of (q, tile, 4-bit mask); the counters are compared exactly.

Stage 5, re-rank + unpack: similarities are sums of small-integer (or integer * 2^-6) products, exact in fp32 in any order, so index and
similarity bits are compared against float64 (stable descending order = first index on ties).  A similarity of -0.0 is not reachable: the
fma chain starts at +0.0, and (+0.0) + (-0.0) and x + (-x) are +0.0 under round-to-nearest, so a -0.0 key never meets a +0.0 key in qkey.  The
"zero similarities" case (query 4: every product is +0.0 or -0.0) therefore checks what can be checked - every similarity comes out as +0.0,
bit for bit, and the first listed index wins among them - not an ordering of the two zeros.

Stage 6, chained: every row with float64 S >= the float64 k-th best S lies in a listed (tile, block), the overflow flag clear.
"""
import functools
import os

import numpy as np

from launch_harness import Ops as _Ops, bit_diff as _bit_diff, fbits, rng as _rng

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24
SUM = 16 * U
SLACK_REL = 2.0 ** -20
F1_0001 = float(np.float32(1.0001))
F1_02 = float(np.float32(1.02))
C_ROUND = {True: float(np.float32(0.7e-3)), False: float(np.float32(1.2e-3))}  # keyed by "the int8 shadow was scanned"
N_SMALL = 128 * 3 + 77
N_BIG = 128 * 515 - 51
TILES = 515
COARSE_WG, SEL_SEG, SEL_SUB, TOPK_MAX = 256, 16, 64, 16
CTL_WORDS, CTL_OVERFLOW, CTL_SEG0, CTL_STRIDE = 32 + 64 * 32, 1, 32, 32
NINF = -np.inf

# max(err / delta) of class B and of the chained cases' coarse entries as printed by tests/test_gpu_match_stages.py on an MI355X
RATIOS_SEEN = {
    "i8_D512_B": {33: 0.7070, 130: 0.7070}, "f16_D64_B": {33: 0.0661, 130: 0.0795}, "f16_D128_B": {33: 0.0640, 130: 0.0640},
    "f16_D256_B": {33: 0.0690, 130: 0.0690}, "f16_D512_B": {33: 0.0723, 130: 0.0723}, "i8_D512_chain": {33: 0.7070}, "f16_D512_chain": {33: 0.0723},
    "shadow8 sqrt(max_err2) / float64 error norm": 1.0000500,
}


def tiles_of(n):
    return (n + 127) // 128


# ------------------------------------------------------------------------------------------------ layouts
def g16_index(g, k, D):
    return ((((g >> 7) * 4 + ((g >> 5) & 3)) * (D >> 4) + (k >> 4)) * 64 + ((k >> 3) & 1) * 32 + (g & 31)) * 8 + (k & 7)


def g8_offset(g, k, D=512):
    ks = k >> 4
    return ((((g >> 7) * 4 + ((g >> 5) & 3)) * (D >> 5) + (ks >> 1)) * 64 + ((k >> 3) & 1) * 32 + (g & 31)) * 16 + (ks & 1) * 8 + (k & 7)


def _padded(rows, pad, fill):
    n, D = rows.shape
    full = np.full((tiles_of(n) * 128, D), fill, rows.dtype)
    full[:n] = rows
    if pad is not None:
        full[n:] = pad
    return full


def to_g16(rows, pad=None):
    """rows [N][D] (fp16) -> the fragment-ordered gallery, flat; pad: the rows of the last tile behind N (None: zeros)."""
    full = _padded(rows, pad, 0)
    D = full.shape[1]
    return np.ascontiguousarray(full.reshape(-1, 4, 32, D // 16, 2, 8).transpose(0, 1, 3, 4, 2, 5)).reshape(-1)


def from_g16(flat, D):
    return np.ascontiguousarray(flat.reshape(-1, 4, D // 16, 2, 32, 8).transpose(0, 1, 4, 2, 3, 5)).reshape(-1, D)


def to_g8(rows, pad=None):
    """biased bytes [N][512] -> the int8 shadow, flat; pad None: 0x80."""
    full = _padded(rows, pad, 0x80)
    return np.ascontiguousarray(full.reshape(-1, 4, 32, 16, 2, 2, 8).transpose(0, 1, 3, 5, 2, 4, 6)).reshape(-1)


def from_g8(flat):
    return np.ascontiguousarray(flat.reshape(-1, 4, 16, 2, 32, 2, 8).transpose(0, 1, 4, 2, 5, 3, 6)).reshape(-1, 512)


# ------------------------------------------------------------------------------------------------ the harness's operation list
class Ops(_Ops):
    def scratch(self, F, tiles, pair_cap=8192, g8="-", scale="-", tilemax=None, wgmax=None, ctl=None, pairs=None, qkey=None):
        """the ScreenScratch buffers, exactly as large as the launches may write (every byte behind them is a guard)"""
        self.buf("tilemax", F * tiles * 16, tilemax)
        self.buf("wgmax", COARSE_WG * F * 4, wgmax)
        self.buf("pairs", pair_cap * 8, pairs)
        self.buf("ctl", CTL_WORDS * 4, ctl)
        self.buf("qkey", F * 8, qkey)
        self.op("scratch", "tilemax", "wgmax", "pairs", pair_cap, "ctl", "qkey", g8, scale)


# ------------------------------------------------------------------------------------------------ stage 1: shadow build
def shadow8_reference(rows):
    """(biased bytes [n][512] uint8, scale [n] fp32, q [n][512] fp32) of fp32 rows, in numpy float32: the arithmetic of the documented quantiser."""
    v = np.asarray(rows, np.float32)
    bad = ~np.isfinite(v).all(1)
    with np.errstate(all="ignore"):
        m = np.where(bad, np.float32(0), np.abs(np.where(bad[:, None], np.float32(0), v)).max(1)).astype(np.float32)
        pos = m > 0
        safe = np.where(pos, m, np.float32(1))
        inv = np.where(pos, np.float32(127) / safe, np.float32(0)).astype(np.float32)
        sc = np.where(pos, safe / np.float32(127), np.float32(0)).astype(np.float32)
        q = np.clip(np.rint(np.where(bad[:, None], np.float32(0), v) * inv[:, None]), -127, 127).astype(np.float32)
    assert inv.dtype == np.float32 and sc.dtype == np.float32 and q.dtype == np.float32
    return (q.astype(np.int32) + 128).astype(np.uint8), sc, q


def shadow8_bounds(rows):
    """dict: e_true (float64 max ||row - scale q8||), e_lo / e_hi (the interval of sqrt(max_err2)), n2_lo / n2_hi; finite rows only."""
    _, sc, q = shadow8_reference(rows)
    v = np.asarray(rows, np.float64)
    d = np.linalg.norm(v - sc.astype(np.float64)[:, None] * q, axis=1)
    vn = np.linalg.norm(v, axis=1)
    slack = U * (vn + 2 * d)
    out = dict(e_true=d.max(), e_lo=(np.maximum(d - slack, 0) * np.sqrt(F1_0001 * (1 - SUM))).max(), e_hi=((d + slack) * np.sqrt(F1_0001 * (1 + SUM))).max())
    out.update(norm_bounds(v))
    assert out["e_lo"] >= out["e_true"], "for these rows the 1.0001 factor does not cover the fp32 error of the measurement"
    return out


def norm_bounds(rows):
    n2 = (np.asarray(rows, np.float64) ** 2).sum(1)
    return dict(n2_lo=(n2 * (1 - SUM)).max(), n2_hi=(n2 * (1 + SUM)).max(), gmax_true=np.sqrt(n2.max()))


def unit_rows(r, n, D=512):
    g = r.standard_normal((n, D)).astype(np.float32)
    return g / np.linalg.norm(g, axis=1, keepdims=True).astype(np.float32)


def shadow_rows(n, what, nonfinite):
    """fp32 rows [n][512] with the quantiser's edge rows spread over blocks and tiles (the last, ragged tile included)"""
    r = _rng("shadow", what)
    g = unit_rows(r, n)
    at = lambda i: i % n
    g[at(5)] = 0
    g[at(5), 3] = 1.0                       # one-hot
    g[at(40)] = 0                           # all-zero: scale 0, bytes 128
    g[at(70)] *= np.float32(1e-6)
    g[at(101):at(101) + 3] *= np.float32(3.0)
    k = int(np.abs(g[at(130)]).argmax())
    g[at(130), (k + 1) % 512] = -1.5 * abs(g[at(130), k])   # the largest element negative
    g[at(200)] = ((np.arange(512) % 126) + 0.5) / 128.0 * np.where(np.arange(512) % 2, -1, 1)   # m = 127 / 128 below: v * inv = j + 0.5 exactly
    g[at(200), 7] = 127.0 / 128.0
    g[n - 1] = g[at(200)][::-1]
    g[n - 3] *= np.float32(3.0)
    if nonfinite:
        g[at(33), 9] = np.nan
        g[n - 2, 500] = np.inf
        g[at(64), 0] = -np.inf
    return g


def build_shadow(ops):
    N = N_SMALL
    rows_total = tiles_of(N) * 128
    checks = []

    def add8(cid, g):
        ops.case(cid)
        ops.rbuf("gal", g)
        ops.buf("g8", rows_total * 512)
        ops.buf("scale", rows_total * 4)
        ops.buf("bits", 8)
        ops.op("shadow8", "gal", N, "g8", "scale", "bits")
        files = (ops.dump("g8"), ops.dump("scale"), ops.dump("bits"))
        ops.end()
        checks.append(lambda f=files, g=g, cid=cid: check_shadow8(ops, cid, f, g, None))

    add8("i8_finite", shadow_rows(N, "a", False))
    add8("i8_nonfinite", shadow_rows(N, "b", True))

    # the row-range form on a buffer that already holds other rows: two ranges that start and end mid-tile
    base = shadow_rows(N, "c", False)
    ops.case("i8_rows")
    ops.rbuf("gal", base)
    ops.buf("g8", rows_total * 512)
    ops.buf("scale", rows_total * 4)
    ops.buf("bits", 8)
    ops.op("shadow8", "gal", N, "g8", "scale", "bits")
    merged, steps = base.copy(), []
    for j, (row0, n, nonfinite) in enumerate(((37, 150, False), (200, 229, True))):
        new = shadow_rows(n, "d%d" % j, nonfinite)
        ops.rbuf("rows%d" % j, new)
        ops.op("shadow8_rows", "rows%d" % j, row0, n, "g8", "scale", "bits")
        merged = merged.copy()
        merged[row0:row0 + n] = new
        steps.append(((ops.dump("g8", j), ops.dump("scale", j), ops.dump("bits", j)), merged, new))
    ops.end()
    for files, merged_j, new in steps:
        checks.append(lambda f=files, g=merged_j, new=new: check_shadow8(ops, "i8_rows", f, g, new))

    for D in (64, 512):
        cid = "f16_D%d" % D
        g = shadow_rows(N, "e", False)[:, :D].copy()
        g[11, 0], g[11, 1], g[11, 2] = 1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 3e-8   # ties to even, a value below half the smallest subnormal
        g[12] *= np.float32(1e-3)                                                # subnormal halves
        ops.case(cid)
        ops.rbuf("gal", g)
        ops.buf("g16", rows_total * D * 2)
        ops.buf("bits", 8, np.zeros(2, np.int32))
        ops.buf("bits2", 8, np.zeros(2, np.int32))
        ops.op("shadow16", "gal", N, D, "g16", "bits")
        ops.op("norm16", "g16", 37, 300, D, "bits2")
        files = (ops.dump("g16"), ops.dump("bits"), ops.dump("bits2"))
        ops.end()
        checks.append(lambda f=files, g=g, D=D, cid=cid: check_shadow16(ops, cid, f, g, D))

    def check():
        bad = _guards(ops)
        for c in checks:
            bad += c()
        return bad
    return check


def _guards(ops):
    res = ops.results()
    return ["%s: not reached" % c for c in ops.cases if c not in res] + ["%s: %d guard or input bytes changed" % (c, n) for c, n in res.items() if n]


def _maxima(bits, i):
    return float(np.sqrt(np.float64(bits.view(np.float32)[i])))


def check_shadow8(ops, cid, files, g, measured_rows):
    """g: the rows the shadow must now hold; measured_rows: the rows whose maxima the bits hold (None: all of g)"""
    g8, scale, bits = ops.read(files[0], np.uint8), ops.read(files[1], np.float32), ops.read(files[2], np.int32)
    if g8 is None or scale is None or bits is None:
        return ["%s: outputs missing" % cid]
    want_b, want_s, _ = shadow8_reference(g)
    pad = tiles_of(len(g)) * 128 - len(g)
    bad = _bit_diff(cid + " g8", g8, to_g8(want_b))
    bad += _bit_diff(cid + " scale", scale, np.concatenate([want_s, np.zeros(pad, np.float32)]))
    m = g if measured_rows is None else measured_rows
    finite = np.isfinite(m).all(1)
    if not finite.all():
        if not (np.isnan(bits.view(np.float32)).all()):
            bad.append("%s: a non-finite row must leave both maxima NaN, got %r" % (cid, bits.view(np.float32)))
        return bad
    b = shadow8_bounds(m)
    e, n2 = _maxima(bits, 0), float(bits.view(np.float32)[1])
    print("%s: sqrt(max_err2) = %.9g, float64 max error norm %.9g (ratio %.7f, allowed up to %.7f); max_norm2 %.9g in [%.9g, %.9g]" %
          (cid, e, b["e_true"], e / b["e_true"], b["e_hi"] / b["e_true"], n2, b["n2_lo"], b["n2_hi"]))
    if not e >= b["e_true"]:
        bad.append("%s: sqrt(max_err2) = %.9g is below the float64 error norm %.9g" % (cid, e, b["e_true"]))
    if not e <= b["e_hi"]:
        bad.append("%s: sqrt(max_err2) = %.9g is above the derived %.9g" % (cid, e, b["e_hi"]))
    if not b["n2_lo"] <= n2 <= b["n2_hi"]:
        bad.append("%s: max_norm2 = %.9g outside [%.9g, %.9g]" % (cid, n2, b["n2_lo"], b["n2_hi"]))
    return bad


def check_shadow16(ops, cid, files, g, D):
    g16, bits, bits2 = ops.read(files[0], np.uint16), ops.read(files[1], np.int32), ops.read(files[2], np.int32)
    if g16 is None or bits is None or bits2 is None:
        return ["%s: outputs missing" % cid]
    h = g.astype(np.float16)
    bad = _bit_diff(cid + " g16", g16, to_g16(h).view(np.uint16))
    for name, got, rows in (("max_norm2 of the build", bits, g), ("max_norm2 of launch_rows_norm<half_t>", bits2, h[37:337])):
        b, n2 = norm_bounds(rows), float(got.view(np.float32)[1])
        if not b["n2_lo"] <= n2 <= b["n2_hi"]:
            bad.append("%s: %s = %.9g outside [%.9g, %.9g]" % (cid, name, n2, b["n2_lo"], b["n2_hi"]))
    return bad


# ------------------------------------------------------------------------------------------------ stage 2: coarse scan
def tile_entries(vals, n_live):
    """vals [F][tiles * 128] -> [F][tiles][4]: the maximum over each 32-row block's live rows; NaN values are no candidates (fmaxf from -inf)"""
    v = np.where(np.isnan(vals), NINF, vals)
    v[:, n_live:] = NINF
    return v.reshape(v.shape[0], -1, 4, 32).max(3)


def wg_maxima(tilemax):
    """[F][tiles][4] -> wgmax [256][F]: workgroup w walks the tiles w, w + 256, ..."""
    F, T, _ = tilemax.shape
    p = np.full((F, -(-T // COARSE_WG) * COARSE_WG, 4), NINF, tilemax.dtype)
    p[:, :T] = tilemax
    return np.ascontiguousarray(p.reshape(F, -1, COARSE_WG, 4).max((1, 3)).T)


@functools.lru_cache(maxsize=None)
def coarse_a_base():
    """(G int8 [tiles * 128][512] pad rows included, Q fp32 [130][512], scales fp32 [tiles * 128])"""
    r = _rng("coarse_a")
    Q = r.integers(-2, 3, size=(130, 512)).astype(np.float32)
    G = np.empty((TILES * 128, 512), np.int8)
    G[:N_BIG] = r.integers(-127, 128, size=(N_BIG, 512), dtype=np.int8)
    n_pad = TILES * 128 - N_BIG
    G[N_BIG:] = (127 * np.sign(Q[np.arange(n_pad) % 130])).astype(np.int8)  # pad row i: the largest product query i can have
    j = np.arange(128)
    base = ((1 + (2 * j + 1) / 512.0) * 2.0 ** (-12 + (j * 11) // 127)).astype(np.float32)  # ascending, distinct, none a power of two
    scales = np.empty((TILES, 128), np.float32)
    for t in range(TILES):
        rest = list(r.permutation(124))
        row = np.empty(128, np.int64)
        taken = set()
        for w in range(4):  # the largest scale of block w at row (4 t + w) % 32 of it
            pos = w * 32 + (4 * t + w) % 32
            row[pos] = 124 + w
            taken.add(pos)
        row[[p for p in range(128) if p not in taken]] = rest
        scales[t] = base[row]
    scales = scales.reshape(-1)
    scales[N_BIG:] = 1.0
    return G, Q, scales


@functools.lru_cache(maxsize=None)
def coarse_a_reference(kind, D=512):
    """float32 values [130][tiles * 128] of every (query, row), pad rows included, exact: int8: fp32(acc) * scale; fp16: acc"""
    G, Q, scales = coarse_a_base()
    acc = Q[:, :D] @ G[:, :D].astype(np.float32).T   # integers below 2^24: exact in fp32 whatever the order
    assert np.abs(acc).max() < 2 ** 24 and np.array_equal(acc, np.rint(acc))
    if kind == "i8":
        return acc * scales[None, :]                 # one fp32 rounding
    assert np.abs(acc).max() < 2 ** 17               # multiples of 2^-6 below 2^11
    return acc * np.float32(2.0 ** -6)


def coarse_a_conditions(kind, D=512):
    """The premises of class A beyond exactness, asserted on the reference."""
    vals = coarse_a_reference(kind, D)
    G, Q, scales = coarse_a_base()
    live = np.where(np.arange(vals.shape[1]) < N_BIG, vals, NINF)
    pos = live.reshape(130, -1, 32).argmax(2)
    assert set(np.unique(pos)) == set(range(32)), "the winning row does not visit all 32 rows of a block"
    assert {0, 1} == set(np.unique((pos >> 2) & 1)), "both halves of the accumulator layout (rows 4 hi + ...)"
    n_pad = TILES * 128 - N_BIG
    qs = np.arange(min(n_pad, 130))
    assert (vals[qs, N_BIG + qs] > live[qs].max(1)).all(), "a counted pad row must win"
    if kind == "i8":
        s = scales.reshape(TILES, 128)
        assert all(len(np.unique(s[t])) == 128 for t in range(TILES - 1)) and (s[:-1].max(1) / s[:-1].min(1) >= 2 ** 10).all()
        m, _ = np.frexp(scales[:N_BIG])
        assert (m != 0.5).all()
    sc = scales[None, :256] if kind == "i8" else np.float32(2.0 ** -6)
    full = tile_entries((Q[:, :D] @ G[:256, :D].astype(np.float32).T) * sc, 256)
    for ks in range(D // 16):   # the maxima of the first two tiles change when any one k-step is left out
        keep = np.ones(D, bool)
        keep[ks * 16:ks * 16 + 16] = False
        part = tile_entries((Q[:, :D][:, keep] @ G[:256, :D][:, keep].astype(np.float32).T) * sc, 256)
        assert (part != full).mean() > 0.9, ks


def coarse_outputs(ops, cid, F, tag=""):
    return dict(cid=cid, F=F, tilemax=ops.dump("tilemax", tag), wgmax=ops.dump("wgmax", tag), ctl=ops.dump("ctl", tag), qkey=ops.dump("qkey", tag))


def read_coarse(ops, out):
    tm, wg, ctl, qkey = ops.read(out["tilemax"], np.float32), ops.read(out["wgmax"], np.float32), ops.read(out["ctl"], np.int32), ops.read(out["qkey"], np.uint64)
    if tm is None or wg is None or ctl is None or qkey is None:
        return None, ["%s F=%d: outputs missing" % (out["cid"], out["F"])]
    bad = []
    if "k" not in out and (ops.read(out["pairs"], np.uint8) != 0x5a).any():
        bad.append("%s F=%d: the coarse scan wrote into the pair list" % (out["cid"], out["F"]))
    if ctl.any() or qkey.any():
        bad.append("%s F=%d: ctl / qkey are not zero behind the scan (%d / %d words set)" % (out["cid"], out["F"], np.count_nonzero(ctl), np.count_nonzero(qkey)))
    return (tm.reshape(out["F"], TILES, 4), wg.reshape(COARSE_WG, out["F"])), bad


def build_coarse_a(ops, kind, D=512, nonfinite=False):
    """class A of one shadow type: int8 at F = 1, 33, 65, 130; fp16 (one D) at F = 33, 130.  nonfinite: F = 33 with a NaN query, an inf query
    and (fp16) a NaN gallery row - what the stages behind really receive from non-finite inputs."""
    G, Q, scales = coarse_a_base()
    cid = "%s_D%d_A%s" % (kind, D, "_nonfinite" if nonfinite else "")
    vals = coarse_a_reference(kind, D).copy()
    Qc = Q[:, :D].copy()
    ops.case(cid)
    if kind == "i8":
        ops.rbuf("g8", to_g8((G[:N_BIG].astype(np.int16) + 128).astype(np.uint8), (G[N_BIG:].astype(np.int16) + 128).astype(np.uint8)))
        ops.rbuf("scale", scales)
        shadow = ("g8", "scale")
    else:
        g16 = (G[:, :D].astype(np.float32) * np.float32(2.0 ** -6)).astype(np.float16)
        if nonfinite:
            g16[1000, 3] = np.nan
            vals[:, 1000] = np.nan
        ops.rbuf("g16", to_g16(g16[:N_BIG], g16[N_BIG:]))
        shadow = ("-", "-")
    if nonfinite:
        col = 17
        Qc[5, 40] = np.nan
        Qc[6, col] = np.inf
        vals[5] = np.nan
        gc = G[:, col].astype(np.float32)
        if kind == "f16":
            gc[1000] = np.nan
        vals[6] = np.where(gc > 0, np.inf, np.where(gc < 0, NINF, np.nan))   # inf * g + finite terms; inf * 0 = NaN
    outs = []
    for F in ((33,) if nonfinite else (1, 33, 65, 130) if kind == "i8" else (33, 130)):
        ops.buf("q%d" % F, F * D * 4, Qc[:F])
        _scratch_for(ops, F, shadow, "_%d" % F)
        ops.op("coarse", "-" if kind == "i8" else "g16", N_BIG, D, "q%d" % F, F)
        outs.append(_dump_scratch(ops, cid, F, "_%d" % F))
    ops.end()

    def check():
        bad = []
        want = tile_entries(vals.copy(), N_BIG)
        for out in outs:
            got, b = read_coarse(ops, out)
            bad += b
            if got is None:
                continue
            F = out["F"]
            bad += _bit_diff("%s F=%d tilemax" % (cid, F), got[0], want[:F])
            bad += _bit_diff("%s F=%d wgmax" % (cid, F), got[1], wg_maxima(want[:F]))
        return bad
    return check


def _scratch_for(ops, F, shadow, tag, pair_cap=8192):
    """a scratch set of its own per launch (names carry the tag): every buffer exactly the size the launch may write"""
    ops.buf("tilemax" + tag, F * TILES * 16)
    ops.buf("wgmax" + tag, COARSE_WG * F * 4)
    ops.buf("pairs" + tag, pair_cap * 8)
    ops.buf("ctl" + tag, CTL_WORDS * 4)
    ops.buf("qkey" + tag, F * 8)
    ops.op("scratch", "tilemax" + tag, "wgmax" + tag, "pairs" + tag, pair_cap, "ctl" + tag, "qkey" + tag, shadow[0], shadow[1])


def _dump_scratch(ops, cid, F, tag):
    return dict(cid=cid, F=F, tilemax=ops.dump("tilemax" + tag), wgmax=ops.dump("wgmax" + tag), ctl=ops.dump("ctl" + tag), qkey=ops.dump("qkey" + tag),
                pairs=ops.dump("pairs" + tag))


# ---- class B and the chained cases: one realistic gallery, near-ties included
NEAR_Q, NEAR_ROWS = 8, 40


@functools.lru_cache(maxsize=None)
def realistic():
    """(gallery fp32 [N_BIG][512], queries fp32 [130][512], the near-tie rows [8][40]).  Unit rows with the stress rows of
    test_int8_shadow_screening_is_exact_whatever_the_rows_look_like; for queries 0-7, 40 rows in 40 different tiles that are copies of the query
    perturbed far below one int8 step (float64 similarity within 1e-4 of the best).  Queries: 0-7 the near-tie directions, 8-15 gallery rows,
    16-30 noisy copies, 31 a 30x-scaled and 32 a 0.01x-scaled copy, then unrelated unit vectors with a few scaled 0.01x / 30x."""
    r = _rng("realistic")
    g = unit_rows(r, N_BIG)
    g[100] = 0
    g[100, 3] = 1.0
    g[200] *= np.float32(1e-6)
    g[300] = 0
    g[400:410] *= np.float32(3.0)
    g[5000] = g[64000]
    g[6000] = g[64001] * np.float32(1 + 1e-6)
    g[N_BIG - 1] = g[64002]
    q = unit_rows(r, 130)
    near = []
    for i in range(NEAR_Q):
        tiles = 4 + r.choice(TILES - 4, NEAR_ROWS, replace=False)   # (behind the stress rows)
        rows = np.minimum(tiles * 128 + r.integers(0, 128, NEAR_ROWS), N_BIG - 2)
        g[rows] = q[i] + r.uniform(-3e-5, 3e-5, (NEAR_ROWS, 512)).astype(np.float32)
        near.append(rows)
    src = r.integers(1000, 60000, 25)
    q[8:16] = g[src[:8]]
    q[16:31] = g[src[8:23]] + np.float32(0.05) * r.standard_normal((15, 512)).astype(np.float32) / np.float32(np.sqrt(512))
    q[31] = g[src[23]] * np.float32(30)
    q[32] = g[src[24]] * np.float32(0.01)
    q[40] *= np.float32(0.01)
    q[41] *= np.float32(30)
    q[42] = g[405] * np.float32(30)
    q[43] = g[200] / np.linalg.norm(g[200])
    g[ADV_A], g[list(ADV_B)], q[ADV_Q] = adversarial_rows(r)
    assert not set(np.array(near).ravel()) & ({ADV_A} | set(ADV_B))
    return g, q, np.array(near)


# Query ADV_Q and five rows whose quantisation error is ALIGNED with it - the case the 1.02 gerr term of the bound exists for (random rows never
# come near it: their err / delta is ~ 0.1).  s: a +-1 pattern over 510 columns; columns 0 and 1 are free (s = 0).  Row A = sc (40 s + 0.49 s),
# rows B = sc (40 s - 0.49 s), column 0 = 127 sc in both (it pins the scale: q8 = 40 s exactly, e_A = +0.49 sc s, e_B = -0.49 sc s), column 1 =
# 0 in A and 100 sc in B.  sc is chosen so that ||e|| is just below the largest error norm of the gallery (the 3x rows'), so gerr stays theirs.
# q = 0.8 s / sqrt(510) + 0.6 (a unit vector orthogonal to s), its column 1 set so that S(q, A) = S(q, B) + 3e-5: A is the query's best row and
# the four B rows tie 3e-5 below it, while the coarse values are S(A) - eps and S(B) + eps with eps = q.e ~ 0.8 ||e||: between delta computed with
# 0.5 gerr and the real delta.
ADV_Q, ADV_A, ADV_B = 9, 50 * 128 + 77, (150 * 128 + 5, 250 * 128 + 40, 350 * 128 + 70, 450 * 128 + 127)


def adversarial_rows(r):
    s = r.choice([-1.0, 1.0], 512)
    s[:2] = 0
    sc = 0.0245 / (0.49 * np.sqrt(510.0))
    w = r.standard_normal(512)
    w[:2] = 0
    w -= s * (w @ s) / 510.0
    q = 0.8 * s / np.sqrt(510.0) + 0.6 * w / np.linalg.norm(w)
    A = sc * (40.49 * s)
    B = sc * (39.51 * s)
    A[0] = B[0] = 127 * sc
    B[1] = 100 * sc
    A32, B32 = A.astype(np.float32), B.astype(np.float32)
    q32 = q.astype(np.float32)
    rest = q32.astype(np.float64) @ (A32.astype(np.float64) - B32.astype(np.float64))   # column 1 of q is still 0
    q32[1] = np.float32((rest - 3e-5) / float(B32[1]))
    return A32, B32, q32


@functools.lru_cache(maxsize=None)
def realistic_S(D=512):
    """float64 S [130][N_BIG] of the first D columns: one BLAS call"""
    g, q, _ = realistic()
    return q[:, :D].astype(np.float64) @ g[:, :D].astype(np.float64).T


def deltas(q, is_i8, gmax, gerr):
    """delta per query in float64 from the product's fp32 constants"""
    qn = np.linalg.norm(np.asarray(q, np.float64), axis=1)
    return qn * (C_ROUND[is_i8] * float(gmax) + (F1_02 * float(gerr) if is_i8 else 0.0))


def shadow_exact_S(kind, D=512):
    """the coarse similarity of the reference's own shadow in exact arithmetic: float64 sum of fp16(q) * q8 * scale (int8) / fp16(q) * fp16(g)"""
    g, q, _ = realistic()
    qh = q[:, :D].astype(np.float16).astype(np.float64)
    if kind == "i8":
        _, sc, q8 = shadow8_reference(g)
        return qh @ (q8.astype(np.float64) * sc.astype(np.float64)[:, None]).T
    return qh @ g[:, :D].astype(np.float16).astype(np.float64).T


def block_max(S, n_live=N_BIG):
    p = np.full((S.shape[0], tiles_of(n_live) * 128), NINF)
    p[:, :n_live] = S
    return p.reshape(S.shape[0], -1, 4, 32).max(3)


def build_coarse_b(ops, kind, D=512, chained=False):
    """shadow build -> bounds -> coarse (F = 33 and 130) on the realistic gallery; chained: F = 33 only, then the selection for k = 1 and k = 4"""
    g, q, _ = realistic()
    gD, qD = np.ascontiguousarray(g[:, :D]), np.ascontiguousarray(q[:, :D])
    cid = "%s_D%d_%s" % (kind, D, "chain" if chained else "B")
    ops.case(cid)
    ops.rbuf("gal", gD)
    ops.buf("bits", 8, np.zeros(2, np.int32))
    if kind == "i8":
        ops.buf("g8", TILES * 128 * 512)
        ops.buf("scale", TILES * 128 * 4)
        ops.op("shadow8", "gal", N_BIG, "g8", "scale", "bits")
        shadow, g16 = ("g8", "scale"), "-"
    else:
        ops.buf("g16", TILES * 128 * D * 2)
        ops.op("shadow16", "gal", N_BIG, D, "g16", "bits")
        shadow, g16 = ("-", "-"), "g16"
    ops.op("bounds", "bits")
    bits_file = ops.dump("bits")
    outs = []
    for F in ((33,) if chained else (33, 130)):
        ops.rbuf("q%d" % F, qD[:F])
        ks = (1, 4) if chained else (None,)
        for k in ks:
            tag = "_%d_%s" % (F, k)
            _scratch_for(ops, F, shadow, tag)
            ops.op("coarse", g16, N_BIG, D, "q%d" % F, F)
            out = _dump_scratch(ops, cid, F, tag)   # (the coarse outputs: dumped before the selection touches ctl)
            if chained:
                ops.buf("kth" + tag, F * 4)
                ops.op("select_kth", N_BIG, D, "q%d" % F, F, k, "kth" + tag if k > 1 else "-", 1 if kind == "i8" else 0)
                out.update(k=k, pairs=ops.dump("pairs" + tag, "_sel"), ctl_sel=ops.dump("ctl" + tag, "_sel"))
            outs.append(out)
    ops.end()

    def check():
        bad = []
        bits = ops.read(bits_file, np.int32)
        if bits is None:
            return ["%s: outputs missing" % cid]
        gerr, gmax = (_maxima(bits, 0) if kind == "i8" else 0.0), _maxima(bits, 1)
        S = realistic_S(D)
        ref = block_max(S)
        for out in outs:
            got, b = read_coarse(ops, out)
            bad += b
            if got is None:
                continue
            F = out["F"]
            d = deltas(qD[:F], kind == "i8", gmax, gerr)
            with np.errstate(invalid="ignore"):   # (a block of pad rows only: -inf on both sides)
                err = np.where(got[0] == ref[:F], 0.0, np.abs(got[0].astype(np.float64) - ref[:F]))
            ratio = err / d[:, None, None]
            print("%s F=%d%s: max(err / delta) = %.4f (gerr %.6g, gmax_norm %.6g)" % (cid, F, " k=%d" % out["k"] if chained else "", np.nanmax(ratio), gerr, gmax))
            if not (ratio <= 1).all():
                i = tuple(int(v) for v in np.argwhere(~(ratio <= 1))[0])
                bad.append("%s F=%d: %d coarse entries are further than delta from the float64 block maximum, first at (q, tile, block) = %s: %r against %r, delta %.4g" %
                           (cid, F, (~(ratio <= 1)).sum(), i, got[0][i], ref[:F][i], d[i[0]]))
            bad += _bit_diff("%s F=%d wgmax" % (cid, F), got[1], wg_maxima(got[0]))
            if chained:
                bad += check_chained(ops, out, S[:F], cid)
        return bad
    return check


def read_pairs(pairs, ctl, pair_cap):
    """(overflow flag, counts [64], list of 64 lists of (q, tile, mask))"""
    sub_cap = pair_cap // SEL_SUB
    counts = ctl[CTL_SEG0:CTL_SEG0 + SEL_SUB * CTL_STRIDE:CTL_STRIDE]
    p = pairs.reshape(pair_cap, 2)
    lists = []
    for s in range(SEL_SUB):
        e = p[s * sub_cap:s * sub_cap + min(int(counts[s]), sub_cap)]
        lists.append([(int(a), int(b) & ((1 << 28) - 1), (int(b) >> 28) & 15) for a, b in e])
    return int(ctl[CTL_OVERFLOW]), counts.copy(), lists


def check_chained(ops, out, S, cid, pair_cap=8192):
    """every row with float64 S >= the float64 k-th best S lies in a listed (tile, block); no overflow"""
    pairs, ctl = ops.read(out["pairs"], np.int32), ops.read(out["ctl_sel"], np.int32)
    if pairs is None or ctl is None:
        return ["%s k=%d: selection outputs missing" % (cid, out["k"])]
    ovf, counts, lists = read_pairs(pairs, ctl, pair_cap)
    bad = []
    if ovf:
        bad.append("%s k=%d: the pair list overflowed (largest sub-list %d of %d)" % (cid, out["k"], counts.max(), pair_cap // SEL_SUB))
    listed = np.zeros((S.shape[0], TILES * 4), bool)
    for sub in lists:
        for q, t, mask in sub:
            for b in range(4):
                if mask >> b & 1:
                    listed[q, t * 4 + b] = True
    kth = np.sort(S, axis=1)[:, -out["k"]]
    need = np.argwhere(S >= kth[:, None])
    miss = [(int(q), int(r)) for q, r in need if not listed[q, r // 32]]
    print("%s k=%d: %d pairs listed, largest sub-list %d; %d (query, row) at or above the k-th best" % (cid, out["k"], counts.sum(), counts.max(), len(need)))
    if miss:
        bad.append("%s k=%d: %d rows at or above the float64 k-th best similarity are in no listed block, first (q, row) = %s" % (cid, out["k"], len(miss), miss[0]))
    return bad


# ------------------------------------------------------------------------------------------------ stage 3: k-th entry
KTH_K, KTH_ENT = (2, 3, 16), (4, 12, 4 * 515, 4 * 1031)


def kth_rows(n_ent, k):
    """tilemax rows [6][n_ent]: random; the 16 largest in one thread's list (indices = 5 mod 256); the 16 largest all equal; NaN, -inf and +inf
    sprinkled; fewer than k entries that count; the k-th and (k+1)-th equal"""
    r = _rng("kth", n_ent, k)
    t = r.standard_normal((6, n_ent)).astype(np.float32)
    idx = np.arange(5, n_ent, 256)[:16]
    t[1, idx] = 10 + np.arange(len(idx), dtype=np.float32)
    t[2, r.choice(n_ent, min(16, n_ent), replace=False)] = 7.5
    sp = r.permutation(n_ent)
    t[3, sp[:n_ent // 4]] = np.nan
    t[3, sp[n_ent // 4:n_ent // 2]] = NINF
    t[3, sp[n_ent // 2:n_ent // 2 + 1]] = np.inf
    t[4] = np.where(r.integers(0, 2, n_ent) == 0, np.nan, NINF)
    t[4, r.choice(n_ent, min(k - 1, n_ent), replace=False)] = r.standard_normal(min(k - 1, n_ent))
    top = np.argsort(-t[5])
    if n_ent > k:
        t[5, top[k]] = t[5, top[k - 1]]
    return t


def kth_reference(rows, k):
    out = np.full(len(rows), NINF, np.float32)
    for i, row in enumerate(rows):
        v = np.sort(row[~np.isnan(row) & (row > NINF)])[::-1]
        if len(v) >= k:
            out[i] = v[k - 1]
    return out


def build_kth(ops):
    checks = []
    D = 64
    for n_ent in KTH_ENT:
        for k in KTH_K:
            cid = "kth_n%d_k%d" % (n_ent, k)
            tiles = n_ent // 4
            rows = kth_rows(n_ent, k)
            F = len(rows)
            ops.case(cid)
            ops.rbuf("q", unit_rows(_rng("kthq"), F, D))
            ops.scratch(F, tiles, tilemax=rows, wgmax=np.zeros((COARSE_WG, F), np.float32), ctl=np.zeros(CTL_WORDS, np.int32), qkey=np.zeros(F, np.uint64))
            ops.buf("kth", F * 4)
            ops.op("bounds_set", fbits(0.01), fbits(1.0))
            ops.op("select_kth", tiles * 128, D, "q", F, k, "kth", 1)
            f = ops.dump("kth")
            f2 = ops.dump("tilemax")
            ops.end()
            checks.append(lambda cid=cid, f=f, f2=f2, rows=rows, k=k: _bit_diff(cid, ops.read(f, np.float32), kth_reference(rows, k)) +
                          _bit_diff(cid + " tilemax (an input)", ops.read(f2, np.float32), rows))
    return lambda: _guards(ops) + [m for c in checks for m in c()]


# ------------------------------------------------------------------------------------------------ stage 4: pair selection
def select_reference(tilemax, wgmax, Q, gmax, gerr, is_i8, pair_cap, kth=None, abs_thr=None, tile_min=0, strict=True):
    """-> (overflow, counts [64], sets [64] of (q, tile, mask), thr [F], slack [F]); asserts that no entry lies within the slack of thr"""
    F, T, _ = tilemax.shape
    sub_cap = pair_cap // SEL_SUB
    sets = [set() for _ in range(SEL_SUB)]
    thr_all, slack_all = np.zeros(F), np.zeros(F)
    for q in range(F):
        col = wgmax[:, q].astype(np.float64)
        anynan = bool(np.isnan(col).any())
        m = np.fmax.reduce(np.concatenate([[NINF], col]))
        if kth is not None:
            m = float(kth[q])
        qn = float(np.linalg.norm(Q[q].astype(np.float64)))
        bounded = (not anynan) and qn < 6.0e4 and float(gmax) < 6.0e4 and float(gerr if is_i8 else 0.0) < 6.0e4
        delta = qn * (C_ROUND[is_i8] * float(gmax) + (F1_02 * float(gerr) if is_i8 else 0.0))
        if abs_thr is not None:
            thr, kd = (abs_thr - delta, 1) if bounded else (NINF, 0)
        else:
            thr, kd = (m - 2 * delta, 2) if (bounded and np.isfinite(m)) else (NINF, 0)
        slack = kd * delta * SLACK_REL + U * abs(thr) if np.isfinite(thr) else 0.0
        thr_all[q], slack_all[q] = thr, slack
        e = tilemax[q].astype(np.float64)
        if np.isfinite(thr) and strict:
            close = np.abs(e[tile_min:] - thr) <= slack
            assert not close.any(), "query %d: %d entries lie inside the slack interval of the threshold" % (q, close.sum())
        with np.errstate(invalid="ignore"):
            inside = ~(e < thr)
        mask = (inside * np.array([1, 2, 4, 8])).sum(1)
        for t in np.nonzero(mask)[0]:
            if t >= tile_min:
                seg = next(s for s in range(SEL_SEG) if T * s // SEL_SEG <= t < T * (s + 1) // SEL_SEG)
                sets[seg + SEL_SEG * (q & 3)].add((q, int(t), int(mask[t])))
    counts = np.array([len(s) for s in sets], np.int32)
    return int((counts > sub_cap).any()), counts, sets, thr_all, slack_all


def select_inputs(variant):
    """dict of the inputs of one selection case (F = 5, 515 tiles, D = 64): see build_select for the variants"""
    r = _rng("select", variant)
    F, T, D = 5, TILES, 64
    is_i8 = variant != "fp16"
    Q = (r.standard_normal((F, D)) * np.array([0.3, 1.0, 2.5, 0.7, 1.3])[:, None]).astype(np.float32)
    gmax, gerr = np.float32(1.25), np.float32(0.0123)
    d = dict(F=F, T=T, D=D, is_i8=is_i8, pair_cap=8192, k=1, abs_thr=None, tile_min=0)
    if variant == "qnorm":
        Q[3] *= np.float32(6.0e4 / np.linalg.norm(Q[3]) * 1.001)
    if variant == "gmax":
        gmax = np.float32(6.5e4)
    m = np.array([0.81, 0.42, 1.7, -0.3, 0.05])   # the best coarse entry of each query
    tilemax = np.empty((F, T, 4), np.float32)
    k = 3 if variant == "topk" else 1
    if variant == "abs":
        d.update(abs_thr=float(np.float32(0.37)), tile_min=100)
    qn = np.linalg.norm(Q.astype(np.float64), axis=1)
    delta = qn * (C_ROUND[is_i8] * float(gmax) + (F1_02 * float(gerr) if is_i8 else 0.0))
    for q in range(F):
        top = d["abs_thr"] if variant == "abs" else m[q]
        band = (1 if variant == "abs" else 2) * delta[q]
        thr = top - band
        slack = band * SLACK_REL + U * abs(thr)
        lo = thr - 3 * band - 0.5
        tilemax[q] = r.uniform(lo, thr - 0.5 * band, (T, 4))          # background: well outside
        edge = sorted({T * s // SEL_SEG for s in range(SEL_SEG)} | {T * (s + 1) // SEL_SEG - 1 for s in range(SEL_SEG)})
        for j, t in enumerate(edge):                                   # the first and the last tile of every segment
            if (j + q) % 3:
                tilemax[q, t, (j + q) % 4] = thr + band * r.uniform(0.05, 0.9)
        free = [t for t in range(T) if t not in edge]
        pick = r.choice(free, 24, replace=False)
        for j, t in enumerate(pick[:8]):
            tilemax[q, t, j % 4] = thr + 4 * slack                     # just inside
        for j, t in enumerate(pick[8:16]):
            tilemax[q, t, j % 4] = thr - 4 * slack                     # just outside
        for j, t in enumerate(pick[16:20]):
            tilemax[q, t] = thr + band * 0.5                           # all four blocks
        tilemax[q, pick[20], 1] = np.nan                               # a NaN entry is listed
        if variant == "overflow" and q == 2:                           # enough pairs in (segment 5, queries = 2 mod 4) to fill it past its end
            for t in range(162, 176):
                tilemax[q, t, t % 4] = thr + band * 0.3
        if variant != "abs":                                           # the entries that make `top` the (k-th) largest
            for j in range(k):
                tilemax[q, pick[21 + j % 3], 3 - j] = top + (k - 1 - j) * 0.25 * band if j < k - 1 else top
    wg = np.full((COARSE_WG, F), NINF, np.float32)
    for q in range(F):
        wg[:, q] = r.uniform(-1, 0, COARSE_WG) + np.nanmax(tilemax[q]) - 1
        wg[(q * 37) % COARSE_WG, q] = np.nanmax(tilemax[q])
    if variant == "nonfinite":
        wg[:, 1] = np.inf                 # m = +inf
        wg[77, 2] = np.nan                # a NaN among the workgroup maxima
        wg[:, 3] = NINF                   # m = -inf
    if variant == "overflow":
        d["pair_cap"] = SEL_SUB * 8
    d.update(Q=Q, gmax=gmax, gerr=gerr, tilemax=tilemax, wgmax=wg, k=k)
    if variant == "overflow":             # thin the lists to at most 8 per sub-list, then one sub-list to exactly 9
        d["tilemax"] = tilemax = _thin_for_overflow(d)
    return d


def _thin_for_overflow(d):
    """at most sub_cap = 8 pairs in every sub-list but one, which gets sub_cap + 1"""
    tm = d["tilemax"].copy()
    tm[np.isnan(tm)] = -100.0
    _, counts, sets, thr, _ = select_reference(tm, d["wgmax"], d["Q"], d["gmax"], d["gerr"], d["is_i8"], d["pair_cap"])
    target = 16 * 2 + 5   # sub-list of segment 5, queries = 2 mod 4
    for s, members in enumerate(sets):
        members = sorted(members)
        keep = 9 if s == target else min(len(members), 8 if s % 3 else 5)
        for q, t, _ in members[keep:]:
            tm[q, t] = -100.0
        assert s != target or len(members) >= 9
    return tm


def select_case_reference(d):
    kth = None
    if d["k"] > 1:
        kth = kth_reference(d["tilemax"].reshape(d["F"], -1), d["k"])
    return select_reference(d["tilemax"], d["wgmax"], d["Q"], d["gmax"], d["gerr"], d["is_i8"], d["pair_cap"], kth, d["abs_thr"], d["tile_min"])


SELECT_VARIANTS = ("top1", "fp16", "topk", "abs", "nonfinite", "qnorm", "gmax", "overflow")


def build_select(ops):
    checks = []
    for variant in SELECT_VARIANTS:
        d = select_inputs(variant)
        cid = "select_" + variant
        F, T, D = d["F"], d["T"], d["D"]
        ops.case(cid)
        ops.rbuf("q", d["Q"])
        ops.scratch(F, T, pair_cap=d["pair_cap"], tilemax=d["tilemax"], wgmax=d["wgmax"], ctl=np.zeros(CTL_WORDS, np.int32), qkey=np.zeros(F, np.uint64))
        ops.op("bounds_set", fbits(d["gerr"]), fbits(d["gmax"]))
        if d["abs_thr"] is not None:
            ops.op("select_thr", T * 128, D, "q", F, fbits(d["abs_thr"]), d["tile_min"], int(d["is_i8"]))
        else:
            ops.buf("kth", F * 4)
            ops.op("select_kth", T * 128, D, "q", F, d["k"], "kth" if d["k"] > 1 else "-", int(d["is_i8"]))
        files = (ops.dump("pairs"), ops.dump("ctl"), ops.dump("tilemax"), ops.dump("wgmax"), ops.dump("qkey"))
        ops.end()
        checks.append(lambda cid=cid, d=d, files=files: check_select(ops, cid, d, files))
    return lambda: _guards(ops) + [m for c in checks for m in c()]


def check_select(ops, cid, d, files):
    pairs, ctl = ops.read(files[0], np.int32), ops.read(files[1], np.int32)
    if pairs is None or ctl is None:
        return ["%s: outputs missing" % cid]
    bad = _bit_diff(cid + " tilemax (an input)", ops.read(files[2], np.float32), d["tilemax"]) + _bit_diff(cid + " wgmax (an input)", ops.read(files[3], np.float32), d["wgmax"])
    if ops.read(files[4], np.uint64).any():
        bad.append("%s: qkey was written" % cid)
    want_ovf, want_counts, want_sets, _, _ = select_case_reference(d)
    ovf, counts, lists = read_pairs(pairs, ctl, d["pair_cap"])
    sub_cap = d["pair_cap"] // SEL_SUB
    other = np.ones(CTL_WORDS, bool)
    other[CTL_OVERFLOW] = False
    other[CTL_SEG0:CTL_SEG0 + SEL_SUB * CTL_STRIDE:CTL_STRIDE] = False
    if ctl[other].any():
        bad.append("%s: control words other than the flag and the 64 counters were written" % cid)
    if ovf != want_ovf:
        bad.append("%s: overflow flag %d, reference %d" % (cid, ovf, want_ovf))
    if not np.array_equal(counts, want_counts):
        s = int(np.argmax(counts != want_counts))
        bad.append("%s: sub-list counts differ, first sub-list %d: %d, reference %d" % (cid, s, counts[s], want_counts[s]))
    for s in range(SEL_SUB):
        got = set(lists[s])
        if len(got) != len(lists[s]):
            bad.append("%s: sub-list %d holds a pair twice" % (cid, s))
        if want_counts[s] <= sub_cap:
            if got != want_sets[s]:
                bad.append("%s: sub-list %d: %d pairs missing, %d unexpected, e.g. %s" % (cid, s, len(want_sets[s] - got), len(got - want_sets[s]), sorted(want_sets[s] ^ got)[:3]))
        elif not (got <= want_sets[s] and len(got) == sub_cap):
            bad.append("%s: the overflowing sub-list %d must hold %d of the reference's pairs" % (cid, s, sub_cap))
    if d["tile_min"] and any(t < d["tile_min"] for sub in lists for _, t, _ in sub):
        bad.append("%s: a tile below tile_min is listed" % cid)
    return bad


# ------------------------------------------------------------------------------------------------ stage 5: re-rank and unpack
def exact_ranking(S, k, row_offset=0, labels=None, excluded=None):
    """float64 S [F][N] -> (idx [F][k] int32, sim [F][k] fp32): higher similarity first, lower index first, NaN never, -1 / -inf when exhausted"""
    F, N = S.shape
    idx, sim = np.full((F, k), -1, np.int32), np.full((F, k), NINF, np.float32)
    for q in range(F):
        s = S[q].copy()
        ok = ~np.isnan(s)
        if labels is not None:
            ok &= labels != excluded[q]
        cand = np.nonzero(ok)[0]
        order = cand[np.argsort(-s[cand], kind="stable")][:k]
        idx[q, :len(order)] = order + row_offset
        sim[q, :len(order)] = s[order]
        assert np.array_equal(sim[q, :len(order)].astype(np.float64), s[order]), "class A similarities must be exact in fp32"
    return idx, sim


def rerank_gallery(D, half):
    """(rows fp32 [N_SMALL][D] holding integers (half: integers * 2^-6), pad rows [51][D], queries [8][D])"""
    r = _rng("rerank", D)
    N = N_SMALL
    scale = np.float32(2.0 ** -6 if half else 1.0)
    g = r.integers(-3, 4, size=(N, D)).astype(np.float32)
    q = r.integers(-2, 3, size=(8, D)).astype(np.float32)
    best = lambda i: 3 * np.sign(q[i]) + (q[i] == 0)       # the row with the largest similarity query i can see
    g[[5, 40, 70, 300]] = best(0)                           # q0: equal maxima in block 0, block 1 (same wave), block 2 (the other wave) and tile 2
    g[100] = best(1)                                        # q1: strictly better, but its block is not flagged
    g[30] = best(1) - (np.arange(D) == np.abs(q[1]).argmax()) * np.sign(q[1])   # the second best: one step lower in a column the query sees
    g[N - 1] = best(2)                                      # q2: the last live row; the pad rows behind it would win (half only: they exist there)
    g[192:224] = -np.sign(q[3]) * r.integers(1, 4, size=(32, D))   # q3: its one listed block (rows 192 - 223) has negative similarities only
    q[4] = np.where(np.arange(D) % 2, 0.0, -0.0)            # q4, zero similarities: every product is +0.0 or -0.0, every sum +0.0 (no -0.0 is reachable); first index wins
    g[10, 3] = np.nan                                       # q5: a NaN row never wins (row 10 is listed for it)
    g[11] = best(5) - 2 * (np.arange(D) == np.abs(q[5]).argmax()) * np.sign(q[5])
    pad = np.tile(best(2), (tiles_of(N) * 128 - N, 1)).astype(np.float32) * 2
    return g * scale, pad * scale, q


def rerank_lists():
    """hand-written pair list: query -> [(tile, mask)]; query 6 has no pair"""
    return {0: [(0, 0b0111), (2, 0b0010)], 1: [(0, 0b0001), (1, 0b1111)], 2: [(3, 0b0111), (0, 0b1000)], 3: [(1, 0b0100)], 4: [(1, 0b0011), (0, 0b0100)],
            5: [(0, 0b0001)], 7: [(t, 0b1111) for t in range(4)]}


def listed_rows(lists, q, N):
    rows = []
    for t, mask in lists.get(q, []):
        for b in range(4):
            if mask >> b & 1:
                rows += [g for g in range(t * 128 + b * 32, t * 128 + b * 32 + 32) if g < N]
    return np.array(sorted(rows), np.int64)


def build_rerank(ops):
    """launch_match_top1_excluding(screened = true) behind hand-written pair lists: GT = float and half, D = 512 and 64, with and without the
    overflow flag set by hand"""
    checks = []
    N, F, pair_cap = N_SMALL, 8, SEL_SUB * 8
    sub_cap = pair_cap // SEL_SUB
    lists = rerank_lists()
    for D in (512, 64):
        for half in (False, True):
            for overflow in (False, True):
                cid = "rerank_D%d_%s%s" % (D, "half" if half else "float", "_overflow" if overflow else "")
                g, pad, q = rerank_gallery(D, half)
                labels = (np.arange(N) % 7).astype(np.int32)
                excluded = np.array([-1, -1, -1, -1, -1, -1, -1, 5], np.int32)   # q7 lists every tile and leaves out identity 5
                q[7] = q[0]
                assert labels[5] == 5 and labels[40] == 5 and labels[70] != 5       # q7 = q0 without rows 5 and 40: row 70 wins
                pairs, ctl = np.zeros((pair_cap, 2), np.int32), np.zeros(CTL_WORDS, np.int32)
                for qq, ent in lists.items():
                    for j, (t, mask) in enumerate(ent):
                        sub = (3 * qq + 5 * j) % SEL_SUB   # (the re-rank walks every sub-list: any will do)
                        n = ctl[CTL_SEG0 + sub * CTL_STRIDE]
                        assert n < sub_cap
                        pairs[sub * sub_cap + n] = (qq, (t | mask << 28) - ((1 << 32) if mask >> 3 else 0))   # (bit 31 set: the int32 view)
                        ctl[CTL_SEG0 + sub * CTL_STRIDE] = n + 1
                ctl[CTL_OVERFLOW] = int(overflow)
                ops.case(cid)
                if half:
                    ops.rbuf("g16", to_g16(g.astype(np.float16), pad.astype(np.float16)))
                else:
                    ops.rbuf("gal", g)
                ops.rbuf("q", q)
                ops.rbuf("labels", labels)
                ops.rbuf("excluded", excluded)
                ops.scratch(F, tiles_of(N), pair_cap=pair_cap, tilemax=np.zeros((F, tiles_of(N), 4), np.float32), wgmax=np.zeros((COARSE_WG, F), np.float32),
                            ctl=ctl, pairs=pairs, qkey=np.zeros(F, np.uint64))
                pb = tiles_of(N)
                ops.buf("partial", pb * F * 8)
                ops.buf("idx", F * 4)
                ops.buf("sim", F * 4)
                ops.buf("ovf", 4)
                ops.op("rerank_excl", "-" if half else "gal", "g16" if half else "-", N, D, "q", F, "partial", pb, "labels", "excluded", "idx", "sim", "ovf")
                files = (ops.dump("idx"), ops.dump("sim"), ops.dump("ovf"), ops.dump("qkey"), ops.dump("pairs"), ops.dump("partial"))
                ops.end()

                def check(cid=cid, g=g, q=q, labels=labels, excluded=excluded, overflow=overflow, files=files, pairs=pairs, half=half):
                    idx, sim, ovf, qkey = (ops.read(f, t) for f, t in zip(files[:4], (np.int32, np.float32, np.int32, np.uint64)))
                    if idx is None or sim is None or ovf is None or qkey is None:
                        return ["%s: outputs missing" % cid]
                    rows = g.astype(np.float16).astype(np.float64) if half else g.astype(np.float64)
                    with np.errstate(invalid="ignore"):
                        S = np.where(np.isnan(rows).any(1)[None, :], np.nan, q.astype(np.float64) @ np.nan_to_num(rows).T)
                    S = S + 0.0   # (numpy's matmul may give -0.0; the device's chain starts at +0.0 and cannot: module docstring, stage 5)
                    if overflow:
                        want_i, want_s = exact_ranking(S, 1, labels=labels, excluded=excluded)
                    else:
                        want_i, want_s = np.full((F, 1), -1, np.int32), np.full((F, 1), NINF, np.float32)
                        for qq in range(F):
                            rr = listed_rows(lists, qq, N)
                            if len(rr):
                                i, s = exact_ranking(S[qq:qq + 1, rr], 1, labels=labels[rr], excluded=excluded[qq:qq + 1])
                                want_i[qq], want_s[qq] = (rr[i[0, 0]] if i[0, 0] >= 0 else -1), s[0, 0]
                    bad = _bit_diff(cid + " idx", idx, want_i) + _bit_diff(cid + " sim", sim, want_s)
                    if int(ovf[0]) != int(overflow):
                        bad.append("%s: *overflow_out = %d" % (cid, ovf[0]))
                    if qkey.any():
                        bad.append("%s: qkey is not back at zero behind the unpack" % cid)
                    bad += _bit_diff(cid + " pairs (an input)", ops.read(files[4], np.int32), pairs)
                    if not overflow and (ops.read(files[5], np.uint8) != 0x5a).any():
                        bad.append("%s: the gated exact scan wrote partials although the list did not overflow" % cid)
                    return bad
                checks.append(check)
    return lambda: _guards(ops) + [m for c in checks for m in c()]


def rerank_conditions():
    """the hand-written lists exercise what they claim to (asserted on the reference; no GPU)"""
    lists = rerank_lists()
    for D in (512, 64):
        for half in (False, True):
            g, pad, q = rerank_gallery(D, half)
            rows = g.astype(np.float64)
            S = q.astype(np.float64) @ np.nan_to_num(rows).T
            r0 = listed_rows(lists, 0, N_SMALL)
            assert {5, 40, 70, 300} <= set(r0) and len({S[0, i] for i in (5, 40, 70, 300)}) == 1 and S[0, 5] == S[0, r0].max()
            r1 = listed_rows(lists, 1, N_SMALL)
            assert 100 not in r1 and S[1, 100] > S[1, r1].max() and 30 in r1
            assert (q[2].astype(np.float64) @ pad.astype(np.float64).T > S[2].max()).all() and N_SMALL - 1 in listed_rows(lists, 2, N_SMALL)
            assert (S[3, listed_rows(lists, 3, N_SMALL)] < 0).all()
            assert not S[4].any()
            assert 10 in listed_rows(lists, 5, N_SMALL) and np.isnan(g[10]).any()
            assert 6 not in lists


@functools.lru_cache(maxsize=None)
def screened_inputs(D, half):
    """launch_match_screened on a real coarse scan: (rows fp32 [N_BIG][D], queries [12][D]).  The class A integers of the coarse cases (x 2^-6 when
    stored as fp16) with planted duplicates: query 0's three best rows are identical and sit in one block, in the other wave of the tile and in
    another tile; query 1's two best are identical and 60 000 rows apart; query 2's best is the last live row."""
    G, Q, _ = coarse_a_base()
    g = G[:N_BIG, :D].astype(np.float32)
    q = Q[:12, :D].copy()
    best = lambda i: 127 * np.sign(q[i]) + (q[i] == 0)
    g[[7 * 128 + 3, 7 * 128 + 17, 7 * 128 + 70, 40000]] = best(0)
    g[[123, 60123]] = best(1)
    g[N_BIG - 1] = best(2)
    if half:
        g = g * np.float32(2.0 ** -6)
    return g, q


def build_screened(ops):
    checks = []
    for D, half in ((512, False), (512, True), (64, False), (64, True)):
        g, q = screened_inputs(D, half)
        F = len(q)
        cid = "screened_D%d_%s" % (D, "half" if half else "float")
        ops.case(cid)
        ops.rbuf("q", q)
        ops.buf("bits", 8, np.zeros(2, np.int32))
        i8 = D == 512 and not half
        g16 = to_g16(g.astype(np.float16))
        assert np.array_equal(g.astype(np.float16).astype(np.float32), g)
        if not half:
            ops.rbuf("gal", g)
        if i8:
            ops.buf("g8", TILES * 128 * 512)
            ops.buf("scale", TILES * 128 * 4)
            ops.op("shadow8", "gal", N_BIG, "g8", "scale", "bits")
        else:
            ops.rbuf("g16", g16)
            ops.op("norm16", "g16", 0, N_BIG, D, "bits")
        ops.op("bounds", "bits")
        pb = 512
        outs = []
        for k, row_offset in ((1, 0), (3, 1000)):
            tag = "_k%d" % k
            _scratch_for(ops, F, ("g8", "scale") if i8 else ("-", "-"), tag)
            ops.buf("kth" + tag, F * 4)
            ops.buf("partial" + tag, 128 * F * 8)
            ops.buf("idx" + tag, F * k * 4)
            ops.buf("sim" + tag, F * k * 4)
            ops.op("screened", "-" if half else "gal", "-" if i8 else "g16", N_BIG, D, "q", F, k, "kth" + tag, "partial" + tag, pb, "idx" + tag, "sim" + tag, row_offset)
            outs.append((k, row_offset, ops.dump("idx" + tag), ops.dump("sim" + tag), ops.dump("qkey" + tag), ops.dump("ctl" + tag)))
        ops.end()

        def check(cid=cid, g=g, q=q, outs=outs):
            S = q.astype(np.float64) @ g.astype(np.float64).T
            bad = []
            for k, row_offset, fi, fs, fq, fc in outs:
                idx, sim, qkey, ctl = ops.read(fi, np.int32), ops.read(fs, np.float32), ops.read(fq, np.uint64), ops.read(fc, np.int32)
                if idx is None or sim is None or qkey is None or ctl is None:
                    bad.append("%s k=%d: outputs missing" % (cid, k))
                    continue
                want_i, want_s = exact_ranking(S, k, row_offset)
                bad += _bit_diff("%s k=%d idx" % (cid, k), idx, want_i) + _bit_diff("%s k=%d sim" % (cid, k), sim, want_s)
                if ctl[CTL_OVERFLOW]:
                    bad.append("%s k=%d: the pair list overflowed: the exact scan answered, not the re-rank" % (cid, k))
                if qkey.any():
                    bad.append("%s k=%d: qkey is not back at zero" % (cid, k))
            return bad
        checks.append(check)
    return lambda: _guards(ops) + [m for c in checks for m in c()]


# ------------------------------------------------------------------------------------------------ the groups: one harness process each
def _single(fn, *a, **kw):
    def build(ops):
        check = fn(ops, *a, **kw)
        return lambda: _guards(ops) + check()
    return build


GROUPS = {
    "shadow": build_shadow,
    "coarse_i8_A": _single(build_coarse_a, "i8"),
    "coarse_f16_D64_A": _single(build_coarse_a, "f16", 64),
    "coarse_f16_D128_A": _single(build_coarse_a, "f16", 128),
    "coarse_f16_D256_A": _single(build_coarse_a, "f16", 256),
    "coarse_f16_D512_A": _single(build_coarse_a, "f16", 512),
    "coarse_i8_nonfinite": _single(build_coarse_a, "i8", 512, True),
    "coarse_f16_nonfinite": _single(build_coarse_a, "f16", 512, True),
    "coarse_i8_B": _single(build_coarse_b, "i8"),
    "coarse_f16_D64_B": _single(build_coarse_b, "f16", 64),
    "coarse_f16_D128_B": _single(build_coarse_b, "f16", 128),
    "coarse_f16_D256_B": _single(build_coarse_b, "f16", 256),
    "coarse_f16_D512_B": _single(build_coarse_b, "f16", 512),
    "kth": build_kth,
    "select": build_select,
    "rerank": build_rerank,
    "screened": build_screened,
    "chain_i8": _single(build_coarse_b, "i8", 512, True),
    "chain_f16": _single(build_coarse_b, "f16", 512, True),
}
