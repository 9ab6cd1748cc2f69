"""The exact fp32 scan (match_kernel / match_reduce_kernel, csrc/kernels_match.hip) and the device merges, restated outside the library, and the
cases that tests/test_gpu_match_exact.py runs through tests/cpp/match_exact_check.cpp: every instantiation launched alone on guarded buffers.

THE DEFINITION.  S(q, g) is a chain of D fused multiply-adds in fp32 that starts at +0.0; per 8 columns the order is k = 8 ks + (0, 4, 1, 5, 2, 6,
3, 7) (exact_row_dot, frt_kernels.h; the MFMA chain of match_kernel: lanes 0 - 31 carry k = 8 ks + s, lanes 32 - 63 k = 8 ks + 4 + s).  fp16-stored
rows are widened exactly first.  fmaf32() is the correctly rounded fp32 of a b + c: the product of two fp32 values is exact in float64, the sum
takes ONE float64 rounding, and only when that float64 sum sits exactly on the midpoint of two neighbouring fp32 values while the exact sum does not
(Knuth's TwoSum gives the residual) can rounding it again go the wrong way; there the residual's sign picks the neighbour.  chain_S() is that chain,
vectorised over (query, row).  ranking(): higher similarity first, then the lower global index; NaN is never a candidate; with labels an identity
counts once (its best row); -1 / -inf behind the end.

THE BOUND.  gamma(D) = D u / (1 - D u), u = 2^-24: a chain of D fmas in ANY order is within gamma(D) sum_k |q_k g_k| of the float64 sum (one
rounding per step, Higham's gamma_n; the float64 reference's own error, D 2^-53 relative, is 2^-29 of it and is not added).  Nothing goes on top.

THE CLASSES, per launcher and row type (float rows, fragment-ordered half rows):
  A  exact: small integers (x 2^-6 when stored as fp16), sums exact in any order; index, similarity bits, labels and the full matrix are compared
     bit for bit against float64.  Query 0's best row is planted at rows 2 and 5 (one 32-row block, both lane halves of the epilogue), 40 (another
     wave), 198 (another workgroup) and 393 (the second tile of workgroup 0 at partial_blocks = 3); row 10 holds a NaN; query 4 is all zeros.
  C  chain: unit rows, noisy queries, and for the first queries rows planted within a few ulps of the winner; every written similarity equals
     chain_S bit for bit, every index / label equals ranking(chain_S).  tests/test_match_exact_ref.py shows that the float64 winner and the chain
     winner differ for some query, so an order other than the chain's cannot pass by luck.
  B  bound: on the class C data every written similarity is within gamma(D) sum |q_k g_k| of float64; max(err / bound) is printed per case.

THE CASE TABLE (N = 461 = 4 tiles, the last ragged, unless stated; every case for float and for half rows):
  top1         F 1 / 32 (NQ 1), 33 / 64 (NQ 2), 65 / 130 (NQ 4) x D 32 / 96 / 512; partial_blocks 3 (workgroup 0 walks tiles 0 and 3), 4, 6 (two
               workgroups own no tile and leave -1 partials); row_offset 0 and 1000; N = 1 and N = 2
  full         F 32 (NQ 1) and 130 (NQ 4) at D = 512, F = 33 at D = 32 and 96; N = 65 869 (515 tiles > the grid of 512: the tile walk), F = 33, D = 32
  topk         k 1 / 5, F 32 (NQ 1 EXCL) and 33 / 130 (NQ 4 EXCL), row_offset 0 / 1000, partial_blocks 3 / 4 / 6; N = 2 with k = 3
  topk_labels  labels arange(N) % 7 with k = 5; 3 labels with k = 5 (empty slots); row_offset 1000; F 32 (NQ 1 EXCL LAB) and 33 / 130 (NQ 4)
  top1_excl    the excluded label owns the overall best row (query 0: rows 2, 5 and 198 leave, row 40 wins); -1 = no exclusion; F 32 and 130
  merge, merge_labels   shards 1 / 2 / 3 / 8 x n 1 / 64 / 65 / 130 x k 1 / 5 / 16, lists of tests/test_topk_merge.py and tests/test_identity_merge.py
               (ties across shards, empty slots, queries without any entry, fewer labels than k), against oracle.match.merge_topk and
               test_identity_merge.reference_merge
Seen on an MI355X: RATIOS_SEEN below."""
import functools

import numpy as np

import match_stage_ref as R
from launch_harness import bit_diff, rng

U = 2.0 ** -24
N_WORK = R.N_SMALL   # 461: 4 tiles, the last one ragged
N_BIG = R.N_BIG      # 65 869: 515 tiles
F_ALL = 130
K_ORDER = (0, 4, 1, 5, 2, 6, 3, 7)
PLANTED = (2, 5, 40, 128 + 70, 3 * 128 + 9)
NAN_ROW, ZERO_Q = 10, 4
NEAR_Q, NEAR_ROWS = 24, 4   # class C: queries with planted near-winners, rows per query
NINF = -np.inf

# max(err / bound) of class B as printed by tests/test_gpu_match_exact.py on an MI355X: (float rows, half rows).  The device's bits are the chain's,
# so these are chain_S's own distances from float64: a sequential chain's error grows like sqrt(D) u, the bound like D u.
RATIOS_SEEN = {
    "D512_N461": (0.0282, 0.0276), "D96_N461": (0.0711, 0.0693), "D32_N461": (0.1374, 0.1248), "D32_N1": (0.0938, 0.0948), "D32_N2": (0.1167, 0.1185),
    "full_D32_N65869": (0.1698, 0.1463),
}


# ------------------------------------------------------------------------------------------------ the definition
def _fma_exact(a, b, c):
    """flat float64 arrays holding fp32 values -> fp32, correctly rounded a * b + c (the slow path: every element examined)"""
    with np.errstate(all="ignore"):
        p = a * b
        s = p + c
        t = s - p
        e = (p - (s - t)) + (c - t)              # TwoSum: p + c = s + e exactly
        r = s.astype(np.float32)
        r64 = r.astype(np.float64)
        other = np.where(r64 < s, np.nextafter(r, np.float32(np.inf)), np.nextafter(r, np.float32(-np.inf)))
        mid = 0.5 * (r64 + other.astype(np.float64))
        fix = (s == mid) & (e != 0) & np.isfinite(r64) & (r64 != s)
        return np.where(fix, np.where(e > 0, np.maximum(r, other), np.minimum(r, other)), r)


def fmaf32(a, b, c):
    """the correctly rounded fp32 of a * b + c (fp32 in, fp32 out; any broadcastable shapes)"""
    a, b, c = (np.asarray(x, np.float32).astype(np.float64) for x in (a, b, c))
    with np.errstate(all="ignore"):
        s = a * b + c
        r = np.asarray(s.astype(np.float32))
    # a float64 on an fp32 midpoint ends in 1 and 28 zeros (normal fp32 range); subnormal results take the slow path as well
    cand = ((np.asarray(s).view(np.uint64) & np.uint64(0x1FFFFFFF)) == np.uint64(0x10000000)) | (np.abs(s) < 2.0 ** -125)
    if cand.any():
        aa, bb, cc = np.broadcast_arrays(a, b, c)
        r = r.copy()
        r[cand] = _fma_exact(aa[cand], bb[cand], cc[cand])
    return r


def fmaf32_naive(a, b, c):
    """what fmaf32 would be without the correction: the float64 sum rounded again"""
    a, b, c = (np.asarray(x, np.float32).astype(np.float64) for x in (a, b, c))
    with np.errstate(all="ignore"):
        return (a * b + c).astype(np.float32)


def chain_S(q, rows, fma=fmaf32):
    """q fp32 [F][D], rows fp32 or fp16 [N][D] -> fp32 [F][N]: exact_row_dot's chain"""
    q = np.asarray(q, np.float32)
    g = np.asarray(rows).astype(np.float32)   # (fp16 widens exactly)
    D = q.shape[1]
    assert g.shape[1] == D and D % 8 == 0
    acc = np.zeros((q.shape[0], g.shape[0]), np.float32)
    for k0 in range(0, D, 8):
        for s in K_ORDER:
            acc = fma(g[None, :, k0 + s], q[:, None, k0 + s], acc)
    return acc


def exact_row_dot_literal(q, rows):
    """the loop of exact_row_dot (frt_kernels.h) statement by statement, one (query, row) at a time: what chain_S must equal"""
    q = np.asarray(q, np.float32)
    g = np.asarray(rows).astype(np.float32)
    out = np.zeros((q.shape[0], g.shape[0]), np.float32)
    for i in range(q.shape[0]):
        for j in range(g.shape[0]):
            acc = np.float32(0)
            for k0 in range(0, q.shape[1], 8):
                a, b = g[j, k0:k0 + 4], g[j, k0 + 4:k0 + 8]
                x, y = q[i, k0:k0 + 4], q[i, k0 + 4:k0 + 8]
                for s2 in range(4):
                    acc = fmaf32(a[s2], x[s2], acc)[()]
                    acc = fmaf32(b[s2], y[s2], acc)[()]
            out[i, j] = acc
    return out


def S64(q, rows):
    """float64 S [F][N]; a row that holds a NaN gives NaN for every query (0 x NaN included), and no -0.0 (the chain starts at +0.0)"""
    g = np.asarray(rows).astype(np.float64)
    with np.errstate(invalid="ignore"):
        S = np.asarray(q, np.float64) @ np.nan_to_num(g).T
    return np.where(np.isnan(g).any(1)[None, :], np.nan, S) + 0.0


def abs_S64(q, rows):
    return np.abs(np.asarray(q, np.float64)) @ np.abs(np.nan_to_num(np.asarray(rows).astype(np.float64))).T


def gamma(D):
    return D * U / (1.0 - D * U)


def ranking(S, k, row_offset=0, labels=None, excluded=None, identities=False):
    """S [F][N] (fp32 values, any float type) -> (idx [F][k] int32, sim [F][k] fp32), with identities=True (label [F][k] int32, idx, sim).
    Higher similarity first, then the lower global index; NaN never; labels + excluded [F]: the rows labelled excluded[q] take no part;
    identities: an identity counts once, with its best row; -1 / -inf (/ -1) behind the end."""
    S = np.asarray(S, np.float64)
    if not identities:
        return R.exact_ranking(S, k, row_offset, labels, excluded)
    F, N = S.shape
    lab, idx, sim = np.full((F, k), -1, np.int32), np.full((F, k), -1, np.int32), np.full((F, k), NINF, np.float32)
    for q in range(F):
        cand = np.nonzero(~np.isnan(S[q]))[0]
        order = cand[np.argsort(-S[q, cand], kind="stable")]
        first = order[np.sort(np.unique(labels[order], return_index=True)[1])][:k]   # the best row of every identity, in rank order
        lab[q, :len(first)], idx[q, :len(first)], sim[q, :len(first)] = labels[first], first + row_offset, S[q, first]
    return lab, idx, sim


# ------------------------------------------------------------------------------------------------ inputs
def stored(g, half):
    """the values the device reads: fp32 rows, or their fp16 storage"""
    return g.astype(np.float16) if half else g


@functools.lru_cache(maxsize=None)
def exact_data(D, half, N=N_WORK):
    """class A: (rows [N][D], queries [130][D]) by match_stage_ref.rerank_gallery's construction"""
    r = rng("match_exact A", D, N)
    scale = np.float32(2.0 ** -6 if half else 1.0)
    g = r.integers(-3, 4, size=(N, D)).astype(np.float32)
    q = r.integers(-2, 3, size=(F_ALL, D)).astype(np.float32)
    best = 3 * np.sign(q[0]) + (q[0] == 0)
    for p in PLANTED:
        if p < N:
            g[p] = best
    q[ZERO_Q] = np.where(np.arange(D) % 2, 0.0, -0.0)
    if N > NAN_ROW:
        g[NAN_ROW, 3] = np.nan
    g = g * scale
    assert np.array_equal(g.astype(np.float16).astype(np.float32)[~np.isnan(g)], g[~np.isnan(g)])
    return stored(g, half), q


@functools.lru_cache(maxsize=None)
def chain_data(D, half, N=N_WORK):
    """class C: (rows [N][D] as stored, queries [130][D]).  Unit rows; query i is a noisy copy of row src[i]; for i < NEAR_Q, NEAR_ROWS other rows
    are copies of src[i] moved by a few ulps of the similarity: fp32 rows by a relative 2^-17 in every column, fp16 rows by one fp16 step up in
    one column and one down in another, the pair chosen so that S moves by +-1 to 3 ulps."""
    r = rng("match_exact C", D, N, half)
    g = r.standard_normal((N, D)).astype(np.float32)
    g /= np.linalg.norm(g, axis=1, keepdims=True).astype(np.float32)
    g = stored(g, half)
    nq = min(F_ALL, N)
    perm = r.permutation(N)
    src = np.resize(perm[:nq], F_ALL)
    q = g[src].astype(np.float32) + np.float32(0.3) * r.standard_normal((F_ALL, D)).astype(np.float32) / np.float32(np.sqrt(D))
    q /= np.linalg.norm(q, axis=1, keepdims=True).astype(np.float32)
    free = list(perm[nq:])
    for i in range(NEAR_Q):
        for j in range(NEAR_ROWS):
            if not free:
                break
            row = free.pop()
            w = g[src[i]].copy()
            if half:   # one fp16 step up in column k1, one down in column k2: S moves by q_k1 step_k1 - q_k2 step_k2
                up = np.nextafter(w, np.float16(np.inf)).astype(np.float64) - w.astype(np.float64)
                down = w.astype(np.float64) - np.nextafter(w, np.float16(-np.inf)).astype(np.float64)
                move = (q[i].astype(np.float64) * up)[:, None] - (q[i].astype(np.float64) * down)[None, :]
                np.fill_diagonal(move, np.inf)
                target = (1 + j % 3) * 2.0 ** -24 * (1 if j % 2 else -1)
                k1, k2 = np.unravel_index(int(np.argmin(np.abs(move - target))), move.shape)
                w[k1], w[k2] = np.nextafter(w[k1], np.float16(np.inf)), np.nextafter(w[k2], np.float16(-np.inf))
            else:
                w = (w * (np.float32(1) + r.uniform(-2.0 ** -17, 2.0 ** -17, D).astype(np.float32))).astype(np.float32)
            g[row] = w
    return g, q


@functools.lru_cache(maxsize=None)
def reference(cls, D, half, N=N_WORK):
    """(rows, queries, S the launches must write [fp32 values; class A: exact], float64 S, sum |q_k g_k|)"""
    g, q = (exact_data if cls == "A" else chain_data)(D, half, N)
    s64 = S64(q, g)
    if cls == "A":
        S = s64.astype(np.float32)
        assert np.array_equal(S.astype(np.float64), s64, equal_nan=True)
    else:
        S = chain_S(q, g)
    return g, q, S, s64, abs_S64(q, g)


def labels_of(N, what):
    lab = (np.arange(N) % (3 if what == "three" else 7)).astype(np.int32)
    if what == "excl" and N > 5:
        lab[5] = lab[2]   # rows 2, 5 and 198 = 2 (mod 7) share identity 2: without it query 0's winner is row 40
    return lab


def excluded_of(S, labels):
    """per query the label of its overall best row (it owns the winner), every third query -1 = no exclusion; query 0 keeps its owner"""
    best = ranking(S, 1)[0][:, 0]
    ex = labels[np.maximum(best, 0)].astype(np.int32)
    ex[best < 0] = -1
    ex[3::3] = -1
    return ex


# ------------------------------------------------------------------------------------------------ the launches of one (class, D, row type)
# (op, F, partial_blocks, row_offset, k, labels): what runs at N = 461 for every class and row type
def launches(D):
    if D == 512:
        L = [("top1", F, pb, 0, 1, None) for F, pb in ((1, 4), (32, 3), (33, 4), (64, 6), (65, 3), (130, 4))]
        L += [("top1", 130, 6, 1000, 1, None), ("top1", 33, 3, 1000, 1, None), ("top1", 32, 6, 1000, 1, None)]
        L += [("full", 32, 0, 0, 0, None), ("full", 130, 0, 0, 0, None)]
        L += [("topk", 32, 3, 0, 5, None), ("topk", 33, 4, 1000, 5, None), ("topk", 130, 6, 1000, 5, None), ("topk", 1, 4, 0, 1, None), ("topk", 65, 3, 0, 1, None)]
        L += [("topk_labels", 32, 3, 0, 5, "seven"), ("topk_labels", 130, 4, 1000, 5, "seven"), ("topk_labels", 33, 6, 0, 5, "three"), ("topk_labels", 32, 4, 1000, 5, "three")]
        L += [("top1_excl", 32, 3, 0, 1, "excl"), ("top1_excl", 130, 6, 0, 1, "excl")]
        return L
    # D = 32: one k-step, every iteration an epilogue and a buffer swap; D = 96: not a multiple of 64
    return [("top1", 32, 3, 0, 1, None), ("top1", 64, 4, 1000, 1, None), ("top1", 130, 6, 0, 1, None), ("full", 33, 0, 0, 0, None),
            ("topk", 32, 6, 1000, 5, None), ("topk", 65, 3, 0, 5, None), ("topk_labels", 1, 3, 1000, 5, "seven"), ("topk_labels", 64, 4, 0, 5, "three"),
            ("top1_excl", 32, 6, 0, 1, "excl"), ("top1_excl", 33, 3, 0, 1, "excl")]


def kernel_launches(op, k):
    """how many product kernels the launcher of `op` starts (tools/match_exact_coverage.py attributes a trace's kernels with it)"""
    return {"top1": 2, "full": 1, "topk": 2 * k, "topk_labels": 2 * k, "top1_excl": 2, "merge": 1, "merge_labels": 1}[op]


def _rows_buf(ops, g, half):
    if half:
        ops.rbuf("g16", R.to_g16(g))
        return "-", "g16"
    ops.rbuf("gal", g)
    return "gal", "-"


def _emit(ops, names, N, D, launch, tag, labels_done, S):
    """one launch on output buffers of its own, exactly as large as it may write; returns the files to read back"""
    op, F, pb, off, k, lab = launch
    gal, g16 = names
    t = "_" + tag
    if op != "full":
        ops.buf("partial" + t, pb * F * 8)
    if lab and lab not in labels_done:
        ops.rbuf("labels_" + lab, labels_of(N, lab))
        labels_done.add(lab)
    if op == "top1":
        ops.buf("idx" + t, F * 4)
        ops.buf("sim" + t, F * 4)
        ops.op("top1", gal, g16, N, D, "q", F, "partial" + t, pb, "idx" + t, "sim" + t, off)
        return {"idx": ops.dump("idx" + t), "sim": ops.dump("sim" + t), "partial": ops.dump("partial" + t)}
    if op == "full":
        ops.buf("out" + t, F * N * 4)
        ops.op("full", gal, g16, N, D, "q", F, "out" + t)
        return {"out": ops.dump("out" + t)}
    if op == "topk":
        ops.buf("idx" + t, F * k * 4)
        ops.buf("sim" + t, F * k * 4)
        ops.op("topk", gal, g16, N, D, "q", F, k, "partial" + t, pb, "idx" + t, "sim" + t, off)
        return {"idx": ops.dump("idx" + t), "sim": ops.dump("sim" + t), "partial": ops.dump("partial" + t)}
    if op == "topk_labels":
        ops.buf("ctl" + t, R.CTL_WORDS * 4)
        for n in ("lab", "idx", "sim"):
            ops.buf(n + t, F * k * 4)
        ops.op("topk_labels", gal, g16, N, D, "q", F, k, "partial" + t, pb, "labels_" + lab, "ctl" + t, "lab" + t, "idx" + t, "sim" + t, off)
        return {"lab": ops.dump("lab" + t), "idx": ops.dump("idx" + t), "sim": ops.dump("sim" + t), "ctl": ops.dump("ctl" + t)}
    assert op == "top1_excl"
    ops.rbuf("excluded" + t, excluded_of(S[:F], labels_of(N, lab)))
    ops.buf("ctl" + t, R.CTL_WORDS * 4)
    ops.buf("ovf" + t, 4)
    ops.buf("idx" + t, F * 4)
    ops.buf("sim" + t, F * 4)
    ops.op("top1_excl", gal, g16, N, D, "q", F, "partial" + t, pb, "labels_" + lab, "excluded" + t, "ctl" + t, "idx" + t, "sim" + t, "ovf" + t)
    return {n: ops.dump(n + t) for n in ("idx", "sim", "ctl", "ovf", "partial")}


def expected(launch, N, S):
    """what the launch must write, from S [130][N] (the similarities it must compute): {output: array}"""
    op, F, pb, off, k, lab = launch
    S = S[:F]
    if op == "top1":
        i, s = ranking(S, 1, off)
        return {"idx": i[:, 0], "sim": s[:, 0]}
    if op == "full":
        return {"out": S}
    if op == "topk":
        i, s = ranking(S, k, off)
        return {"idx": i, "sim": s}
    if op == "topk_labels":
        l, i, s = ranking(S, k, off, labels_of(N, lab), identities=True)
        return {"lab": l, "idx": i, "sim": s}
    labels = labels_of(N, lab)
    i, s = ranking(S, 1, 0, labels, excluded_of(S, labels))
    return {"idx": i[:, 0], "sim": s[:, 0]}


def _check_launch(ops, cid, launch, files, N, S, s64, sabs, D, ratios):
    op, F, pb, off, k, lab = launch
    name = "%s %s F=%d pb=%d off=%d k=%d %s" % (cid, op, F, pb, off, k, lab or "")
    dtypes = {"idx": np.int32, "lab": np.int32, "sim": np.float32, "out": np.float32}
    want = expected(launch, N, S)
    got = {n: ops.read(files[n], dtypes[n]) for n in want}
    bad = []
    for n in want:
        g, w = got[n], np.ascontiguousarray(want[n])
        if n == "out" and g is not None and g.size == w.size:   # a NaN is compared as a NaN, not by its payload
            nan = np.isnan(w).reshape(-1)
            if (np.isnan(g) != nan).any():
                bad.append("%s out: NaN entries differ from the reference's" % name)
            g, w = np.where(nan, np.float32(0), g), np.where(nan, np.float32(0), w.reshape(-1))
        bad += bit_diff("%s %s" % (name, n), g, w)
    if any(v is None for v in got.values()):
        return bad
    # class B: every similarity written for a live entry against float64, whatever the chain says
    if s64 is not None:
        if op == "full":
            err, bound = np.abs(got["out"].reshape(F, N).astype(np.float64) - s64[:F]), gamma(D) * sabs[:F]
        else:
            idx = got["idx"].reshape(F, -1).astype(np.int64) - off
            live = (idx >= 0) & (idx < N)
            rows = np.where(live, idx, 0)
            qq = np.arange(F)[:, None]
            err = np.where(live, np.abs(got["sim"].reshape(F, -1).astype(np.float64) - s64[:F][qq, rows]), 0.0)
            bound = np.where(live, gamma(D) * sabs[:F][qq, rows], 1.0)
        with np.errstate(invalid="ignore", divide="ignore"):
            ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
        ratio = np.nan_to_num(ratio, nan=np.inf)
        if ratio.max() > 1.0:
            bad.append("%s: a similarity is %.3f x gamma(D) sum |q_k g_k| away from float64" % (name, ratio.max()))
        ratios.append(float(ratio.max()))
    if "partial" in files:
        part = ops.read(files["partial"], np.int32)
        tiles = R.tiles_of(N)
        if part is None or part.size != pb * F * 2:
            bad.append("%s: partials missing" % name)
        elif pb > tiles and (part.reshape(pb, F, 2)[tiles:, :, 1] != -1).any():
            bad.append("%s: a workgroup without a tile left a partial other than -1" % name)
    if "ctl" in files:
        ctl = ops.read(files["ctl"], np.uint8)
        if ctl is None or (ctl != 0x5a).any():
            bad.append("%s: the control words were written by an unscreened launch" % name)
    if "ovf" in files:
        ovf = ops.read(files["ovf"], np.uint8)
        if ovf is None or (ovf != 0x5a).any():
            bad.append("%s: *overflow_out was written by an unscreened launch" % name)
    return bad


def build_scan(ops, cls, half, shapes=((512, N_WORK), (96, N_WORK), (32, N_WORK))):
    """every launcher on the class' data: one case per (D, N), the rows and queries loaded once, every launch on outputs of its own"""
    todo = []
    for D, N in shapes:
        g, q, S, s64, sabs = reference(cls, D, half, N)
        cid = "%s_%s_D%d_N%d" % (cls, "half" if half else "float", D, N)
        ops.case(cid)
        names = _rows_buf(ops, g, half)
        ops.rbuf("q", q)
        done = set()
        for j, launch in enumerate(small_launches(N) if N < 128 else launches(D)):
            files = _emit(ops, names, N, D, launch, "%d" % j, done, S)
            todo.append((cid, launch, files, N, S, s64 if cls == "C" else None, sabs, D))
        ops.end()

    def check():
        bad, ratios = [], {}
        for cid, launch, files, N, S, s64, sabs, D in todo:
            bad += _check_launch(ops, cid, launch, files, N, S, s64, sabs, D, ratios.setdefault(cid, []))
        for cid, r in ratios.items():
            if r:
                print("%s: class B max(err / bound) = %.4f over %d launches" % (cid, max(r), len(r)))
        return R._guards(ops) + bad
    return check


def small_launches(N):
    """N = 1 and N = 2: one ragged tile, k > N"""
    return [("top1", 32, 1, 0, 1, None), ("top1", 33, 3, 1000, 1, None), ("top1", 65, 1, 0, 1, None), ("full", 33, 0, 0, 0, None), ("full", 1, 0, 0, 0, None),
            ("topk", 32, 1, 0, 3, None), ("topk", 65, 2, 1000, 3, None), ("topk_labels", 32, 1, 1000, 3, "seven"), ("topk_labels", 33, 2, 0, 3, "seven"),
            ("top1_excl", 32, 1, 0, 1, "excl"), ("top1_excl", 33, 2, 0, 1, "excl")]


def build_full_big(ops, half):
    """launch_match_full sizes its own grid (512 workgroups): at 515 tiles workgroups 0 - 2 walk two tiles.  F = 33 (NQ 4), D = 32; classes A and C."""
    todo = []
    N, D, F = N_BIG, 32, 33
    for cls in ("A", "C"):
        g, q = (exact_data if cls == "A" else chain_data)(D, half, N)
        q = q[:F]
        cid = "%s_%s_full_N%d" % (cls, "half" if half else "float", N)
        ops.case(cid)
        names = _rows_buf(ops, g, half)
        ops.rbuf("q", q)
        ops.buf("out", F * N * 4)
        ops.op("full", names[0], names[1], N, D, "q", F, "out")
        todo.append((cid, cls, g, q, ops.dump("out")))
        ops.end()

    def check():
        bad = []
        for cid, cls, g, q, fn in todo:
            out = ops.read(fn, np.float32)
            s64 = S64(q, g)
            want = s64.astype(np.float32) if cls == "A" else chain_S(q, g)
            bad += bit_diff(cid + " out", out, want)
            if cls == "C" and out is not None and out.size == want.size:
                ratio = np.abs(out.reshape(F, N).astype(np.float64) - s64) / (gamma(D) * abs_S64(q, g))
                print("%s: class B max(err / bound) = %.4f" % (cid, ratio.max()))
                if not ratio.max() <= 1.0:
                    bad.append("%s: a similarity is %.3f x gamma(D) sum |q_k g_k| away from float64" % (cid, ratio.max()))
        return R._guards(ops) + bad
    return check


# ------------------------------------------------------------------------------------------------ the device merges
MERGE_SHAPES = [(s, n, k) for s in (1, 2, 3, 8) for n in (1, 64, 65, 130) for k in (1, 5, R.TOPK_MAX)]


def merge_lists(shards, n, k, labelled):
    """the lists of tests/test_topk_merge.py / tests/test_identity_merge.py (ties across shards, empty slots), with queries that have no entry in
    any shard; labelled: 3 labels for every other shape (fewer identities than k), else 20"""
    import test_identity_merge
    import test_topk_merge
    r = rng("merge", shards, n, k, labelled)
    if labelled:
        n_labels = 3 if (shards + n + k) % 2 else 20
        lab, idx, sim = test_identity_merge.shard_lists(r, shards, n, k, n_labels)
    else:
        idx, sim = test_topk_merge.random_lists(r, shards, n, k, ties=True)
        lab = None
    for q in range(0, n, 7):   # queries with no entry at all (n = 1: its only query every other shape)
        if n > 1 or (shards + k) % 2:
            idx[:, q], sim[:, q] = -1, NINF
            if labelled:
                lab[:, q] = -1
    return lab, idx, sim


def merge_reference(lab, idx, sim):
    if lab is None:
        from oracle import match
        return match.merge_topk(idx, sim)
    import test_identity_merge
    return test_identity_merge.reference_merge(lab, idx, sim)


def build_merge(ops, labelled):
    todo = []
    for shards, n, k in MERGE_SHAPES:
        lab, idx, sim = merge_lists(shards, n, k, labelled)
        cid = "merge%s_s%d_n%d_k%d" % ("_labels" if labelled else "", shards, n, k)
        ops.case(cid)
        ops.rbuf("idx_all", idx)
        ops.rbuf("sim_all", sim)
        outs = ["idx", "sim"]
        if labelled:
            ops.rbuf("lab_all", lab)
            outs = ["lab"] + outs
        for o in outs:
            ops.buf(o, n * k * 4)
        if labelled:
            ops.op("merge_labels", "lab_all", "idx_all", "sim_all", shards, n, k, "lab", "idx", "sim")
        else:
            ops.op("merge", "idx_all", "sim_all", shards, n, k, "idx", "sim")
        todo.append((cid, lab, idx, sim, [ops.dump(o) for o in outs]))
        ops.end()

    def check():
        bad = []
        for cid, lab, idx, sim, files in todo:
            want = merge_reference(lab, idx, sim)
            for fn, w, what in zip(files, want, ("lab", "idx", "sim") if lab is not None else ("idx", "sim")):
                bad += bit_diff("%s %s" % (cid, what), ops.read(fn, w.dtype), w)
        return R._guards(ops) + bad
    return check


# ------------------------------------------------------------------------------------------------ the groups: one harness process each
SMALL_SHAPES = ((32, 1), (32, 2))
GROUPS = {
    "A_float": lambda ops: build_scan(ops, "A", False),
    "A_half": lambda ops: build_scan(ops, "A", True),
    "C_float": lambda ops: build_scan(ops, "C", False),
    "C_half": lambda ops: build_scan(ops, "C", True),
    "A_small_N": lambda ops: _both(ops, lambda half: build_scan(ops, "A", half, SMALL_SHAPES)),
    "C_small_N": lambda ops: _both(ops, lambda half: build_scan(ops, "C", half, SMALL_SHAPES)),
    "full_515_tiles_float": lambda ops: build_full_big(ops, False),
    "full_515_tiles_half": lambda ops: build_full_big(ops, True),
    "merge": lambda ops: build_merge(ops, False),
    "merge_labels": lambda ops: build_merge(ops, True),
}


def _both(ops, fn):
    checks = [fn(False), fn(True)]
    return lambda: sorted(set(checks[0]() + checks[1]()))
