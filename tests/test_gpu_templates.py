"""The template gallery (frt_matcher_build_templates; include/frt.h "Template gallery"): one row per identity, the
re-normalised sum of the identity's stored rows, plus per identity the member that agrees least with its own template.

The reference for every value is NumPy in float64 on the rows this file generates (for fp16 storage: on those rows rounded to fp16, which is
what the matcher stores).  Tolerances, derived and not tuned (u = 2^-24, the unit roundoff of fp32):
  base case (M <= 8 rows per identity, D <= 512)   2^-19 absolute on templates and min_sim: a sum of M <= 8 terms, a 512-term norm and a
      512-term dot of vectors of norm <= 1 with ||s|| >= 0.7 M each err by at most about (M + D) u relative to values <= 1 in the worst case
      and by about sqrt(M + D) u ~ 1.4e-6 typically; 2^-19 = 1.9e-6.
  other shapes (M = 300, D = 96, D = 1024)         the worst-case bounds themselves, |t_k| <= 1 and ||g|| <= 1: templates (M + D / 2 + 2) u
      (partial sums of M terms, the square root of a D-term sum of squares, one division), min_sim (M + 2 D) u (the template's error
      carried through the dot, plus the dot's own D terms).
Everything that is not a rounded real number - labels, counts, rows, and the answers of the template gallery against a freshly loaded
one - is compared with ==."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
TOL = 2.0 ** -19
PKG = os.path.join(ROOT, "face-recognition-cpp-tensorrt_amd")


# ---------------------------------------------------------------------------------------------------------------- inputs and reference
def make_identities(counts, D, seed, planted_cos=0.6, member_cos=0.95, label_of=lambda i: 3 * i + 5):
    """Unit rows: identity i has counts[i] members at cosine member_cos to its seeded centre, their off-centre parts orthonormal to the centre
    and (while they fit, M < D) to each other; for M >= 3 one seeded member lies at planted_cos instead.  The rows are shuffled so that the
    identities interleave.  -> rows [N, D] float32, labels [N] int32, planted {label: row}"""
    rng = np.random.Generator(np.random.PCG64(seed))
    rows, labels, planted_member = [], [], {}
    for i, M in enumerate(counts):
        basis = np.linalg.qr(rng.standard_normal((D, min(M + 1, D))))[0].T  # orthonormal: centre, then one direction per member
        centre = basis[0]
        p = int(rng.integers(M)) if M >= 3 else -1
        for j in range(M):
            u = basis[1 + j] if 1 + j < len(basis) else None
            if u is None:  # more members than dimensions: a random direction, made orthogonal to the centre
                u = rng.standard_normal(D)
                u -= (u @ centre) * centre
                u /= np.linalg.norm(u)
            c = planted_cos if j == p else member_cos
            rows.append(c * centre + np.sqrt(1 - c * c) * u)
            labels.append(label_of(i))
            if j == p:
                planted_member[label_of(i)] = len(rows) - 1
    perm = rng.permutation(len(rows))
    inv = np.argsort(perm)
    rows = np.ascontiguousarray(np.array(rows)[perm], np.float32)
    labels = np.array(labels, np.int32)[perm]
    return rows, labels, {l: int(inv[r]) for l, r in planted_member.items()}


def stored(rows, fp16):
    """the values the matcher keeps, as float64"""
    return (rows.astype(np.float16) if fp16 else rows).astype(np.float64)


def reference(rows64, labels, row_offset=0):
    """the definition in float64 -> dict(labels, n_rows, T, min_sim, min_row, members, gap); gap = runner-up minus minimum (inf for M == 1)"""
    first = {}
    for r, l in enumerate(labels.tolist()):
        first.setdefault(l, []).append(r)
    out = dict(labels=np.array(list(first), np.int32), members=list(first.values()), T=[], min_sim=[], min_row=[], gap=[])
    out["n_rows"] = np.array([len(m) for m in out["members"]], np.int32)
    for m in out["members"]:
        s = rows64[m].sum(0)
        n = np.sqrt(s @ s)
        t = s / n if n > 0 else np.zeros_like(s)
        sims = rows64[m] @ t
        out["T"].append(t)
        out["min_sim"].append(sims.min())
        out["min_row"].append(m[int(np.argmin(sims))] + row_offset)  # (argmin: the first among equals, and m ascends)
        out["gap"].append(np.partition(sims, 1)[1] - sims.min() if len(m) > 1 else np.inf)
    for k in ("T", "min_sim", "gap"):
        out[k] = np.array(out[k], np.float64)
    out["min_row"] = np.array(out["min_row"], np.int32)
    return out


_CACHE = {}


def base_case(D, fp16):
    """75 identities with 1 + (i mod 8) members: 330 rows.  Computed once per (D, storage) and left unchanged."""
    key = ("base", D, fp16)
    if key not in _CACHE:
        rows, labels, planted = make_identities([1 + (i % 8) for i in range(75)], D, seed=271 + D)
        assert rows.shape == (330, D)
        _CACHE[key] = (rows, labels, planted, reference(stored(rows, fp16), labels))
    return _CACHE[key]


def load(mm, rows, labels, fp16=False, screening=True, row_offset=0):
    mm.setScreening(screening)
    mm.setStorage(fp16)
    mm.init(rows)
    mm.setStorage(False)
    mm.setRowOffset(row_offset)
    if labels is not None:
        mm.set_labels(labels)


def check_outputs(got, ref, rows64, planted, tol_t, tol_sim):
    labels, n_rows, min_sim, min_row, T = got
    assert labels.dtype == np.int32 and np.array_equal(labels, ref["labels"])
    assert n_rows.dtype == np.int32 and np.array_equal(n_rows, ref["n_rows"])
    assert T.dtype == np.float32 and T.shape == ref["T"].shape
    et, es = np.abs(T - ref["T"]).max(), np.abs(min_sim - ref["min_sim"]).max()
    print("templates: max |error| %.3g (bound %.3g)   min_sim: max |error| %.3g (bound %.3g)" % (et, tol_t, es, tol_sim))
    assert et <= tol_t and es <= tol_sim
    for i, m in enumerate(ref["members"]):
        if len(m) >= 3:
            assert ref["gap"][i] >= 0.11, (i, ref["gap"][i])  # the planted member is the minimum by a margin no rounding closes
            assert min_row[i] == ref["min_row"][i] == planted[int(labels[i])], i
        elif len(m) == 2:
            assert min_row[i] in m, i
        else:
            assert min_row[i] == m[0] and abs(min_sim[i] - np.linalg.norm(rows64[m[0]])) <= tol_sim, i


@pytest.fixture(scope="module")
def src(frt):
    m = frt.MatMul(0)
    yield m
    m.close()


@pytest.fixture(scope="module")
def dst(frt):
    m = frt.MatMul(0)
    yield m
    m.close()


@pytest.fixture(scope="module")
def fresh(frt):
    m = frt.MatMul(0)
    yield m
    m.close()


# ---------------------------------------------------------------------------------------------------------------- the definition
@pytest.mark.parametrize("D,fp16", [(512, False), (128, False), (512, True)], ids=["d512_fp32", "d128_fp32", "d512_fp16"])
def test_base_case_matches_the_float64_definition(frt, src, dst, D, fp16):
    rows, labels, planted, ref = base_case(D, fp16)
    load(src, rows, labels, fp16)
    assert src.labels_info() == (75, 8)
    gen = src.generation()
    dgen = dst.generation()
    got = src.buildTemplates(dst, want_templates=True)
    check_outputs(got, ref, stored(rows, fp16), planted, TOL, TOL)
    assert src.generation() == gen and src.m == 330        # the source is only read
    assert dst.generation() != dgen and dst.m == 75 and dst.k == D and dst.labels_info() == (75, 1)
    # the template gallery answers with persons: asked with the templates themselves, each finds itself, under its identity's label
    idx, sim = dst.top1(got[4])
    assert np.array_equal(idx, np.arange(75))
    lab, idx3, _ = dst.topk_labels(got[4], 3)
    assert np.array_equal(lab[:, 0], got[0]) and np.array_equal(idx3[:, 0], np.arange(75))


@pytest.mark.parametrize("fp16", [False, True], ids=["fp32", "fp16"])
def test_an_identity_of_300_rows_among_singletons(frt, src, fp16):
    """more rows than any register-resident path holds: the second read of the rows, and 75 batches of adds in row order"""
    D, M = 512, 300
    rows, labels, planted = make_identities([1, 1, M, 1, 1, 1, 1, 1, 1, 1, 1], D, seed=9)
    ref = reference(stored(rows, fp16), labels)
    load(src, rows, labels, fp16)
    got = src.buildTemplates(None, want_templates=True)
    check_outputs(got, ref, stored(rows, fp16), planted, (M + D / 2 + 2) * U, (M + 2 * D) * U)
    assert got[1].max() == M


@pytest.mark.parametrize("D,fp16", [(96, False), (1024, False), (1024, True)], ids=["d96_fp32", "d1024_fp32", "d1024_fp16"])
def test_widths_that_leave_lanes_idle_or_take_two_column_chunks(frt, src, dst, D, fp16):
    """D = 96: a row ends inside the wave's first 256 columns.  D = 1024: two chunks of 512 columns, the unnormalised sum parked in the output row"""
    rows, labels, planted = make_identities([1 + (i % 8) for i in range(13)], D, seed=40 + D)
    ref = reference(stored(rows, fp16), labels)
    load(src, rows, labels, fp16)
    got = src.buildTemplates(dst, want_templates=True)
    check_outputs(got, ref, stored(rows, fp16), planted, (8 + D / 2 + 2) * U, (8 + 2 * D) * U)
    assert dst.m == 13 and dst.k == D
    assert np.array_equal(dst.top1(got[4])[0], np.arange(13))


def test_zero_sum_gives_a_zero_template(frt, src, dst):
    D = 512
    g = np.random.Generator(np.random.PCG64(5)).standard_normal((2, D)).astype(np.float32)
    g /= np.linalg.norm(g, axis=1, keepdims=True)
    rows = np.ascontiguousarray(np.stack([g[1], g[0], -g[0]]), np.float32)
    load(src, rows, np.array([4, 9, 9], np.int32))
    labels, n_rows, min_sim, min_row, T = src.buildTemplates(dst, want_templates=True)
    assert labels.tolist() == [4, 9] and n_rows.tolist() == [1, 2]
    assert not T[1].any() and min_sim[1] == 0.0 and min_row[1] == 1  # both members agree equally (not at all): the lower row
    assert abs(min_sim[0] - 1.0) <= TOL and min_row[0] == 0 and np.abs(T[0] - g[1].astype(np.float64)).max() <= TOL
    assert dst.m == 2


def test_row_offset_shifts_min_row(frt, src):
    rows, labels, planted, ref = base_case(512, False)
    load(src, rows, labels, row_offset=1000)
    try:
        labels_o, n_rows, min_sim, min_row = src.buildTemplates()
    finally:
        src.setRowOffset(0)
    three = ref["n_rows"] != 2
    assert np.array_equal(min_row[three], ref["min_row"][three] + 1000)
    assert all(r - 1000 in m for r, m in zip(min_row.tolist(), ref["members"]))
    assert np.array_equal(labels_o, ref["labels"]) and np.abs(min_sim - ref["min_sim"]).max() <= TOL


def test_empty_source_leaves_an_empty_destination(frt, src, dst):
    rows, labels, _, _ = base_case(512, False)
    load(dst, rows, labels)
    load(src, np.zeros((0, 512), np.float32), None)
    out = src.buildTemplates(dst, want_templates=True)
    assert [len(o) for o in out] == [0] * 5 and out[4].shape == (0, 512)
    assert dst.m == 0 and dst.labels_info() == (0, 0)
    with pytest.raises(frt.FrtError) as e:
        dst.top1(rows[:1])
    assert e.value.code == frt.FRT_ERR_EMPTY
    dst.gallery_add_labeled(rows[:2], [7, 8])  # an empty gallery of width 512: it takes labelled rows of that width
    assert dst.m == 2 and dst.top1(rows[:2])[0].tolist() == [0, 1]


# ---------------------------------------------------------------------------------------------------------------- dst == a fresh load
def queries_for(T, F, seed):
    """F seeded queries: near-copies of templates spread over the gallery, then random directions"""
    rng = np.random.Generator(np.random.PCG64(seed))
    near = T[np.linspace(0, len(T) - 1, F // 2).astype(np.int64)] + 0.02 * rng.standard_normal((F // 2, T.shape[1]))
    q = np.concatenate([near, rng.standard_normal((F - F // 2, T.shape[1]))])
    return np.ascontiguousarray(q / np.linalg.norm(q, axis=1, keepdims=True), np.float32)


def same_answers(a, b, q):
    for fn in (lambda m: m.top1(q), lambda m: m.topk(q, 3), lambda m: m.topk_labels(q, 3)):
        for x, y in zip(fn(a), fn(b)):
            assert x.dtype == y.dtype and np.array_equal(x.view(np.int32), y.view(np.int32))  # similarities by their bits


def test_destination_answers_like_a_fresh_load_of_the_templates(frt, src, dst, fresh):
    rows, labels, _, _ = base_case(512, False)
    load(src, rows, labels)
    load(dst, rows[:5], None)  # whatever it held before is gone
    labels_o, _, _, _, T = src.buildTemplates(dst, want_templates=True)
    load(fresh, T, labels_o)
    same_answers(dst, fresh, queries_for(T, 40, 77))


def big_case():
    """32 768 + 77 identities with 1 or 2 rows each: the template gallery is large enough to screen (>= 32 768 rows)"""
    if "big" not in _CACHE:
        rng = np.random.Generator(np.random.PCG64(123))
        I, D = 32768 + 77, 512
        centres = rng.standard_normal((I, D)).astype(np.float32)
        owner = np.concatenate([np.arange(I), np.arange(0, I, 2)])  # every second identity has a second row
        rows = centres[owner] + 0.3 * rng.standard_normal((len(owner), D)).astype(np.float32)
        rows /= np.linalg.norm(rows, axis=1, keepdims=True)
        perm = rng.permutation(len(owner))
        _CACHE["big"] = (np.ascontiguousarray(rows[perm], np.float32), owner[perm].astype(np.int32))
    return _CACHE["big"]


@pytest.fixture(scope="module")
def big_src(frt):
    rows, labels = big_case()
    m = frt.MatMul(0)
    load(m, rows, labels)
    yield m
    m.close()


@pytest.mark.parametrize("screening,fp16", [(True, False), (False, False), (True, True)], ids=["screened_int8", "exact_scan", "fp16_storage"])
def test_a_screening_destination_answers_like_a_fresh_load(frt, big_src, dst, fresh, screening, fp16):
    I = 32768 + 77
    assert big_src.labels_info() == (I, 2)
    dst.setScreening(screening)
    dst.setStorage(fp16)  # the destination's OWN storage mode decides how the templates are kept
    try:
        labels_o, n_rows, _, _, T = big_src.buildTemplates(dst, want_templates=True)
        assert dst.m == I and dst.labels_info() == (I, 1) and sorted(set(n_rows.tolist())) == [1, 2]
        assert dst.scanBytes() == I * 512 * (4 if not screening else 2 if fp16 else 1)
        load(fresh, T, labels_o, fp16, screening)
        same_answers(dst, fresh, queries_for(T, 40, 78))
    finally:
        dst.setStorage(False)
        dst.setScreening(True)
        fresh.setScreening(True)


def test_rebuild_after_edits_equals_a_build_from_the_resulting_rows(frt, src, dst, fresh):
    rows, labels, _, _ = base_case(512, False)
    extra, extra_labels, _ = make_identities([2, 1, 3], 512, seed=600, label_of=lambda i: (8, 11, 4000)[i])  # two known labels and a new one
    gone = [0, 17, 18, 200, 329]
    load(src, rows, labels)
    src.buildTemplates(dst)
    src.gallery_add_labeled(extra, extra_labels)
    src.galleryRemove(gone)
    got = src.buildTemplates(dst, want_templates=True)
    keep = np.setdiff1d(np.arange(len(rows) + len(extra)), gone)
    rows2, labels2 = np.concatenate([rows, extra])[keep], np.concatenate([labels, extra_labels])[keep]
    other_src, other_dst = fresh, frt.MatMul(0)
    try:
        load(other_src, rows2, labels2)
        want = other_src.buildTemplates(other_dst, want_templates=True)
        for g, w in zip(got, want):
            assert g.dtype == w.dtype and np.array_equal(g.view(np.int32), w.view(np.int32))
        ref = reference(rows2.astype(np.float64), labels2)
        assert np.array_equal(got[0], ref["labels"]) and np.array_equal(got[1], ref["n_rows"]) and np.abs(got[4] - ref["T"]).max() <= TOL
        same_answers(dst, other_dst, queries_for(got[4], 40, 79))
    finally:
        other_dst.close()


# ---------------------------------------------------------------------------------------------------------------- errors, audit
def test_error_paths_and_the_audit_only_call(frt, src, dst):
    rows, labels, _, ref = base_case(512, False)
    load(src, rows, None)
    with pytest.raises(frt.FrtError) as e:
        src.buildTemplates(dst)
    assert e.value.code == frt.FRT_ERR_INVALID and "no labels" in str(e.value)
    src.set_labels(labels)
    with pytest.raises(frt.FrtError) as e:
        src.buildTemplates(src)
    assert e.value.code == frt.FRT_ERR_INVALID and "same matcher" in str(e.value)
    assert src.m == 330 and src.labels_info() == (75, 8)  # untouched by the refused call
    with_dst = src.buildTemplates(dst, want_templates=True)
    audit = src.buildTemplates(None, want_templates=True)
    for a, b in zip(audit, with_dst):
        assert np.array_equal(a.view(np.int32), b.view(np.int32))
    # every output pointer may be NULL
    assert frt.lib.frt_matcher_build_templates(src._h, None, None, None, None, None, None) == frt.FRT_OK


# ---------------------------------------------------------------------------------------------------------------- the C++ shell
def intern(names):
    table = {}
    return np.array([table.setdefault(n, len(table)) for n in names], np.int32)


def python_answer(frt, mm, tm, rows, names, emb, k):
    """matchTemplates / auditTemplates through the binding: labels interned in first-appearance order, so label i is template row i"""
    mm.init(np.ascontiguousarray(rows, np.float32))
    mm.set_labels(intern(names))
    labels, n_rows, min_sim, min_row = mm.buildTemplates(tm)
    who = list(dict.fromkeys(names))
    assert labels.tolist() == list(range(len(who)))
    idx, sim = tm.topk(emb, k)
    match = [(who[i], float(s)) for i, s in zip(idx[0], sim[0]) if i >= 0]
    return match, [(who[i], int(n_rows[i]), float(min_sim[i]), int(min_row[i])) for i in range(len(who))]


def test_shell_demo_matches_the_python_binding(frt, synth, blobs, tmp_path):
    rpath, _ = blobs("ir")
    exe = str(tmp_path / "template_demo")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "template_demo.cpp"), "-o", exe, os.path.join(PKG, "libfrt.so"), "-Wl,-rpath," + PKG,
                           "-Wl,-rpath,/opt/rocm/lib"])
    N, k = 400, 3
    face = synth.make_frame(11, 112, 112)
    boxes = np.zeros(1, frt.BBOX_DTYPE)
    boxes[0] = (0, 0, 112, 112, 1.0)
    rec = frt.ArcFaceIR50(rpath, 640, 480, (3, 112, 112), 512, 1, 4, 0.65)
    emb = rec.forward(face, boxes).copy()
    rec.close()
    # four faces per user ("u<i % 100>"): user 10 holds the face itself (row 10) and a second photo of it (row 110); user 55 looks alike
    gal = synth.make_gallery(N)
    gal[10] = emb[0]
    gal[110] = synth.make_queries(emb, [0], noise=0.01, seed=1)[0]
    gal[55] = synth.make_queries(emb, [0], noise=0.03, seed=2)[0]
    names = ["u%d" % (i % 100) for i in range(N)]
    (tmp_path / "face.bin").write_bytes(face.tobytes())
    (tmp_path / "gal.bin").write_bytes(gal.tobytes())
    (tmp_path / "emb.bin").write_bytes(emb[0].tobytes())
    (tmp_path / "names.txt").write_text("".join(n + "\n" for n in names))
    out = subprocess.run([exe, rpath, str(tmp_path / "face.bin"), str(tmp_path / "gal.bin"), str(N), str(tmp_path / "names.txt"), str(k),
                          str(tmp_path / "emb.bin")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    got_match, got_audit = [], []
    for l in (l.split() for l in out.stdout.splitlines()):
        if l and l[0] == "step":
            assert len(l) == 3 + 2 * int(l[2])
            got_match.append([(l[3 + 2 * j], float(l[4 + 2 * j])) for j in range(int(l[2]))])
        elif l and l[0] == "audit":
            assert len(l) == 3 + 4 * int(l[2])
            got_audit.append([(l[3 + 4 * j], int(l[4 + 4 * j]), float(l[5 + 4 * j]), int(l[6 + 4 * j])) for j in range(int(l[2]))])
    assert len(got_match) == 3 and len(got_audit) == 3
    # the same three galleries through the Python binding
    mm, tm = frt.MatMul(0), frt.MatMul(0)
    try:
        want = [python_answer(frt, mm, tm, gal, names, emb, k)]
        rows = np.concatenate([gal, emb[:1], gal[7:8]])
        who = names + [names[55], "zed"]
        want.append(python_answer(frt, mm, tm, rows, who, emb, k))
        keep = [i for i, n in enumerate(who) if n != names[10]]
        want.append(python_answer(frt, mm, tm, rows[keep], [who[i] for i in keep], emb, k))
    finally:
        mm.close()
        tm.close()
    for step, (gm, ga, (wm, wa)) in enumerate(zip(got_match, got_audit, want)):
        assert [n for n, _ in gm] == [n for n, _ in wm], step
        assert np.abs(np.array([s for _, s in gm]) - np.array([s for _, s in wm])).max() < 1e-5, step  # (the shell embeds the face itself)
        assert [(n, r, row) for n, r, _, row in ga] == [(n, r, row) for n, r, _, row in wa], step
        assert np.array_equal(np.array([s for _, _, s, _ in ga], np.float32), np.array([s for _, _, s, _ in wa], np.float32)), step
    assert got_match[0][0][0] == names[10] and got_match[2][0][0] == names[55]
    assert len(got_audit[0]) == 100 and len(got_audit[1]) == 101 and len(got_audit[2]) == 100 and got_audit[1][-1][0] == "zed"
