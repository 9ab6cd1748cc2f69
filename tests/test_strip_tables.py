"""The strip tables of the recogniser's strip convs (strip_tables, csrc/kernels_arc.hip; layout: csrc/frt_kernels.h, "Strip tables"), without a GPU.
tests/cpp/strip_tables_dump.cpp (host code against libfrt.so) prints the tables of every strip geometry the dispatch reaches over the launch
space of tests/golden/arc_conv_plan.txt.  Here

  * every integer is compared with a restatement of the rules in plain integer // and %: the compact strip (nt * 32 consecutive pixels of the
    flattened index, a window of the STACKED images - H rows and one zero separator row per image - with patch pixel 0 the zero pixel), the
    padded strip (R rows of n_img images with one halo column each side, slots enumerated over the padded row width when `linear`);
  * the kernel's use of them is replayed for B = the first batch that reaches the geometry, first + 1, 128 and 256, with the kernel's one
    batch-dependent liveness rule (pixel index < B * H * W): every live DMA entry points inside the logical tensor, every pixel of the patch
    window is staged exactly once (eight 16-byte pieces, the ninth piece of a patch row is padding), every tap of every live output pixel
    reads the patch row that holds its input pixel - or a zero row outside the image - and the output pixels of all strips of the launch
    cover [0, B * H * W) exactly once."""
import subprocess

import numpy as np
import pytest

from launch_harness import build

PROW = 144  # bytes per patch pixel row in LDS


@pytest.fixture(scope="module")
def dumped(tmp_path_factory):
    exe = build(tmp_path_factory.mktemp("strip_tables"), "strip_tables_dump")
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    geoms, lines, i = [], out.stdout.splitlines(), 0
    while i < len(lines):
        head = lines[i].split()
        assert head[0] == "geom"
        v = [int(x) for x in head[1:]]
        g = dict(zip("H W compact linear nt R n_img nslot threads first last period ppx stride".split(), v))
        rows = [np.array(lines[i + 1 + k].split(), dtype=np.int64) for k in range(g["period"])]
        assert all(len(r) == g["stride"] for r in rows)
        geoms.append((g, np.stack(rows)))
        i += 1 + g["period"]
    return geoms


def restate(g):
    """(period, ppx, [period][stride]) from the rules, integer arithmetic only."""
    H, W, NT, R, T, nslot, n_img = g["H"], g["W"], g["nt"], g["R"], g["threads"], g["nslot"], g["n_img"]
    P, S = H * W, NT * 32
    if g["compact"]:
        period = np.lcm(P, S) // S
        ppx = period * S
    else:
        period = (H + R - 1) // R
        ppx = n_img * P
    stride = nslot * T + NT * 64 + (NT * 4 if g["compact"] else NT * 32)
    out = np.full((period, stride), -1, np.int64)
    piece = np.arange(nslot * T)  # DMA slot q of thread t stages 16-byte piece q * T + t of the patch image
    prow, pos = piece // 9, piece % 9
    lane = np.arange(64)
    for sp in range(period):
        if g["compact"]:
            m_lo = sp * S  # first pixel of the strip, in the period
            top = (m_lo // P) * (H + 1) + (m_lo % P) // W - 1  # stacked row of patch row 0: one above the first pixel's
            pp = prow - 1  # patch pixel 0 is the zero pixel
            sr = top + pp // W
            live = (pos < 8) & (pp >= 0) & (pp // W < R) & (sr >= 0) & (sr % (H + 1) < H)
            out[sp, :nslot * T] = np.where(live, ((sr // (H + 1)) * H + sr % (H + 1)) * W + pp % W, -1)
            for j in range(NT):
                m = m_lo + j * 32 + (lane & 31)
                srow = (m // P) * (H + 1) + (m % P) // W
                col = (m % P) % W
                own = 1 + (srow - top) * W + col  # the patch pixel that holds the slot's own input pixel; tap (0, 0) reads one row up, one column left
                out[sp, nslot * T + j * 64:nslot * T + (j + 1) * 64] = (own - W - 1) * PROW + (lane >> 5) * 16
                for k, c in enumerate((0, W - 1)):
                    bits = sum(1 << int(l) for l in lane if col[l] == c)
                    for half, word in enumerate((bits & 0xffffffff, bits >> 32)):  # two's complement ints, low word first
                        out[sp, nslot * T + NT * 64 + 4 * j + 2 * k + half] = word - (1 << 32) if word >= 1 << 31 else word
        else:
            Wp, row0 = W + 2, sp * R
            patch_px = (R + 2) * Wp
            il, rem = prow // patch_px, prow % patch_px
            iy, ix = row0 + rem // Wp - 1, rem % Wp - 1
            live = (pos < 8) & (il < n_img) & (iy >= 0) & (iy < H) & (ix >= 0) & (ix < W)
            out[sp, :nslot * T] = np.where(live, (il * H + iy) * W + ix, -1)
            sl = np.arange(S)
            if g["linear"]:  # slot = patch row of tap (0, 0); slots in the two halo columns and past the strip's rows are dead
                pidx = np.where(sl < R * Wp, sl, 0)
                rr, cc = sl // Wp, sl % Wp
                eoff = np.where((rr < R) & (row0 + rr < H) & (cc < W), (row0 + rr) * W + cc, -1)
            else:  # slots are the pixels of the n_img * R rows in order
                valid = sl < n_img * R * W
                i2, r2 = sl // (R * W), sl % (R * W)
                pidx = np.where(valid, (i2 * (R + 2) + r2 // W) * Wp + r2 % W, 0)
                eoff = np.where(valid, row0 * W + sl, -1)
            for j in range(NT):
                out[sp, nslot * T + j * 64:nslot * T + (j + 1) * 64] = pidx[j * 32 + (lane & 31)] * PROW + (lane >> 5) * 16
            out[sp, nslot * T + NT * 64:] = eoff
    return period, ppx, out


def test_every_geometry_of_the_plan_is_dumped(dumped):
    keys = {(g["H"], g["compact"], g["nt"]) for g, _ in dumped}
    # the full-batch kernels of the headline step and the padded strips of the 28x28 and 56x56 layers
    assert {(14, 1, 7), (7, 1, 4), (28, 0, 7), (56, 0, 7)} <= keys, keys


def test_tables_match_the_restated_rules(dumped):
    for g, tab in dumped:
        period, ppx, want = restate(g)
        assert (period, ppx) == (g["period"], g["ppx"]), g
        assert want.shape == tab.shape, g
        ne = np.argwhere(want != tab)
        assert len(ne) == 0, "%s: %d entries differ, first at [position, index] = %s: %d, restated %d" % (g, len(ne), ne[0], tab[tuple(ne[0])], want[tuple(ne[0])])
    # the periods the layout's description names
    per = {(g["H"], g["nt"]): (g["period"], g["ppx"] // (g["H"] * g["W"])) for g, _ in dumped if g["compact"]}
    assert per[(14, 7)] == (7, 8) and per[(7, 4)] == (49, 128)


def _replay(g, tab, B):
    H, W, NT, R, T, nslot, n_img = g["H"], g["W"], g["nt"], g["R"], g["threads"], g["nslot"], g["n_img"]
    P, S, M = H * W, NT * 32, B * H * W
    period, ppx = g["period"], g["ppx"]
    Wp = W if g["compact"] else W + 2
    n_strips = (M + S - 1) // S if g["compact"] else ((B + n_img - 1) // n_img) * period
    n_per = (n_strips + period - 1) // period
    o_pb, o_tail = nslot * T, nslot * T + NT * 64
    piece = np.arange(nslot * T)
    n_rows = (nslot * T + 8) // 9
    covered = np.zeros(M, np.int64)
    for s in range(n_strips):
        k, sp = s // period, s % period
        off = k * ppx
        # ---- output pixels of the strip (the epilogue's rule)
        sl = np.arange(S)
        if g["compact"]:
            m = s * S + sl
            out_live = m < M
        else:
            e = tab[sp, o_tail:o_tail + S]
            m = off + e
            out_live = (e >= 0) & (m < M)
        assert (m[out_live] >= 0).all()
        np.add.at(covered, m[out_live], 1)
        if k not in (0, n_per - 2, n_per - 1):
            continue  # the tables repeat: the first period and the two around the end of the batch are replayed in full
        # ---- the patch image the DMAs stage (the prologue's rule): entry -> pixel, live iff inside the batch
        ent = tab[sp, :nslot * T]
        px = np.where((ent >= 0) & (ent + off < M), ent + off, -1)
        assert (px < M).all() and ((px >= 0) | (px == -1)).all()
        rows = np.full((n_rows, 9), -1, np.int64)
        rows[piece // 9, piece % 9] = px
        assert (rows[:, 8] == -1).all(), (g, s, "the ninth piece of a patch row is padding")
        assert (rows[:, :8] == rows[:, :1]).all(), (g, s, "the eight pieces of a patch row belong to one pixel")
        held = rows[:, 0]
        livepx = held[held >= 0]
        assert len(np.unique(livepx)) == len(livepx), (g, s, "a pixel is staged twice")
        # ---- every tap of every live output pixel reads its input pixel, or zeros outside the image
        pb = tab[sp, o_pb:o_pb + NT * 64].reshape(NT, 64)
        assert (pb[:, 32:] == pb[:, :32] + 16).all() and (pb[:, :32] % PROW == 0).all()
        pidx = (pb[:, :32] // PROW).reshape(-1)  # per slot
        if g["compact"]:
            pidx = np.where(s * S + sl < M, pidx, 0)  # the kernel points slots behind the batch at the zero pixel
            masks = tab[sp, o_tail:o_tail + 4 * NT].astype(np.uint32).reshape(NT, 2, 2)
            assert (masks[:, :, 0] == masks[:, :, 1]).all(), "a mask's two lane halves belong to the same 32 slots"
            bit = lambda which: ((masks[:, which, 0][:, None] >> np.arange(32, dtype=np.uint32)[None, :]) & 1).reshape(-1).astype(bool)
            first_col, last_col = bit(0), bit(1)
        b, y, x = m // P, (m % P) // W, (m % P) % W
        for kh in range(3):
            for kw in range(3):
                row = pidx + kh * Wp + kw
                if g["compact"]:
                    row = np.where((first_col if kw == 0 else last_col) if kw != 1 else False, 0, row)
                assert (row[out_live] >= 0).all() and ((row[out_live] + 1) * PROW <= nslot * T * 16).all()
                yy, xx = y + kh - 1, x + kw - 1
                inside = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
                want = np.where(inside, (b * H + yy) * W + xx, -1)
                got = held[np.where(out_live, row, 0)]
                bad = out_live & (got != want)
                assert not bad.any(), (g, "B", B, "strip", s, "tap", (kh, kw), "slot", int(np.argwhere(bad)[0]), int(got[bad][0]), int(want[bad][0]))
    assert (covered == 1).all(), (g, B, "output pixels covered %d..%d times" % (covered.min(), covered.max()))


def test_replay_of_the_kernel_rules(dumped):
    for g, tab in dumped:
        for B in sorted({g["first"], min(g["first"] + 1, 256), 128, 256}):
            # (a compact geometry's window height R is the worst case of the batches that plan it: replayed inside that range only)
            if not g["compact"] or g["first"] <= B <= g["last"]:
                _replay(g, tab, B)
