"""Every op of the mnet0.25 detector, ALONE, against float64 (reference and bounds: tests/det_op_ref.py; the program that runs them:
tests/cpp/det_op_check.cpp, which launches op i through frt_detector::run_op - the call forward() makes).  The network-level tests see these
kernels through 23 launches and a softmax; here each op runs on its predecessor's reference output:
  * every output element is inside the error bound derived in det_op_ref's docstring; max(err / bound) is printed per (op, batch);
  * no word outside the op's logical output has changed: frame slot B of every buffer (the detector is created with max_batch = B + 1),
    the other channels of the SSH concat, every other buffer, the op's own inputs;
  * the op list the harness dumps is the reference's network: kinds, dimensions, and the graph rebuilt from the device addresses.
One harness process per (blob, geometry, batch), each under its own timeout (17 cases with Slim and RFB below).  A process that ends on a HIP error, a signal or the timeout
ends the module: the remaining parameters fail with its message and launch nothing.

Cases, from the dispatch (B = frames per call; "|" = a threshold between two of the batches run).  640x640, B = 1, 2, 3, 6, 12:
  op  shape                  kernel by batch                                                                    threshold (file: function)
  0   3->8 /2                conv3x3_kernel<8> (no split weights: Cout < 16)                                    kernels_det.hip: launch_conv3x3_multi
  1   8->16 @320             dwpw_row4_kernel<16, 2> (launch_dwpw_mfma declines Cin, Cout <= 32 at stride 1)    kernels_det.hip: launch_dwpw
  2   16->32 /2 @160         dwpw_mfma_kernel<4, 1, 16, 1, 2, 2-D> (fp32 MFMA)                                  kernels_det_mfma.hip: launch_dwpw_mfma
  3   32->32 @160            dwpw_pixs_kernel<16, 4> B <= 2 | <32, 2> B <= 5 | dwpw_row4_kernel<32, 2, MF>      launch_dwpw: blocks <= 256 / <= 512
  4   32->64 /2 @80          dwpw_mfma_kernel<2, 2, 32, .., SPLIT> (one chunk: PRE = 0)                         launch_fused
  5   64->64 @80             dwpw_mfma_kernel<2, 2, 32, .., SPLIT, PRE 2> B <= 2 | dwpw_wave_kernel<64, 64>     kernels_det_wave.hip: launch_dwpw_wave, B >= 3
  6   64->128 /2 @40         dwpw_mfma_kernel<1, 4, 32, .., SPLIT, PRE 2> B <= 5 | PRE 0                        launch_fused: nblocks * cgroups <= 256
  7-11 128->128 @40          ..<1, 4, 32, .., SPLIT, PRE 4> B <= 5 | PRE 0 B <= 11 | dwpw_wave_kernel<128, 128> launch_fused; launch_dwpw_wave, B >= 12
  12  128->256 /2 @20        ..<1, 2, 32, 1, .., PRE 4> B <= 5 | <1, 4, 32, 2, .., PRE 4>                       launch_dwpw_mfma: total <= 2048
  13  256->256 @20           as 12 up to B = 11 | dwpw_wave_kernel<256, 256>                                    launch_dwpw_wave, B >= 12
  14, 15  1x1 256 / 128->64  pw_mfma_kernel<1, true>                                                            launch_dwpw_mfma: n_pix_groups >= 2048
  17  1x1 64->64 @80 + add   pw_mfma_kernel<1, true> B <= 10 | pw_mfma_kernel<2, true>                          the same (200 pixel groups per frame)
  16, 18  3x3 64->64         conv3x3_split_kernel<4, 1> x 2 channel groups; op 18: B <= 7 | <4, 2>              kernels_det_conv3h.hip: launch_conv3x3_split, base <= 384
  19  3x3 64->32+16, 3 lv    conv3x3_split_kernel<4, 1> x 2 B <= 5 | <4, 2>                                     the same (71 tiles per frame)
  20, 21  3x3 16->32 / 16    conv3x3_split_kernel<1, 1>
  22  heads                  heads_kernel<16>
  u8  frames = input         det_conv1_u8_kernel (op 0); det_stem_kernel (ops 0 - 2) at every batch             launch_det_stem
100x172 (maps 50x86, 25x43, 13x22, 7x11, 4x6; B = 1, 2, 6): no map is a multiple of 4 wide, so launch_dwpw_mfma declines every conv_dw block
and the scalar kernels run - dwpw_kernel<16, true, 1> (op 1), <32, true, 1> (op 2), dwpw_pixs_kernel<16, 4> (op 3), dw_kernel +
dwpw_kernel<32, false, 1> (ops 4 - 13); the 1x1 convs and the 3x3 convs stay on pw_mfma_kernel<1, true> / conv3x3_split_kernel with ragged
tiles, and the nearest upsample 4 -> 7 -> 13 is not 2x.  101x173, frames = input: det_conv1_u8_kernel's odd right edge at B = 1 and 2
(launch_det_stem declines: the 26x44 output is not 8x8-tileable), every op once more on odd maps.  det_ldm at 100x172, B = 2: the landmark head.
The kernels each case actually ran are recorded from a kernel trace in profiles/det_ops/ ("Detector ops one at a time").

96x160, frames = input (maps 48x80, 24x40, 12x20, 6x10, 3x5; B = 1, 3): maps of 4-pixel segments that are no multiple of the kernels' tiles - op 2 on
the linear-tile fp32 MFMA variant dwpw_mfma_kernel<4, 1, 16, 1, 2, false, false, 0> (960 pixels in tiles of 128), ops 4 and 5 on the split
dwpw_mfma_kernel with a ragged last tile (240 pixels in tiles of 64), from op 6 (Wo = 10) the scalar kernels again, det_stem_kernel where
most tiles are ring tiles.

Range edges: merge1 (3x3 split), the 64 -> 64 conv_dw block (op 5) and the 64 -> 64 lateral run twice more at 640x640, B = 2 and 3 (op 5: on
dwpw_mfma_kernel at B = 2 and on dwpw_wave_kernel with its fragment-order weights at B = 3), and the two without a depthwise stage at 100x172, B = 2, on their own input times a power of two: once with the largest value
entering the hi / lo split in [2^14, 2^15), once with the largest input in [2^-20, 2^-19), where every hi is a subnormal fp16 number.  The same
bound holds.  (A conv_dw block splits its depthwise output, relu(w x + b): scaling the input down leaves the bias, so its low case only shows
that tiny inputs do no harm.)

The softmax allowance of the heads is measured, not derived: the largest |conf - float64 reference| seen on an MI355X is 4.19e-7 (640x640,
frame 0, level 0, the same at B = 1 .. 12; 2.0e-7 .. 3.3e-7 at the other geometries); det_op_ref allows 4 x that, 1.68e-6, on top of the
derived part.  Largest max(err / bound) seen over all cases: 0.56 (the 64 -> 64 lateral on inputs near 2^-20, where the 2^-25 term is
the whole bound), 0.21 for the first conv, below 0.18 everywhere else - with the fp32 kernels held to the fp32 bound (16 roundings per group
of 16 channels, no hi / lo terms) and only the launches that det_op_ref.runs_split names to the split kernels' bound."""
import os
import shutil

import numpy as np
import pytest

import det_op_ref as R
from launch_harness import Runner, build, read_results

GEOM = {"640x640": (640, 640), "100x172": (100, 172), "101x173": (101, 173), "96x160": (96, 160)}
# (blob, geometry, B, run the u8 launchers, range-edge ops)
CASES = [("det", "640x640", B, True, ("conv3", "dwpw", "pw") if B in (2, 3) else ()) for B in (1, 2, 3, 6, 12)]
CASES += [("det", "100x172", B, False, ("conv3", "pw") if B == 2 else ()) for B in (1, 2, 6)]
CASES += [("det", "101x173", 1, True, ()), ("det", "101x173", 2, True, ()), ("det_ldm", "100x172", 2, False, ())]
CASES += [("det", "96x160", B, True, ()) for B in (1, 3)]
MAX_B = {("det", "640x640"): 12, ("det", "100x172"): 6, ("det", "101x173"): 2, ("det_ldm", "100x172"): 2, ("det", "96x160"): 3}

_runner = Runner()
_refs = {}  # (blob, geometry) -> (frames, x, net, ops, cache) for the largest batch of the geometry, computed once


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return build(tmp_path_factory.mktemp("det_op_check"), "det_op_check", opt="-O2")


def _reference(synth, blobs, blob, geom):
    if (blob, geom) not in _refs:
        h, w = GEOM[geom]
        frames = synth.make_frames(MAX_B[(blob, geom)], h, w)  # a different frame per batch slot: a batch-index error cannot cancel
        x = R.preprocess(frames)
        net, ops = R.forward(blobs(blob)[1], x)
        for i in R.split_ops(ops):  # otherwise the comparison below means nothing
            assert all(0 < p.rng[0] < 65504 for p in ops[i].probs), i
        _refs[(blob, geom)] = (frames, x, net, ops, {})
    return _refs[(blob, geom)]


def _parse_oplist(path):
    ops = {}
    for line in open(path).read().splitlines():
        t = line.split()
        assert t[0] == "op" and t[3] == "p", line
        ops.setdefault(int(t[1]), (t[2], []))[1].append({k: int(v) for k, v in (kv.split("=") for kv in t[5:])})
    return ops


def _check_topology(listed, ops, geom, landmarks):
    """The dumped op list against the reference's network: kinds, dimensions, and the graph rebuilt from the addresses."""
    bad = []
    if sorted(listed) != list(range(R.N_OPS)):
        return ["the op list has ops %s" % sorted(listed)]
    addr = {}
    for i, (kind, probs) in sorted(listed.items()):
        ref = ops[i]
        if kind != ref.kind or len(probs) != len(ref.probs):
            bad.append("op %d: %s with %d problems, reference %s with %d" % (i, kind, len(probs), ref.kind, len(ref.probs)))
            continue
        for k, (d, p) in enumerate(zip(probs, ref.probs)):
            got = (d.get("Cin", d.get("C")), d["H"], d["W"])
            if got != tuple(p.dims):
                bad.append("op %d p%d: input %s, reference %s" % (i, k, got, p.dims))
            if kind != "heads":
                o = p.out.shape[1:]
                cout = d["Cout"] if kind == "dwpw" else d["split"]
                if (cout, d["Ho"], d["Wo"]) != tuple(o):
                    bad.append("op %d p%d: output %s, reference %s" % (i, k, (cout, d["Ho"], d["Wo"]), o))
                addr[(i, "out", k)] = (d["out"], d.get("out_coff", 0))
                if p.out2 is not None:
                    if (d["Cout"] - d["split"], d["out2_coff"]) != (p.out2.shape[1], 0) or not d["out2"]:
                        bad.append("op %d p%d: second output %d channels" % (i, k, d["Cout"] - d["split"]))
                    addr[(i, "out2", k)] = (d["out2"], d["out2_coff"])
                elif d.get("out2"):
                    bad.append("op %d p%d: a second output the reference does not have" % (i, k))
                if d["relu"] != 1 or d["stride"] != (1 if p.out.shape[2] == p.dims[1] else 2):
                    bad.append("op %d p%d: stride %d, relu %d" % (i, k, d["stride"], d["relu"]))
            if i > 0 and i < 22 and d["in"] != addr[p.src][0]:
                bad.append("op %d p%d reads %d, not the output of op %d (%d)" % (i, k, d["in"], p.src[0], addr[p.src][0]))
            if kind == "dwpw":
                want = addr[p.add_src][0] if p.add_src else 0
                if d["add"] != want or (want and (d["add_h"], d["add_w"]) != tuple(p.add.shape[2:])):
                    bad.append("op %d: add source %d (%d x %d), reference %d" % (i, d["add"], d["add_h"], d["add_w"], want))
    for k in range(3):  # the concat: ops 19, 20, 21 write channels 0, 32, 48 of the tensor the heads read
        cat = [addr[(19, "out", k)], addr[(20, "out", k)], addr[(21, "out", k)]]
        if [c[1] for c in cat] != [0, 32, 48] or len({c[0] for c in cat}) != 1 or listed[22][1][k]["in"] != cat[0][0]:
            bad.append("level %d: the SSH concat is %s, the heads read %d" % (k, cat, listed[22][1][k]["in"]))
    tensors = [a[0] for key, a in addr.items() if not (key[0] in (20, 21) and key[1] == "out")]
    if len(set(tensors)) != len(tensors):
        bad.append("two tensors of the network share an address")
    h, w = GEOM[geom]
    base = 0
    for k, d in enumerate(listed[22][1]):
        fh, fw = -(-h // (8 << k)), -(-w // (8 << k))
        if (d["H"], d["W"], d["base"], bool(d["ldm"])) != (fh, fw, base, landmarks):
            bad.append("heads level %d: %s" % (k, d))
        base += fh * fw * 2
    if listed[22][1][0]["A"] != base:
        bad.append("heads: A = %d, the anchor table has %d" % (listed[22][1][0]["A"], base))
    return bad


def _compare(name, got, ref, bound, ratios):
    """Failure messages ([] = inside the bound everywhere); the ratio goes to `ratios`."""
    if got.shape != ref.shape:
        return ["%s: shape %s, reference %s" % (name, got.shape, ref.shape)]
    err = np.abs(got.astype(np.float64) - ref)
    ratios[name] = float(np.nanmax(err / bound)) if not np.isnan(err).all() else float("nan")
    ok = err <= bound  # (a NaN is not)
    if ok.all():
        return []
    i = tuple(int(v) for v in np.argwhere(~ok)[0])
    return ["%s: %d of %d values outside the bound, first at %s: %r, reference %r, bound %.3g" % (name, (~ok).sum(), ok.size, i, float(got[i]), float(ref[i]), float(bound[i]))]


def _edge_scale(net, op, p, B, which):
    """The power of two that puts the largest value entering the split of op into [2^14, 2^15) ('hi'), or the largest input into [2^-20, 2^-19) ('lo')."""
    x = np.asarray(p.inp[:B], np.float64)
    if which == "lo":
        return -20 - int(np.floor(np.log2(np.abs(x).max())))
    k = 14 - int(np.floor(np.log2(p.rng[0])))
    for _ in range(8):
        m = net.run(op.index, [x * 2.0 ** k], [None if p.add is None else p.add[:B]])[0][4][0]
        if 2.0 ** 14 <= m < 2.0 ** 15:
            return k
        k += 1 if m < 2.0 ** 14 else -1
    raise AssertionError("no power of two puts the split input of op %d into [2^14, 2^15)" % op.index)


def prepare(wd, blob_path, refs, geom, B, u8, edges):
    """Writes the work directory of one harness process (tests/cpp/det_op_check.cpp); returns the references of the range-edge runs."""
    frames, x, net, ops, _ = refs
    h, w = GEOM[geom]
    shutil.copy(blob_path, os.path.join(wd, "blob.frtw"))
    extra, edge_ref = [], {}
    for op in ops:
        for k, p in enumerate(op.probs):
            p.inp[:B].tofile(os.path.join(wd, "op%d.p%d.in" % (op.index, k)))
            if p.add is not None:
                p.add[:B].tofile(os.path.join(wd, "op%d.p%d.add" % (op.index, k)))
    for fam in edges:
        op = ops[R.FAMILY_OPS[fam]]
        p = op.probs[0]
        for which in ("hi", "lo"):
            k = _edge_scale(net, op, p, B, which)
            scaled = np.ascontiguousarray(p.inp[:B] * np.float32(2.0 ** k))
            assert np.array_equal(scaled.astype(np.float64), p.inp[:B].astype(np.float64) * 2.0 ** k)  # exact: no fp32 underflow or overflow
            scaled.tofile(os.path.join(wd, "op%d.p0.in.%s" % (op.index, which)))
            res = net.run(op.index, [scaled], [None if p.add is None else p.add[:B]])[0]
            assert res[4][0] < 65504
            edge_ref[(op.index, which)] = res
            extra.append("%d %s" % (op.index, which))
            print("op %d %s: input x 2^%d, largest value entering the split %.4g, smallest non-zero %.3g" % (op.index, which, k, res[4][0], res[4][1]))
    if u8:
        frames[:B].tofile(os.path.join(wd, "frames.u8"))
    with open(os.path.join(wd, "job.txt"), "w") as f:
        f.write("%d %d %d %d %d %d\n%s\n" % (w, h, h, w, B, int(u8), "\n".join(extra)))
    return edge_ref


@pytest.mark.gpu
@pytest.mark.parametrize("blob,geom,B,u8,edges", CASES, ids=["%s-%s-B%d" % c[:3] for c in CASES])
def test_det_ops_alone(blob, geom, B, u8, edges, harness, synth, blobs, tmp_path):
    _runner.require_running()
    refs = _reference(synth, blobs, blob, geom)
    frames, x, net, ops, cache = refs
    h, w = GEOM[geom]
    work = tmp_path / "ops"
    work.mkdir()
    wd = str(work)
    try:
        edge_ref = prepare(wd, blobs(blob)[0], refs, geom, B, u8, edges)
        _runner.run(harness, wd, "%s %s B = %d" % (blob, geom, B), 120)
        failures, ratios = [], {}
        results = {name: cols[0] for name, cols in read_results(wd).items()}
        if os.path.exists(os.path.join(wd, "oplist.txt")):
            listed = _parse_oplist(os.path.join(wd, "oplist.txt"))
            failures += _check_topology(listed, ops, geom, net.landmarks)
        else:
            failures.append("no op list")
        rd = lambda name, shape: np.fromfile(os.path.join(wd, name), np.float32).reshape(shape)
        for name, changed in results.items():
            if changed not in ("0", "n/a"):
                failures.append("%s: %s words outside the logical output changed" % (name, changed))
        for op in ops:
            name = "op%d" % op.index
            if name not in results:
                failures.append(name + ": not reached")
                continue
            if op.kind == "heads":
                A = sum(p.out[0].shape[1] for p in op.probs)
                for hi, (what, per) in enumerate((("loc", 4), ("conf", 2), ("ldm", 10))[:len(op.probs[0].out)]):
                    got = rd("%s.%s" % (name, what), (B, A, per))
                    want = np.concatenate([p.out[hi] for p in op.probs], 1)[:B]
                    bound = np.concatenate([p.bound[hi] for p in op.probs], 1)[:B]
                    failures += _compare("%s.%s" % (name, what), got, want, bound, ratios)
                    if what == "conf":
                        print("%s: max |conf - reference| = %.3g" % (name, np.abs(got - want).max()))
                continue
            for k, p in enumerate(op.probs):
                failures += _compare("%s.p%d.out" % (name, k), rd("%s.p%d.out" % (name, k), (B,) + p.out.shape[1:]), p.out[:B], p.bound[:B], ratios)
                if p.out2 is not None:
                    failures += _compare("%s.p%d.out2" % (name, k), rd("%s.p%d.out2" % (name, k), (B,) + p.out2.shape[1:]), p.out2[:B], p.bound2[:B], ratios)
        for (i, which), res in edge_ref.items():
            name = "op%d.%s" % (i, which)
            if name not in results:
                failures.append(name + ": not reached")
                continue
            failures += _compare("op%d.p0.out.%s" % (i, which), rd("op%d.p0.out.%s" % (i, which), res[0].shape), res[0], res[1], ratios)
        if u8:
            if results.get("u8conv") == "0":
                p = ops[0].probs[0]
                failures += _compare("u8conv.out", rd("u8conv.out", (B,) + p.out.shape[1:]), p.out[:B], p.bound[:B], ratios)
            else:
                failures.append("launch_det_conv1_u8 did not run: %r" % results.get("u8conv"))
            # Where launch_det_stem must run, so that a silent decline cannot pass.  This restates the launcher's own condition
            # (kernels_det_stem.hip: launch_det_stem - even H and W, op 2's output a whole number of 8x8 tiles, at least 3 x 3 of them):
            # a change there has to be made here too.
            tileable = h % 32 == 0 and w % 32 == 0 and h >= 96 and w >= 96
            if tileable != (results.get("u8stem") not in (None, "n/a")):
                failures.append("launch_det_stem: %r on a %d x %d input" % (results.get("u8stem"), h, w))
            elif tileable:
                if "stem" not in cache:
                    cache["stem"] = R.stem_chain(net, x)
                failures += _compare("u8stem.out", rd("u8stem.out", (B,) + cache["stem"][0].shape[1:]), cache["stem"][0][:B], cache["stem"][1][:B], ratios)
        for name in sorted(ratios, key=lambda n: (int(n[2:].split(".")[0]) if n[2].isdigit() else 99, n)):
            print("%s %s B=%d %s: max(err / bound) = %.3f" % (blob, geom, B, name, ratios[name]))
        _runner.require_ended_well()
        assert not failures, "%d failures:\n%s" % (len(failures), "\n".join(failures[:40]))
    finally:
        shutil.rmtree(wd, ignore_errors=True)


# ------------------------------------------------------------------------------------------------ Slim and RFB
# Same harness, the float64 restatement of tests/det_slim_op_ref.py (checked against tests/slim_ref.py's network by tests/test_det_op_ref.py).
# One geometry, 100x172 (maps 50x86, 25x43, 13x22, 7x11, 4x6, 2x3): every conv_dw block on the scalar kernels, the heads of levels 0 - 2 and the
# dense head of level 3 writing their own anchor ranges of d_loc / d_conf / d_ldm (every other anchor must keep the sentinel), RFB's conv8 as its
# five launches on channel slices.  B = 1 and 3.
SENTINEL = 0x7149f2ca
SLIM_CASES = [(rfb, B) for rfb in (False, True) for B in (1, 3)]
_slim_refs = {}


def _slim_reference(frt, synth, tmp_path_factory, rfb):
    import det_slim_op_ref as S
    if rfb not in _slim_refs:
        sd = synth.slim_state(5, rfb=rfb)
        kind = frt.weights_io.KIND_RETINAFACE_RFB if rfb else frt.weights_io.KIND_RETINAFACE_SLIM
        path = frt.write_weights(str(tmp_path_factory.mktemp("slim_ops") / "blob.frtw"), sd, kind)
        net = S.SlimNet(sd, rfb)
        ops = net.forward(R.preprocess(synth.make_frames(3, 100, 172)))
        for op in ops:
            if op.kind == "dwpw":
                assert 0 < op.probs[0].rng[0] < 65504, op.index
        _slim_refs[rfb] = (path, net, ops)
    return _slim_refs[rfb]


def prepare_slim(wd, blob_path, ops, B):
    """Writes the work directory of one Slim / RFB harness process."""
    shutil.copy(blob_path, os.path.join(wd, "blob.frtw"))
    for op in ops:
        for k, p in enumerate(op.probs):
            p.inp[:B].tofile(os.path.join(wd, "op%d.p%d.in" % (op.index, k)))
            if op.kind == "rfb_tail":
                p.add[:B].tofile(os.path.join(wd, "op%d.p%d.in1" % (op.index, k)))
    with open(os.path.join(wd, "job.txt"), "w") as f:
        f.write("172 100 100 172 %d 0\n" % B)


def _check_slim_topology(listed, net, ops):
    """The graph rebuilt from the dumped device addresses against the reference's tensors (det_slim_op_ref: Prob.src / add_src, SlimNet.outs):
    every input is its producer's output, at the reference's channel offset; distinct tensors have distinct addresses."""
    bad, addr = [], {}
    width = {"red": 24, "ta": 44, "tb": 16, "cat": 48}  # channels of the tensors that are read or written in slices (the harness dumps them for rfb_conv)

    def same(name, a, what):
        if addr.setdefault(name, a) != a:
            bad.append("%s is at %d, tensor %s at %d" % (what, a, name, addr[name]))

    for op in ops:
        for k, (d, p) in enumerate(zip(listed[op.index][1], op.probs)):
            what = "op %d p%d" % (op.index, k)
            name, coff = p.src
            if name != "x" and name not in addr:
                bad.append("%s reads %s, which no earlier op wrote" % (what, name))
            same(name, d["in"], what + " in")
            if d.get("in_coff", 0) != coff or (name in width and d.get("in_ctotal", width[name]) != width[name]):
                bad.append("%s reads channels from %d of %s, reference %d" % (what, d.get("in_coff", 0), d.get("in_ctotal"), coff))
            if p.add_src:
                if p.add_src[0] not in addr:
                    bad.append("%s reads %s, which no earlier op wrote" % (what, p.add_src[0]))
                same(p.add_src[0], d["in1"], what + " in1")
            for key, (oname, ocoff) in zip(("out", "out2"), net.outs.get((op.index, k), [])):
                same(oname, d[key], what + " " + key)
                if key == "out" and (d.get("out_coff", 0) != ocoff or (oname in width and d.get("out_ctotal", width[oname]) != width[oname])):
                    bad.append("%s writes channels from %d of %s, reference %d" % (what, d.get("out_coff", 0), d.get("out_ctotal"), ocoff))
    if len(set(addr.values())) != len(addr):
        bad.append("two tensors of the network share an address: %s" % addr)
    return bad


@pytest.mark.gpu
@pytest.mark.parametrize("rfb,B", SLIM_CASES, ids=["%s-100x172-B%d" % ("rfb" if r else "slim", b) for r, b in SLIM_CASES])
def test_slim_rfb_ops_alone(rfb, B, harness, frt, synth, tmp_path_factory, tmp_path):
    _runner.require_running()
    path, net, ops = _slim_reference(frt, synth, tmp_path_factory, rfb)
    tag = "%s 100x172 B=%d" % ("rfb" if rfb else "slim", B)
    work = tmp_path / "ops"
    work.mkdir()
    wd = str(work)
    try:
        prepare_slim(wd, path, ops, B)
        _runner.run(harness, wd, tag, 120)
        failures, ratios, listed = [], {}, {}
        results = {name: cols[0] for name, cols in read_results(wd).items()}
        if os.path.exists(os.path.join(wd, "oplist.txt")):
            listed = _parse_oplist(os.path.join(wd, "oplist.txt"))
        if sorted(listed) != list(range(len(ops))):
            failures.append("the op list has ops %s" % sorted(listed))
        elif all(listed[op.index][0] == op.kind and len(listed[op.index][1]) == len(op.probs) for op in ops):
            failures += _check_slim_topology(listed, net, ops)
        for name, changed in results.items():
            if changed != "0":
                failures.append("%s: %s words outside the logical output changed" % (name, changed))
        rd = lambda name, shape: np.fromfile(os.path.join(wd, name), np.float32).reshape(shape)
        A = sum(p.out[0].shape[1] for op in ops[-2:] for p in op.probs)
        base = 0
        for op in ops:
            name = "op%d" % op.index
            if name not in results or op.index not in listed:
                failures.append(name + ": not reached")
                continue
            kind, probs = listed[op.index]
            if kind != op.kind or len(probs) != len(op.probs) or any((d.get("Cin", d.get("C", p.dims[0])), d["H"], d["W"]) != tuple(p.dims) for d, p in zip(probs, op.probs)):
                failures.append("%s: the op list says %s %s, the reference %s %s" % (name, kind, probs, op.kind, [p.dims for p in op.probs]))
                continue
            if op.kind in ("slim_heads", "dense_head"):
                own = np.zeros(A, bool)
                for hi, (what, per) in enumerate((("loc", 4), ("conf", 2), ("ldm", 10))[:len(net.heads)]):
                    got = rd("%s.%s" % (name, what), (B, A, per))
                    b0 = base
                    for k, p in enumerate(op.probs):
                        n = p.out[hi].shape[1]
                        if probs[k]["base"] != b0:
                            failures.append("%s level %d: anchor base %d, the anchor table has %d" % (name, k, probs[k]["base"], b0))
                        failures += _compare("%s.p%d.%s" % (name, k, what), got[:, b0:b0 + n], p.out[hi][:B], p.bound[hi][:B], ratios)
                        own[b0:b0 + n] = True
                        b0 += n
                    other = got[:, ~own].view(np.uint32) != SENTINEL
                    if other.any():
                        failures.append("%s.%s: %d words of other levels' anchors changed" % (name, what, other.sum()))
                base = b0
                continue
            for k, p in enumerate(op.probs):
                failures += _compare("%s.p%d.out" % (name, k), rd("%s.p%d.out" % (name, k), (B,) + p.out.shape[1:]), p.out[:B], p.bound[:B], ratios)
                if p.out2 is not None:
                    failures += _compare("%s.p%d.out2" % (name, k), rd("%s.p%d.out2" % (name, k), (B,) + p.out2.shape[1:]), p.out2[:B], p.bound2[:B], ratios)
        for name in sorted(ratios, key=lambda n: (int(n[2:].split(".")[0]), n)):
            print("%s %s: max(err / bound) = %.3f" % (tag, name, ratios[name]))
        _runner.require_ended_well()
        assert not failures, "%d failures:\n%s" % (len(failures), "\n".join(failures[:40]))
    finally:
        shutil.rmtree(wd, ignore_errors=True)
