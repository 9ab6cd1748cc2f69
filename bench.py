#!/usr/bin/env python3
"""Headline benchmark: faces/sec end-to-end (detect + crop + embed + match), 640x640, batch = 32 frames, 1M x 512 gallery.

    python bench.py --gpus N --steps K --warmup W
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P bench.py --gpus N ...

One "step" = one pass of the whole hot path over one batch of 32 synthetic 640x640 frames: letterbox/normalise ->
RetinaFace-mnet0.25 -> decode + NMS (K = 4 faces per frame) -> bicubic crop -> ArcFace IR-50 (fp16 MFMA convs, fp32 accumulate) ->
cosine top-1 against a 1M x 512 fp32 gallery.  Nothing is cached between steps and no stage is skipped.

THE MATCH STAGE IS NOT SURVEY 8(d)'s 2.048 GB fp32 scan: it is an int8-SCREENED coarse scan (0.51 GB shadow gallery, fp16 MFMA products of
exactly widened int8 rows) + an EXACT fp32 re-rank of every 32-row block the rigorous error bound cannot exclude.  Its results
are bit-identical to the exact scan's (tests/test_gpu_match.py), its cost depends on the queries: the default workload's queries match
nothing in the gallery ("miss": ~ 11 candidate blocks per query); `match_legs` in the --full line carries the same step with the queries planted
in the gallery ("hit") and with the screening switched off ("worst_case" = the exact fp32 scan of 8(d), frt_matcher_set_screening(m, 0)).

TIMED REGION: u8 frames in PINNED HOST memory -> per-face (box, top-1 index, similarity) records back in host memory,
through frt_pipeline_submit / frt_pipeline_wait with three batches in flight (H2D of 39 MB per step on the copy stream, D2H of the
4.6 KB record block).  The figure with frames and results resident in HBM (frt_pipeline_run_dev) is reported beside it in
`hbm_resident` (--full); `--resident` makes it the primary one.  With N > 1 every rank (one process per GPU) owns a full gallery replica and
its own 32 frames (weak scaling; `--strong` splits ONE 32-frame batch over the ranks - BASELINE configs[3] as written, also reported
as a side object of every N > 1 --full run).  Frames are independent, so there is NO collective on the data path; with N > 1 the per-face
result records of every step are all-gathered over RCCL on a side stream inside the timed region (configs[3]'s exchange step).
`--sharded-gallery` runs configs[4] instead: the gallery is row-sharded over the ranks and stored as fp16, the embeddings are rounded to
fp16 and all-gathered, every rank searches its shard for its top-k lists (global indices), the lists are all-gathered and merged on the
device (higher similarity first, lower global index on ties).  Every data-path exchange is an ncclAllGather issued by libfrt.so itself
(frt_comm_*, the C-ABI a C++ host binds); torch.distributed only hands the communicator id to the ranks and carries the benchmark's
barrier / max-over-ranks bookkeeping.

Prints ONE JSON line on rank 0 (contract in the task statement) with extra objects:
  roofline      dominant kernel family = the ArcFace 3x3 implicit-GEMM convs; achieved = algorithmic FLOPs of those launches /
                their HIP-event time, measured live on the stream they run on during one step of the timed region; peak = 2.5 PFLOP/s
                dense fp16 MFMA (MI355X_MICROARCH.md); sustained_peak (--full) = what THIS device sustains on the kernel's instruction mix
                under its power limit, measured in this process right after the timed region (frt_probe_sustained_mfma).
  cpu_baseline  --full only (null otherwise): the oracle (reference-faithful CPU restatement, oracle/) timed on this box's host cores over
                bounded samples of the same workload, rank 0 at N = 1 only: the full CPU pipeline and the reference's HOST-side work alone
                (pre/post-processing + O(F*N) argmax), each with all cores and with one thread.

A plain run sets up, warms up, times the steps, writes --dump-outputs and prints the line.  Everything measured beyond that takes
runs of its own and is behind --full: the other boundary (hbm_resident / host_boundary), steady_state, sync_call_latency_ms,
strong_scaling (N > 1), the serial roofline and roofline.stages, overlap_efficiency, match_legs, strong_scaling_proxy,
roofline.sustained_peak and cpu_baseline.  --no-extras / --no-cpu-baseline drop parts of that set again.
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

PEAK_FP16_MFMA_TFLOPS = 2500.0  # dense; /opt/skills/guides/MI355X_MICROARCH.md "Peak BF16/FP16 MFMA"
PEAK_FP32_MATRIX_TFLOPS = 157.3  # same guide: fp32 matrix / vector
PEAK_HBM_BPS = 8.0e12            # same guide: HBM3E
DET_ACT_BYTES_PER_640_FRAME = 27.45e6 * 4  # detector activations (fp32) written + read once per 640x640 frame
DET_FP16_BYTES_PER_640_FRAME = 54.9e6       # the same tensors at the reference engine's fp16 (2 B x 27.45 M elements, written + read)
DEPTH = 3                        # batches in flight at the host boundary


# ----------------------------------------------------------------------------------------------------------------------
# CPU baseline (oracle = checker, timed here as the reported baseline only)
# ----------------------------------------------------------------------------------------------------------------------
def _cpu_full(det_sd, rec_sd, gallery, frames, K, budget_s):
    """Full CPU pipeline, frames one at a time like the reference (src/app.cpp:304-310)."""
    import oracle
    from oracle import match, nets
    H, W = frames.shape[1:3]
    faces = n = 0
    t0 = time.perf_counter()
    for fr in frames:
        x = oracle.det_preprocess(fr, H, W)
        loc, conf = nets.retinaface_forward(det_sd, x[None])
        boxes = oracle.postprocess(loc[0], conf[0], W, H, W, H, 0.4, 0.6, K)
        crops = oracle.crop_faces(fr, boxes)
        emb = nets.arcface_forward(rec_sd, oracle.face_normalize(crops))
        match.top1(emb, gallery)
        faces += len(boxes)
        n += 1
        if time.perf_counter() - t0 > budget_s:
            break
    return faces, n, time.perf_counter() - t0


def _cpu_host_work(heads, embeds, gallery, frames, K, budget_s):
    """Only what the REFERENCE does on the host around its GPU engines: letterbox + normalise + planarise (retinaface.cpp:106-136),
    anchor regeneration + decode + sort + NMS (:154-271), crop + bicubic + normalise (arcface.cpp:3-17,116-129) and the arg-max over a
    materialised [F, N] similarity matrix (arcface.cpp:203-217).  Network outputs are precomputed (they come from the GPU there)."""
    import oracle
    H, W = frames.shape[1:3]
    faces = n = 0
    sims = np.ascontiguousarray(np.random.default_rng(0).random((K, gallery.shape[0]), dtype=np.float32))  # what cuBLASLt hands back
    t0 = time.perf_counter()
    while True:
        for i, fr in enumerate(frames):
            oracle.det_preprocess(fr, H, W)
            boxes = oracle.postprocess(heads[i][0], heads[i][1], W, H, W, H, 0.4, 0.6, K)
            oracle.face_normalize(oracle.crop_faces(fr, boxes))
            for row in sims[:len(boxes)]:
                int(np.argmax(row))  # std::max_element over one row of the F x N matrix
            faces += len(boxes)
            n += 1
        if time.perf_counter() - t0 > budget_s:
            break
    return faces, n, time.perf_counter() - t0


def cpu_baseline(det_sd, rec_sd, gallery, frames, K):
    """The oracle timed on this box's host cores.  The all-core leg used to be SLOWER than one thread (torch-CPU oversubscribed on a
    256-thread host: 3.3 against 10.9 faces/s, round-3 review item 12): the primary value is now the best of a thread sweep, with the
    thread count it was reached at in `cores`."""
    import torch

    import oracle
    from oracle import nets
    ncpu = int(torch.get_num_threads())
    nproc = os.cpu_count() or 1
    H, W = frames.shape[1:3]
    heads = []
    for fr in frames[:8]:
        loc, conf = nets.retinaface_forward(det_sd, oracle.det_preprocess(fr, H, W)[None])
        heads.append((loc[0], conf[0]))
    sweep = {}
    try:
        for nt in [t for t in (1, 4, 8, 16, 32, 64) if t <= nproc]:
            torch.set_num_threads(nt)
            _cpu_full(det_sd, rec_sd, gallery, frames[:1], K, 0.0)  # thread pool up, caches warm
            f, n, dt = _cpu_full(det_sd, rec_sd, gallery, frames, K, 6.0 if nt == 1 else 3.0)
            sweep[nt] = {"value": round(f / dt, 3), "sample": "%d frame(s), %d faces, %.1f s" % (n, f, dt)}
        best = max(sweep, key=lambda t: sweep[t]["value"])
        torch.set_num_threads(best)
        f, n, dt = _cpu_host_work(heads, None, gallery, frames[:8], K, 3.0)
        host_best = f / dt  # (the oracle's C code is single-threaded; more threads only change NumPy/torch internals)
        torch.set_num_threads(1)
        f, n, dt = _cpu_host_work(heads, None, gallery, frames[:8], K, 3.0)
        host_1 = f / dt
    finally:
        torch.set_num_threads(ncpu)
    out = {"value": sweep[best]["value"], "unit": "faces/sec", "cores": best, "kind": "port",
           "sample": "full CPU pipeline (oracle nets fp32 on torch-CPU, C post-processing/crop, NumPy %dx512 match) on frames of the same "
                     "640x640 workload, one at a time like the reference; best of a thread sweep, reached with %d threads: %s"
                     % (gallery.shape[0], best, sweep[best]["sample"]),
           "thread_sweep": {str(t): v for t, v in sweep.items()},
           "single_thread": {"value": sweep[1]["value"], "cores": 1, "sample": sweep[1]["sample"]},
           "reference_host_work_only": {
               "what": "only the work the reference itself does on the host around its TensorRT/cuBLASLt calls: letterbox+normalise, anchor "
                       "regeneration+decode+sort+NMS, crop+bicubic+normalise, arg-max over a materialised [F,N] fp32 row per face "
                       "(retinaface.cpp:106-136,154-271; arcface.cpp:3-17,116-129,203-217); network outputs precomputed",
               "value": round(host_best, 3), "unit": "faces/sec", "cores": best,
               "single_thread": {"value": round(host_1, 3), "cores": 1}},
           "host": {"nproc": nproc, "cpu": _cpu_model()}}
    return out


def _cpu_model():
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("model name"):
                    return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


# ----------------------------------------------------------------------------------------------------------------------
# power / clock evidence: rocm-smi sampled by a side thread while the timed region runs
# ----------------------------------------------------------------------------------------------------------------------
class SmiSampler:
    def __init__(self, device, period=0.25):
        self.device, self.period, self.samples, self._stop, self._t = device, period, [], threading.Event(), None

    def _run(self):
        while not self._stop.is_set():
            t = time.time()
            try:
                o = subprocess.run(["rocm-smi", "-d", str(self.device), "--showpower", "--showclocks", "--json"], capture_output=True,
                                   text=True, timeout=5).stdout
                card = next(iter(json.loads(o).values()))
                rec = {"t": round(t, 3)}
                for k, v in card.items():
                    kl = k.lower()
                    if "power" in kl and "(w)" in kl:
                        rec["power_w"] = float(v)
                    elif kl.startswith("sclk clock speed"):
                        rec["sclk_mhz"] = float(str(v).strip("()Mhz "))
                    elif kl.startswith("mclk clock speed"):
                        rec["mclk_mhz"] = float(str(v).strip("()Mhz "))
                self.samples.append(rec)
            except Exception:  # noqa: BLE001  (rocm-smi missing / format change: evidence only, never fatal)
                pass
            self._stop.wait(self.period)

    def __enter__(self):
        self._t = threading.Thread(target=self._run, daemon=True)
        self._t.start()
        return self

    def __exit__(self, *a):
        self._stop.set()
        self._t.join(10)


DUMP_LIMIT_BYTES = 64 << 20


def record_arrays(recs):
    """Per-face result records (frt.RESULT_DTYPE) as one array per field, boxes as [F, 4] (x1, y1, x2, y2)."""
    return {"boxes": np.stack([recs[k] for k in ("x1", "y1", "x2", "y2")], 1), "score": recs["score"], "frame": recs["frame"],
            "match_idx": recs["match_idx"], "match_sim": recs["match_sim"], "valid": recs["valid"]}


def dump_outputs(path, arrays):
    """--dump-outputs: every array as <path>/<name>.npy; integers widened to float64 (exact), floats as float32 (float64 kept)."""
    os.makedirs(path, exist_ok=True)
    conv = {}
    for name, a in arrays.items():
        a = np.asarray(a)
        conv[name] = np.ascontiguousarray(a, dtype=np.float64 if (a.dtype.kind in "iub" or a.dtype == np.float64) else np.float32)
    total = sum(a.nbytes for a in conv.values())
    if total > DUMP_LIMIT_BYTES:
        raise SystemExit("bench.py: --dump-outputs would write %d bytes (limit %d)" % (total, DUMP_LIMIT_BYTES))
    for name, a in conv.items():
        np.save(os.path.join(path, name + ".npy"), a)


def visible_devices():
    """HIP devices this process can see, counted in a child process (the launcher itself does not initialise HIP: only the ranks it
    starts open the devices)."""
    code = ("import sys; sys.path.insert(0, %r); import __graft_entry__ as e; print(e.load_pkg().device_count())" % ROOT)
    try:
        o = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
        return int(o.stdout.strip().splitlines()[-1])
    except (ValueError, IndexError, subprocess.SubprocessError):
        return 0


def spawn_ranks(n, argv):
    """`python bench.py --gpus N` without a launcher: re-exec under torch.distributed.run with N ranks (LOCAL_RANK -> device)."""
    import socket
    check = os.environ.get("FRT_BENCH_LAUNCH_CHECK") == "1"   # CPU test of this launcher: no devices needed
    if not check:
        have = visible_devices()
        if have < n:
            print("bench.py: --gpus %d asked for, %d HIP device(s) visible: refusing to run (a %d-rank job on fewer devices would not measure "
                  "what it says)" % (n, have, n), file=sys.stderr)
            return 2
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n), "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + list(argv)
    print("bench.py: starting %d ranks: %s" % (n, " ".join(cmd)), file=sys.stderr)
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")  # dmabuf IPC (RCCL across processes on this driver)
    env.setdefault("OMP_NUM_THREADS", "8")
    return subprocess.call(cmd, env=env)


def launch_check(args, json_out):
    """FRT_BENCH_LAUNCH_CHECK=1 (tests/test_distributed.py, no GPU): every rank joins a gloo group and rank 0 reports how many ranks really
    started - the launcher's contract (`n_gpus` == --gpus) without a device."""
    import torch
    import torch.distributed as dist
    rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29513")
    dist.init_process_group("gloo", rank=rank, world_size=world)
    t = torch.tensor([1, int(os.environ.get("LOCAL_RANK", "0"))], dtype=torch.int64)
    dist.all_reduce(t)
    dist.barrier()
    dist.destroy_process_group()
    if int(t[0]) != args.gpus:
        print("launch check: %d ranks joined, --gpus %d" % (int(t[0]), args.gpus), file=sys.stderr)
        return 3
    if rank == 0:
        print(json.dumps({"launch_check": True, "n_gpus": int(t[0]), "local_rank_sum": int(t[1])}), file=json_out, flush=True)
    return 0


def main():
    # the contract is ONE JSON line on stdout: keep the real stdout for it and send everything else that writes to fd 1 (RCCL prints a
    # five-line version banner there when its communicator is created) to stderr
    sys.stdout.flush()
    json_out = os.fdopen(os.dup(1), "w")
    os.dup2(2, 1)
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=32, help="frames per step per GPU (per step in total with --strong)")
    ap.add_argument("--faces", type=int, default=4, help="det_maxFacesPerScene (K)")
    ap.add_argument("--gallery", type=int, default=1_000_000)
    ap.add_argument("--frame", default="640x640", help="frame size WxH (default 640x640 = the metric; 1920x1080 = BASELINE config 3's "
                                                       "video frames, letterboxed to the 640x640 detector input). Implies --no-cpu-baseline when not 640x640")
    ap.add_argument("--mode", default="ir", choices=["ir", "ir_se"], help="IR-50 (the reference's network) or IR-SE-50")
    ap.add_argument("--full", action="store_true", help="after the line's own measurement, run every side measurement too (other boundary, steady "
                                                        "state, serial roofline and stages, match legs, strong-scaling proxy, sustained peak, CPU "
                                                        "baseline); off by default: a plain run does only what the headline figure needs")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--resident", action="store_true", help="primary timed region with frames/results resident in HBM (frt_pipeline_run_dev)")
    ap.add_argument("--strong", action="store_true", help="strong scaling: ONE batch of --batch frames split over the ranks (BASELINE configs[3])")
    ap.add_argument("--in-flight", type=int, default=DEPTH, help="batches in flight at the host boundary (1..11; default 3, 2 N + 2 with --pair N).  With --strong every rank "
                                                                 "keeps this many of its small batches in the stage pipeline at once")
    ap.add_argument("--sharded-gallery", action="store_true",
                    help="BASELINE configs[4]: gallery row-sharded over the ranks and stored as fp16; RCCL all-gather of embeddings and of the top-1 winners")
    ap.add_argument("--fp32", action="store_true", help="recogniser in fp32 end to end (frt_embedder_set_precision(e, 1)): BASELINE configs[1]'s \"fp32\" "
                                                        "(with --batch 1 --gallery 10000); the metric's own configuration stays fp16 MFMA")
    ap.add_argument("--exact-match", action="store_true", help="match stage = the exact fp32 scan of the whole gallery on every call "
                                                               "(frt_matcher_set_screening(m, 0): SURVEY 8(d)'s 2.048 GB per call) instead of the screened top-1")
    ap.add_argument("--pair", type=int, nargs="?", const=2, default=0,
                    help="frt_pipeline_set_pairing(p, N): crop + recogniser + match of N = 2 (default when the flag is given), 3 or 4 consecutive calls as one "
                         "pass (results when the group is complete; objects are created for N times the frames of a step).  Only meaningful for small "
                         "steps: N * batch * faces must fit the recogniser's 128-face pass")
    ap.add_argument("--no-gather", action="store_true", help="N > 1: skip the per-step RCCL all-gather of the result records")
    ap.add_argument("--topk", type=int, default=5, help="--sharded-gallery: length of the per-query lists every rank answers with (1..16)")
    ap.add_argument("--dump-final", default=None, help="--sharded-gallery: write the last step's gathered fp16 queries and merged top-k lists (npz) "
                                                       "for an external check against the oracle (tests/test_gpu_dist.py)")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="after the timed region, write what its last step returned (the per-face records; with --sharded-gallery also the merged "
                         "top-k lists) as DIR/<name>.npy in float32 / float64, for an output-by-output comparison of two builds")
    ap.add_argument("--stage-profile", default=None, help="write a per-stage HIP-event breakdown (extra untimed steps) to this file")
    ap.add_argument("--no-profile", action="store_true", help="do not record per-kernel HIP events in the timed region")
    ap.add_argument("--no-extras", action="store_true", help="with --full: no side measurements on the device (the CPU baseline stays)")
    ap.add_argument("--ab-old-lib", default=None, help="measurement only: run the timed region on an OLDER build of libfrt.so (path) for a same-box A/B "
                                                       "(tools/ab_lib.sh); symbols it lacks are skipped with a warning.  Never a reported number")
    ap.add_argument("--smi-trace", default=None, help="write the rocm-smi power/clock samples taken during the timed region to this file")
    ap.add_argument("--wait-spin-us", type=int, default=50000,
                    help="how long libfrt's host waits busy-poll before they back off (frt_set_wait_spin_us).  The library's default is 200 us "
                         "(a server's request threads must not burn cores); this driver owns its core and one late wake-up is a third of a "
                         "20-step region, so it asks for 50 ms and says so in config.host_wait")
    args = ap.parse_args()
    if not args.full:
        args.no_extras = args.no_cpu_baseline = True   # a plain run: the headline figure's own measurement only
    depth = max(1, min(11, args.in_flight))
    if args.pair and args.in_flight == DEPTH:
        depth = 2 * args.pair + 2   # grouped calls complete N at a time: two groups in the later stages + the detector's calls ahead of them
    if args.gpus < 1:
        raise SystemExit("--gpus must be >= 1")
    if args.steps < 1:
        raise SystemExit("--steps must be >= 1")
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        # `python bench.py --gpus N` as typed: this process becomes the launcher - one rank per GPU under torch.distributed.run
        # (the same command line the driver uses), rank 0's JSON line passes through on stdout.  Never a silent one-rank run.
        os.dup2(json_out.fileno(), 1)
        raise SystemExit(spawn_ranks(args.gpus, sys.argv[1:]))
    if "WORLD_SIZE" in os.environ and int(os.environ["WORLD_SIZE"]) != args.gpus and os.environ.get("FRT_BENCH_FORCE_DIST") != "1":
        raise SystemExit("bench.py: WORLD_SIZE (%s) != --gpus (%d): start as many ranks as --gpus says" % (os.environ["WORLD_SIZE"], args.gpus))
    if os.environ.get("FRT_BENCH_LAUNCH_CHECK") == "1":
        raise SystemExit(launch_check(args, json_out))

    import torch
    import torch.distributed as dist

    if args.ab_old_lib:
        import types
        os.environ["FRT_LIB"] = os.path.abspath(args.ab_old_lib)
        sys.modules["frt_amd_ab_old_library"] = types.ModuleType("frt_amd_ab_old_library")  # (the binding's import is strict otherwise)
    import __graft_entry__ as entry
    frt = entry.load_pkg()
    fd = frt.dist

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if frt.device_count() < 1 or not torch.cuda.is_available():
        raise SystemExit("bench.py needs a HIP device (libfrt has no CPU path)")
    if local_rank >= frt.device_count():
        raise SystemExit("bench.py: rank %d has no device of its own (LOCAL_RANK %d, %d visible)" % (rank, local_rank, frt.device_count()))
    frt.set_wait_spin_us(args.wait_spin_us)
    torch.cuda.set_device(local_rank)
    use_dist = world > 1 or os.environ.get("FRT_BENCH_FORCE_DIST") == "1"  # the env switch exercises the RCCL path on one GPU
    s = frt.synth
    K, H, W = args.faces, 640, 640   # detector input
    FW, FH = (int(v) for v in args.frame.lower().split("x"))
    if (FW, FH) != (W, H):
        args.no_cpu_baseline = True
    # frames of this rank: weak = its own --batch frames; strong = its share of ONE --batch-frame batch
    if args.strong:
        fb, fe = fd.shard_range(args.batch, rank, world)
        B = max(fe - fb, 1)
        frame_start = fb
    else:
        B = args.batch
        frame_start = rank * B
    F = B * K
    tmp = tempfile.mkdtemp(prefix="frt_bench_%d_" % rank)
    det_sd = s.retinaface_state(1)
    rec_sd = s.arcface_state(2, args.mode, calib=s.load_calibration(args.mode))
    det_path = frt.write_weights(os.path.join(tmp, "det.frtw"), det_sd, 1)
    rec_path = frt.write_weights(os.path.join(tmp, "rec.frtw"), rec_sd, 2 if args.mode == "ir" else 3)
    cap = max(args.pair, 1)   # --pair N: room for N calls' face slots (the condition for pairing, include/frt.h)
    det = frt.RetinaFace(det_path, FW, FH, (3, H, W), B * cap, K, 0.4, 0.6, device=local_rank)
    rec = frt.ArcFaceIR50(rec_path, FW, FH, (3, 112, 112), 512, F * cap, K, 0.65, device=local_rank)
    if args.fp32:
        rec.setPrecision(True)
    gallery = s.make_gallery(args.gallery)
    t_load = time.perf_counter()
    if args.sharded_gallery:
        gb, ge = fd.gallery_shard(args.gallery, rank, world)
        rec.matmul.setStorage(True)                    # fp16-stored shard
        rec.setGallery(gallery[gb:ge])
        rec.initMatMul()
        rec.matmul.setRowOffset(gb)
    else:
        rec.setGallery(gallery)  # bulk initKnownEmbeds + addEmbedding x N through the streaming loader (pinned chunks, async copies)
        rec.initMatMul()
    gallery_load_s = time.perf_counter() - t_load
    if args.exact_match:
        rec.matmul.setScreening(False)
    _sb = rec.matmul.scanBytes()
    _rows = max(int(frt.lib.frt_matcher_num_rows(rec.matmul._h)), 1)
    scan_mode = "int8" if _sb == 512 * _rows else ("fp16" if (_sb == 1024 * _rows and not args.sharded_gallery) else "exact")
    pipe = frt.Pipeline(det, rec, B * cap, match=not args.sharded_gallery)  # sharded gallery: the pipeline produces embeddings, match + merge follow below
    if args.pair:
        pipe.set_pairing(args.pair)
    # The caller's stream (NOT torch's default stream: that is the legacy NULL stream, and every operation on it - an event record, a
    # collective's stream hand-over - is a barrier against all blocking streams, including the pipeline's stage streams: measured 7.9
    # instead of 3.6 ms per step) is created, handed to the pipeline and USED once - so that the pipeline's lazily created upload stream
    # exists too - before any other stream user of the process (RCCL's process group, libfrt's communicator) comes into being.  Measured
    # with tools/queue_probe.py: in this order every later stream creation leaves the step alone (0.78 ms per 4-frame step); a caller's
    # stream that first meets the pipeline after RCCL's streams exist can cost 2x at small batches (1.65 ms) and 4.5 % at 32 frames.
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    pipe.set_stream(stream.cuda_stream)
    _prime = s.make_frames(B, FH, FW, start=frame_start + 9000)
    pipe.run(_prime, want_embeds=False)
    pipe.run(_prime, want_embeds=False)
    del _prime
    if use_dist:
        # AFTER the pipeline exists: RCCL creates streams of its own, and a stream created before the pipeline's stage streams can change
        # how ROCm maps those onto hardware queues (the stages then share a queue with somebody's pending waits and stop overlapping)
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29511")
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local_rank))

        def bcast_id(uid):
            box = [uid]
            dist.broadcast_object_list(box, src=0)
            return box[0]

        # the data-path communicator: RCCL through the C ABI (created last: it owns a stream)
        cg = fd.CommGroup(frt, rank, world, local_rank, bcast_id if world > 1 else None)

    # two alternating batches so that consecutive steps never see the same pixels
    batches = [s.make_frames(B, FH, FW, start=frame_start), s.make_frames(B, FH, FW, start=frame_start + 4096)]
    h_frames = [torch.from_numpy(b).pin_memory() for b in batches]
    h_np = [t.numpy() for t in h_frames]
    RD = frt.RESULT_DTYPE
    h_res = [torch.zeros(F * RD.itemsize, dtype=torch.uint8).pin_memory() for _ in range(12)]
    h_views = [r.numpy().view(RD) for r in h_res]
    d_frames = [t.cuda() for t in h_frames]
    NRING = 12
    d_res = [torch.zeros(F * RD.itemsize, dtype=torch.uint8, device="cuda") for _ in range(NRING)]
    d_all = [torch.zeros(world * F * RD.itemsize, dtype=torch.uint8, device="cuda") for _ in range(NRING)] if use_dist else None
    h_all = [torch.zeros(world * F * RD.itemsize, dtype=torch.uint8).pin_memory() for _ in range(NRING)] if use_dist else None
    # the exchange stream: H2D of the records, ncclAllGather, D2H.  A torch-owned stream handed to frt_comm_all_gather (a C++ host would use
    # the communicator's own, frt_comm_stream): torch's pinned-memory allocator records events on every stream a pinned block was used
    # on when the block is freed, so the stream must outlive the tensors - which a stream owned by the communicator would not at exit
    side = torch.cuda.Stream() if use_dist else None
    ev_side = [torch.cuda.Event() for _ in range(NRING)] if use_dist else None
    gather = use_dist and not args.no_gather

    # ---- sharded-gallery mode (configs[4]): the pipeline has no matcher stage and produces embeddings; match + merge follow here
    if args.sharded_gallery:
        TK = args.topk
        d_emb = [torch.zeros(F, 512, device="cuda") for _ in range(NRING)]
        d_emb16 = torch.zeros(F, 512, dtype=torch.float16, device="cuda")            # what travels: fp16 embeddings
        d_q16 = torch.zeros(world * F, 512, dtype=torch.float16, device="cuda")      # every rank's queries
        d_li = torch.zeros(world * F, TK, dtype=torch.int32, device="cuda")          # this rank's lists for ALL queries
        d_ls = torch.zeros(world * F, TK, dtype=torch.float32, device="cuda")
        d_gi = torch.zeros(world, world * F, TK, dtype=torch.int32, device="cuda")   # every rank's lists
        d_gs = torch.zeros(world, world * F, TK, dtype=torch.float32, device="cuda")
        d_fi = torch.zeros(world * F, TK, dtype=torch.int32, device="cuda")          # merged
        d_fs = torch.zeros(world * F, TK, dtype=torch.float32, device="cuda")
        final = [None]

    # ---------------------------------------------------------------------------------------------------- step bodies
    step_times = [] if os.environ.get("FRT_BENCH_STEP_TIMES") else None  # diagnostic: host timestamps of every submit / wait (printed to stderr)

    def run_host(n_steps, profile_step=None):
        """pinned host frames -> host records, DEPTH batches in flight (frt_pipeline_submit / frt_pipeline_wait)."""
        tickets = []
        for i in range(n_steps):
            if len(tickets) >= depth:
                pipe.wait(tickets.pop(0))
                if step_times is not None:
                    step_times.append(("wait", i, time.perf_counter()))
            if i == profile_step:
                frt.profile_enable(1)
            tickets.append(pipe.submit(h_np[i & 1], h_views[i % 12]))
            if step_times is not None:
                step_times.append(("submit", i, time.perf_counter()))
            if i == profile_step:
                frt.profile_enable(-1)  # pause: keep the records, stop recording (host-side flag, no sync)
        for t in tickets:
            pipe.wait(t)
            if step_times is not None:
                step_times.append(("drain", t, time.perf_counter()))

    def run_host_dist(n_steps, profile_step=None):
        """Same boundary with N > 1: the step itself is run_host's (frt_pipeline_submit / frt_pipeline_wait, DEPTH batches in flight); the
        step's records - 5 KB per rank - then go through the RCCL all-gather on a side stream (H2D of the records, all-gather, D2H of
        the gathered block), off the pipeline's streams and off the host's critical path.  (Feeding the pipeline from torch streams
        instead - upload stream + run_dev_after + side-stream gather straight from the device records - measured 3.8 ms per step
        against 3.3 for this form on one rank, with or without the collective and with gloo in place of RCCL: 39 MB uploads enqueued
        from the benchmark's own stream pool do not overlap the stages the way the library's copy stream does.)"""
        tickets = []

        def gather_async(slot):
            if not gather:
                return
            with torch.cuda.stream(side):
                d_res[slot].copy_(h_res[slot], non_blocking=True)
                if gather:
                    cg.all_gather(d_res[slot], d_all[slot], side.cuda_stream)   # ncclAllGather from libfrt (frt_comm_all_gather)
                    h_all[slot].copy_(d_all[slot], non_blocking=True)
                ev_side[slot].record(side)

        for i in range(n_steps):
            if len(tickets) >= depth:
                t, slot = tickets.pop(0)
                pipe.wait(t)
                gather_async(slot)
            slot = i % NRING
            if i >= NRING and gather:
                ev_side[slot].synchronize()       # the slot's previous records have left the host buffer (long done)
            if i == profile_step:
                frt.profile_enable(1)
            tickets.append((pipe.submit(h_np[i & 1], h_views[slot]), slot))
            if i == profile_step:
                frt.profile_enable(-1)
        for t, slot in tickets:
            pipe.wait(t)
            gather_async(slot)
        side.synchronize()

    def run_resident(n_steps, profile_step=None):
        for i in range(n_steps):
            if i == profile_step:
                frt.profile_enable(1)
            pipe.run_dev(d_frames[i & 1].data_ptr(), B, d_res[i % NRING].data_ptr(), None)
            if i == profile_step:
                frt.profile_enable(-1)
        if args.pair:
            pipe.sync()   # (a last call without a partner: its later stages are queued here, inside the region)

    def run_sharded(n_steps, profile_step=None):
        for i in range(n_steps):
            r = i % NRING
            if i == profile_step:
                frt.profile_enable(1)
            pipe.run_dev(d_frames[i & 1].data_ptr(), B, d_res[r].data_ptr(), d_emb[r].data_ptr())
            if i == profile_step:
                frt.profile_enable(-1)
            cs = stream.cuda_stream
            nq = world * F
            frt.embeds_to_half_dev(d_emb[r].data_ptr(), F * 512, d_emb16.data_ptr(), cs)    # fp16 embeddings (configs[4])
            if use_dist:
                cg.all_gather(d_emb16, d_q16, cs)                                          # exchange 1: every rank gets every query
                q_ptr = d_q16.data_ptr()
            else:
                q_ptr = d_emb16.data_ptr()
            rec.matmul.topk_dev(q_ptr, nq, TK, d_li.data_ptr(), d_ls.data_ptr(), cs, fp16=True)   # this shard's lists, global indices
            if use_dist:
                cg.all_gather(d_li, d_gi, cs)                                              # exchange 2: the top-k lists
                cg.all_gather(d_ls, d_gs, cs)
                frt.merge_topk_dev(world, nq, TK, d_gi.data_ptr(), d_gs.data_ptr(), d_fi.data_ptr(), d_fs.data_ptr(), cs)
                final[0] = (d_fi, d_fs)
            else:
                final[0] = (d_li, d_ls)

    if args.sharded_gallery:
        run = run_sharded
    elif args.resident:
        run = run_resident
    elif use_dist:
        run = run_host_dist
    else:
        run = run_host

    run(max(args.warmup, 1))
    torch.cuda.synchronize()
    if args.sharded_gallery or args.resident:
        res = np.frombuffer(d_res[(max(args.warmup, 1) - 1) % NRING].cpu().numpy().tobytes(), RD)
    else:
        res = h_views[(max(args.warmup, 1) - 1) % 12]
    faces_per_step = int(res["valid"].sum())

    profile = not args.no_profile
    # Per-launch HIP events (roofline object) are recorded for ONE step (the last) of the timed region: left on for every step
    # they cost ~0.5 ms per step (two event packets around each of ~55 conv launches) - 11 % of the number being measured.  libfrt
    # runs a profiled call serially on the pipeline stream (no other stage competes for the dispatch), so the bracketed time is the
    # kernel's own duration - the number rocprofv3 reports; with four streams in flight it was 2.7x that.
    sampled_step = args.steps - 1 if profile else None
    frt.profile_enable(0)
    smi = SmiSampler(local_rank) if (rank == 0 and args.smi_trace) else None  # (one rocm-smi call takes longer than a 20-step region)
    if use_dist:
        dist.barrier()
    torch.cuda.synchronize()
    if smi:
        smi.__enter__()
    if step_times is not None:
        del step_times[:]
    t0 = time.perf_counter()
    run(args.steps, sampled_step)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    if step_times:
        prev = t0
        for what, i, t in step_times:
            print("[step-times] %-6s %3d  +%.3f ms" % (what, i, 1e3 * (t - prev)), file=sys.stderr)
            prev = t
        print("[step-times] region %.3f ms" % (1e3 * dt), file=sys.stderr)
        step_times = None
    if smi:
        smi.__exit__()
    if gather and run is run_host_dist and args.steps >= 1:
        # the last step's gathered block must hold this rank's own records at its rank offset
        r = (args.steps - 1) % 4
        own = h_all[r][rank * F * RD.itemsize:(rank + 1) * F * RD.itemsize]
        assert torch.equal(own, h_res[r]), "all-gather mismatch"
    if args.dump_outputs:
        # what the last timed step handed back, before the untimed extras below reuse the same buffers
        last = (args.steps - 1) % NRING
        if run is run_host or run is run_host_dist:
            recs = h_views[last].copy()
        else:
            recs = np.frombuffer(d_res[last].cpu().numpy().tobytes(), RD)
        outputs = record_arrays(recs)
        if args.sharded_gallery:
            fi, fs = final[0]
            outputs["topk_idx"] = fi.cpu().numpy()[:world * F]
            outputs["topk_sim"] = fs.cpu().numpy()[:world * F]
        suffix = "" if world == 1 else "_rank%d" % rank
        dump_outputs(args.dump_outputs, {k + suffix: v for k, v in outputs.items()})
    if use_dist:
        dist.barrier()
        t = torch.tensor([dt], dtype=torch.float64, device="cuda")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
        nf = torch.tensor([faces_per_step], dtype=torch.int64, device="cuda")
        dist.all_reduce(nf, op=dist.ReduceOp.SUM)
        total_faces_per_step = int(nf.item())
    else:
        total_faces_per_step = faces_per_step

    def conv_table(labels, ms, work):
        t = {}
        for l, m, w in zip(labels, ms, work):
            if m > 0 and l.startswith("conv"):  # conv_patch / conv_s2 / conv_s2c64 / conv64 / conv_glds (3x3 and the 1x1 shortcuts)
                e = t.setdefault(l, [0.0, 0.0, 0])
                e[0] += float(m)
                e[1] += float(w)
                e[2] += 1
        return t

    roofline = None
    dom = None
    if profile:
        labels, ms, work = frt.profile_collect()
        frt.profile_enable(0)
        live = conv_table(labels, ms, work)
        if live:
            dom = max(live, key=lambda k: live[k][0])  # the kernel symbol with the most time in the timed region
            tot_ms, tot_flop, n = live[dom]
            ach = tot_flop / (tot_ms * 1e-3) / 1e12
            fam_ms = sum(v[0] for v in live.values())
            fam = sum(v[1] for v in live.values()) / (fam_ms * 1e-3) / 1e12
            roofline = {"bound": "mfma", "achieved": round(ach, 2), "peak": PEAK_FP16_MFMA_TFLOPS, "unit": "TFLOP/s",
                        "frac": round(ach / PEAK_FP16_MFMA_TFLOPS, 4), "traffic": None,
                        "kernel": dom + " (ArcFace 3x3 conv; fp16 in, fp32 accumulate)",
                        "launches": n, "avg_launch_us": round(1e3 * tot_ms / n, 2), "flop_per_launch": round(tot_flop / n, 1),
                        "share_of_step_time": round(tot_ms / (1e3 * dt / args.steps), 4),
                        "all_3x3_conv_kernels": {"achieved": round(fam, 2), "frac": round(fam / PEAK_FP16_MFMA_TFLOPS, 4),
                                                 "share_of_step_time": round(fam_ms / (1e3 * dt / args.steps), 4),
                                                 "per_kernel": {k: {"launches": v[2], "avg_launch_us": round(1e3 * v[0] / v[2], 2),
                                                                    "achieved": round(v[1] / (v[0] * 1e-3) / 1e12, 1)} for k, v in live.items()}},
                        "note": "achieved/frac/avg_launch_us: live HIP-event durations of every launch of the kernel in ONE step (step %d of %d) "
                                "inside the timed region; that call runs serially on the pipeline stream so that the events bracket the kernel "
                                "alone (events on every step would cost 11 %% of the step time, and under the stage-stream pipeline the bracketed "
                                "time includes other streams' dispatches)" % (args.steps, args.steps)}
            try:  # HBM bytes per launch of the dominant kernel from the committed PMC passes (tools/collect_profiles.sh)
                import glob
                for path in sorted(glob.glob(os.path.join(ROOT, "profiles", "**", "*_pmc_hbm.json"), recursive=True), reverse=True):  # newest round first
                    with open(path) as f:
                        pmc = json.load(f)
                    per = pmc.get("per_kernel", {})
                    # (profiler symbols may carry trailing template arguments the label lacks: match on the common prefix)
                    ent = per.get(dom) or next((v for k, v in per.items() if k.startswith(dom.rstrip(">")) or dom.startswith(k.rstrip(">"))), None) \
                        or (pmc if pmc.get("kernel") == dom else None)
                    if ent:
                        roofline["traffic"] = ent["hbm_bytes_per_launch"]
                        roofline["traffic_note"] = os.path.basename(path) + ": " + pmc["note"]
                        break
            except (OSError, ValueError, KeyError):
                pass

    extras = {}
    if not args.no_extras and not args.sharded_gallery:
        # ---- the other boundary, same number of steps, untimed by the contract
        other, tag = (run_resident, "hbm_resident") if not args.resident else (run_host_dist if use_dist else run_host, "host_boundary")
        other(3)
        torch.cuda.synchronize()
        if use_dist:
            dist.barrier()
        ta = time.perf_counter()
        other(args.steps)
        torch.cuda.synchronize()
        dta = time.perf_counter() - ta
        extras[tag] = {"faces_per_sec_this_rank": round(faces_per_step * args.steps / dta, 1), "ms_per_step": round(1e3 * dta / args.steps, 4),
                       "steps": args.steps,
                       "note": ("frt_pipeline_run_dev: frames and result records resident in HBM, no PCIe traffic in the region"
                                if tag == "hbm_resident" else "pinned host frames in, host records out (PCIe inclusive)")}
        # ---- steady state: the contract region includes the pipeline fill, the drain and the serial profiled step, which weigh 10 %
        #      of a 20-step region; the same loop over >= 100 steps without the profiled step is the steady-state rate
        if args.steps < 100:
            n_ss = 100
            tb = time.perf_counter()
            run(n_ss)
            torch.cuda.synchronize()
            dtb = time.perf_counter() - tb
            extras["steady_state"] = {"steps": n_ss, "faces_per_sec_this_rank": round(faces_per_step * n_ss / dtb, 1),
                                      "ms_per_step": round(1e3 * dtb / n_ss, 4),
                                      "note": "same loop as the timed region over %d steps, no profiled step (the %d-step contract region "
                                              "carries pipeline fill + drain + one serial profiled step)" % (n_ss, args.steps)}
    if not use_dist and not args.no_extras and not args.sharded_gallery:
        # ---- latency of ONE synchronous call (frt_pipeline_run: pinned host frames in, host records out, nothing else in flight)
        lat = []
        for i in range(12):
            tl = time.perf_counter()
            pipe.run(h_np[i & 1], want_embeds=False)
            lat.append(time.perf_counter() - tl)
        extras["sync_call_latency_ms"] = {"median": round(1e3 * float(np.median(lat[2:])), 3), "min": round(1e3 * float(np.min(lat[2:])), 3),
                                          "note": "frt_pipeline_run, one %d-frame batch at a time (no batches in flight): the reference's request/reply shape" % B}
    if use_dist and not args.strong and not args.sharded_gallery and not args.no_extras:
        # ---- BASELINE configs[3] as written: ONE 32-frame batch split over the ranks (strong scaling), gallery replicated
        sb, se = fd.shard_range(args.batch, rank, world)
        nb = se - sb
        if nb > 0:
            for _ in range(3):
                pipe.run_dev(d_frames[0].data_ptr(), nb, d_res[0].data_ptr(), None)
        torch.cuda.synchronize()
        dist.barrier()
        ts = time.perf_counter()
        for i in range(args.steps):
            if nb > 0:
                pipe.run_dev(d_frames[i & 1].data_ptr(), nb, d_res[i % NRING].data_ptr(), None)
        torch.cuda.synchronize()
        dts = time.perf_counter() - ts
        tt = torch.tensor([dts], dtype=torch.float64, device="cuda")
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        extras["strong_scaling"] = {"frames_per_step_total": args.batch, "frames_this_rank": nb, "faces_per_sec": round(args.batch * K * args.steps / float(tt.item()), 1),
                                    "ms_per_step": round(1e3 * float(tt.item()) / args.steps, 4),
                                    "note": "BASELINE configs[3]: one %d-frame batch split over %d ranks, HBM-resident frames" % (args.batch, world)}

    if roofline is not None and not args.no_extras:
        # Same measurement again, serially (extra untimed steps with the pipeline switched off), for the record.
        pipe.set_overlap(False)
        frt.profile_enable(1)
        for i in range(3):
            pipe.run_dev(d_frames[i & 1].data_ptr(), B, d_res[0].data_ptr(), d_emb[0].data_ptr() if args.sharded_gallery else None)
        torch.cuda.synchronize()
        labels, ms, work = frt.profile_collect()
        frt.profile_enable(0)
        pipe.set_overlap(True)
        ser = conv_table(labels, ms, work)
        if dom in ser:
            ach = ser[dom][1] / (ser[dom][0] * 1e-3) / 1e12
            roofline["serial_achieved"] = round(ach, 2)
            roofline["serial_frac"] = round(ach / PEAK_FP16_MFMA_TFLOPS, 4)
            roofline["serial_avg_launch_us"] = round(1e3 * ser[dom][0] / ser[dom][2], 2)
        # live (two earlier steps still in flight on the stage streams) against alone, per kernel: how much each loses to co-runners
        for k, e in roofline["all_3x3_conv_kernels"]["per_kernel"].items():
            if k in ser:
                e["alone_avg_launch_us"] = round(1e3 * ser[k][0] / ser[k][2], 2)

    overlap_eff = None
    if (args.stage_profile or not args.no_extras) and rank == 0:  # extra, untimed SERIAL steps with stage-level HIP events
        frt.profile_enable(2)
        for i in range(3):
            pipe.run_dev(d_frames[i & 1].data_ptr(), B, d_res[0].data_ptr(), d_emb[0].data_ptr() if args.sharded_gallery else None)
        torch.cuda.synchronize()
        labels, ms, work = frt.profile_collect()
        frt.profile_enable(0)
        agg = {}
        for l, m, w in zip(labels, ms, work):
            a = agg.setdefault(l, [0.0, 0.0, 0])
            a[0] += m
            a[1] += w
            a[2] += 1
        if args.stage_profile:
            with open(args.stage_profile, "w") as f:
                json.dump({k: {"ms_per_step": v[0] / 3, "work_per_step": v[1] / 3, "launch_groups_per_step": v[2] / 3} for k, v in agg.items()}, f, indent=1)
        st = {k: v[0] / 3 for k, v in agg.items()}
        stage_ms = {"detector": st.get("det_preprocess", 0) + st.get("det_network", 0) + st.get("det_postprocess", 0),
                    "recogniser": st.get("crop_faces", 0) + st.get("align_faces", 0) + st.get("embed_network", 0),
                    "match": st.get("match_top1", 0) + st.get("match_topk", 0) + st.get("pack_results", 0)}
        step_ms = 1e3 * dt / args.steps
        if roofline is not None and max(stage_ms.values()) > 0:
            # every stage against ITS bound (round-3 review item 14): algorithmic bytes / flops of one step over the stage's own serial time
            wk = {k: v[1] / 3 for k, v in agg.items()}
            det_bytes = DET_ACT_BYTES_PER_640_FRAME * (H * W) / (640.0 * 640.0) * B
            det_bytes16 = DET_FP16_BYTES_PER_640_FRAME * (H * W) / (640.0 * 640.0) * B
            det_flop = wk.get("det_network", 0.0)
            rec_flop = wk.get("embed_network", 0.0)
            n_rows = int(frt.lib.frt_matcher_num_rows(rec.matmul._h))
            # bytes per element of the per-call scan: int8 shadow (fp32-stored galleries, round 4), fp16 shadow / fp16-stored shard, or the fp32 rows
            scan_b = float(rec.matmul.scanBytes())   # what ONE top-1 call reads: the int8 / fp16 shadow when screened, the stored rows otherwise
            scan_bpe = int(round(scan_b / (512.0 * max(n_rows, 1))))
            i8 = scan_bpe == 1
            mt_ms = st.get("match_top1", 0) + st.get("match_topk", 0)

            def frac(x, ms, peak):
                return round(x / (ms * 1e-3) / peak, 4) if ms > 0 else None
            roofline["stages"] = {
                "detector": {"bound": "hbm", "ms": round(stage_ms["detector"], 4), "bytes": int(det_bytes), "flop": det_flop,
                             "achieved_TBps": round(det_bytes / (stage_ms["detector"] * 1e-3) / 1e12, 3) if stage_ms["detector"] > 0 else None,
                             "frac_hbm": frac(det_bytes, stage_ms["detector"], PEAK_HBM_BPS),
                             "bytes_fp16_algorithmic": int(det_bytes16),
                             "frac_hbm_fp16_algorithmic": frac(det_bytes16, stage_ms["detector"], PEAK_HBM_BPS),
                             "frac_fp32_matrix": frac(det_flop, stage_ms["detector"], PEAK_FP32_MATRIX_TFLOPS * 1e12),
                             "note": "ALGORITHMIC bytes: fp32 NCHW activations, every tensor of the layer-by-layer network written once and read once (27.45 M "
                                     "elements per 640x640 frame, DESIGN 3); since round 4 the fused stem kernel never writes two of them (-0.63 GB per 32 "
                                     "frames), so frac_hbm prices the work done, not the traffic on the bus.  "
                                     "frac_hbm_fp16_algorithmic is the same stage against SURVEY 8(d)'s own denominator (54.9 MB per frame: the tensors at "
                                     "the reference engine's fp16); the activations stay fp32 here because fp16 storage of even the first tensor moves "
                                     "7.5 % of the box coordinates against the fp32 oracle (profiles/r02/r02_det_fp16_storage_study.txt)"},
                "recogniser": {"bound": "mfma", "ms": round(stage_ms["recogniser"], 4), "flop": rec_flop,
                               "achieved_TFLOPs": round(rec_flop / (stage_ms["recogniser"] * 1e-3) / 1e12, 1) if stage_ms["recogniser"] > 0 else None,
                               "frac_mfma": frac(rec_flop, stage_ms["recogniser"], PEAK_FP16_MFMA_TFLOPS * 1e12),
                               "note": "crop + all %d faces through ArcFace; flop = every conv / linear of the pass" % F},
                "match": {"bound": "hbm", "ms": round(mt_ms, 4), "bytes": int(scan_b),
                          "achieved_TBps": round(scan_b / (mt_ms * 1e-3) / 1e12, 3) if mt_ms > 0 else None,
                          "frac_hbm": frac(scan_b, mt_ms, PEAK_HBM_BPS),
                          # the coarse scan is an fp16 MFMA GEMM [F x 512] x [512 x N]: with the int8 shadow and a full query block it is no longer
                          # HBM-bound, so its matrix-core fraction is reported beside the HBM one
                          "flop": 2.0 * 512 * n_rows * F, "frac_mfma": frac(2.0 * 512 * n_rows * F, mt_ms, PEAK_FP16_MFMA_TFLOPS * 1e12),
                          "note": "one scan of the %s per call (%d rows x 512 x %d B)" % ("int8 shadow gallery" if i8 else "gallery", n_rows, scan_bpe)},
                "note": "serial stage times: HIP events around each stage in 3 extra untimed serial steps; peaks 8 TB/s HBM, 157.3 TF fp32 matrix, 2.5 PF fp16 MFMA"}
        if max(stage_ms.values()) > 0:
            overlap_eff = {"value": round(max(stage_ms.values()) / step_ms, 4), "serial_stage_ms": {k: round(v, 4) for k, v in stage_ms.items()},
                           "serial_sum_ms": round(sum(stage_ms.values()), 4), "step_ms": round(step_ms, 4),
                           "note": "max(serial stage time) / pipelined step time: 1.0 = the step costs what its slowest stage costs alone "
                                   "(stage times: HIP events around each stage in 3 extra serial steps on this rank)"}

    # ---- the match stage under other query populations, the sustained matrix-core rate, and the strong-scaling shape (N = 1 side legs)
    match_legs = None
    proxy = None
    if rank == 0 and not use_dist and not args.no_extras and not args.sharded_gallery and not args.resident:
        def serial_match_ms():
            frt.profile_enable(2)
            for i in range(3):
                pipe.run_dev(d_frames[i & 1].data_ptr(), B, d_res[0].data_ptr(), None)
            torch.cuda.synchronize()
            lb, mm, _w = frt.profile_collect()
            frt.profile_enable(0)
            return sum(m for l, m in zip(lb, mm) if l in ("match_top1", "match_topk")) / 3.0

        def step_rate(n):
            run(3)
            torch.cuda.synchronize()
            ta = time.perf_counter()
            run(n)
            torch.cuda.synchronize()
            d = time.perf_counter() - ta
            return round(faces_per_step * n / d, 1), round(1e3 * d / n, 4)

        n_leg = max(args.steps, 50)
        n_rows = int(frt.lib.frt_matcher_num_rows(rec.matmul._h))
        match_legs = {"note": "the same pipelined step (%d steps each, untimed by the contract) with other match-stage conditions; match_stage_ms = HIP events around "
                              "the stage in 3 serial steps; answers are identical in all three modes by construction (tests/test_gpu_match.py)" % n_leg}
        if scan_mode != "exact":
            f, m = step_rate(n_leg)
            match_legs["miss"] = {"faces_per_sec": f, "ms_per_step": m, "match_stage_ms": round(serial_match_ms(), 4), "scan_bytes": rec.matmul.scanBytes(),
                                  "what": "the default workload: embeddings of synthetic faces against an i.i.d. gallery - no query matches, every query keeps ~ 11 candidate blocks for the exact re-rank"}
            # worst case: no screening at all = SURVEY 8(d)'s match (4 * 512 * N bytes per call, fp32 MFMA, fused first maximum)
            rec.matmul.setScreening(False)
            f, m = step_rate(n_leg)
            wc_ms = serial_match_ms()
            wb = rec.matmul.scanBytes()
            match_legs["worst_case"] = {"faces_per_sec": f, "ms_per_step": m, "match_stage_ms": round(wc_ms, 4), "scan_bytes": wb,
                                        "achieved_TBps": round(wb / (wc_ms * 1e-3) / 1e12, 3) if wc_ms > 0 else None,
                                        "frac_hbm": round(wb / (wc_ms * 1e-3) / PEAK_HBM_BPS, 4) if wc_ms > 0 else None,
                                        "frac_fp32_matrix": round(2.0 * 512 * n_rows * F / (wc_ms * 1e-3) / (PEAK_FP32_MATRIX_TFLOPS * 1e12), 4) if wc_ms > 0 else None,
                                        "what": "frt_matcher_set_screening(m, 0): the exact fp32 scan of the whole gallery on every call (src/matmul.h:7-16 + the "
                                                "first maximum of src/arcface.cpp:203-217 fused) - what any query population costs at most"}
            rec.matmul.setScreening(True)
            # hit: plant this workload's own embeddings in the gallery (every query then has its row, similarity 1)
            embs = []
            for hb in h_np:
                _r, e = pipe.run(hb, want_embeds=True)
                embs.append(np.array(e[:F], np.float32))
            emb = np.concatenate(embs)
            ok = np.isfinite(emb).all(axis=1) & (np.linalg.norm(emb, axis=1) > 0.5)
            rows = np.random.default_rng(11).choice(n_rows, size=len(emb), replace=False)
            g2 = np.array(gallery, np.float32, copy=True)
            g2[rows[ok]] = emb[ok]
            rec.setGallery(g2)
            rec.initMatMul()
            f, m = step_rate(n_leg)
            hit_ms = serial_match_ms()
            res_hit = h_views[(n_leg - 1) % 12]
            planted = {int(r) for r in rows[ok]}
            found = int(sum(1 for x in res_hit[res_hit["valid"] != 0]["match_idx"] if int(x) in planted))
            match_legs["hit"] = {"faces_per_sec": f, "ms_per_step": m, "match_stage_ms": round(hit_ms, 4), "scan_bytes": rec.matmul.scanBytes(),
                                 "queries_answered_with_a_planted_row": found, "queries": int((res_hit["valid"] != 0).sum()),
                                 "what": "the gallery with this workload's %d embeddings planted at random rows: every query has its own row (similarity 1), the "
                                         "screening keeps one candidate block per query" % int(ok.sum())}
            rec.setGallery(gallery)   # back to the workload's gallery
            rec.initMatMul()
            del g2
        # ---- BASELINE configs[3] as written, per-rank shape at 8 GPUs: ONE 32-frame batch split 8 ways = 4 frames per step on this GPU
        nb = max(B // 8, 1)
        for i in range(6):
            pipe.run_dev(d_frames[i & 1].data_ptr(), nb, d_res[i % NRING].data_ptr(), None)
        torch.cuda.synchronize()
        n_px = max(args.steps, 100) * 3
        tp = time.perf_counter()
        for i in range(n_px):
            pipe.run_dev(d_frames[i & 1].data_ptr(), nb, d_res[i % NRING].data_ptr(), None)
        torch.cuda.synchronize()
        ms4 = 1e3 * (time.perf_counter() - tp) / n_px
        # the DEFAULT mode of the library at the host boundary (frt_pipeline_submit / wait, adaptive pairing: a call's later stages share a pass with
        # the next call's only while the recogniser is busy anyway) and the same loop with pairing switched off
        host_legs = {}
        if not args.pair and 2 * nb <= B:
            def host_leg(n, depth_p=11):
                tk = []
                for i in range(n):
                    if len(tk) >= depth_p:
                        pipe.wait(tk.pop(0))
                    tk.append(pipe.submit(h_np[i & 1][:nb], h_views[i % 12][:nb * K]))
                for t in tk:
                    pipe.wait(t)
            try:
                for mode_p, name_p in ((-1, "adaptive"), (0, "off")):
                    pipe.set_pairing(mode_p)
                    host_leg(24)
                    pa, sa = pipe.pairing_stats()
                    tp = time.perf_counter()
                    host_leg(n_px)
                    ms_h = 1e3 * (time.perf_counter() - tp) / n_px
                    pb, sb = pipe.pairing_stats()
                    host_legs[name_p] = (ms_h, n_px / float(max(pb - pa + sb - sa, 1)))
                pipe.set_pairing(-1)
                for dq in (8, 6):
                    host_leg(24, dq)
                    tp = time.perf_counter()
                    host_leg(n_px, dq)
                    host_legs["adaptive_%d" % dq] = (1e3 * (time.perf_counter() - tp) / n_px, 0.0)
            finally:
                pipe.set_pairing(-1)
        # the same with consecutive calls GROUPED (frt_pipeline_set_pairing): one recogniser pass + one match call per two / four 4-frame calls, results
        # when the group is complete.  The pipeline of this run has room for it when the calls' face slots together fit its 32-frame capacity.
        grouped = {}
        for gsz in (2, 4):
            if gsz * nb > B or args.pair:
                continue
            try:
                pipe.set_pairing(gsz)
                for i in range(3 * gsz):
                    pipe.run_dev(d_frames[i & 1].data_ptr(), nb, d_res[i % NRING].data_ptr(), None)
                pipe.sync()
                torch.cuda.synchronize()
                pa, sa = pipe.pairing_stats()
                n_g = (n_px // gsz) * gsz
                tp = time.perf_counter()
                for i in range(n_g):
                    pipe.run_dev(d_frames[i & 1].data_ptr(), nb, d_res[i % NRING].data_ptr(), None)
                pipe.sync()
                torch.cuda.synchronize()
                ms_g = 1e3 * (time.perf_counter() - tp) / n_g
                pb, sb = pipe.pairing_stats()
                grouped[gsz] = (ms_g, gsz * (pb - pa) / float(n_g))
            finally:
                pipe.set_pairing(-1)
        ms32 = extras.get("hbm_resident", {}).get("ms_per_step")
        if "steady_state" in extras and not ms32:
            ms32 = extras["steady_state"]["ms_per_step"]
        if not ms32:
            ms32 = 1e3 * dt / args.steps
        ms_def = host_legs["adaptive"][0] if "adaptive" in host_legs else ms4
        proxy = {"frames_per_step": nb, "ms_per_%d_frame_step" % nb: round(ms_def, 4), "ms_per_%d_frame_step" % B: round(ms32, 4),
                 "projected_x_at_8": round(ms32 / ms_def, 3) if nb * 8 == B else None,
                 "measured_on_hardware": False,
                 "default_mode": None if "adaptive" not in host_legs else {
                     "ms_per_%d_frame_step" % nb: round(host_legs["adaptive"][0], 4), "calls_per_recogniser_pass": round(host_legs["adaptive"][1], 3),
                     "boundary": "frt_pipeline_submit / frt_pipeline_wait (pinned host frames in, host records out), 11 calls in flight (what the staging ring takes)",
                     "ms_per_%d_frame_step_by_calls_in_flight" % nb: {"11": round(host_legs["adaptive"][0], 4), "8": round(host_legs["adaptive_8"][0], 4),
                                                                    "6": round(host_legs["adaptive_6"][0], 4), "<=5": "as pairing_off (nothing is ever held)"},
                     "what": "the library as shipped (frt_pipeline_set_pairing(p, -1), adaptive): a submit is held back only while at least five earlier "
                             "tickets are still running; held submits are merged into ONE call (one detector pass, one recogniser pass, one match call, "
                             "up to four tickets) and released as soon as fewer than five tickets are running; a caller with up to five calls in flight "
                             "sees the unpaired pipeline and its latency (profiles/r06_adaptive_hold_sweep.txt, "
                             "tests/test_gpu_pipeline.py::test_adaptive_pairing_*)"},
                 "pairing_off": None if "off" not in host_legs else {
                     "ms_per_%d_frame_step" % nb: round(host_legs["off"][0], 4), "projected_x_at_8": round(ms32 / host_legs["off"][0], 3) if nb * 8 == B else None,
                     "calls_per_recogniser_pass": round(host_legs["off"][1], 3), "what": "same loop, frt_pipeline_set_pairing(p, 0): every call its own pass"},
                 "run_dev_unpaired": {"ms_per_%d_frame_step" % nb: round(ms4, 4), "projected_x_at_8": round(ms32 / ms4, 3) if nb * 8 == B else None,
                                      "what": "frt_pipeline_run_dev calls (HBM-resident) are never held by the default mode: the pipeline stream joins each call's results at the call"},
                 "paired": None if 2 not in grouped else {
                     "ms_per_%d_frame_step" % nb: round(grouped[2][0], 4), "projected_x_at_8": round(ms32 / grouped[2][0], 3) if nb * 8 == B else None,
                     "calls_served_by_a_shared_pass": round(grouped[2][1], 3),
                     "what": "frt_pipeline_set_pairing(p, 2): the crop + recogniser + match stages of two consecutive %d-frame calls run as ONE pass (a %d-face "
                             "recogniser pass costs 0.59 ms, a %d-face one 0.92 ms; one gallery scan instead of two); every call's detector stage is queued at "
                             "the call, its results are complete one call later.  Boxes and matched rows identical, embeddings to fp16 rounding "
                             "(tests/test_gpu_pipeline.py).  HBM-resident calls, ALWAYS pairs: it trades one step of latency for throughput" % (nb, nb * K, 2 * nb * K)},
                 "grouped_by_4": None if 4 not in grouped else {
                     "ms_per_%d_frame_step" % nb: round(grouped[4][0], 4), "projected_x_at_8": round(ms32 / grouped[4][0], 3) if nb * 8 == B else None,
                     "calls_served_by_a_shared_pass": round(grouped[4][1], 3),
                     "what": "frt_pipeline_set_pairing(p, 4): four consecutive calls per recogniser pass (%d faces) and match call; results up to three calls "
                             "later" % (4 * nb * K)},
                 "note": "single-GPU proxy for north_star's strong-scaling sentence (one %d-frame batch split over 8 GPUs, gallery replicated, no data-path "
                         "collective): a rank's step is %d frames; projected speed-up at 8 GPUs = (ms per %d-frame step on one GPU, HBM-resident) / (ms per "
                         "%d-frame step in the library's default mode, %d steps back to back with the stages of consecutive calls overlapping).  NOT a "
                         "measured scaling curve: no multi-GPU node was available to this run; the driver's SCALE file is the measurement when there is one" % (B, nb, B, nb, n_px)}
    if roofline is not None and rank == 0 and not args.no_extras:
        # what THIS device sustains on the dominant kernel's K-loop instruction mix (back-to-back fp16 MFMAs on random operands + one ds_read_b128 per MFMA
        # + the weight-fragment global loads) under its power limit: the denominator the 2.5 PFLOP/s nominal peak is not on this part (DESIGN A.1, A.15)
        try:
            sp = {"mfma_only": round(frt.probe_sustained_mfma(local_rank, 0, 0.15), 1), "mfma_lds": round(frt.probe_sustained_mfma(local_rank, 1, 0.15), 1),
                  "mfma_lds_vmem": round(frt.probe_sustained_mfma(local_rank, 2, 0.3), 1)}
            roofline["sustained_peak"] = {"value": sp["mfma_lds_vmem"], "unit": "TFLOP/s", "frac_of_nominal": round(sp["mfma_lds_vmem"] / PEAK_FP16_MFMA_TFLOPS, 4),
                                          "achieved_over_sustained": round(roofline["achieved"] / sp["mfma_lds_vmem"], 4) if sp["mfma_lds_vmem"] > 0 else None,
                                          "by_mix_TFLOPs": sp,
                                          "note": "frt_probe_sustained_mfma in this process right after the timed region: one wave per SIMD on every CU, back-to-back "
                                                  "v_mfma_f32_32x32x16_f16 on random fp16 operands (mfma_only), + one ds_read_b128 per MFMA (mfma_lds), + 4 global "
                                                  "16-byte loads per 28 MFMAs (mfma_lds_vmem = the dominant kernel's K-loop mix); ~ 0.15 - 0.3 s each; the package "
                                                  "is power-limited (1.4 kW), so the nominal 2.5 PFLOP/s is not reachable with real operands"}
        except Exception as e:  # noqa: BLE001  (a measurement aid must never cost the line)
            roofline["sustained_peak"] = {"value": None, "error": str(e)}

    # how many ranks really took part (counted over the process group, not read from the environment)
    n_ranks = 1
    if use_dist:
        nr = torch.tensor([1], dtype=torch.int64, device="cuda")
        dist.all_reduce(nr, op=dist.ReduceOp.SUM)
        n_ranks = int(nr.item())
    if n_ranks != args.gpus:
        raise SystemExit("bench.py: %d rank(s) took part, --gpus %d" % (n_ranks, args.gpus))
    if rank == 0:
        if args.sharded_gallery:
            boundary = "HBM-resident frames -> merged top-1 on the device"
            par = ("frames sharded dp%d, gallery ROW-sharded over %d rank(s) (%d rows each, fp16-stored), ncclAllGather (libfrt frt_comm) of fp16 "
                   "embeddings, per-shard exact top-%d lists with global indices, ncclAllGather of the lists + device merge (higher similarity, "
                   "then lower global index)" % (world, world, (args.gallery + world - 1) // world, args.topk))
        else:
            boundary = ("HBM-resident frames -> HBM-resident records (frt_pipeline_run_dev)" if args.resident else
                        "pinned host frames -> host records, %d batches in flight (frt_pipeline_submit/wait)" % depth)
            par = "frames sharded dp%d (%s), gallery replicated, no data-path collective%s" % (
                world, "strong: one batch split over the ranks" if args.strong else "weak: every rank its own batch",
                "; RCCL all-gather of every step's result records on a side stream inside the timed region" if gather else "")
        out = {
            "metric": "faces/sec end-to-end (detect+embed+match), 640x640 batch=32, 1M gallery",
            "value": round(total_faces_per_step * args.steps / dt, 2),
            "unit": "faces/sec",
            "n_gpus": n_ranks,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(1e3 * dt / args.steps, 4),
            "higher_is_better": True,
            "scaling": "strong" if args.strong else "weak",
            "vs_baseline": None,
            "dtype": ("f32 recogniser end to end (fp32 activations / weights, exact fp32 MFMA products)" if args.fp32 else "f16 MFMA recogniser convs (fp32 accumulate)") + " + fp32-accurate detector (fp32 MFMA, fp16 hi/lo-split MFMA for the 64-channel 3x3 convs) + "
                     + {"exact": "exact f32 MFMA match (full scan of the stored rows)",
                        "fp16": "fp16-screened coarse scan (fp16 MFMA) + exact f32 re-rank match (bit-identical to the exact f32 scan)",
                        "int8": "int8-screened coarse scan (fp16 MFMA on exactly widened int8 rows) + exact f32 re-rank match (bit-identical to the exact f32 scan)"}[scan_mode],
            "data": "synthetic",
            "config": {"workload": "%s; %dx%d frames (640x640 detector input) batch=%d frames/GPU, K=%d faces/frame, %dx512 %s gallery, "
                                   "RetinaFace-mnet0.25 + ArcFace %s" % (boundary, FW, FH, B, K, args.gallery,
                                                                         "fp16-stored row-sharded" if args.sharded_gallery else "fp32 replicated per GPU",
                                                                         "IR-50" if args.mode == "ir" else "IR-SE-50"),
                       "boundary": boundary,
                       "frames_per_step_per_gpu": B, "faces_per_frame": K, "faces_per_step": total_faces_per_step,
                       "gallery_rows": args.gallery, "h2d_bytes_per_step": 0 if (args.resident or args.sharded_gallery) else int(batches[0].nbytes),
                       "gallery_load_s": round(gallery_load_s, 3), "parallelism": par,
                       "pairing": int(args.pair),
                       "host_wait": "frt_set_wait_spin_us(%d): this driver busy-polls for results (library default 200 us, then sleeping polls)" % args.wait_spin_us},
            "roofline": roofline,
            "cpu_baseline": None,
        }
        out.update(extras)
        if match_legs:
            out["match_legs"] = match_legs
            if "worst_case" in match_legs:
                out["match_worst_case"] = match_legs["worst_case"]
        if proxy:
            out["strong_scaling_proxy"] = proxy
        if overlap_eff:
            out["overlap_efficiency"] = overlap_eff
        if smi and smi.samples:
            pw = [x["power_w"] for x in smi.samples if "power_w" in x]
            ck = [x["sclk_mhz"] for x in smi.samples if "sclk_mhz" in x]
            out["power_clock"] = {"samples": len(smi.samples), "power_w_mean": round(float(np.mean(pw)), 1) if pw else None,
                                  "power_w_max": round(float(np.max(pw)), 1) if pw else None,
                                  "sclk_mhz_mean": round(float(np.mean(ck)), 1) if ck else None,
                                  "note": "rocm-smi --showpower --showclocks sampled every 0.25 s by a side thread during the timed region"}
            if args.smi_trace:
                with open(args.smi_trace, "w") as f:
                    json.dump(smi.samples, f)
        if world == 1 and not args.no_cpu_baseline and not args.sharded_gallery:
            out["cpu_baseline"] = cpu_baseline(det_sd, rec_sd, gallery, batches[0], K)
        print(json.dumps(out), file=json_out, flush=True)
    if args.sharded_gallery and args.dump_final and rank == 0:
        torch.cuda.synchronize()
        fi, fs = final[0]
        nq = world * F
        np.savez(args.dump_final, queries_f16=(d_q16 if use_dist else d_emb16).cpu().numpy()[:nq], idx=fi.cpu().numpy()[:nq], sim=fs.cpu().numpy()[:nq],
                 gallery_rows=args.gallery, world=world, k=args.topk, gallery_seed=3)
    if use_dist:
        dist.barrier()
        cg.close()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
