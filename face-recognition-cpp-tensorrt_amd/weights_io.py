"""FRTW weight blob: the build's replacement for the reference's serialized TensorRT ``.engine`` file.

The reference loads an opaque TensorRT engine from ``engineFile`` (``/root/reference/src/retinaface.cpp:31-55``,
``src/arcface.cpp:45-69``) that was produced offline by ``conversion/*/torch2trt.py``.  This build keeps the
"one file per network, path passed to the constructor" contract, but the file is a flat little-endian dump of the
PyTorch ``state_dict`` (names after ``module.`` prefix stripping, as ``conversion/retina/torch2trt.py:41-45`` does);
all folding (BatchNorm), layout permutes and fp16 casts happen inside ``libfrt.so`` at load time.

Layout::

    char[8]  magic  = b"FRTW0001"
    u32      kind   (1 = retinaface mobilenet0.25 trimmed, 2 = arcface IR family, 3 = arcface IR-SE family, 4 = Slim, 5 = RFB)
    u32      n_tensors
    n_tensors x { u16 name_len; char name[name_len]; u8 ndim; u32 dims[ndim]; u64 offset; u64 n_elem }
    ... padding to a 64-byte boundary ...
    float32 data, every tensor 64-byte aligned; ``offset`` is relative to the start of the file.

Kinds 2 and 3 hold any depth of ``conversion/arcface/model_irse.py``: IR-50 / IR-100 / IR-152 (``IR_50``, ``IR_101``, ``IR_152``) and
their SE variants.  ``libfrt.so`` reads the depth from the tensors (``frt_embedder_describe``); the exporter's ``--kind`` names the depth
too and refuses a checkpoint whose tensors are another backbone::

    python weights_io.py backbone_ir50_asia.pth rec.frtw --kind ir50       # also: ir100, ir152, ir_se50, ir_se100, ir_se152

Kinds 4 and 5 are the other two detectors ``conversion/retina/torch2trt.py --network slim | RFB`` exports (``net_slim.py``,
``net_rfb.py``), with or without their landmark heads::

    python weights_io.py slim_Final.pth det.frtw --kind slim               # also: rfb (or RFB), retinaface
"""
import struct
from collections import OrderedDict

import numpy as np

MAGIC = b"FRTW0001"
KIND_RETINAFACE_MNET025 = 1
KIND_ARCFACE_IR50 = 2
KIND_ARCFACE_IR_SE50 = 3
KIND_RETINAFACE_SLIM = 4
KIND_RETINAFACE_RFB = 5
KIND_ARCFACE_IR = KIND_ARCFACE_IR50        # the IR family of any depth
KIND_ARCFACE_IR_SE = KIND_ARCFACE_IR_SE50  # the IR-SE family of any depth
# --kind -> (blob kind, layers, SE) for the recogniser backbones of model_irse.py
ARCFACE_KINDS = {"ir50": (2, 50, False), "ir100": (2, 100, False), "ir152": (2, 152, False),
                 "ir_se50": (3, 50, True), "ir_se100": (3, 100, True), "ir_se152": (3, 152, True)}
IR_STAGES = {50: (3, 4, 14, 3), 100: (3, 13, 30, 3), 152: (3, 8, 36, 3)}  # model_irse.py get_blocks


def _align(n, a=64):
    return (n + a - 1) // a * a


def write_blob(path, state, kind):
    """Write ``state`` (ordered mapping name -> float32 ndarray) as an FRTW blob."""
    items = []
    for name, arr in state.items():
        if name.endswith("num_batches_tracked"):
            continue
        a = np.ascontiguousarray(np.asarray(arr, dtype=np.float32))
        items.append((name, a))
    header_len = 8 + 4 + 4
    for name, a in items:
        header_len += 2 + len(name.encode()) + 1 + 4 * a.ndim + 8 + 8
    off = _align(header_len)
    offsets = []
    for _, a in items:
        offsets.append(off)
        off = _align(off + a.size * 4)
    with open(path, "wb") as f:
        f.write(MAGIC)
        f.write(struct.pack("<II", kind, len(items)))
        for (name, a), o in zip(items, offsets):
            nb = name.encode()
            f.write(struct.pack("<H", len(nb)))
            f.write(nb)
            f.write(struct.pack("<B", a.ndim))
            for d in a.shape:
                f.write(struct.pack("<I", d))
            f.write(struct.pack("<QQ", o, a.size))
        pos = f.tell()
        for (name, a), o in zip(items, offsets):
            if o > pos:
                f.write(b"\0" * (o - pos))
            f.write(a.tobytes())
            pos = o + a.size * 4
    return path


def read_blob(path):
    """Read an FRTW blob back -> (kind, OrderedDict name -> ndarray).  Used by tests only."""
    with open(path, "rb") as f:
        buf = f.read()
    assert buf[:8] == MAGIC, "not an FRTW blob"
    kind, n = struct.unpack_from("<II", buf, 8)
    p = 16
    out = OrderedDict()
    for _ in range(n):
        (ln,) = struct.unpack_from("<H", buf, p)
        p += 2
        name = buf[p:p + ln].decode()
        p += ln
        ndim = buf[p]
        p += 1
        dims = struct.unpack_from("<" + "I" * ndim, buf, p)
        p += 4 * ndim
        off, ne = struct.unpack_from("<QQ", buf, p)
        p += 16
        out[name] = np.frombuffer(buf, dtype=np.float32, count=ne, offset=off).reshape(dims).copy()
    return kind, out


def arcface_layout(state):
    """(num_layers, se) of an IR / IR-SE state dict; ValueError naming the first tensor that does not fit one of the six backbones.
    The same rules as libfrt's loader (csrc/frt_weights.hpp arc_layout), restated on the names and shapes."""
    n = 0
    while "body.%d.res_layer.1.weight" % n in state:
        n += 1
    se = "body.0.res_layer.5.fc1.weight" in state
    stages, prev = [], 64
    for i in range(n):
        p = "body.%d" % i
        depth, cin = np.shape(state[p + ".res_layer.1.weight"])[:2]
        sc = p + ".shortcut_layer.0.weight" in state
        if i == 0 or sc or depth != prev:
            stages.append(0)
        stages[-1] += 1
        if len(stages) > 4 or depth != (64, 128, 256, 512)[len(stages) - 1] or cin != prev or sc != (cin != depth):
            raise ValueError("%s.res_layer.1.weight: unit %d does not fit an IR backbone" % (p, i))
        if (p + ".res_layer.5.fc1.weight" in state) != se:
            raise ValueError("%s.res_layer.5.fc1.weight: SE units mixed with plain ones" % p)
        prev = depth
    left = sorted(k for k in state if k.startswith("body.") and not (k.split(".")[1].isdigit() and int(k.split(".")[1]) < n))
    if left:
        raise ValueError("unexpected tensor %s" % left[0])
    for layers, table in IR_STAGES.items():
        if tuple(stages) == table:
            return layers, se
    raise ValueError("body.0 - body.%d: stage table %s is none of %s" % (n - 1, tuple(stages), sorted(IR_STAGES.values())))


DETECTOR_KINDS = {"retinaface": KIND_RETINAFACE_MNET025, "slim": KIND_RETINAFACE_SLIM, "rfb": KIND_RETINAFACE_RFB, "RFB": KIND_RETINAFACE_RFB}
_DETECTOR_NAMES = {KIND_RETINAFACE_MNET025: "RetinaFace mobilenet0.25", KIND_RETINAFACE_SLIM: "Slim", KIND_RETINAFACE_RFB: "RFB"}


def detector_family(state):
    """Blob kind of a detector state dict by its distinctive tensors: 5 (RFB: conv8 is a BasicRFB), 4 (Slim: conv8 is a conv_dw block),
    1 (mnet0.25: body.stage1.*); ValueError when it is none of them.  The full tensor-by-tensor check is libfrt's
    (frt_detector_describe)."""
    if any(k.startswith("conv8.branch0.") for k in state):
        return KIND_RETINAFACE_RFB
    if "conv8.0.weight" in state and "conv14.0.weight" in state:
        return KIND_RETINAFACE_SLIM
    if any(k.startswith("body.stage1.") for k in state):
        return KIND_RETINAFACE_MNET025
    raise ValueError("not a RetinaFace mobilenet0.25 / Slim / RFB state dict (no body.stage1.*, conv8.0.* or conv8.branch0.* tensors)")


def export_pth(pth_path, out_path, kind):
    """``.pth`` -> FRTW blob; the replacement for ``conversion/*/torch2trt.py``.

    Strips the ``module.`` prefix and unwraps a ``state_dict`` key exactly like
    ``/root/reference/conversion/retina/torch2trt.py:41-61``.

    ``kind`` is a blob kind (1 - 5), a name of ``ARCFACE_KINDS`` or of ``DETECTOR_KINDS``; a named kind refuses (ValueError) a checkpoint
    whose tensors are another backbone / detector.
    """
    import torch

    sd = torch.load(pth_path, map_location="cpu")
    if isinstance(sd, dict) and "state_dict" in sd:
        sd = sd["state_dict"]
    clean = OrderedDict()
    for k, v in sd.items():
        k = k.split("module.", 1)[-1] if k.startswith("module.") else k
        clean[k] = v.detach().cpu().float().numpy()
    if kind in ARCFACE_KINDS:
        kind, layers, se = ARCFACE_KINDS[kind]
        got = arcface_layout(clean)
        if got != (layers, se):
            raise ValueError("%s holds IR%s-%d, not the IR%s-%d asked for" % (pth_path, "-SE" if got[1] else "", got[0], "-SE" if se else "", layers))
    elif kind in DETECTOR_KINDS:
        kind = DETECTOR_KINDS[kind]
        got = detector_family(clean)
        if got != kind:
            raise ValueError("%s holds a %s detector, not the %s asked for" % (pth_path, _DETECTOR_NAMES[got], _DETECTOR_NAMES[kind]))
    return write_blob(out_path, clean, kind)


if __name__ == "__main__":
    import argparse

    ap = argparse.ArgumentParser(description="Export a PyTorch .pth checkpoint to an FRTW weight blob")
    ap.add_argument("pth")
    ap.add_argument("out")
    ap.add_argument("--kind", choices=list(DETECTOR_KINDS) + list(ARCFACE_KINDS), required=True)
    a = ap.parse_args()
    export_pth(a.pth, a.out, a.kind)
