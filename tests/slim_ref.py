"""CPU restatement of the Slim / RFB detectors for the tests (no test_* file: a helper module).

* ``forward(sd, x, rfb)``: a ``torch.nn.functional`` forward of ``net_slim.Slim`` / ``net_rfb.RFB`` in ``phase='test'`` over the flat
  state dict (``synth.slim_state``) -> (loc [B,A,4], conf [B,A,2] softmaxed, ldm [B,A,10] or None).
* ``anchors(w, h, table)`` / ``postprocess(...)``: ``oracle/postproc.c`` (the reference's ``RetinaFace::postprocessing``) restated in
  Python with the anchor table as a parameter - the same double/float mix, both truncations, strict ``>`` threshold, ``>=`` NMS with
  ``+1`` areas, cap after the NMS, ties by anchor index.  With ``MNET`` it must equal ``oracle.postprocess`` exactly.
"""
import math

import numpy as np

MNET = dict(steps=(8, 16, 32), min_sizes=((10, 20), (32, 64), (128, 256)))
SLIM = dict(steps=(8, 16, 32, 64), min_sizes=((10, 16, 24), (32, 48), (64, 96), (128, 192, 256)))  # cfg_slim == cfg_rfb
BBOX_DTYPE = np.dtype([("x1", "<i4"), ("y1", "<i4"), ("x2", "<i4"), ("y2", "<i4"), ("score", "<f4")])


def _bn(sd, p, x):
    import torch.nn.functional as F
    t = lambda n: _t(sd[p + n])
    return F.batch_norm(x, t(".running_mean"), t(".running_var"), t(".weight"), t(".bias"), False, 0.0, 1e-5)


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a))


def forward(sd, x, rfb=False):
    import torch
    import torch.nn.functional as F
    relu = F.relu
    w = lambda n: _t(sd[n])
    with torch.no_grad():
        h = _t(np.asarray(x, np.float32))

        def conv_dw(p, h, stride):
            c = h.shape[1]
            h = relu(_bn(sd, p + ".1", F.conv2d(h, w(p + ".0.weight"), None, stride, 1, 1, c)))
            return relu(_bn(sd, p + ".4", F.conv2d(h, w(p + ".3.weight"))))

        def basic(p, h, pad=0, dil=1, act=True):
            h = _bn(sd, p + ".bn", F.conv2d(h, w(p + ".conv.weight"), None, 1, pad, dil))
            return relu(h) if act else h

        def rfb_block(h):
            b0 = basic("conv8.branch0.2", basic("conv8.branch0.1", basic("conv8.branch0.0", h, act=False), 1), 2, 2, False)
            b1 = basic("conv8.branch1.2", basic("conv8.branch1.1", basic("conv8.branch1.0", h, act=False), 1), 3, 3, False)
            b2 = basic("conv8.branch2.1", basic("conv8.branch2.0", h, act=False), 1)
            b2 = basic("conv8.branch2.3", basic("conv8.branch2.2", b2, 1), 5, 5, False)
            out = basic("conv8.ConvLinear", torch.cat((b0, b1, b2), 1), act=False)
            return relu(out * 1.0 + basic("conv8.shortcut", h, act=False))

        h = relu(_bn(sd, "conv1.1", F.conv2d(h, w("conv1.0.weight"), None, 2, 1)))
        strides = [1, 2, 1, 2, 1, 1, 1, 2, 1, 1, 2, 1]
        feats = []
        for i, s in enumerate(strides):
            n = i + 2
            h = rfb_block(h) if (rfb and n == 8) else conv_dw("conv%d" % n, h, s)
            if n in (8, 11, 13):
                feats.append(h)
        h = relu(F.conv2d(h, w("conv14.0.weight"), w("conv14.0.bias")))
        h = relu(F.conv2d(h, w("conv14.2.0.weight"), w("conv14.2.0.bias"), 2, 1, 1, 64))
        feats.append(relu(F.conv2d(h, w("conv14.2.2.weight"), w("conv14.2.2.bias"))))
        ldm = "landm.0.0.weight" in sd
        outs = {}
        for head, per in (("loc", 4), ("conf", 2), ("landm", 10)):
            if head == "landm" and not ldm:
                continue
            parts = []
            for k, f in enumerate(feats):
                if k < 3:
                    p = "%s.%d" % (head, k)
                    y = relu(F.conv2d(f, w(p + ".0.weight"), w(p + ".0.bias"), 1, 1, 1, f.shape[1]))
                    y = F.conv2d(y, w(p + ".2.weight"), w(p + ".2.bias"))
                else:
                    y = F.conv2d(f, w("%s.3.weight" % head), w("%s.3.bias" % head), 1, 1)
                parts.append(y.permute(0, 2, 3, 1).reshape(y.shape[0], -1, per))
            outs[head] = torch.cat(parts, 1)
        conf = F.softmax(outs["conf"], dim=-1)
        return outs["loc"].numpy(), conf.numpy(), (outs["landm"].numpy() if ldm else None)


def feature_maps(w, h, table):
    return [(int(math.ceil(h / np.float32(s))), int(math.ceil(w / np.float32(s)))) for s in table["steps"]]


def anchor_count(w, h, table=SLIM):
    return sum(fh * fw * len(ms) for (fh, fw), ms in zip(feature_maps(w, h, table), table["min_sizes"]))


def anchors(w, h, table=SLIM):
    """create_anchor_retinaface (retinaface.cpp:210-240) with the table's steps / sizes -> float32 [A,4] (cx, cy, sx, sy).
    Order: level, row, column, size.  Priors in double narrowed to float."""
    out = []
    for (fh, fw), step, ms in zip(feature_maps(w, h, table), table["steps"], table["min_sizes"]):
        i, j, l = np.meshgrid(np.arange(fh), np.arange(fw), np.arange(len(ms)), indexing="ij")
        msz = np.array(ms, np.float64)[l]
        a = np.stack([(j + 0.5) * float(step) / w, (i + 0.5) * float(step) / h, msz * 1.0 / w, msz * 1.0 / h], -1)
        out.append(a.reshape(-1, 4).astype(np.float32))
    return np.concatenate(out)


def _trunc(v):
    return np.trunc(v).astype(np.int64)


def postprocess(loc, conf, in_w, in_h, frame_w, frame_h, nms_thr=0.4, bbox_thr=0.6, max_faces=4, table=SLIM, return_kept=False):
    """orc_postprocess (oracle/postproc.c) with the anchor table as a parameter -> structured array of Bbox (and the kept anchors)."""
    loc = np.ascontiguousarray(loc, np.float32).reshape(-1, 4)
    conf = np.ascontiguousarray(conf, np.float32).reshape(-1, 2)
    anc = anchors(in_w, in_h, table)
    assert loc.shape[0] == anc.shape[0] == conf.shape[0], (loc.shape, anc.shape)
    f32 = np.float32
    scale_h = f32(in_h) / f32(frame_h)
    scale_w = f32(in_w) / f32(frame_w)
    score = conf[:, 1]
    idx = np.nonzero(score > f32(bbox_thr))[0]
    a = anc[idx].astype(np.float64)
    bb = loc[idx].astype(np.float64)
    # decode: double intermediates, float fields
    cx = (a[:, 0] + bb[:, 0] * 0.1 * a[:, 2]).astype(f32)
    cy = (a[:, 1] + bb[:, 1] * 0.1 * a[:, 3]).astype(f32)
    dexp = np.vectorize(lambda v: math.exp(v) if v < 709 else math.inf, otypes=[np.float64])  # libm exp, as the C restatement
    sx = (a[:, 2] * dexp(bb[:, 2] * 0.2)).astype(f32) if len(idx) else np.zeros(0, f32)
    sy = (a[:, 3] * dexp(bb[:, 3] * 0.2)).astype(f32) if len(idx) else np.zeros(0, f32)
    two = f32(2)
    with np.errstate(invalid="ignore", over="ignore"):
        y1 = _trunc((cx - sx / two) * f32(in_w))
        x1 = _trunc((cy - sy / two) * f32(in_h))
        y2 = _trunc((cx + sx / two) * f32(in_w))
        x2 = _trunc((cy + sy / two) * f32(in_h))
        if scale_h > scale_w:
            pad = (f32(in_h) - scale_w * f32(frame_h)) / two
            y1, y2 = _trunc(y1.astype(f32) / scale_w), _trunc(y2.astype(f32) / scale_w)
            x1, x2 = _trunc((x1.astype(f32) - pad) / scale_w), _trunc((x2.astype(f32) - pad) / scale_w)
        else:
            pad = (f32(in_w) - scale_h * f32(frame_w)) / two
            y1, y2 = _trunc((y1.astype(f32) - pad) / scale_h), _trunc((y2.astype(f32) - pad) / scale_h)
            x1, x2 = _trunc(x1.astype(f32) / scale_h), _trunc(x2.astype(f32) / scale_h)
    y1, y2 = np.clip(y1, 0, frame_w - 1), np.clip(y2, 0, frame_w - 1)
    x1, x2 = np.clip(x1, 0, frame_h - 1), np.clip(x2, 0, frame_h - 1)
    sc = score[idx]
    order = np.lexsort((idx, -sc.astype(np.float64)))  # score descending, ties by anchor index
    n = len(order)
    area = ((x2 - x1 + 1) * (y2 - y1 + 1)).astype(f32)
    dead = np.zeros(n, bool)
    keep = []
    for ii in range(n):
        i = order[ii]
        if dead[ii]:
            continue
        keep.append(i)
        if len(keep) == max_faces:
            break
        rest = order[ii + 1:]
        xx1 = np.maximum(x1[i], x1[rest]).astype(f32)
        yy1 = np.maximum(y1[i], y1[rest]).astype(f32)
        xx2 = np.minimum(x2[i], x2[rest]).astype(f32)
        yy2 = np.minimum(y2[i], y2[rest]).astype(f32)
        w_ = np.maximum(f32(0), xx2 - xx1 + f32(1))
        h_ = np.maximum(f32(0), yy2 - yy1 + f32(1))
        inter = w_ * h_
        with np.errstate(invalid="ignore", divide="ignore"):
            ovr = inter / (area[i] + area[rest] - inter)
        dead[ii + 1:] |= ovr >= f32(nms_thr)
    out = np.zeros(len(keep), BBOX_DTYPE)
    for m, i in enumerate(keep):
        out[m] = (x1[i], y1[i], x2[i], y2[i], sc[i])
    if return_kept:
        return out, idx[np.array(keep, np.int64)] if keep else np.zeros(0, np.int64)
    return out
