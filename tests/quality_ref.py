"""Face quality restated in numpy: the contract of include/frt.h "Face quality" that the device code (kernels_quality.hip, the gate in
kernels_enrol.hip) is held to - every field for equality, the three floats to the bit.  Integers are summed in int64, the floats are one
float64 division of exact integers and one rounding to float32."""
import numpy as np

SIDE = 112
N = SIDE * SIDE                  # 12544 pixels
M = (SIDE - 2) * (SIDE - 2)      # 12100 interior pixels
SMALL, BLURRED, FLAT, DARK, BRIGHT, CLIPPED, LOW_SCORE = 1, 2, 4, 8, 16, 32, 64
FLAG_NAMES = {SMALL: "SMALL", BLURRED: "BLURRED", FLAT: "FLAT", DARK: "DARK", BRIGHT: "BRIGHT", CLIPPED: "CLIPPED", LOW_SCORE: "LOW_SCORE"}
ENROL_OK, ENROL_MANY, ENROL_NONE, ENROL_EMPTY_ROI, ENROL_LOW_QUALITY = 1, 2, 3, 4, 5

QUALITY_DTYPE = np.dtype([("sum_y", "<u4"), ("sum_y2", "<u4"), ("sum_lap", "<i4"), ("n_dark", "<u4"), ("n_bright", "<u4"), ("size", "<i4"),
                          ("sum_lap2", "<u8"), ("mean", "<f4"), ("luma_var", "<f4"), ("sharpness", "<f4"), ("score", "<f4"), ("flags", "<u4"),
                          ("present", "<i4")])
OFFSETS = dict(sum_y=0, sum_y2=4, sum_lap=8, n_dark=12, n_bright=16, size=20, sum_lap2=24, mean=32, luma_var=36, sharpness=40, score=44, flags=48,
               present=52)
RESULT_DTYPE = np.dtype([("x1", "<i4"), ("y1", "<i4"), ("x2", "<i4"), ("y2", "<i4"), ("score", "<f4"), ("frame", "<i4"), ("match_idx", "<i4"),
                         ("match_sim", "<f4"), ("valid", "<i4")])
DEFAULTS = dict(min_size=0, min_sharpness=0.0, min_luma_var=0.0, min_mean=0.0, max_mean=255.0, max_clipped=N, min_score=0.0)


def options(**kw):
    """the gate's thresholds as a dict; unnamed ones keep the defaults, under which nothing can be flagged"""
    o = dict(DEFAULTS)
    for k, v in kw.items():
        if k not in o:
            raise KeyError(k)
        o[k] = v
    return o


def luma(crop):
    """u8 BGR [112][112][3] -> Y int64 [112][112]"""
    c = np.asarray(crop).astype(np.int64)
    assert c.shape == (SIDE, SIDE, 3)
    return (29 * c[..., 0] + 150 * c[..., 1] + 77 * c[..., 2] + 128) >> 8


def laplacian(y):
    """Y [112][112] -> L int64 [110][110] on the interior"""
    return 4 * y[1:-1, 1:-1] - y[:-2, 1:-1] - y[2:, 1:-1] - y[1:-1, :-2] - y[1:-1, 2:]


def quality_one(crop, record=None, opt=None):
    """one crop (and its RESULT_DTYPE record, or None) -> one QUALITY_DTYPE record"""
    o = options() if opt is None else opt
    q = np.zeros((), QUALITY_DTYPE)
    if record is not None and int(record["valid"]) == 0:
        return q                                          # absent: all zero, the crop is not looked at
    y = luma(crop)
    lap = laplacian(y)
    sum_y, sum_y2 = int(y.sum()), int((y * y).sum())
    sum_lap, sum_lap2 = int(lap.sum()), int((lap * lap).sum())
    q["sum_y"], q["sum_y2"], q["sum_lap"], q["sum_lap2"] = sum_y, sum_y2, sum_lap, sum_lap2
    q["n_dark"], q["n_bright"] = int((y < 32).sum()), int((y > 223).sum())
    q["mean"] = np.float32(np.float64(sum_y) / np.float64(N))
    q["luma_var"] = np.float32(np.float64(N * sum_y2 - sum_y * sum_y) / np.float64(N * N))
    q["sharpness"] = np.float32(np.float64(M * sum_lap2 - sum_lap * sum_lap) / np.float64(M * M))
    flags = 0
    if record is not None:
        q["size"] = min(int(record["x2"]) - int(record["x1"]), int(record["y2"]) - int(record["y1"]))
        q["score"] = record["score"]
        if int(q["size"]) < int(o["min_size"]):
            flags |= SMALL
        if q["score"] < np.float32(o["min_score"]):
            flags |= LOW_SCORE
    if q["sharpness"] < np.float32(o["min_sharpness"]):
        flags |= BLURRED
    if q["luma_var"] < np.float32(o["min_luma_var"]):
        flags |= FLAT
    if q["mean"] < np.float32(o["min_mean"]):
        flags |= DARK
    if q["mean"] > np.float32(o["max_mean"]):
        flags |= BRIGHT
    if int(q["n_dark"]) + int(q["n_bright"]) > int(o["max_clipped"]):
        flags |= CLIPPED
    q["flags"] = flags
    q["present"] = 1
    return q


def quality(crops, records=None, opt=None):
    """crops u8 [n][112][112][3], records RESULT_DTYPE [n] or None -> QUALITY_DTYPE [n]"""
    crops = np.asarray(crops)
    out = np.zeros(crops.shape[0], QUALITY_DTYPE)
    for i in range(crops.shape[0]):
        out[i] = quality_one(crops[i], None if records is None else records[i], opt)
    return out


def passes(q):
    return (q["present"] != 0) & (q["flags"] == 0)


def enrol_select(results, quality_records=None):
    """results RESULT_DTYPE [n_frames][max_faces], quality_records QUALITY_DTYPE [n_frames][max_faces] or None -> status int32 [n_frames]:
    the "exactly one face" rule with the gate - an OK frame whose SLOT 0 record carries a flag is LOW_QUALITY"""
    status = np.zeros(results.shape[0], np.int32)
    for f in range(results.shape[0]):
        boxes = int((results[f]["score"] > 0).sum())
        st = ENROL_NONE if boxes == 0 else ENROL_MANY if boxes > 1 else ENROL_OK if results[f, 0]["valid"] != 0 else ENROL_EMPTY_ROI
        if quality_records is not None and st == ENROL_OK and quality_records[f, 0]["flags"] != 0:
            st = ENROL_LOW_QUALITY
        status[f] = st
    return status


# ---- the hand cases and the synthetic crops the tests share
def constant(b, g, r):
    c = np.empty((SIDE, SIDE, 3), np.uint8)
    c[...] = (b, g, r)
    return c


def checkerboard():
    """pixel (r, c) is 255 where r + c is odd, 0 elsewhere, on all three channels"""
    rr, cc = np.meshgrid(np.arange(SIDE), np.arange(SIDE), indexing="ij")
    return np.repeat((((rr + cc) & 1) * 255).astype(np.uint8)[..., None], 3, axis=2)


def single_pixel(r, c, value=255):
    out = np.zeros((SIDE, SIDE, 3), np.uint8)
    out[r, c] = value
    return out


def noise(seed=7):
    return np.random.default_rng(seed).integers(0, 256, (SIDE, SIDE, 3), dtype=np.uint8)


def box_blur5(crop):
    """5 x 5 box mean with edge replication, rounded to nearest (integer arithmetic)"""
    c = np.pad(crop.astype(np.int64), ((2, 2), (2, 2), (0, 0)), mode="edge")
    acc = np.zeros(crop.shape, np.int64)
    for dr in range(5):
        for dc in range(5):
            acc += c[dr:dr + SIDE, dc:dc + SIDE]
    return ((acc + 12) // 25).astype(np.uint8)


def one_channel_constant(seed=8):
    c = noise(seed)
    c[..., 1] = 200
    return c
