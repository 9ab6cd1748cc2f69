"""Face quality (frt_face_quality* / frt_enrol_select_gated_dev / frt_pipeline_run_quality / frt_pipeline_enrol_images_gated), the part that
needs no GPU: the symbols and their bindings, the record layout, and the argument checks - every one of them runs before any device work,
so on a machine without a device a refused call returns its status (not FRT_ERR_DEVICE) and leaves the output buffers' sentinel bytes
alone."""
import ctypes
import os
import re

import numpy as np

import quality_ref as qr
from conftest import ROOT

_vp, _i = ctypes.c_void_p, ctypes.c_int
SIGNATURES = {
    "frt_face_quality_dev": (_i, [_vp, _vp, _i, _vp, _vp, _vp]),
    "frt_face_quality": (_i, [_vp, _vp, _i, _vp, _vp, _i]),
    "frt_enrol_select_gated_dev": (_i, [_vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "frt_pipeline_run_quality": (_i, [_vp, _vp, _i, _vp, _vp, _vp, _vp, _vp]),
    "frt_pipeline_enrol_images_gated": (_i, [_vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, ctypes.POINTER(_i), ctypes.POINTER(_i)]),
}


def _header():
    return open(os.path.join(ROOT, "include", "frt.h")).read()


def test_entry_points_are_declared_exported_and_bound(frt):
    header = _header()
    for name, (res, args) in SIGNATURES.items():
        assert "int %s(" % name in header, name
        fn = getattr(frt.lib, name)
        assert frt.ABI[name] == (res, args) and fn.restype is res and list(fn.argtypes) == args, name
    for decl in ("int frt_face_quality_dev(const void *crops_dev, const void *results_dev /* may be NULL */, int n, const frt_quality_options *options",
                 "int frt_face_quality(const uint8_t *crops, const frt_face_result *results /* may be NULL */, int n, const frt_quality_options *options,",
                 "int frt_enrol_select_gated_dev(const void *results_dev, const void *embeds_dev, int n_frames, int max_faces, void *status_dev, void *face_dev,",
                 "int frt_pipeline_run_quality(frt_pipeline *p, const uint8_t *frames, int n_frames, const frt_quality_options *options, frt_face_result *results,",
                 "int frt_pipeline_enrol_images_gated(frt_pipeline *p, const frt_face_image *images, int n, const int32_t *labels, const frt_quality_options *options,",
                 "Face quality", "NO RECOMMENDED THRESHOLDS"):
        assert decl in header, decl
    # frt_enrol_select_dev and frt_pipeline_enrol_images keep their signatures
    assert frt.ABI["frt_enrol_select_dev"] == (_i, [_vp] * 2 + [_i] * 2 + [_vp] * 5)
    assert frt.ABI["frt_pipeline_enrol_images"] == (_i, [_vp, _vp, _i, _vp, _vp, _vp, _vp, ctypes.POINTER(_i), ctypes.POINTER(_i)])
    assert callable(frt.faceQuality) and callable(frt.face_quality_dev) and callable(frt.enrol_select_gated_dev) and callable(frt.Pipeline.runQuality)
    import inspect
    assert list(inspect.signature(frt.Pipeline.enrolImages).parameters)[-2:] == ["quality", "want_quality"]
    assert list(inspect.signature(frt.faceQuality).parameters) == ["crops", "results", "options", "device"]


def _c_struct(header, name, typedef=True):
    pat = r"typedef struct %s \{(.*?)\} %s;" % (name, name) if typedef else r"\nstruct %s \{(.*?)\};" % name
    body = re.sub(r"/\*.*?\*/", "", re.search(pat, header, re.S).group(1), flags=re.S)
    out = []
    for stmt in body.split(";"):
        stmt = stmt.strip()
        if stmt:
            ctype, names = stmt.split(None, 1)
            out += [(ctype, n.strip()) for n in names.split(",")]
    return out


def test_record_and_option_layouts(frt):
    header = _header()
    rec = _c_struct(header, "frt_face_quality", typedef=False)
    assert rec == [("uint32_t", "sum_y"), ("uint32_t", "sum_y2"), ("int32_t", "sum_lap"), ("uint32_t", "n_dark"), ("uint32_t", "n_bright"),
                   ("int32_t", "size"), ("uint64_t", "sum_lap2"), ("float", "mean"), ("float", "luma_var"), ("float", "sharpness"), ("float", "score"),
                   ("uint32_t", "flags"), ("int32_t", "present")]
    assert frt.QUALITY_DTYPE.itemsize == 56 and frt.QUALITY_DTYPE == qr.QUALITY_DTYPE
    assert {n: frt.QUALITY_DTYPE.fields[n][1] for n in frt.QUALITY_DTYPE.names} == qr.OFFSETS and qr.OFFSETS["sum_lap2"] == 24
    opt = _c_struct(header, "frt_quality_options")
    assert opt == [("int32_t", "min_size"), ("float", "min_sharpness"), ("float", "min_luma_var"), ("float", "min_mean"), ("float", "max_mean"),
                   ("int32_t", "max_clipped"), ("float", "min_score")]
    assert [f[0] for f in frt.QualityOptions._fields_] == [n for _, n in opt] and ctypes.sizeof(frt.QualityOptions) == 28
    d = frt.QualityOptions()
    assert (d.min_size, d.min_sharpness, d.min_luma_var, d.min_mean, d.max_mean, d.max_clipped, d.min_score) == (0, 0, 0, 0, 255, 12544, 0)
    assert frt.FRT_ENROL_LOW_QUALITY == 5 and re.search(r"FRT_ENROL_LOW_QUALITY = 5\b", header)
    assert (frt.FRT_ENROL_OK, frt.FRT_ENROL_MANY, frt.FRT_ENROL_NONE, frt.FRT_ENROL_EMPTY_ROI) == (1, 2, 3, 4)   # no existing value moved
    for bit, name in qr.FLAG_NAMES.items():
        assert re.search(r"FRT_QUALITY_%s = %d\b" % (name, bit), header) and getattr(frt, "QUALITY_" + name) == bit


def _bad_options(frt):
    nan = float("nan")
    return [frt.QualityOptions(min_size=-1), frt.QualityOptions(max_clipped=-1), frt.QualityOptions(min_sharpness=nan),
            frt.QualityOptions(min_luma_var=nan), frt.QualityOptions(min_mean=nan), frt.QualityOptions(max_mean=nan),
            frt.QualityOptions(min_score=nan), frt.QualityOptions(min_mean=100.0, max_mean=99.0)]


def test_refusals_come_before_any_device_work(frt):
    L, INV, CAP = frt.lib, frt.FRT_ERR_INVALID, frt.FRT_ERR_CAPACITY
    crops = np.zeros((2, 112, 112, 3), np.uint8)
    out = np.full(2 * 56, 0xA5, np.uint8)
    ok = frt.QualityOptions(min_size=10, min_mean=50.0, max_mean=50.0)      # min_mean == max_mean is allowed
    adr = ctypes.addressof

    # ---- the host form
    assert L.frt_face_quality(crops.ctypes.data, None, -1, None, out.ctypes.data, 0) == CAP
    assert L.frt_face_quality(crops.ctypes.data, None, (1 << 20) + 1, None, out.ctypes.data, 0) == CAP
    assert L.frt_face_quality(None, None, 2, None, out.ctypes.data, 0) == INV
    assert L.frt_face_quality(crops.ctypes.data, None, 2, None, None, 0) == INV
    assert L.frt_face_quality(None, None, 0, adr(ok), None, 0) == frt.FRT_OK       # nothing to do
    for bad in _bad_options(frt):
        assert L.frt_face_quality(crops.ctypes.data, None, 2, adr(bad), out.ctypes.data, 0) == INV
        assert b"quality options" in L.frt_last_error()
    # ---- the device form: 4096 stands for an aligned device address that is never touched
    assert L.frt_face_quality_dev(4096, None, -1, None, 4096, None) == CAP
    assert L.frt_face_quality_dev(4096, None, (1 << 20) + 1, None, 4096, None) == CAP
    assert L.frt_face_quality_dev(None, None, 2, None, 4096, None) == INV
    assert L.frt_face_quality_dev(4096, None, 2, None, None, None) == INV
    assert L.frt_face_quality_dev(4096 + 8, None, 2, None, 4096, None) == INV      # crops: 16-byte vectors
    assert L.frt_face_quality_dev(4096, None, 2, None, 4096 + 4, None) == INV      # records with a 64-bit field
    assert L.frt_face_quality_dev(None, None, 0, None, None, None) == frt.FRT_OK
    for bad in _bad_options(frt):
        assert L.frt_face_quality_dev(4096, None, 2, adr(bad), 4096, None) == INV
    # ---- the gated selection: frt_enrol_select_dev's refusals
    assert L.frt_enrol_select_gated_dev(None, None, -1, 4, None, None, None, None, None, None) == INV
    assert L.frt_enrol_select_gated_dev(None, None, 3, 0, None, None, None, None, None, None) == INV
    assert L.frt_enrol_select_gated_dev(None, None, 3, 4, None, None, None, None, None, None) == INV
    assert L.frt_enrol_select_gated_dev(None, None, 0, 4, None, None, None, None, None, None) == frt.FRT_OK
    assert L.frt_enrol_select_gated_dev(16, 8, 1, 1, 16, None, 16, 16, None, None) == INV
    assert L.frt_enrol_select_gated_dev(16, 16, 1, 1, 16, None, 16, 16, None, 20) == INV
    # ---- the pipeline calls: a null pipeline, null buffers and the option ranges
    frames = np.zeros((1, 8, 8, 3), np.uint8)
    res = np.full(36 * 4, 0xA5, np.uint8)
    assert L.frt_pipeline_run_quality(None, frames.ctypes.data, 1, None, res.ctypes.data, out.ctypes.data, None, None) == INV
    img = frt.FaceImage(frames.ctypes.data, 8, 8, 24)
    status = np.full(4, 0xA5, np.uint8)
    first, count = _i(-7), _i(-7)
    assert L.frt_pipeline_enrol_images_gated(None, adr(img), 1, None, None, status.ctypes.data, None, out.ctypes.data, None, ctypes.byref(first),
                                             ctypes.byref(count)) == INV
    assert b"null pipeline" in L.frt_last_error()
    for bad in _bad_options(frt):
        assert L.frt_pipeline_enrol_images_gated(None, adr(img), 1, None, adr(bad), status.ctypes.data, None, out.ctypes.data, None, ctypes.byref(first),
                                                 ctypes.byref(count)) == INV
        assert b"quality options" in L.frt_last_error()
    assert L.frt_pipeline_enrol_images_gated(None, None, 1, None, None, status.ctypes.data, None, None, None, None, None) == INV   # a NULL image array
    assert (out == 0xA5).all() and (res == 0xA5).all() and (status == 0xA5).all() and first.value == -7 and count.value == -7


def test_python_shells_refuse_bad_shapes_before_the_library(frt):
    import pytest
    with pytest.raises(ValueError):
        frt.faceQuality(np.zeros((2, 112, 111, 3), np.uint8))
    with pytest.raises(ValueError):
        frt.faceQuality(np.zeros((2, 112, 112, 3), np.uint8), np.zeros(3, frt.RESULT_DTYPE))
    with pytest.raises(TypeError):
        frt.faceQuality(np.zeros((1, 112, 112, 3), np.uint8), options=dict(min_size=3))
    with pytest.raises(frt.FrtError) as e:
        frt.faceQuality(np.zeros((1, 112, 112, 3), np.uint8), options=frt.QualityOptions(min_size=-3))
    assert e.value.code == frt.FRT_ERR_INVALID


def test_shell_declarations_are_present():
    arc = open(os.path.join(ROOT, "include", "frt", "arcface.h")).read()
    for decl in ("struct FaceQuality", "struct QualityOptions", "std::vector<FaceQuality> faceQuality(", "const QualityOptions &quality"):
        assert decl in arc, decl
