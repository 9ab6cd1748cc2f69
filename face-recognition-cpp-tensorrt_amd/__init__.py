"""MI355X-native detect -> crop -> embed -> match hot path of nghiapq77/face-recognition-cpp-tensorrt.

The product is ``libfrt.so`` (hand-written HIP for gfx950 behind the C ABI of ``include/frt.h``).  This package is the
Python-side mirror of the reference's class surface - ``RetinaFace`` (``/root/reference/src/retinaface.h:18-23``),
``ArcFaceIR50`` (``src/arcface.h:19-39``), ``MatMul`` (``src/matmul.h:6-21``), ``getCroppedFaces`` (``src/arcface.h:17``)
- used by the tests and by ``bench.py``; the C++ drop-in shells live in ``include/frt/*.h``.  Every call goes through the
C ABI; there is no Python/CPU fallback: if ``libfrt.so`` is missing the import fails.

The directory name is not an importable identifier; load it with::

    import importlib.util, sys
    spec = importlib.util.spec_from_file_location("frt_amd", ".../face-recognition-cpp-tensorrt_amd/__init__.py",
                                                  submodule_search_locations=[".../face-recognition-cpp-tensorrt_amd"])
    frt_amd = importlib.util.module_from_spec(spec); sys.modules["frt_amd"] = frt_amd; spec.loader.exec_module(frt_amd)
"""
import ctypes
import os
import sys
import weakref

import numpy as np

from . import dist, synth, weights_io  # noqa: F401

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("FRT_LIB") or os.path.join(_HERE, "libfrt.so")  # FRT_LIB: another build of the library (A/B runs: bench.py --ab-old-lib), tools only

if not os.path.exists(LIB_PATH):
    raise ImportError("libfrt.so not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                      "(or `make -C face-recognition-cpp-tensorrt_amd/csrc`).  There is no CPU fallback.")

lib = ctypes.CDLL(LIB_PATH)

# ----------------------------------------------------------------------------------------------------------------------
# C ABI declarations (include/frt.h)
# ----------------------------------------------------------------------------------------------------------------------
FRT_OK, FRT_ERR_INVALID, FRT_ERR_NOT_FOUND, FRT_ERR_FORMAT, FRT_ERR_DEVICE, FRT_ERR_EMPTY, FRT_ERR_EMPTY_ROI, FRT_ERR_CAPACITY = range(8)
FRT_ENROL_OK, FRT_ENROL_MANY, FRT_ENROL_NONE, FRT_ENROL_EMPTY_ROI = 1, 2, 3, 4  # frt_enrol_status: the "exactly one face" rule of /insert/face
FRT_ENROL_LOW_QUALITY = 5  # ... and the gate of the quality-gated calls: one valid face whose quality record carries a flag

BBOX_DTYPE = np.dtype([("x1", "<i4"), ("y1", "<i4"), ("x2", "<i4"), ("y2", "<i4"), ("score", "<f4")])  # == struct Bbox, common.h:13-16
RESULT_DTYPE = np.dtype([("x1", "<i4"), ("y1", "<i4"), ("x2", "<i4"), ("y2", "<i4"), ("score", "<f4"), ("frame", "<i4"),
                         ("match_idx", "<i4"), ("match_sim", "<f4"), ("valid", "<i4")])
assert BBOX_DTYPE.itemsize == 20 and RESULT_DTYPE.itemsize == 36

_vp, _i, _f, _sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_size_t
ABI = {
    "frt_last_error": (ctypes.c_char_p, []),
    "frt_version": (ctypes.c_char_p, []),
    "frt_device_count": (_i, []),
    "frt_set_wait_spin_us": (ctypes.c_long, [ctypes.c_long]),
    "frt_detector_create": (_i, [ctypes.c_char_p, _i, _i, _i, _i, _i, _i, _i, _f, _f, _i, ctypes.POINTER(_vp)]),
    "frt_detector_destroy": (None, [_vp]),
    "frt_detector_num_anchors": (_i, [_vp]),
    "frt_detector_describe": (_i, [ctypes.c_char_p, ctypes.POINTER(_i), ctypes.POINTER(_i), ctypes.POINTER(_i)]),
    "frt_detector_find_faces": (_i, [_vp, _vp, _i, _i, _sz, _vp, _vp]),
    "frt_detector_find_faces_batch": (_i, [_vp, _vp, _i, _i, _i, _sz, _sz, _vp, _vp]),
    "frt_detector_preprocess": (_i, [_vp, _vp, _i, _i, _sz, _vp]),
    "frt_detector_infer": (_i, [_vp, _vp, _i, _vp, _vp]),
    "frt_detector_postprocess": (_i, [_vp, _vp, _vp, _vp, _vp]),
    "frt_crop_faces": (_i, [_vp, _i, _i, _sz, _vp, _i, _i, _i, _vp, _i]),
    "frt_resize_frame": (_i, [_vp, _i, _i, _sz, _vp, _i, _i, _i]),
    "frt_resize_frames_dev": (_i, [_vp, _i, _i, _i, _sz, _sz, _vp, _i, _i, _vp]),
    "frt_embedder_create": (_i, [ctypes.c_char_p, _i, _i, _i, _i, _i, _i, ctypes.POINTER(_vp)]),
    "frt_embedder_destroy": (None, [_vp]),
    "frt_embedder_describe": (_i, [ctypes.c_char_p, ctypes.POINTER(_i), ctypes.POINTER(_i), ctypes.POINTER(_i)]),
    "frt_embedder_preprocess_face": (_i, [_vp, _vp, _vp]),
    "frt_embedder_infer": (_i, [_vp, _vp, _i, _vp]),
    "frt_embedder_forward": (_i, [_vp, _vp, _i, _i, _sz, _vp, _i, _vp, _vp]),
    "frt_matcher_create": (_i, [_i, ctypes.POINTER(_vp)]),
    "frt_matcher_destroy": (None, [_vp]),
    "frt_matcher_init": (_i, [_vp, _vp, _i, _i]),
    "frt_matcher_set_row_offset": (_i, [_vp, _i]),
    "frt_probe_sustained_mfma": (_i, [_i, _i, ctypes.c_double, ctypes.POINTER(ctypes.c_double)]),
    "frt_matcher_set_storage": (_i, [_vp, _i]),
    "frt_matcher_set_screening": (_i, [_vp, _i]),
    "frt_matcher_scan_bytes": (ctypes.c_size_t, [_vp]),
    "frt_matcher_generation": (ctypes.c_uint, [_vp]),
    "frt_matcher_gallery_begin": (_i, [_vp, _i, _i]),
    "frt_matcher_gallery_append": (_i, [_vp, _vp, _i]),
    "frt_matcher_gallery_commit": (_i, [_vp]),
    "frt_matcher_num_rows": (_i, [_vp]),
    "frt_matcher_gallery_reserve": (_i, [_vp, _i]),
    "frt_matcher_gallery_add": (_i, [_vp, _vp, _i]),
    "frt_matcher_gallery_add_dev": (_i, [_vp, _vp, _i]),
    "frt_matcher_gallery_remove": (_i, [_vp, _vp, _i]),
    "frt_matcher_edit_stats": (_i, [_vp, _vp]),
    "frt_matcher_top1_dev": (_i, [_vp, _vp, _i, _vp, _vp, _vp]),
    "frt_matcher_calculate": (_i, [_vp, _vp, _i, _vp]),
    "frt_matcher_top1": (_i, [_vp, _vp, _i, _vp, _vp]),
    "frt_matcher_calculate_top1": (_i, [_vp, _vp, _i, _vp, _vp, _vp]),
    "frt_pinned_alloc": (_i, [_sz, _i, ctypes.POINTER(_vp)]),
    "frt_pinned_free": (None, [_vp]),
    "frt_merge_top1": (_i, [_i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "frt_matcher_topk": (_i, [_vp, _vp, _i, _i, _vp, _vp]),
    "frt_matcher_topk_dev": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp, _vp]),
    "frt_merge_topk": (_i, [_i, _i, _i, _vp, _vp, _vp, _vp]),
    "frt_merge_topk_dev": (_i, [_i, _i, _i, _vp, _vp, _vp, _vp, _vp]),
    "frt_matcher_set_labels": (_i, [_vp, _vp, _i]),
    "frt_matcher_labels_info": (_i, [_vp, ctypes.POINTER(_i), ctypes.POINTER(_i)]),
    "frt_matcher_gallery_add_labeled": (_i, [_vp, _vp, _vp, _i]),
    "frt_matcher_gallery_add_labeled_dev": (_i, [_vp, _vp, _vp, _i]),
    "frt_matcher_topk_labels": (_i, [_vp, _vp, _i, _i, _vp, _vp, _vp]),
    "frt_matcher_topk_labels_dev": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp]),
    "frt_merge_topk_labels": (_i, [_i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "frt_merge_topk_labels_dev": (_i, [_i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "frt_matcher_build_templates": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "frt_matcher_cluster": (_i, [_vp, _f, _vp, _i, _vp]),
    "frt_matcher_cluster_dev": (_i, [_vp, _f, _vp, _vp, _vp]),
    "frt_matcher_separation": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _vp, _vp]),
    "frt_matcher_separation_dev": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp]),
    "frt_embeds_to_half_dev": (_i, [_vp, _sz, _vp, _vp]),
    "frt_comm_get_unique_id": (_i, [_vp]),
    "frt_comm_set_bootstrap_timeout": (ctypes.c_double, [ctypes.c_double]),
    "frt_comm_create": (_i, [_vp, _i, _i, _i, ctypes.POINTER(_vp)]),
    "frt_comm_create_all": (_i, [_i, _vp, _vp]),
    "frt_comm_destroy": (None, [_vp]),
    "frt_comm_rank": (_i, [_vp]),
    "frt_comm_world": (_i, [_vp]),
    "frt_comm_stream": (_vp, [_vp]),
    "frt_comm_all_gather": (_i, [_vp, _vp, _vp, _sz, _vp]),
    "frt_comm_all_gather_multi": (_i, [_i, _vp, _vp, _vp, _sz, _vp]),
    "frt_comm_sync": (_i, [_vp]),
    "frt_embedder_set_se_fused": (_i, [_vp, _i]),
    "frt_embedder_set_precision": (_i, [_vp, _i]),
    "frt_embedder_set_flip": (_i, [_vp, _i]),
    "frt_embedder_get_flip": (_i, [_vp, ctypes.POINTER(_i)]),
    "frt_jpeg_encode_batch_after": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _vp, _sz, _vp, _vp]),
    "frt_detector_geometry": (_i, [_vp, _vp, _vp, _vp, _vp, _vp]),
    "frt_coalescer_create": (_i, [_vp, _vp, _vp, _i, _i, ctypes.POINTER(_vp)]),
    "frt_coalescer_destroy": (None, [_vp]),
    "frt_coalescer_infer": (_i, [_vp, _vp, _i, _i, _sz, _vp, _vp, _vp]),
    "frt_coalescer_infer_crops": (_i, [_vp, _vp, _i, _i, _sz, _vp, _vp, _vp, _vp]),
    "frt_pipeline_submit_crops": (_i, [_vp, _vp, _i, _vp, _vp, _vp, ctypes.POINTER(ctypes.c_long)]),
    "frt_coalescer_stats": (_i, [_vp, _vp, _vp]),
    "frt_pipeline_create": (_i, [_vp, _vp, _vp, _i, ctypes.POINTER(_vp)]),
    "frt_pipeline_destroy": (None, [_vp]),
    "frt_pipeline_run": (_i, [_vp, _vp, _i, _vp, _vp]),
    "frt_pipeline_run_dev": (_i, [_vp, _vp, _i, _vp, _vp]),
    "frt_pipeline_run_dev_after": (_i, [_vp, _vp, _i, _vp, _vp, _vp]),
    "frt_pipeline_set_input_sync": (_i, [_vp, _i]),
    "frt_pipeline_check_overlap": (_i, [_vp, _vp]),
    "frt_pipeline_submit": (_i, [_vp, _vp, _i, _vp, _vp, ctypes.POINTER(ctypes.c_long)]),
    "frt_pipeline_wait": (_i, [_vp, ctypes.c_long]),
    "frt_pipeline_sync": (_i, [_vp]),
    "frt_pipeline_set_stream": (_i, [_vp, _vp]),
    "frt_pipeline_set_overlap": (_i, [_vp, _i]),
    "frt_pipeline_set_graph": (_i, [_vp, _i]),
    "frt_pipeline_set_pairing": (_i, [_vp, _i]),
    "frt_pipeline_pairing_stats": (_i, [_vp, _vp, _vp]),
    "frt_pipeline_graph_stats": (_i, [_vp, _vp, _vp]),
    "frt_pipeline_merge_stats": (_i, [_vp, _vp, _vp]),
    "frt_detector_has_landmarks": (_i, [_vp]),
    "frt_detector_find_faces_landmarks": (_i, [_vp, _vp, _i, _i, _sz, _vp, _vp, _vp]),
    "frt_detector_infer_landmarks": (_i, [_vp, _vp, _i, _vp, _vp, _vp]),
    "frt_align_faces": (_i, [_vp, _i, _i, _sz, _vp, _i, _vp, _i]),
    "frt_embedder_forward_aligned": (_i, [_vp, _vp, _i, _i, _sz, _vp, _i, _vp, _vp]),
    "frt_pipeline_set_align": (_i, [_vp, _i]),
    "frt_jpeg_info": (_i, [_vp, _sz, _vp, _vp, _vp]),
    "frt_jpeg_decoder_create": (_i, [_i, _i, _i, _i, _i, ctypes.POINTER(_vp)]),
    "frt_jpeg_decoder_destroy": (None, [_vp]),
    "frt_jpeg_decode_batch_dev": (_i, [_vp, _vp, _vp, _i, _vp, _i, _i, _vp]),
    "frt_jpeg_decode": (_i, [_vp, _vp, _sz, _vp, _sz, _vp, _vp]),
    "frt_jpeg_read_coefficients": (_i, [_vp, _sz, _vp, _sz, _vp]),
    "frt_jpeg_encode_batch": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _vp, _sz, _vp]),
    "frt_jpeg_write_jfif": (_i, [_i, _i, _i, _vp, _vp, _sz, _vp]),
    "frt_base64_encode": (_sz, [_vp, _sz, _vp, _sz]),
    "frt_preprocess_faces": (_i, [_vp, _i, _vp, _vp, _i]),
    "frt_embedder_embed_faces": (_i, [_vp, _vp, _i, _vp, _vp]),
    "frt_embedder_enrol_faces": (_i, [_vp, _vp, _vp, _i, _vp, _vp, ctypes.POINTER(_i)]),
    "frt_resize_images": (_i, [_vp, _i, _vp, _i, _i, _i]),
    "frt_enrol_select_dev": (_i, [_vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp]),
    "frt_pipeline_run_images": (_i, [_vp, _vp, _i, _vp, _vp, _vp]),
    "frt_pipeline_enrol_images": (_i, [_vp, _vp, _i, _vp, _vp, _vp, _vp, ctypes.POINTER(_i), ctypes.POINTER(_i)]),
    "frt_tile_plan": (_i, [_i, _i, _i, _i, _vp, _vp, _i, ctypes.POINTER(_i)]),
    "frt_cut_tiles": (_i, [_vp, _i, _i, _sz, _vp, _i, _i, _i, _vp, _i]),
    "frt_merge_boxes": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp, _i, _vp, _vp, ctypes.POINTER(_i), _i]),
    "frt_detector_find_faces_tiled": (_i, [_vp, _vp, _i, _i, _sz, _vp, _i, _vp, _vp, _vp, ctypes.POINTER(_i)]),
    "frt_select_faces": (_i, [_vp, _vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, ctypes.POINTER(_i), _i]),
    "frt_pipeline_run_photo_tiled": (_i, [_vp, _vp, _i, _i, _sz, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp, ctypes.POINTER(_i)]),
    "frt_tracker_create": (_i, [_i, _i, _i, _i, _vp, _i, ctypes.POINTER(_vp)]),
    "frt_tracker_destroy": (None, [_vp]),
    "frt_tracker_update_dev": (_i, [_vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp]),
    "frt_tracker_update": (_i, [_vp, _vp, _vp, _vp, _i, _vp, _vp, _vp]),
    "frt_tracker_set_appearance": (_i, [_vp, ctypes.c_float, ctypes.c_float]),
    "frt_tracker_get_appearance": (_i, [_vp, _vp, _vp]),
    "frt_tracker_set_motion": (_i, [_vp, _i]),
    "frt_tracker_get_motion": (_i, [_vp, _vp]),
    "frt_tracker_motion": (_i, [_vp, _i, _vp, _vp]),
    "frt_tracker_update_assoc_dev": (_i, [_vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp]),
    "frt_tracker_update_assoc": (_i, [_vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp]),
    "frt_tracker_tracks": (_i, [_vp, _i, _vp, _vp, _vp]),
    "frt_tracker_reset": (_i, [_vp, _i]),
    "frt_pipeline_run_tracked": (_i, [_vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp]),
    "frt_tracker_gate_dev": (_i, [_vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _i, _vp]),
    "frt_tracker_gate": (_i, [_vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _i]),
    "frt_pipeline_run_tracked_gated": (_i, [_vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "frt_face_quality_dev": (_i, [_vp, _vp, _i, _vp, _vp, _vp]),
    "frt_face_quality": (_i, [_vp, _vp, _i, _vp, _vp, _i]),
    "frt_enrol_select_gated_dev": (_i, [_vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "frt_pipeline_run_quality": (_i, [_vp, _vp, _i, _vp, _vp, _vp, _vp, _vp]),
    "frt_pipeline_enrol_images_gated": (_i, [_vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, ctypes.POINTER(_i), ctypes.POINTER(_i)]),
    "frt_sightings_create": (_i, [_vp, _i, _vp, ctypes.POINTER(_vp)]),
    "frt_sightings_destroy": (None, [_vp]),
    "frt_sightings_update_dev": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp, _vp]),
    "frt_sightings_update": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp]),
    "frt_sightings_close": (_i, [_vp, _i]),
    "frt_sightings_drain": (_i, [_vp, _i, _vp, _vp, _vp, _vp, ctypes.POINTER(_i), _vp]),
    "frt_sightings_open": (_i, [_vp, _i, _vp, _vp, _vp, _vp]),
    "frt_pipeline_run_sighted": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp]),
    "frt_profile_enable": (_i, [_i]),
    "frt_profile_collect": (_i, [_vp, _sz, _vp, _vp, _i]),
}
for _name, (_res, _args) in ABI.items():
    try:
        _fn = getattr(lib, _name)  # AttributeError here == a symbol declared in frt.h is not exported
    except AttributeError:
        # The import is strict: a library that lacks a declared symbol is a broken build.  The one exception is not reachable from the environment:
        # a measurement driver that A/Bs an OLDER build on the same box registers the module name below BEFORE importing this package
        # (bench.py --ab-old-lib); the skipped symbols are listed on stderr.
        if "frt_amd_ab_old_library" in sys.modules:
            sys.stderr.write("[frt_amd] WARNING: %s is missing from %s (A/B against an older build: measurement only)\n" % (_name, LIB_PATH))
            continue
        raise
    _fn.restype = _res
    _fn.argtypes = _args


class FrtError(RuntimeError):
    """Raised on a non-zero frt_status; mirrors the reference's ``std::logic_error`` / ``throw const char*``."""

    def __init__(self, code, msg):
        super().__init__("frt status %d: %s" % (code, msg))
        self.code = code


def _check(rc):
    if rc != FRT_OK:
        raise FrtError(rc, lib.frt_last_error().decode(errors="replace"))


def _ptr(a):
    return ctypes.c_void_p(a.ctypes.data) if a is not None else None


def device_count():
    return lib.frt_device_count()


def set_wait_spin_us(us):
    """How long blocking entry points busy-poll before backing off to sleeping polls (frt_set_wait_spin_us); returns the previous value."""
    return int(lib.frt_set_wait_spin_us(int(us)))


def probe_sustained_mfma(device=0, mix=2, seconds=0.25):
    """TFLOP/s the device sustains on back-to-back fp16 MFMAs with random operands (mix 0), + one LDS read per MFMA (1), + the dominant conv
    kernel's global loads (2): frt_probe_sustained_mfma."""
    out = ctypes.c_double(0.0)
    _check(lib.frt_probe_sustained_mfma(int(device), int(mix), float(seconds), ctypes.byref(out)))
    return float(out.value)


def write_weights(path, state, kind):
    return weights_io.write_blob(path, state, kind)


def describe_weights(path):
    """The backbone a recogniser blob holds (frt_embedder_describe: the validation of ArcFaceIR50's constructor, no device needed)
    -> dict(numLayers=50 | 100 | 152, se=bool, unitsPerStage=(4 ints))."""
    n, se, units = _i(), _i(), (_i * 4)()
    _check(lib.frt_embedder_describe(os.fsencode(path), ctypes.byref(n), ctypes.byref(se), units))
    return dict(numLayers=n.value, se=bool(se.value), unitsPerStage=tuple(units))


DETECTOR_FAMILIES = {1: "mnet0.25", 4: "slim", 5: "rfb"}


def describe_detector_weights(path):
    """The network a detector blob holds (frt_detector_describe: the validation of RetinaFace's constructor, no device needed)
    -> dict(family="mnet0.25" | "slim" | "rfb", kind=1 | 4 | 5, levels=3 | 4, hasLandmarks=bool)."""
    fam, lv, ldm = _i(), _i(), _i()
    _check(lib.frt_detector_describe(os.fsencode(path), ctypes.byref(fam), ctypes.byref(lv), ctypes.byref(ldm)))
    return dict(family=DETECTOR_FAMILIES[fam.value], kind=fam.value, levels=lv.value, hasLandmarks=bool(ldm.value))


# ----------------------------------------------------------------------------------------------------------------------
# class MatMul (src/matmul.h)
# ----------------------------------------------------------------------------------------------------------------------
class MatMul:
    def __init__(self, device=0):
        self._h = _vp()
        _check(lib.frt_matcher_create(device, ctypes.byref(self._h)))
        self.m = self.k = 0

    def init(self, knownEmbeds, numRow=None, numCol=None):
        g = np.ascontiguousarray(knownEmbeds, np.float32)
        numRow = g.shape[0] if numRow is None else numRow
        numCol = g.shape[1] if numCol is None else numCol
        _check(lib.frt_matcher_init(self._h, _ptr(g), int(numRow), int(numCol)))
        self.m, self.k = int(numRow), int(numCol)

    def setStorage(self, fp16):
        """Rows of the NEXT init / galleryBegin are stored as fp16 on the device (BASELINE config 5) when ``fp16`` is true."""
        _check(lib.frt_matcher_set_storage(self._h, 1 if fp16 else 0))

    def setScreening(self, on):
        """``False``: every top-1 call takes the exact fp32 scan of the whole gallery (same answers, the path's worst case)."""
        _check(lib.frt_matcher_set_screening(self._h, 1 if on else 0))

    def scanBytes(self):
        """Gallery bytes one top-1 call reads in the current mode (shadow copy when screened, stored rows otherwise)."""
        return int(lib.frt_matcher_scan_bytes(self._h))

    # streaming load == initKnownEmbeds / addEmbedding x n / initMatMul (src/db.cpp:316-346)
    def galleryBegin(self, rowCapacity, numCol=512):
        _check(lib.frt_matcher_gallery_begin(self._h, int(rowCapacity), int(numCol)))
        self._pending_k = int(numCol)

    def galleryAppend(self, rows):
        """``rows``: float32 array [n, numCol] or a bytes-like blob of raw little-endian float32 rows (SQLite's EMBEDDING column)."""
        if isinstance(rows, (bytes, bytearray, memoryview)):
            a = np.frombuffer(rows, dtype="<f4")
        else:
            a = np.ascontiguousarray(rows, np.float32).reshape(-1)
        if a.size % self._pending_k:
            raise ValueError("galleryAppend: %d floats is not a whole number of %d-float rows" % (a.size, self._pending_k))
        _check(lib.frt_matcher_gallery_append(self._h, _ptr(a), a.size // self._pending_k))

    def galleryCommit(self):
        _check(lib.frt_matcher_gallery_commit(self._h))
        self.m, self.k = int(lib.frt_matcher_num_rows(self._h)), self._pending_k

    # live edits (frt_matcher_gallery_reserve / add / add_dev / remove): the gallery changes in place, no reload
    def _edited(self):
        self.m = int(lib.frt_matcher_num_rows(self._h))

    def galleryReserve(self, rowCapacity):
        """Room for edits up to ``rowCapacity`` rows (an add inside it allocates nothing); never shrinks."""
        _check(lib.frt_matcher_gallery_reserve(self._h, int(rowCapacity)))

    def galleryAdd(self, rows):
        """Append float32 rows [n, numCol] (or one row); they get the indices ``m .. m + n - 1``.  Returns the first new index."""
        a = np.ascontiguousarray(rows, np.float32).reshape(-1, self.k)
        first = int(lib.frt_matcher_num_rows(self._h))
        _check(lib.frt_matcher_gallery_add(self._h, _ptr(a), a.shape[0]))
        self._edited()
        return first

    def galleryAddDev(self, rows_ptr, n):
        """Append ``n`` fp32 rows that are resident on the device (raw address, e.g. the embeddings ``Pipeline.run_dev`` left there); the
        rows must be complete (synchronise their producer first)."""
        first = int(lib.frt_matcher_num_rows(self._h))
        _check(lib.frt_matcher_gallery_add_dev(self._h, _vp(rows_ptr), int(n)))
        self._edited()
        return first

    def galleryRemove(self, indices):
        """Remove the rows ``indices`` (any order, duplicates count once); the rows behind them close up in order."""
        i = np.ascontiguousarray(indices, np.int32).reshape(-1)
        _check(lib.frt_matcher_gallery_remove(self._h, _ptr(i), i.size))
        self._edited()

    def editStats(self):
        """Cumulative dict(rows_uploaded, rows_moved, shadow_rows_rebuilt, reallocations) of the live edits."""
        out = (ctypes.c_long * 4)()
        _check(lib.frt_matcher_edit_stats(self._h, out))
        return dict(zip(("rows_uploaded", "rows_moved", "shadow_rows_rebuilt", "reallocations"), (int(v) for v in out)))

    def generation(self):
        return int(lib.frt_matcher_generation(self._h))

    def top1_dev(self, embeds_ptr, n, idx_ptr, sim_ptr, hip_stream=None):
        """Asynchronous, raw device addresses (queries fp32 [n][k], idx int32 [n], sim fp32 [n])."""
        _check(lib.frt_matcher_top1_dev(self._h, _vp(embeds_ptr), int(n), _vp(idx_ptr), _vp(sim_ptr), _vp(hip_stream) if hip_stream else None))

    def topk(self, embeds, k):
        """Exact top-k lists [n, k] (entry 0 == top1; ties: lower index first; -1 / -inf when the gallery has fewer than k rows)."""
        e = np.ascontiguousarray(embeds, np.float32).reshape(-1, self.k)
        idx = np.empty((e.shape[0], int(k)), np.int32)
        sim = np.empty((e.shape[0], int(k)), np.float32)
        _check(lib.frt_matcher_topk(self._h, _ptr(e), e.shape[0], int(k), _ptr(idx), _ptr(sim)))
        return idx, sim

    def topk_dev(self, embeds_ptr, n, k, idx_ptr, sim_ptr, hip_stream=None, fp16=False):
        """Asynchronous, raw device addresses: queries fp32 (or IEEE fp16 with ``fp16=True``) [n][k_dim], idx int32 [n][k], sim fp32 [n][k]."""
        _check(lib.frt_matcher_topk_dev(self._h, _vp(embeds_ptr), 1 if fp16 else 0, int(n), int(k), _vp(idx_ptr), _vp(sim_ptr),
                                        _vp(hip_stream) if hip_stream else None))

    # identities (frt_matcher_set_labels / labels_info / gallery_add_labeled / topk_labels): one int32 label >= 0 per row; the ranked search
    # then returns the k best IDENTITIES, each with its best row
    def set_labels(self, labels):
        """One label per gallery row (``None`` or an empty list clears them).  ``init`` / ``galleryCommit`` drop the labels."""
        l = np.ascontiguousarray([] if labels is None else labels, np.int32).reshape(-1)
        _check(lib.frt_matcher_set_labels(self._h, _ptr(l) if l.size else None, l.size))

    def labels_info(self):
        """(number of identities, upper bound of the rows one label has); (0, 0) for an unlabelled gallery."""
        n, m = _i(), _i()
        _check(lib.frt_matcher_labels_info(self._h, ctypes.byref(n), ctypes.byref(m)))
        return n.value, m.value

    def gallery_add_labeled(self, rows, labels):
        """``galleryAdd`` for a labelled gallery: one label per new row.  Returns the first new index."""
        a = np.ascontiguousarray(rows, np.float32).reshape(-1, self.k)
        l = np.ascontiguousarray(labels, np.int32).reshape(-1)
        if l.size != a.shape[0]:
            raise ValueError("gallery_add_labeled: one label per row")
        first = int(lib.frt_matcher_num_rows(self._h))
        _check(lib.frt_matcher_gallery_add_labeled(self._h, _ptr(a), _ptr(l), a.shape[0]))
        self._edited()
        return first

    def gallery_add_labeled_dev(self, rows_ptr, labels):
        """``galleryAddDev`` for a labelled gallery: rows on the device (raw address), labels on the host."""
        l = np.ascontiguousarray(labels, np.int32).reshape(-1)
        first = int(lib.frt_matcher_num_rows(self._h))
        _check(lib.frt_matcher_gallery_add_labeled_dev(self._h, _vp(rows_ptr), _ptr(l), l.size))
        self._edited()
        return first

    def topk_labels(self, embeds, k):
        """The k best identities per query -> (label, idx, sim), each [n, k]: entry j is the best row of the j-th best identity (entry 0 ==
        top1; -1 / -1 / -inf when the gallery has fewer than k identities)."""
        e = np.ascontiguousarray(embeds, np.float32).reshape(-1, self.k)
        lab = np.empty((e.shape[0], int(k)), np.int32)
        idx = np.empty((e.shape[0], int(k)), np.int32)
        sim = np.empty((e.shape[0], int(k)), np.float32)
        _check(lib.frt_matcher_topk_labels(self._h, _ptr(e), e.shape[0], int(k), _ptr(lab), _ptr(idx), _ptr(sim)))
        return lab, idx, sim

    def topk_labels_dev(self, embeds_ptr, n, k, label_ptr, idx_ptr, sim_ptr, hip_stream=None, fp16=False):
        """Asynchronous, raw device addresses: queries as ``topk_dev``; label int32 [n][k], idx int32 [n][k], sim fp32 [n][k]."""
        _check(lib.frt_matcher_topk_labels_dev(self._h, _vp(embeds_ptr), 1 if fp16 else 0, int(n), int(k), _vp(label_ptr), _vp(idx_ptr), _vp(sim_ptr),
                                               _vp(hip_stream) if hip_stream else None))

    def buildTemplates(self, dst=None, want_templates=False):
        """One template per identity of this labelled gallery (frt_matcher_build_templates): the re-normalised sum of the identity's stored
        rows, identities in first-appearance order.  Returns ``(labels, n_rows, min_sim, min_row[, templates])``, each ``[I]`` (templates
        ``[I, numCol]`` with ``want_templates``): ``min_row`` is the member row that agrees least with its own template, ``min_sim`` its
        similarity.  ``dst`` (another ``MatMul`` on the same device) is replaced by the template gallery, labelled with ``labels``, in its own
        storage mode; ``None``: an audit only."""
        n = self.labels_info()[0]
        labels, n_rows, min_row = (np.empty(n, np.int32) for _ in range(3))
        min_sim = np.empty(n, np.float32)
        t = np.empty((n, self.k), np.float32) if want_templates else None
        _check(lib.frt_matcher_build_templates(self._h, dst._h if dst is not None else None, _ptr(labels), _ptr(n_rows), _ptr(min_sim), _ptr(min_row),
                                               _ptr(t)))
        if dst is not None:
            dst.k = self.k
            dst._edited()
        return (labels, n_rows, min_sim, min_row) + ((t,) if want_templates else ())

    CLUSTER_STATS = ("clusters", "edges", "screened_chunks", "dense_chunks")

    def cluster(self, threshold, install=False):
        """Single-linkage clustering of the gallery at a similarity threshold (frt_matcher_cluster): rows i < j are joined iff the matcher's
        own exact similarity of the two stored rows is ``>= threshold``.  Returns ``(labels, stats)``: ``labels[i]`` (int32 ``[m]``) is the
        smallest row of i's connected component, ``stats`` a dict of ``CLUSTER_STATS``.  ``install=True`` makes the labels the matcher's own,
        as ``set_labels(labels)`` would: ``topk_labels`` and ``buildTemplates`` then work at once."""
        labels = np.empty(int(lib.frt_matcher_num_rows(self._h)), np.int32)
        stats = (ctypes.c_longlong * 4)()
        _check(lib.frt_matcher_cluster(self._h, float(threshold), _ptr(labels) if labels.size else None, 1 if install else 0, stats))
        return labels, dict(zip(self.CLUSTER_STATS, (int(v) for v in stats)))

    def cluster_dev(self, threshold, labels_ptr, stats_ptr=None, hip_stream=None):
        """Raw device addresses: labels int32 [m], stats 4 x int64 (or ``None``); complete when ``hip_stream`` has run."""
        _check(lib.frt_matcher_cluster_dev(self._h, float(threshold), _vp(labels_ptr) if labels_ptr else None, _vp(stats_ptr) if stats_ptr else None,
                                           _vp(hip_stream) if hip_stream else None))

    SEPARATION_STATS = ("genuine_rows", "impostor_rows", "closer_to_another", "screened_chunks", "exact_chunks")

    def separation(self, thresholds=None):
        """Leave-one-out genuine / impostor scores of this labelled gallery (frt_matcher_separation).  Returns ``(gen_sim, gen_row, imp_sim,
        imp_row, counts, stats)``: for every row the best OTHER row of its own label and the best row of any other label by the matcher's
        exact similarity (``-inf`` / ``-1`` without a candidate), ``counts`` int64 ``[len(thresholds), 2]`` = rows with ``gen_sim < t`` /
        rows with ``imp_sim >= t`` per threshold (at most 64), ``stats`` a dict of ``SEPARATION_STATS``.  ``max(imp_sim)`` is the
        threshold above which ``cluster`` merges no two labels."""
        n = int(lib.frt_matcher_num_rows(self._h))
        t = np.ascontiguousarray([] if thresholds is None else thresholds, np.float32).reshape(-1)
        gen_sim, imp_sim = np.empty(n, np.float32), np.empty(n, np.float32)
        gen_row, imp_row = np.empty(n, np.int32), np.empty(n, np.int32)
        counts = np.zeros((t.size, 2), np.int64)
        stats = (ctypes.c_longlong * 5)()
        _check(lib.frt_matcher_separation(self._h, _ptr(gen_sim) if n else None, _ptr(gen_row) if n else None, _ptr(imp_sim) if n else None,
                                          _ptr(imp_row) if n else None, _ptr(t) if t.size else None, t.size, _ptr(counts) if t.size else None, stats))
        return gen_sim, gen_row, imp_sim, imp_row, counts, dict(zip(self.SEPARATION_STATS, (int(v) for v in stats)))

    def separation_dev(self, gen_sim_ptr, gen_row_ptr, imp_sim_ptr, imp_row_ptr, thresholds=None, counts_ptr=None, stats_ptr=None, hip_stream=None):
        """Raw device addresses (any may be ``None``): sims fp32 [m], rows int32 [m], counts int64 [len(thresholds)][2], stats 5 x int64;
        ``thresholds`` stay on the host.  Complete when ``hip_stream`` has run."""
        t = np.ascontiguousarray([] if thresholds is None else thresholds, np.float32).reshape(-1)
        opt = lambda p: _vp(p) if p else None
        _check(lib.frt_matcher_separation_dev(self._h, opt(gen_sim_ptr), opt(gen_row_ptr), opt(imp_sim_ptr), opt(imp_row_ptr), _ptr(t) if t.size else None,
                                              t.size, opt(counts_ptr), opt(stats_ptr), opt(hip_stream)))

    def setRowOffset(self, row_offset):
        """Sharded gallery: local row 0 is global row ``row_offset`` (top-1 indices become global)."""
        _check(lib.frt_matcher_set_row_offset(self._h, int(row_offset)))

    def calculate(self, embeds, embedCount=None):
        e = np.ascontiguousarray(embeds, np.float32).reshape(-1, self.k)
        n = e.shape[0] if embedCount is None else embedCount
        out = np.empty((n, self.m), np.float32)
        _check(lib.frt_matcher_calculate(self._h, _ptr(e), int(n), _ptr(out)))
        return out

    def calculate_top1(self, embeds, materialize=True):
        """calculate + row-wise first maximum in one call -> (matrix [n, m] or None, idx [n], sim [n])."""
        e = np.ascontiguousarray(embeds, np.float32).reshape(-1, self.k)
        out = np.empty((e.shape[0], self.m), np.float32) if materialize else None
        idx = np.empty(e.shape[0], np.int32)
        sim = np.empty(e.shape[0], np.float32)
        _check(lib.frt_matcher_calculate_top1(self._h, _ptr(e), e.shape[0], _ptr(out), _ptr(idx), _ptr(sim)))
        return out, idx, sim

    def top1(self, embeds):
        e = np.ascontiguousarray(embeds, np.float32).reshape(-1, self.k)
        idx = np.empty(e.shape[0], np.int32)
        sim = np.empty(e.shape[0], np.float32)
        _check(lib.frt_matcher_top1(self._h, _ptr(e), e.shape[0], _ptr(idx), _ptr(sim)))
        return idx, sim

    def close(self):
        if self._h:
            lib.frt_matcher_destroy(self._h)
            self._h = _vp()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def merge_top1(idx_a, sim_a, idx_b, sim_b):
    n = len(idx_a)
    ia, ib = np.ascontiguousarray(idx_a, np.int32), np.ascontiguousarray(idx_b, np.int32)
    sa, sb = np.ascontiguousarray(sim_a, np.float32), np.ascontiguousarray(sim_b, np.float32)
    io, so = np.empty(n, np.int32), np.empty(n, np.float32)
    _check(lib.frt_merge_top1(n, _ptr(ia), _ptr(sa), _ptr(ib), _ptr(sb), _ptr(io), _ptr(so)))
    return io, so


def merge_topk(idx_all, sim_all):
    """Host k-way merge of per-shard top-k lists [shards, n, k] with global indices -> ([n, k], [n, k])."""
    ia = np.ascontiguousarray(idx_all, np.int32)
    sa = np.ascontiguousarray(sim_all, np.float32)
    shards, n, k = ia.shape
    io, so = np.empty((n, k), np.int32), np.empty((n, k), np.float32)
    _check(lib.frt_merge_topk(shards, n, k, _ptr(ia), _ptr(sa), _ptr(io), _ptr(so)))
    return io, so


def merge_topk_dev(shards, n, k, idx_all_ptr, sim_all_ptr, idx_out_ptr, sim_out_ptr, hip_stream=None):
    _check(lib.frt_merge_topk_dev(int(shards), int(n), int(k), _vp(idx_all_ptr), _vp(sim_all_ptr), _vp(idx_out_ptr), _vp(sim_out_ptr),
                                  _vp(hip_stream) if hip_stream else None))


def merge_topk_labels(label_all, idx_all, sim_all):
    """Host merge of per-shard identity lists [shards, n, k] with global indices -> (label, idx, sim), each [n, k]; an identity present in
    several shards counts once, with its best row."""
    la = np.ascontiguousarray(label_all, np.int32)
    ia = np.ascontiguousarray(idx_all, np.int32)
    sa = np.ascontiguousarray(sim_all, np.float32)
    shards, n, k = ia.shape
    if la.shape != ia.shape or sa.shape != ia.shape:
        raise ValueError("merge_topk_labels: label, idx and sim lists differ in shape")
    lo, io, so = np.empty((n, k), np.int32), np.empty((n, k), np.int32), np.empty((n, k), np.float32)
    _check(lib.frt_merge_topk_labels(shards, n, k, _ptr(la), _ptr(ia), _ptr(sa), _ptr(lo), _ptr(io), _ptr(so)))
    return lo, io, so


def merge_topk_labels_dev(shards, n, k, label_all_ptr, idx_all_ptr, sim_all_ptr, label_out_ptr, idx_out_ptr, sim_out_ptr, hip_stream=None):
    _check(lib.frt_merge_topk_labels_dev(int(shards), int(n), int(k), _vp(label_all_ptr), _vp(idx_all_ptr), _vp(sim_all_ptr), _vp(label_out_ptr),
                                         _vp(idx_out_ptr), _vp(sim_out_ptr), _vp(hip_stream) if hip_stream else None))


def embeds_to_half_dev(src_ptr, n_values, dst_ptr, hip_stream=None):
    _check(lib.frt_embeds_to_half_dev(_vp(src_ptr), int(n_values), _vp(dst_ptr), _vp(hip_stream) if hip_stream else None))


# ----------------------------------------------------------------------------------------------------------------------
# RCCL communicator behind the C ABI (frt_comm_*): the exchange step of the multi-GPU path from C++, no torch.distributed
# ----------------------------------------------------------------------------------------------------------------------
COMM_ID_BYTES = 128


def comm_unique_id():
    b = np.zeros(COMM_ID_BYTES, np.uint8)
    _check(lib.frt_comm_get_unique_id(_ptr(b)))
    return b.tobytes()


class Comm:
    def __init__(self, unique_id, rank, world, device=0):
        self._h = _vp()
        b = np.frombuffer(bytes(unique_id), np.uint8)
        assert b.size == COMM_ID_BYTES
        _check(lib.frt_comm_create(_ptr(b), int(rank), int(world), int(device), ctypes.byref(self._h)))
        self.rank, self.world = int(rank), int(world)

    @property
    def stream(self):
        """raw hipStream_t of the communicator's exchange stream"""
        return int(lib.frt_comm_stream(self._h) or 0)

    def all_gather(self, send_ptr, recv_ptr, bytes_per_rank, hip_stream=None):
        _check(lib.frt_comm_all_gather(self._h, _vp(send_ptr), _vp(recv_ptr), int(bytes_per_rank), _vp(hip_stream) if hip_stream else None))

    def sync(self):
        _check(lib.frt_comm_sync(self._h))

    def close(self):
        if self._h:
            lib.frt_comm_destroy(self._h)
            self._h = _vp()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ----------------------------------------------------------------------------------------------------------------------
# class RetinaFace (src/retinaface.h)
# ----------------------------------------------------------------------------------------------------------------------
class RetinaFace:
    def __init__(self, engineFile, frameWidth, frameHeight, inputShape=(3, 640, 640), maxBatchSize=1, maxFacesPerScene=4,
                 nms_threshold=0.4, bbox_threshold=0.6, inputName="input_det", outputNames=("output_det0", "output_det1"), device=0):
        assert len(inputShape) == 3 and len(outputNames) == 2  # retinaface.cpp:8,86 (binding names are accepted and ignored)
        self._h = _vp()
        self.frameWidth, self.frameHeight = int(frameWidth), int(frameHeight)
        self.inputShape = tuple(int(x) for x in inputShape)
        self.maxBatchSize, self.maxFacesPerScene = int(maxBatchSize), int(maxFacesPerScene)
        _check(lib.frt_detector_create(os.fsencode(engineFile), self.frameWidth, self.frameHeight, *self.inputShape, self.maxBatchSize,
                                       self.maxFacesPerScene, nms_threshold, bbox_threshold, device, ctypes.byref(self._h)))
        self.numAnchors = lib.frt_detector_num_anchors(self._h)
        self.hasLandmarks = bool(lib.frt_detector_has_landmarks(self._h))
        self.family = describe_detector_weights(engineFile)["family"]  # "mnet0.25", "slim" or "rfb"

    # ---- optional alignment mode (no counterpart in the reference, see include/frt.h)
    def findFaceLandmarks(self, img):
        """-> (boxes, landmarks [n][5][2] as (x=col, y=row) frame pixels)."""
        img = np.ascontiguousarray(img, np.uint8)
        out = np.zeros(self.maxFacesPerScene, BBOX_DTYPE)
        ldm = np.zeros((self.maxFacesPerScene, 5, 2), np.float32)
        n = ctypes.c_int(0)
        _check(lib.frt_detector_find_faces_landmarks(self._h, _ptr(img), img.shape[0], img.shape[1], img.strides[0], _ptr(out), _ptr(ldm),
                                                     ctypes.byref(n)))
        return out[:n.value].copy(), ldm[:n.value].copy()

    def doInferenceLandmarks(self, chw):
        x = np.ascontiguousarray(chw, np.float32).reshape((-1,) + self.inputShape)
        b = x.shape[0]
        loc = np.empty((b, self.numAnchors, 4), np.float32)
        conf = np.empty((b, self.numAnchors, 2), np.float32)
        ldm = np.empty((b, self.numAnchors, 10), np.float32)
        _check(lib.frt_detector_infer_landmarks(self._h, _ptr(x), b, _ptr(loc), _ptr(conf), _ptr(ldm)))
        return loc, conf, ldm

    def findFace(self, img):
        img = np.ascontiguousarray(img, np.uint8)
        out = np.zeros(self.maxFacesPerScene, BBOX_DTYPE)
        n = ctypes.c_int(0)
        _check(lib.frt_detector_find_faces(self._h, _ptr(img), img.shape[0], img.shape[1], img.strides[0], _ptr(out), ctypes.byref(n)))
        return out[:n.value].copy()

    def findFaceBatch(self, frames):
        frames = np.ascontiguousarray(frames, np.uint8)
        nf = frames.shape[0]
        out = np.zeros((nf, self.maxFacesPerScene), BBOX_DTYPE)
        n = np.zeros(nf, np.int32)
        _check(lib.frt_detector_find_faces_batch(self._h, _ptr(frames), nf, frames.shape[1], frames.shape[2], frames.strides[1],
                                                 frames.strides[0], _ptr(out), _ptr(n)))
        return [out[i, :n[i]].copy() for i in range(nf)]

    def findFaceTiled(self, img, overlap=None, overview=True, metric=1, drop_cut=True, threshold=None, max_out=256, landmarks=False,
                      sources=False):
        """Large photos by tiles (frt_detector_find_faces_tiled): a photo of any size -> boxes in PHOTO coordinates, found on overlapping
        frameHeight x frameWidth tiles (and, with overview, on the whole photo resized to one) and merged by one NMS on the device.
        overlap: None = a quarter of the tile, an int, or (rows, cols); threshold None = the detector's nms_threshold; metric 0 IoU, 1
        intersection over the smaller area.  At most maxFacesPerScene boxes per tile.  -> boxes [, landmarks [n][5][2]] [, source indices
        tile * maxFacesPerScene + slot]."""
        img = _photo(img)
        opt = tileOptions(self.frameHeight, self.frameWidth, overlap, overview, metric, drop_cut, threshold)
        max_out = int(max_out)
        cap = max(max_out, 1)
        out = np.zeros(cap, BBOX_DTYPE)
        src = np.full(cap, -1, np.int32)
        ldm = np.zeros((cap, 5, 2), np.float32) if landmarks else None
        n = ctypes.c_int(0)
        _check(lib.frt_detector_find_faces_tiled(self._h, _ptr(img), img.shape[0], img.shape[1], img.strides[0], ctypes.addressof(opt), max_out,
                                                 _ptr(out), _ptr(ldm), _ptr(src), ctypes.byref(n)))
        res = (out[:n.value].copy(),) + ((ldm[:n.value].copy(),) if landmarks else ()) + ((src[:n.value].copy(),) if sources else ())
        return res[0] if len(res) == 1 else res

    def preprocess(self, img):
        img = np.ascontiguousarray(img, np.uint8)
        out = np.empty(self.inputShape, np.float32)
        _check(lib.frt_detector_preprocess(self._h, _ptr(img), img.shape[0], img.shape[1], img.strides[0], _ptr(out)))
        return out

    def doInference(self, chw):
        x = np.ascontiguousarray(chw, np.float32).reshape((-1,) + self.inputShape)
        b = x.shape[0]
        loc = np.empty((b, self.numAnchors, 4), np.float32)
        conf = np.empty((b, self.numAnchors, 2), np.float32)
        _check(lib.frt_detector_infer(self._h, _ptr(x), b, _ptr(loc), _ptr(conf)))
        return loc, conf

    def postprocessing(self, loc, conf):
        loc = np.ascontiguousarray(loc, np.float32).reshape(self.numAnchors, 4)
        conf = np.ascontiguousarray(conf, np.float32).reshape(self.numAnchors, 2)
        out = np.zeros(self.maxFacesPerScene, BBOX_DTYPE)
        n = ctypes.c_int(0)
        _check(lib.frt_detector_postprocess(self._h, _ptr(loc), _ptr(conf), _ptr(out), ctypes.byref(n)))
        return out[:n.value].copy()

    def close(self):
        if self._h:
            lib.frt_detector_destroy(self._h)
            self._h = _vp()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def resizeFrame(img, width, height, device=0):
    """``cv::resize(img, img, Size(width, height))`` (src/app.cpp:166,301: default INTER_LINEAR) on the device -> u8 [height][width][3]."""
    img = np.ascontiguousarray(img, np.uint8)
    out = np.empty((int(height), int(width), 3), np.uint8)
    _check(lib.frt_resize_frame(_ptr(img), img.shape[0], img.shape[1], img.strides[0], _ptr(out), int(height), int(width), device))
    return out


def getCroppedFaces(frame, outputBbox, resize_w=112, resize_h=112, device=0):
    """``getCroppedFaces`` (src/arcface.cpp:3-17) -> u8 BGR [n][resize_h][resize_w][3]."""
    frame = np.ascontiguousarray(frame, np.uint8)
    boxes = np.ascontiguousarray(outputBbox, BBOX_DTYPE)
    out = np.zeros((len(boxes), resize_h, resize_w, 3), np.uint8)
    _check(lib.frt_crop_faces(_ptr(frame), frame.shape[0], frame.shape[1], frame.strides[0], _ptr(boxes), len(boxes), resize_w, resize_h,
                              _ptr(out), device))
    return out


def alignFaces(frame, landmarks, device=0):
    """Optional alignment mode: 5-point similarity warp to the ArcFace template -> u8 BGR [n][112][112][3]."""
    frame = np.ascontiguousarray(frame, np.uint8)
    lm = np.ascontiguousarray(landmarks, np.float32).reshape(-1, 10)
    out = np.zeros((len(lm), 112, 112, 3), np.uint8)
    _check(lib.frt_align_faces(_ptr(frame), frame.shape[0], frame.shape[1], frame.strides[0], _ptr(lm), len(lm), _ptr(out), device))
    return out


# ----------------------------------------------------------------------------------------------------------------------
# large photos by tiles (frt_tile_plan / frt_cut_tiles / frt_merge_boxes; RetinaFace.findFaceTiled)
# ----------------------------------------------------------------------------------------------------------------------
class TileOptions(ctypes.Structure):  # == frt_tile_options
    _fields_ = [("overlap_rows", ctypes.c_int32), ("overlap_cols", ctypes.c_int32), ("overview", ctypes.c_int32), ("metric", ctypes.c_int32),
                ("drop_cut", ctypes.c_int32), ("merge_threshold", ctypes.c_float)]


TILE_DTYPE = np.dtype([("row0", "<i4"), ("col0", "<i4"), ("rows", "<i4"), ("cols", "<i4"), ("kind", "<i4")])  # == frt_tile


def tileOptions(tile_rows, tile_cols, overlap=None, overview=True, metric=1, drop_cut=True, threshold=None):
    """overlap: None = a quarter of the tile on each axis, an int for both axes, or (rows, cols); threshold None = -1 (the detector's)."""
    if overlap is None:
        overlap = (int(tile_rows) // 4, int(tile_cols) // 4)
    elif np.isscalar(overlap):
        overlap = (overlap, overlap)
    return TileOptions(int(overlap[0]), int(overlap[1]), int(bool(overview)), int(metric), int(bool(drop_cut)), -1.0 if threshold is None else float(threshold))


def _photo(img):
    """H x W x 3 u8 with contiguous pixels; a view with padded rows keeps its row stride."""
    a = np.asarray(img)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
        raise ValueError("a photo is an H x W x 3 uint8 array")
    if a.shape[0] and a.shape[1] and (a.strides[2] != 1 or a.strides[1] != 3 or a.strides[0] < a.shape[1] * 3):
        a = np.ascontiguousarray(a)
    return a


def tilePlan(rows, cols, tile_rows, tile_cols, overlap=None, overview=True):
    """frt_tile_plan -> the tiles as a TILE_DTYPE array: the grid row-major, the overview last."""
    opt = tileOptions(tile_rows, tile_cols, overlap, overview)
    tiles = np.zeros(4096, TILE_DTYPE)  # (the plan's own cap)
    n = ctypes.c_int(0)
    _check(lib.frt_tile_plan(int(rows), int(cols), int(tile_rows), int(tile_cols), ctypes.addressof(opt), _ptr(tiles), len(tiles), ctypes.byref(n)))
    tiles = tiles[:n.value].copy()
    return tiles


def cutTiles(img, tiles, tile_rows, tile_cols, device=0):
    """frt_cut_tiles -> u8 [n_tiles][tile_rows][tile_cols][3]: grid tiles cut from the photo (128 outside it), the overview resized."""
    img = _photo(img)
    tiles = np.ascontiguousarray(tiles, TILE_DTYPE)
    out = np.zeros((len(tiles), int(tile_rows), int(tile_cols), 3), np.uint8)
    _check(lib.frt_cut_tiles(_ptr(img), img.shape[0], img.shape[1], img.strides[0], _ptr(tiles), len(tiles), int(tile_rows), int(tile_cols),
                             _ptr(out), device))
    return out


def mergeBoxes(boxes, n_boxes, tiles, photo_rows, photo_cols, tile_rows, tile_cols, metric=1, drop_cut=True, threshold=0.4, max_out=256,
               device=0, full=False):
    """frt_merge_boxes: boxes [n_tiles][slots] in tile coordinates + n_boxes [n_tiles] -> (boxes in photo coordinates, source indices
    tile * slots + slot), best first.  full: the whole max_out-long arrays (zeros / -1 behind the count) and the count."""
    boxes = np.ascontiguousarray(boxes, BBOX_DTYPE)
    tiles = np.ascontiguousarray(tiles, TILE_DTYPE)
    n_boxes = np.ascontiguousarray(n_boxes, np.int32)
    if boxes.ndim != 2 or boxes.shape[0] != len(tiles) or n_boxes.shape != (len(tiles),):
        raise ValueError("boxes are [n_tiles][slots], n_boxes [n_tiles]")
    opt = tileOptions(tile_rows, tile_cols, 0, False, metric, drop_cut, threshold)
    cap = max(int(max_out), 1)
    out = np.zeros(cap, BBOX_DTYPE)
    src = np.full(cap, -1, np.int32)
    n = ctypes.c_int(0)
    _check(lib.frt_merge_boxes(_ptr(boxes), _ptr(n_boxes), _ptr(tiles), len(tiles), boxes.shape[1], int(photo_rows), int(photo_cols), int(tile_rows),
                               int(tile_cols), ctypes.addressof(opt), int(max_out), _ptr(out), _ptr(src), ctypes.byref(n), device))
    return (out, src, n.value) if full else (out[:n.value].copy(), src[:n.value].copy())


def selectFaces(boxes, src=None, landmarks=None, min_face=0, max_batch=128, device=0):
    """frt_select_faces, the stage between the tiled merge and the recogniser: boxes [n] (+ source indices [n], landmarks [n][5][2]) -> the
    boxes with min(x2 - x1, y2 - y1) >= min_face (min_face <= 0: all), dense and in order.  Returns a dict of the WHOLE arrays - "boxes",
    "src" (None without src), "landmarks" (None without landmarks), "keep_pos" [n], zeros / -1 behind the count; "pass_count"
    [ceil(n / max_batch)]: faces per recogniser pass - and "n_kept"."""
    boxes = np.ascontiguousarray(boxes, BBOX_DTYPE).reshape(-1)
    n = len(boxes)
    s = l = None
    if src is not None:
        s = np.ascontiguousarray(src, np.int32).reshape(-1)
        if s.size != n:
            raise ValueError("selectFaces: one source index per box")
    if landmarks is not None:
        l = np.ascontiguousarray(landmarks, np.float32).reshape(-1, 5, 2)
        if len(l) != n:
            raise ValueError("selectFaces: five landmarks per box")
    max_batch = int(max_batch)
    out = np.zeros(n, BBOX_DTYPE)
    src_out = np.full(n, -1, np.int32) if s is not None else None
    ldm_out = np.zeros((n, 5, 2), np.float32) if l is not None else None
    pos = np.full(n, -1, np.int32)
    passes = np.zeros(-(-n // max_batch) if max_batch > 0 else 0, np.int32)
    k = ctypes.c_int(0)
    _check(lib.frt_select_faces(_ptr(boxes), _ptr(s), _ptr(l), n, int(min_face), max_batch, _ptr(out), _ptr(src_out), _ptr(ldm_out), _ptr(pos),
                                _ptr(passes), ctypes.byref(k), device))
    return dict(boxes=out, src=src_out, landmarks=ldm_out, keep_pos=pos, pass_count=passes, n_kept=k.value)


# ----------------------------------------------------------------------------------------------------------------------
# face images instead of frames (frt_preprocess_faces / frt_embedder_embed_faces / frt_embedder_enrol_faces)
# ----------------------------------------------------------------------------------------------------------------------
class FaceImage(ctypes.Structure):  # == frt_face_image
    _fields_ = [("bgr", _vp), ("rows", ctypes.c_int32), ("cols", ctypes.c_int32), ("row_stride", _sz)]


def _face_images(faces):
    """list of H x W x 3 u8 arrays -> (frt_face_image array, the arrays it points into).  A view whose pixels are contiguous within a row is
    passed with its row stride, not copied."""
    keep = []
    for f in faces:
        a = np.asarray(f)
        if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
            raise ValueError("face images are H x W x 3 uint8 arrays")
        if a.shape[0] and a.shape[1] and (a.strides[2] != 1 or a.strides[1] != 3 or a.strides[0] < a.shape[1] * 3):
            a = np.ascontiguousarray(a)
        keep.append(a)
    arr = (FaceImage * max(len(keep), 1))()
    for i, a in enumerate(keep):
        arr[i] = FaceImage(a.ctypes.data, a.shape[0], a.shape[1], a.strides[0])
    return arr, keep


def preprocessFaces(faces, device=0):
    """``cv::resize(face, face, Size(112, 112))`` where the size differs (src/app.cpp:84-87, :152-155, :255-258: default INTER_LINEAR) +
    ``preprocessFace`` for a list of face images of any sizes, one launch -> (u8 BGR [n][112][112][3], float32 planar RGB [n][3][112][112])."""
    arr, keep = _face_images(faces)
    n = len(keep)
    crops = np.zeros((n, 112, 112, 3), np.uint8)
    chw = np.zeros((n, 3, 112, 112), np.float32)
    _check(lib.frt_preprocess_faces(arr, n, _ptr(crops), _ptr(chw), device))
    return crops, chw


def resizeImages(images, width, height, device=0):
    """``resizeFrame`` for a list of H x W x 3 u8 images of any sizes, one launch (frt_resize_images) -> u8 [n][height][width][3]."""
    arr, keep = _face_images(images)
    n = len(keep)
    out = np.zeros((n, int(height), int(width), 3), np.uint8)
    _check(lib.frt_resize_images(arr, n, _ptr(out), int(height), int(width), device))
    return out


def enrol_select_dev(results_ptr, embeds_ptr, n_frames, max_faces, status_ptr, face_ptr, rows_ptr, count_ptr, hip_stream=None):
    """frt_enrol_select_dev: the "exactly one face" rule on device-resident pipeline records; raw device addresses, asynchronous."""
    _check(lib.frt_enrol_select_dev(_vp(results_ptr), _vp(embeds_ptr), int(n_frames), int(max_faces), _vp(status_ptr), _vp(face_ptr) if face_ptr else None,
                                    _vp(rows_ptr), _vp(count_ptr), _vp(hip_stream) if hip_stream else None))


# ----------------------------------------------------------------------------------------------------------------------
# class ArcFaceIR50 (src/arcface.h)
# ----------------------------------------------------------------------------------------------------------------------
def enrol_select_gated_dev(results_ptr, embeds_ptr, n_frames, max_faces, status_ptr, face_ptr, rows_ptr, count_ptr, hip_stream=None, quality_ptr=None):
    """frt_enrol_select_gated_dev: ``enrol_select_dev`` with the quality gate - an OK frame whose slot 0 record (``quality_ptr``:
    QUALITY_DTYPE [n_frames, max_faces] on the device, None: no gate) carries a flag is FRT_ENROL_LOW_QUALITY and adds no row."""
    _check(lib.frt_enrol_select_gated_dev(_vp(results_ptr), _vp(embeds_ptr), int(n_frames), int(max_faces), _vp(status_ptr),
                                          _vp(face_ptr) if face_ptr else None, _vp(rows_ptr), _vp(count_ptr), _vp(hip_stream) if hip_stream else None,
                                          _vp(quality_ptr) if quality_ptr else None))


# ----------------------------------------------------------------------------------------------------------------------
# face quality: is a crop good enough to use (include/frt.h "Face quality"; tests/quality_ref.py restates it in numpy)
# ----------------------------------------------------------------------------------------------------------------------
QUALITY_DTYPE = np.dtype([("sum_y", "<u4"), ("sum_y2", "<u4"), ("sum_lap", "<i4"), ("n_dark", "<u4"), ("n_bright", "<u4"), ("size", "<i4"),
                          ("sum_lap2", "<u8"), ("mean", "<f4"), ("luma_var", "<f4"), ("sharpness", "<f4"), ("score", "<f4"), ("flags", "<u4"),
                          ("present", "<i4")])  # == struct frt_face_quality
assert QUALITY_DTYPE.itemsize == 56 and QUALITY_DTYPE.fields["sum_lap2"][1] == 24
QUALITY_SMALL, QUALITY_BLURRED, QUALITY_FLAT, QUALITY_DARK, QUALITY_BRIGHT, QUALITY_CLIPPED, QUALITY_LOW_SCORE = 1, 2, 4, 8, 16, 32, 64


class QualityOptions(ctypes.Structure):  # == frt_quality_options; the defaults flag nothing - there are no recommended thresholds
    _fields_ = [("min_size", ctypes.c_int32), ("min_sharpness", ctypes.c_float), ("min_luma_var", ctypes.c_float), ("min_mean", ctypes.c_float),
                ("max_mean", ctypes.c_float), ("max_clipped", ctypes.c_int32), ("min_score", ctypes.c_float)]

    def __init__(self, min_size=0, min_sharpness=0.0, min_luma_var=0.0, min_mean=0.0, max_mean=255.0, max_clipped=12544, min_score=0.0):
        super().__init__(min_size, min_sharpness, min_luma_var, min_mean, max_mean, max_clipped, min_score)


def _quality_options(options):
    if options is not None and not isinstance(options, QualityOptions):
        raise TypeError("options must be a QualityOptions or None")
    return ctypes.addressof(options) if options is not None else None


def faceQuality(crops, results=None, options=None, device=0):
    """frt_face_quality: u8 BGR crops [n, 112, 112, 3] (and, optionally, their RESULT_DTYPE records [n]: a record with valid == 0 marks an
    absent slot, whose crop is not read) -> QUALITY_DTYPE [n].  A face passes iff ``present`` and ``flags == 0``."""
    crops = np.ascontiguousarray(crops, np.uint8)
    if crops.ndim != 4 or crops.shape[1:] != (112, 112, 3):
        raise ValueError("crops must be [n, 112, 112, 3]")
    n = crops.shape[0]
    if results is not None:
        results = np.ascontiguousarray(results, RESULT_DTYPE).reshape(-1)
        if results.size != n:
            raise ValueError("one record per crop")
    out = np.zeros(n, QUALITY_DTYPE)
    _check(lib.frt_face_quality(_ptr(crops), _ptr(results), n, _quality_options(options), _ptr(out), int(device)))
    return out


def face_quality_dev(crops_ptr, results_ptr, n, quality_ptr, options=None, hip_stream=None):
    """frt_face_quality_dev: asynchronous on ``hip_stream``; raw device addresses (``results_ptr`` may be None)."""
    _check(lib.frt_face_quality_dev(_vp(crops_ptr), _vp(results_ptr) if results_ptr else None, int(n), _quality_options(options), _vp(quality_ptr),
                                    _vp(hip_stream) if hip_stream else None))


class ArcFaceIR50:
    classCount = 0  # the reference keeps this as a process-wide static (arcface.cpp:19); per-instance here

    def __init__(self, engineFile, frameWidth=640, frameHeight=480, inputShape=(3, 112, 112), outputDim=512, maxBatchSize=1,
                 maxFacesPerScene=4, knownPersonThreshold=0.65, inputName="input", outputName="output", device=0):
        assert len(inputShape) == 3
        self._h = _vp()
        self.outputDim, self.maxBatchSize, self.maxFacesPerScene = int(outputDim), int(maxBatchSize), int(maxFacesPerScene)
        self.knownPersonThresh = knownPersonThreshold
        _check(lib.frt_embedder_create(os.fsencode(engineFile), *[int(x) for x in inputShape], self.outputDim, self.maxBatchSize, device,
                                       ctypes.byref(self._h)))
        d = describe_weights(engineFile)
        self._num_layers, self._se = d["numLayers"], d["se"]
        self.matmul = MatMul(device)
        self.croppedFaces = []  # list of dicts: face (u8 BGR crop), x1, y1, x2, y2  (struct CroppedFace, arcface.h:11-15)
        self.classNames = []
        self.classCount = 0
        self._known = None
        self._embeds = np.zeros((0, self.outputDim), np.float32)

    @property
    def numLayers(self):
        """Depth of the backbone the engine file holds: 50, 100 or 152 (the class keeps the reference's name for all six)."""
        return self._num_layers

    @property
    def se(self):
        """True for the IR-SE backbones."""
        return self._se

    def setPrecision(self, fp32):
        """``True``: fp32 activations / weights / products end to end (BASELINE configs[1]'s "fp32"; slow, a few faces per call);
        ``False`` (default): fp16 on the matrix cores with fp32 accumulation."""
        _check(lib.frt_embedder_set_precision(self._h, 1 if fp32 else 0))

    def setFlip(self, on):
        """``True``: flip-augmented embeddings, ``normalize(pre(face) + pre(mirrored face))``, on every path through this object
        (frt_embedder_set_flip; about twice the recogniser time per face).  Gallery and probes must be embedded in the same mode."""
        _check(lib.frt_embedder_set_flip(self._h, 1 if on else 0))

    @property
    def flip(self):
        """Whether flip-augmented embeddings are on (``setFlip``)."""
        on = _i(0)
        _check(lib.frt_embedder_get_flip(self._h, ctypes.byref(on)))
        return bool(on.value)

    def setSeFused(self, enable):
        """IR-SE only: SE tail inside conv2's epilogue (default) or as stand-alone launches (equal to float rounding)."""
        _check(lib.frt_embedder_set_se_fused(self._h, 1 if enable else 0))

    def preprocessFace(self, face):
        face = np.ascontiguousarray(face, np.uint8)
        out = np.empty((3, 112, 112), np.float32)
        _check(lib.frt_embedder_preprocess_face(self._h, _ptr(face), _ptr(out)))
        return out

    def doInference(self, chw, batchSize=None):
        x = np.ascontiguousarray(chw, np.float32).reshape(-1, 3, 112, 112)
        b = x.shape[0] if batchSize is None else batchSize
        out = np.empty((b, self.outputDim), np.float32)
        _check(lib.frt_embedder_infer(self._h, _ptr(x), b, _ptr(out)))
        return out

    def initKnownEmbeds(self, num):
        self._known = np.zeros((int(num), self.outputDim), np.float32)

    def addEmbedding(self, className, embedding):
        self.classNames.append(className)
        self._known[self.classCount] = np.asarray(embedding, np.float32)
        self.classCount += 1

    def addEmbeddings(self, classNames, embeddings):
        """Bulk variant."""
        e = np.asarray(embeddings, np.float32)
        self._known[self.classCount:self.classCount + len(e)] = e
        self.classNames.extend(classNames)
        self.classCount += len(e)

    def setGallery(self, embeddings, classNames=None):
        """initKnownEmbeds + N x addEmbedding without per-row copies; ``classNames`` defaults to the row indices."""
        self._known = np.ascontiguousarray(embeddings, np.float32)
        self.classCount = len(self._known)
        self.classNames = classNames if classNames is not None else range(self.classCount)

    def resetEmbeddings(self):
        self.classCount = 0
        self.classNames = []

    def initMatMul(self):
        self.matmul.init(self._known[:self.classCount], self.classCount, self.outputDim)

    # live enrolment (/insert/face and /delete/user without /reload): the device rows and classNames / classCount move together.  The host
    # copy behind initKnownEmbeds / addEmbedding is not involved; a later load cycle replaces the gallery as /reload does.
    def enrolEmbedding(self, className, embedding):
        """One row, or rows [n, outputDim] with ``className`` a list of n names.  Returns the first new row index."""
        e = np.ascontiguousarray(embedding, np.float32).reshape(-1, self.outputDim)
        names = [className] if isinstance(className, (str, bytes)) or e.shape[0] == 1 and not isinstance(className, (list, tuple)) else list(className)
        if len(names) != e.shape[0]:
            raise ValueError("enrolEmbedding: %d names for %d rows" % (len(names), e.shape[0]))
        if self.matmul.k == 0:  # never loaded: an empty gallery of this width first
            self.matmul.galleryBegin(0, self.outputDim)
            self.matmul.galleryCommit()
        first = self.matmul.galleryAdd(e)
        self.classNames = list(self.classNames) + names
        self.classCount = len(self.classNames)
        return first

    def removeClass(self, className):
        """Remove every row of ``className`` (as /delete/user does); returns how many there were."""
        rows = [i for i, n in enumerate(self.classNames) if n == className]
        if rows:
            self.matmul.galleryRemove(rows)
            gone = set(rows)
            self.classNames = [n for i, n in enumerate(self.classNames) if i not in gone]
            self.classCount = len(self.classNames)
        return len(rows)

    def forward(self, image, outputBbox):
        image = np.ascontiguousarray(image, np.uint8)
        boxes = np.ascontiguousarray(outputBbox, BBOX_DTYPE)
        n = len(boxes)
        embeds = np.zeros((n, self.outputDim), np.float32)
        crops = np.zeros((n, 112, 112, 3), np.uint8)
        if n:
            _check(lib.frt_embedder_forward(self._h, _ptr(image), image.shape[0], image.shape[1], image.strides[0], _ptr(boxes), n,
                                            _ptr(embeds), _ptr(crops)))
        self._embeds = embeds
        self.croppedFaces = [dict(face=crops[i], x1=int(b["x1"]), y1=int(b["y1"]), x2=int(b["x2"]), y2=int(b["y2"])) for i, b in enumerate(boxes)]
        return embeds

    def forwardAligned(self, image, outputBbox, landmarks):
        """``forward`` with the optional aligned crop (boxes are only carried into ``croppedFaces``)."""
        image = np.ascontiguousarray(image, np.uint8)
        boxes = np.ascontiguousarray(outputBbox, BBOX_DTYPE)
        lm = np.ascontiguousarray(landmarks, np.float32).reshape(-1, 10)
        n = len(lm)
        assert len(boxes) == n
        embeds = np.zeros((n, self.outputDim), np.float32)
        crops = np.zeros((n, 112, 112, 3), np.uint8)
        if n:
            _check(lib.frt_embedder_forward_aligned(self._h, _ptr(image), image.shape[0], image.shape[1], image.strides[0], _ptr(lm), n,
                                                    _ptr(embeds), _ptr(crops)))
        self._embeds = embeds
        self.croppedFaces = [dict(face=crops[i], x1=int(b["x1"]), y1=int(b["y1"]), x2=int(b["x2"]), y2=int(b["y2"])) for i, b in enumerate(boxes)]
        return embeds

    # face images instead of frames: /recognize (src/app.cpp:243-287), /insert/face with api_imgIsCropped (:148-162), gen (:69-99)
    def forwardFaces(self, faces):
        """``forward`` for pre-cropped face images (a list of H x W x 3 u8 arrays of any sizes): resize to 112 x 112 + preprocessFace on the
        device, full recogniser passes while the next images upload.  Leaves what ``forward`` leaves: the embeddings, and ``croppedFaces``
        with the resized face and the box 0, 0, 112, 112 that /recognize builds (src/app.cpp:266-267)."""
        arr, keep = _face_images(faces)
        n = len(keep)
        embeds = np.zeros((n, self.outputDim), np.float32)
        crops = np.zeros((n, 112, 112, 3), np.uint8)
        _check(lib.frt_embedder_embed_faces(self._h, arr, n, _ptr(embeds), _ptr(crops)))
        self._embeds = embeds
        self.croppedFaces = [dict(face=crops[i], x1=0, y1=0, x2=112, y2=112) for i in range(n)]
        return embeds

    def enrolFaces(self, classNames, faces, labels=None):
        """``enrolEmbedding`` from the face images themselves: embeds them and appends the rows to the live gallery in one edit, device to
        device.  ``labels``: one int per image for a labelled gallery (``MatMul.set_labels``).  Returns (first new row index, embeddings)."""
        arr, keep = _face_images(faces)
        names = list(classNames)
        n = len(keep)
        if len(names) != n:
            raise ValueError("enrolFaces: %d names for %d images" % (len(names), n))
        l = None
        if labels is not None:
            l = np.ascontiguousarray(labels, np.int32).reshape(-1)
            if l.size != n:
                raise ValueError("enrolFaces: one label per image")
        if self.matmul.k == 0:  # never loaded: an empty gallery of this width first
            self.matmul.galleryBegin(0, self.outputDim)
            self.matmul.galleryCommit()
        embeds = np.zeros((n, self.outputDim), np.float32)
        first = _i(0)
        _check(lib.frt_embedder_enrol_faces(self._h, self.matmul._h, arr, n, _ptr(l), _ptr(embeds), ctypes.byref(first)))
        self.matmul._edited()
        self.classNames = list(self.classNames) + names
        self.classCount = len(self.classNames)
        return first.value, embeds

    def featureMatching(self):
        if not len(self.classNames) or not self.croppedFaces:
            raise FrtError(FRT_ERR_EMPTY, "Feature matching: No faces in database or no faces found")  # arcface.cpp:198
        return self.matmul.calculate(self._embeds, len(self.croppedFaces))

    def getOutputs(self, output_sims):
        sims = np.asarray(output_sims, np.float32).reshape(len(self.croppedFaces), self.classCount)
        arg = sims.argmax(1)  # first maximum == std::max_element (arcface.cpp:210)
        return [self.classNames[a] for a in arg], [float(sims[i, a]) for i, a in enumerate(arg)]

    def matchTop1(self):
        """Fused featureMatching + getOutputs on the device (never materialises the F x N matrix)."""
        if not len(self.classNames) or not self.croppedFaces:
            raise FrtError(FRT_ERR_EMPTY, "Feature matching: No faces in database or no faces found")
        idx, sim = self.matmul.top1(self._embeds)
        return [self.classNames[a] for a in idx], [float(s) for s in sim]

    def close(self):
        if self._h:
            lib.frt_embedder_destroy(self._h)
            self._h = _vp()
        self.matmul.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ----------------------------------------------------------------------------------------------------------------------
# request coalescer (opt-in): concurrent one-frame requests -> pipeline batches (frt_coalescer_*)
# ----------------------------------------------------------------------------------------------------------------------
class Coalescer:
    def __init__(self, detector, recognizer, max_frames, window_us=100, match=True):
        self._h = _vp()
        self.det, self.rec = detector, recognizer
        self.max_faces = detector.maxFacesPerScene
        _check(lib.frt_coalescer_create(detector._h, recognizer._h, recognizer.matmul._h if match else None, int(max_frames), int(window_us),
                                        ctypes.byref(self._h)))

    def infer(self, frame, want_embeds=True, want_crops=False):
        """One frame (u8 BGR [H, W, 3]) -> (records of its boxes, embeddings [n, 512] or None[, u8 crops [n, 112, 112, 3]]).  Blocks; call
        it from many threads."""
        frame = np.ascontiguousarray(frame, np.uint8)
        res = np.zeros(self.max_faces, RESULT_DTYPE)
        emb = np.zeros((self.max_faces, 512), np.float32) if want_embeds else None
        crops = np.zeros((self.max_faces, 112, 112, 3), np.uint8) if want_crops else None
        n = ctypes.c_int(0)
        _check(lib.frt_coalescer_infer_crops(self._h, _ptr(frame), frame.shape[0], frame.shape[1], frame.shape[1] * 3, _ptr(res), _ptr(emb), _ptr(crops),
                                             ctypes.byref(n)))
        out = (res[:n.value], (emb[:n.value] if want_embeds else None))
        return out + (crops[:n.value],) if want_crops else out

    def stats(self):
        b, f = ctypes.c_long(0), ctypes.c_long(0)
        _check(lib.frt_coalescer_stats(self._h, ctypes.byref(b), ctypes.byref(f)))
        return int(b.value), int(f.value)

    def close(self):
        if self._h:
            lib.frt_coalescer_destroy(self._h)
            self._h = _vp()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ----------------------------------------------------------------------------------------------------------------------
# face tracker: the state that joins the consecutive frames of a video stream, on the device (include/frt.h "Face tracker")
# ----------------------------------------------------------------------------------------------------------------------
TRACK_DTYPE = np.dtype([("track_id", "<i4"), ("slot", "<i4"), ("age", "<i4"), ("hits", "<i4"), ("n_embeds", "<i4"), ("confirmed", "<i4"),
                        ("match_idx", "<i4"), ("match_sim", "<f4")])  # == frt_track_result
TRACK_STATE_DTYPE = np.dtype([("live", "<i4"), ("id", "<i4"), ("x1", "<i4"), ("y1", "<i4"), ("x2", "<i4"), ("y2", "<i4"), ("score", "<f4"),
                              ("born", "<i4"), ("hits", "<i4"), ("missed", "<i4"), ("n_embeds", "<i4"), ("match_idx", "<i4"),
                              ("match_sim", "<f4")])  # == frt_track_state
TRACK_ASSOC_DTYPE = np.dtype([("how", "<i4"), ("gap", "<i4"), ("ovr", "<f4"), ("sim", "<f4")])  # == frt_track_assoc
TRACK_ASSOC_ABSENT, TRACK_ASSOC_IOU, TRACK_ASSOC_APPEARANCE, TRACK_ASSOC_BIRTH, TRACK_ASSOC_UNTRACKED = range(5)  # frt_track_assoc.how
TRACK_REID_OFF, TRACK_MIN_SIM_OFF = 2.0, -2.0
assert TRACK_DTYPE.itemsize == 32 and TRACK_STATE_DTYPE.itemsize == 52 and TRACK_ASSOC_DTYPE.itemsize == 16


class TrackOptions(ctypes.Structure):  # == frt_track_options
    _fields_ = [("iou_threshold", ctypes.c_float), ("max_missed", ctypes.c_int32), ("min_hits", ctypes.c_int32), ("decay", ctypes.c_float)]


# the gate in front of the recogniser (include/frt.h "Gate")
TRACK_GATE_DTYPE = np.dtype([("decision", "<i4"), ("slot", "<i4"), ("ovr", "<f4"), ("why", "<i4")])  # == frt_track_gate
TRACK_GATE_ABSENT, TRACK_GATE_EMBED, TRACK_GATE_FOLLOW = range(3)  # frt_track_gate.decision
TRACK_GATE_NO_TRACK, TRACK_GATE_UNCONFIRMED, TRACK_GATE_FEW_EMBEDS, TRACK_GATE_LOW_OVERLAP, TRACK_GATE_REFRESH = 1, 2, 4, 8, 16  # .why
assert TRACK_GATE_DTYPE.itemsize == 16


class TrackGateOptions(ctypes.Structure):  # == frt_track_gate_options; no defaults: nobody has measured these on real video
    _fields_ = [("refresh", ctypes.c_int32), ("min_embeds", ctypes.c_int32), ("skip_iou", ctypes.c_float)]


def _stream_ids(stream_ids, n):
    if stream_ids is None:
        return None
    ids = np.ascontiguousarray(stream_ids, np.int32).reshape(-1)
    if ids.size != n:
        raise ValueError("one stream id per frame")
    return ids


class Tracker:
    """``n_streams`` independent video streams of up to ``max_tracks`` tracks each.  An update takes the pipeline's records and embeddings
    of one frame per stream and returns, per face slot, a stable track id, the track's age / hits / confirmed flag and the identity of the
    track's running template (when a matcher - a ``MatMul`` - with rows is given).  ``reid_threshold`` / ``iou_min_sim`` (None: off) switch
    the appearance term on (include/frt.h "Appearance"): a lost face whose embedding is at least ``reid_threshold`` like a track's running sum
    is re-attached to it, and an overlap match whose similarity is below ``iou_min_sim`` is refused.  ``motion_gain`` (None or 0: off; 1 ..
    256) switches the constant-velocity term on (include/frt.h "Motion"): every overlap is then taken with the track's predicted box."""

    def __init__(self, n_streams, max_tracks=16, max_faces=4, dim=512, iou_threshold=0.3, max_missed=5, min_hits=3, decay=1.0, device=0,
                 reid_threshold=None, iou_min_sim=None, motion_gain=None):
        self._h = _vp()
        self.n_streams, self.max_tracks, self.max_faces, self.dim = int(n_streams), int(max_tracks), int(max_faces), int(dim)
        opt = TrackOptions(iou_threshold, max_missed, min_hits, decay)
        _check(lib.frt_tracker_create(self.n_streams, self.max_tracks, self.max_faces, self.dim, ctypes.addressof(opt), int(device), ctypes.byref(self._h)))
        try:
            if reid_threshold is not None or iou_min_sim is not None:
                self.setAppearance(reid_threshold, iou_min_sim)
            if motion_gain is not None:
                self.setMotion(motion_gain)
        except Exception:
            self.close()
            raise

    def setAppearance(self, reid_threshold=None, iou_min_sim=None):
        """``reid_threshold`` in (0, 1], ``iou_min_sim`` in [-1, 1]; None switches either off.  Takes effect with the next update."""
        _check(lib.frt_tracker_set_appearance(self._h, TRACK_REID_OFF if reid_threshold is None else float(reid_threshold),
                                              TRACK_MIN_SIM_OFF if iou_min_sim is None else float(iou_min_sim)))

    def getAppearance(self):
        """-> (reid_threshold, iou_min_sim), None where off"""
        r, m = ctypes.c_float(), ctypes.c_float()
        _check(lib.frt_tracker_get_appearance(self._h, ctypes.addressof(r), ctypes.addressof(m)))
        return (None if r.value == TRACK_REID_OFF else r.value, None if m.value == TRACK_MIN_SIM_OFF else m.value)

    def setMotion(self, gain=None):
        """``gain`` 1 .. 256: the weight of a new measurement in a track's velocity, in 1/256; None or 0 switches motion off.  Takes effect
        with the next update or gate; off -> on starts every velocity from zero."""
        _check(lib.frt_tracker_set_motion(self._h, 0 if gain is None else int(gain)))

    def getMotion(self):
        """-> the gain, 0 where off"""
        g = ctypes.c_int(-1)
        _check(lib.frt_tracker_get_motion(self._h, ctypes.addressof(g)))
        return g.value

    def motion(self, stream):
        """-> (vel int32 [max_tracks, 2]: (vx, vy) of every slot in 1/256 pixel per update, pred BBOX_DTYPE [max_tracks]: the box each slot
        is compared with in the NEXT update, zeros for a free slot).  Refused while motion is off."""
        vel = np.zeros((self.max_tracks, 2), np.int32)
        pred = np.zeros(self.max_tracks, BBOX_DTYPE)
        _check(lib.frt_tracker_motion(self._h, int(stream), _ptr(vel), _ptr(pred)))
        return vel, pred

    def update(self, results, embeds, stream_ids=None, matcher=None, want_templates=True, want_assoc=False):
        """results RESULT_DTYPE [n * max_faces], embeds float32 [n * max_faces, dim] (host) -> (TRACK_DTYPE [n, max_faces], templates
        float32 [n, max_faces, dim] or None[, with ``want_assoc``: TRACK_ASSOC_DTYPE [n, max_faces], how each detection was associated])."""
        results = np.ascontiguousarray(results, RESULT_DTYPE).reshape(-1)
        if results.size == 0 or results.size % self.max_faces:
            raise ValueError("results must hold max_faces records per frame")
        n = results.size // self.max_faces
        embeds = np.ascontiguousarray(embeds, np.float32)
        if embeds.size != results.size * self.dim:
            raise ValueError("embeds must be [n * max_faces, dim]")
        ids = _stream_ids(stream_ids, n)
        trk = np.zeros((n, self.max_faces), TRACK_DTYPE)
        tpl = np.zeros((n, self.max_faces, self.dim), np.float32) if want_templates else None
        if want_assoc:
            assoc = np.zeros((n, self.max_faces), TRACK_ASSOC_DTYPE)
            _check(lib.frt_tracker_update_assoc(self._h, matcher._h if matcher is not None else None, _ptr(results), _ptr(embeds), n, _ptr(ids), _ptr(trk),
                                                _ptr(tpl), _ptr(assoc)))
            return trk, tpl, assoc
        _check(lib.frt_tracker_update(self._h, matcher._h if matcher is not None else None, _ptr(results), _ptr(embeds), n, _ptr(ids), _ptr(trk), _ptr(tpl)))
        return trk, tpl

    def updateDev(self, results_ptr, embeds_ptr, n_frames, tracks_ptr, templates_ptr=None, stream_ids=None, matcher=None, hip_stream=None, assoc_ptr=None):
        """Asynchronous on ``hip_stream``; the pointers are raw device addresses (``frt_pipeline_run_dev``'s results_dev / embeds_dev);
        ``assoc_ptr``: room for n_frames * max_faces TRACK_ASSOC_DTYPE records, or None."""
        ids = _stream_ids(stream_ids, int(n_frames))
        _check(lib.frt_tracker_update_assoc_dev(self._h, matcher._h if matcher is not None else None, _vp(results_ptr), _vp(embeds_ptr), int(n_frames),
                                                _ptr(ids), _vp(tracks_ptr), _vp(templates_ptr) if templates_ptr else None,
                                                _vp(assoc_ptr) if assoc_ptr else None, _vp(hip_stream) if hip_stream else None))

    def gate(self, boxes, refresh, min_embeds, skip_iou, stream_ids=None, n_boxes=None, max_batch=128):
        """The gate alone (frt_tracker_gate; include/frt.h "Gate"): boxes BBOX_DTYPE [n * max_faces] of one frame per stream (``n_boxes``
        int32 [n]: the detector's counts, None: every slot with score > 0 is present) -> (TRACK_GATE_DTYPE [n, max_faces], the work list int32
        [n * max_faces] - the face indices to embed, ascending, -1 behind them -, n_embed, pass_count int32 [ceil(n * max_faces / max_batch)]).
        Reads the state, writes none.  ``refresh`` / ``min_embeds`` / ``skip_iou`` have no defaults."""
        boxes = np.ascontiguousarray(boxes, BBOX_DTYPE).reshape(-1)
        if boxes.size == 0 or boxes.size % self.max_faces:
            raise ValueError("boxes must hold max_faces boxes per frame")
        n = boxes.size // self.max_faces
        ids = _stream_ids(stream_ids, n)
        if n_boxes is not None:
            n_boxes = np.ascontiguousarray(n_boxes, np.int32).reshape(-1)
            if n_boxes.size != n:
                raise ValueError("one box count per frame")
        opt = TrackGateOptions(int(refresh), int(min_embeds), float(skip_iou))
        max_batch = int(max_batch)
        gate = np.zeros((n, self.max_faces), TRACK_GATE_DTYPE)
        lst = np.zeros(boxes.size, np.int32)
        cnt = np.zeros(1, np.int32)
        passes = np.zeros(max(-(-boxes.size // max(max_batch, 1)), 1), np.int32)
        _check(lib.frt_tracker_gate(self._h, ctypes.addressof(opt), _ptr(boxes), _ptr(n_boxes), n, _ptr(ids), _ptr(gate), _ptr(lst), _ptr(cnt),
                                    _ptr(passes), max_batch))
        return gate, lst, int(cnt[0]), passes

    def gateDev(self, boxes_ptr, n_frames, refresh, min_embeds, skip_iou, gate_ptr, list_ptr, n_embed_ptr, pass_count_ptr, max_batch, stream_ids=None,
                n_boxes_ptr=None, hip_stream=None):
        """Asynchronous on ``hip_stream`` (frt_tracker_gate_dev); the pointers are raw device addresses."""
        ids = _stream_ids(stream_ids, int(n_frames))
        opt = TrackGateOptions(int(refresh), int(min_embeds), float(skip_iou))
        _check(lib.frt_tracker_gate_dev(self._h, ctypes.addressof(opt), _vp(boxes_ptr), _vp(n_boxes_ptr) if n_boxes_ptr else None, int(n_frames),
                                        _ptr(ids), _vp(gate_ptr), _vp(list_ptr), _vp(n_embed_ptr), _vp(pass_count_ptr), int(max_batch),
                                        _vp(hip_stream) if hip_stream else None))

    def tracks(self, stream, want_sums=False):
        """-> (slots TRACK_STATE_DTYPE [max_tracks], every slot, live or not; counters dict(next_id, tick, dropped)[; sums [max_tracks, dim]])"""
        slots = np.zeros(self.max_tracks, TRACK_STATE_DTYPE)
        sums = np.zeros((self.max_tracks, self.dim), np.float32) if want_sums else None
        cnt = np.zeros(3, np.int32)
        _check(lib.frt_tracker_tracks(self._h, int(stream), _ptr(slots), _ptr(sums), _ptr(cnt)))
        counters = dict(next_id=int(cnt[0]), tick=int(cnt[1]), dropped=int(cnt[2]))
        return (slots, counters, sums) if want_sums else (slots, counters)

    def reset(self, stream=-1):
        """Free the slots of ``stream`` (-1: of every stream) and zero its tick / dropped; track ids are never reused."""
        _check(lib.frt_tracker_reset(self._h, int(stream)))

    def close(self):
        for book in list(getattr(self, "_books", ())):  # the books borrow this tracker: they go first
            book.destroy()
        if self._h:
            lib.frt_tracker_destroy(self._h)
            self._h = _vp()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ----------------------------------------------------------------------------------------------------------------------
# sighting book: one record per finished track, with its best shot (include/frt.h "Sightings")
# ----------------------------------------------------------------------------------------------------------------------
SIGHTING_DTYPE = np.dtype([("stream", "<i4"), ("track_id", "<i4"), ("first_tick", "<i4"), ("last_tick", "<i4"), ("close_tick", "<i4"),
                           ("reason", "<i4"), ("hits", "<i4"), ("n_embeds", "<i4"), ("confirmed", "<i4"), ("match_idx", "<i4"), ("match_sim", "<f4"),
                           ("n_shots", "<i4"), ("best_tick", "<i4"), ("x1", "<i4"), ("y1", "<i4"), ("x2", "<i4"), ("y2", "<i4"), ("score", "<f4"),
                           ("best_sharpness", "<f4"), ("best_luma_var", "<f4"), ("best_mean", "<f4"), ("best_flags", "<u4"), ("best_size", "<i4"),
                           ("reserved", "<i4")])  # == frt_sighting; x1 .. score: best_box
SHOT_RANK_SHARPNESS, SHOT_RANK_SIZE, SHOT_RANK_SCORE = range(3)
SIGHTING_EXPIRED, SIGHTING_REPLACED, SIGHTING_CLOSED = 1, 2, 3  # frt_sighting.reason; 0: open
assert SIGHTING_DTYPE.itemsize == 96


class SightingOptions(ctypes.Structure):  # == frt_sighting_options
    _fields_ = [("rank", ctypes.c_int32), ("min_hits", ctypes.c_int32), ("keep_crops", ctypes.c_int32)]


class Sightings:
    """The sighting book of one :class:`Tracker` (which it borrows: close the book first).  It shadows every live track, keeps the track's
    best shot - ``rank``: by sharpness, size or detector score, an unflagged shot before a flagged one - and queues one SIGHTING_DTYPE record,
    with the best shot's embedding, the track's template and (``keep_crops``) the crop, when the track ends.  One ``update`` follows one
    tracker update of the same frames and stream ids."""

    def __init__(self, tracker, capacity, rank=SHOT_RANK_SHARPNESS, min_hits=1, keep_crops=True):
        self._h = _vp()
        self.tracker, self.capacity, self.keep_crops = tracker, int(capacity), bool(keep_crops)
        opt = SightingOptions(int(rank), int(min_hits), int(keep_crops))
        _check(lib.frt_sightings_create(tracker._h, self.capacity, ctypes.addressof(opt), ctypes.byref(self._h)))
        tracker.__dict__.setdefault("_books", weakref.WeakSet()).add(self)  # Tracker.close destroys its books before itself

    def update(self, results, tracks, embeds, quality, templates=None, crops=None, stream_ids=None):
        """Host arrays of one tracker update: results RESULT_DTYPE, tracks TRACK_DTYPE, quality QUALITY_DTYPE [n * max_faces]; embeds,
        templates (or None) float32 [n * max_faces, dim]; crops u8 [n * max_faces, 112, 112, 3], required iff the book keeps crops."""
        t = self.tracker
        results = np.ascontiguousarray(results, RESULT_DTYPE).reshape(-1)
        if results.size == 0 or results.size % t.max_faces:
            raise ValueError("results must hold max_faces records per frame")
        F, n = results.size, results.size // t.max_faces
        tracks = np.ascontiguousarray(tracks, TRACK_DTYPE).reshape(-1)
        quality = np.ascontiguousarray(quality, QUALITY_DTYPE).reshape(-1)
        embeds = np.ascontiguousarray(embeds, np.float32)
        if tracks.size != F or quality.size != F or embeds.size != F * t.dim:
            raise ValueError("tracks, quality [n * max_faces] and embeds [n * max_faces, dim] must match results")
        if templates is not None:
            templates = np.ascontiguousarray(templates, np.float32)
            if templates.size != F * t.dim:
                raise ValueError("templates must be [n * max_faces, dim]")
        if crops is not None:
            crops = np.ascontiguousarray(crops, np.uint8)
            if crops.size != F * 112 * 112 * 3:
                raise ValueError("crops must be [n * max_faces, 112, 112, 3]")
        ids = _stream_ids(stream_ids, n)
        _check(lib.frt_sightings_update(self._h, _ptr(results), _ptr(tracks), _ptr(embeds), _ptr(templates), _ptr(quality), _ptr(crops), n, _ptr(ids)))

    def updateDev(self, results_ptr, tracks_ptr, embeds_ptr, quality_ptr, n_frames, templates_ptr=None, crops_ptr=None, stream_ids=None, hip_stream=None):
        """Asynchronous on ``hip_stream`` behind the tracker's last queued update; the pointers are raw device addresses."""
        ids = _stream_ids(stream_ids, int(n_frames))
        _check(lib.frt_sightings_update_dev(self._h, _vp(results_ptr), _vp(tracks_ptr), _vp(embeds_ptr), _vp(templates_ptr) if templates_ptr else None,
                                            _vp(quality_ptr), _vp(crops_ptr) if crops_ptr else None, int(n_frames), _ptr(ids),
                                            _vp(hip_stream) if hip_stream else None))

    def close(self, stream=-1):
        """End every open entry of ``stream`` (-1: of every stream) with reason SIGHTING_CLOSED: the end of a stream, or before
        ``Tracker.reset``.  (``destroy`` frees the book.)"""
        _check(lib.frt_sightings_close(self._h, int(stream)))

    def drain(self, max_out, want_embeds=True, want_templates=True, want_crops=None):
        """The oldest ``min(queued, max_out)`` sightings, removed from the queue -> (records SIGHTING_DTYPE [n], best embeddings [n, dim] or
        None, templates [n, dim] or None, crops u8 [n, 112, 112, 3] or None, counters dict(queued - before the call -, overflowed, discarded,
        closed))."""
        max_out, D = int(max_out), self.tracker.dim
        want_crops = self.keep_crops if want_crops is None else bool(want_crops)
        cap = max(max_out, 1)
        rec = np.zeros(cap, SIGHTING_DTYPE)
        emb = np.zeros((cap, D), np.float32) if want_embeds else None
        tpl = np.zeros((cap, D), np.float32) if want_templates else None
        crops = np.zeros((cap, 112, 112, 3), np.uint8) if want_crops else None
        n, cnt = ctypes.c_int(0), np.zeros(4, np.int32)
        _check(lib.frt_sightings_drain(self._h, max_out, _ptr(rec), _ptr(crops), _ptr(emb), _ptr(tpl), ctypes.byref(n), _ptr(cnt)))
        k = n.value
        counters = dict(queued=int(cnt[0]), overflowed=int(cnt[1]), discarded=int(cnt[2]), closed=int(cnt[3]))
        return (rec[:k].copy(), emb[:k].copy() if want_embeds else None, tpl[:k].copy() if want_templates else None,
                crops[:k].copy() if want_crops else None, counters)

    def open(self, stream, want_embeds=True, want_templates=True, want_crops=None):
        """The open entries of one stream -> (records SIGHTING_DTYPE [max_tracks], a free slot all zero, best embeddings, templates
        [max_tracks, dim] or None, crops [max_tracks, 112, 112, 3] or None)."""
        T, D = self.tracker.max_tracks, self.tracker.dim
        want_crops = self.keep_crops if want_crops is None else bool(want_crops)
        rec = np.zeros(T, SIGHTING_DTYPE)
        emb = np.zeros((T, D), np.float32) if want_embeds else None
        tpl = np.zeros((T, D), np.float32) if want_templates else None
        crops = np.zeros((T, 112, 112, 3), np.uint8) if want_crops else None
        _check(lib.frt_sightings_open(self._h, int(stream), _ptr(rec), _ptr(emb), _ptr(tpl), _ptr(crops)))
        return rec, emb, tpl, crops

    def destroy(self):
        if self._h:
            lib.frt_sightings_destroy(self._h)
            self._h = _vp()

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


# ----------------------------------------------------------------------------------------------------------------------
# batched device-resident pipeline (new surface)
# ----------------------------------------------------------------------------------------------------------------------
class Pipeline:
    def __init__(self, detector, recognizer, max_frames, match=True):
        """``match=False``: no matcher stage (records carry match_idx = -1); the caller matches the embeddings itself, e.g. against a
        sharded gallery (dist.py)."""
        self._h = _vp()
        self.det, self.rec = detector, recognizer
        self.max_frames = int(max_frames)
        self.max_faces = detector.maxFacesPerScene
        self._match = bool(match)
        _check(lib.frt_pipeline_create(detector._h, recognizer._h, recognizer.matmul._h if match else None, self.max_frames, ctypes.byref(self._h)))

    def run(self, frames, want_embeds=True):
        frames = np.ascontiguousarray(frames, np.uint8)
        n = frames.shape[0]
        res = np.zeros(n * self.max_faces, RESULT_DTYPE)
        emb = np.zeros((n * self.max_faces, 512), np.float32) if want_embeds else None
        _check(lib.frt_pipeline_run(self._h, _ptr(frames), n, _ptr(res), _ptr(emb)))
        return res, emb

    # whole photos of any sizes: the head of /inference (src/app.cpp:296-301) and /insert/face without api_imgIsCropped (:163-187)
    def runImages(self, images, want_embeds=True, want_crops=False):
        """``run`` for a list of H x W x 3 u8 images of any sizes: each is stretched to the detector's frame size on the device (cv::resize,
        INTER_LINEAR) and the chunks of ``max_frames`` images run back to back -> (records [n * max_faces], ``frame`` = index of the image,
        embeddings [n * max_faces, 512] or None[, u8 crops [n * max_faces, 112, 112, 3]])."""
        arr, keep = _face_images(images)
        n = len(keep)
        res = np.zeros(n * self.max_faces, RESULT_DTYPE)
        emb = np.zeros((n * self.max_faces, 512), np.float32) if want_embeds else None
        crops = np.zeros((n * self.max_faces, 112, 112, 3), np.uint8) if want_crops else None
        _check(lib.frt_pipeline_run_images(self._h, arr, n, _ptr(res), _ptr(emb), _ptr(crops)))
        return (res, emb, crops) if want_crops else (res, emb)

    def runTiled(self, photo, overlap=None, overview=True, metric=1, drop_cut=True, threshold=None, min_face=0, max_out=256, want_embeds=True,
                 want_crops=False, landmarks=False, sources=False):
        """A large photo by tiles, recognised in one call (frt_pipeline_run_photo_tiled): ``RetinaFace.findFaceTiled`` with these options,
        the boxes with min(x2 - x1, y2 - y1) >= ``min_face`` kept, then ``forward`` (``forwardAligned`` after ``set_align(True)``) and the
        top-1 match, all on the device, the photo uploaded once.  -> (records [n] with boxes in PHOTO coordinates and ``frame`` 0, embeddings
        [n, 512] or None[, u8 crops [n, 112, 112, 3]][, landmarks [n, 5, 2]][, source indices [n]])."""
        img = _photo(photo)
        opt = tileOptions(self.det.frameHeight, self.det.frameWidth, overlap, overview, metric, drop_cut, threshold)
        max_out = int(max_out)
        cap = max(max_out, 1)
        res = np.zeros(cap, RESULT_DTYPE)
        emb = np.zeros((cap, 512), np.float32) if want_embeds else None
        crops = np.zeros((cap, 112, 112, 3), np.uint8) if want_crops else None
        ldm = np.zeros((cap, 5, 2), np.float32) if landmarks else None
        src = np.full(cap, -1, np.int32) if sources else None
        n = ctypes.c_int(0)
        _check(lib.frt_pipeline_run_photo_tiled(self._h, _ptr(img), img.shape[0], img.shape[1], img.strides[0], ctypes.addressof(opt), int(min_face),
                                                max_out, _ptr(res), _ptr(ldm), _ptr(emb), _ptr(crops), _ptr(src), ctypes.byref(n)))
        k = n.value
        out = (res[:k].copy(), emb[:k].copy() if want_embeds else None)
        out += ((crops[:k].copy(),) if want_crops else ()) + ((ldm[:k].copy(),) if landmarks else ()) + ((src[:k].copy(),) if sources else ())
        return out

    def runTracked(self, tracker, frames, stream_ids=None, want_embeds=True, want_templates=True):
        """``run`` with a :class:`Tracker` behind it on the pipeline stream (frt_pipeline_run_tracked): ``frames`` are the current frames of
        the streams ``stream_ids`` (None: frame i is stream i) -> (records, embeddings or None - exactly ``run``'s -, track records
        TRACK_DTYPE [n, max_faces], templates [n, max_faces, 512] or None)."""
        frames = np.ascontiguousarray(frames, np.uint8)
        n = frames.shape[0]
        if frames.shape[1:] != (self.det.frameHeight, self.det.frameWidth, 3):
            raise ValueError("runTracked: frames must be [n, frameHeight, frameWidth, 3]")
        ids = _stream_ids(stream_ids, n)
        res = np.zeros(n * self.max_faces, RESULT_DTYPE)
        emb = np.zeros((n * self.max_faces, 512), np.float32) if want_embeds else None
        trk = np.zeros((n, self.max_faces), TRACK_DTYPE)
        tpl = np.zeros((n, self.max_faces, 512), np.float32) if want_templates else None
        _check(lib.frt_pipeline_run_tracked(self._h, tracker._h, _ptr(frames), n, _ptr(ids), _ptr(res), _ptr(trk), _ptr(emb), _ptr(tpl)))
        return res, emb, trk, tpl

    def runTrackedGated(self, tracker, frames, refresh, min_embeds, skip_iou, stream_ids=None, want_gate=False, want_embeds=True,
                        want_templates=True, want_crops=False):
        """``runTracked`` with the gate in front of the recogniser (frt_pipeline_run_tracked_gated; include/frt.h "Gate"): only the faces no
        confirmed track follows are cropped, embedded and matched; a followed face keeps its box, has valid 0 and a zero embedding row, and its
        identity is its track's -> (records, embeddings [n * max_faces, 512] or None, track records, templates or None, n_embed[, gate
        records TRACK_GATE_DTYPE [n, max_faces]][, u8 crops [n_embed, 112, 112, 3] of the embedded faces in list order])."""
        frames = np.ascontiguousarray(frames, np.uint8)
        n = frames.shape[0]
        if frames.shape[1:] != (self.det.frameHeight, self.det.frameWidth, 3):
            raise ValueError("runTrackedGated: frames must be [n, frameHeight, frameWidth, 3]")
        ids = _stream_ids(stream_ids, n)
        F = n * self.max_faces
        opt = TrackGateOptions(int(refresh), int(min_embeds), float(skip_iou))
        res = np.zeros(F, RESULT_DTYPE)
        emb = np.zeros((F, 512), np.float32) if want_embeds else None
        trk = np.zeros((n, self.max_faces), TRACK_DTYPE)
        tpl = np.zeros((n, self.max_faces, 512), np.float32) if want_templates else None
        gate = np.zeros((n, self.max_faces), TRACK_GATE_DTYPE) if want_gate else None
        crops = np.zeros((F, 112, 112, 3), np.uint8) if want_crops else None
        ne = ctypes.c_int32(0)
        _check(lib.frt_pipeline_run_tracked_gated(self._h, tracker._h, ctypes.addressof(opt), _ptr(frames), n, _ptr(ids), _ptr(res), _ptr(trk), _ptr(gate),
                                                  _ptr(emb), _ptr(tpl), _ptr(crops), ctypes.addressof(ne)))
        out = (res, emb, trk, tpl, ne.value)
        return out + ((gate,) if want_gate else ()) + ((crops[:ne.value].copy(),) if want_crops else ())

    def runSighted(self, tracker, book, frames, quality=None, stream_ids=None, want_embeds=True, want_quality=True):
        """``runTracked`` and ``runQuality`` in one call with a :class:`Sightings` book behind them on the pipeline stream
        (frt_pipeline_run_sighted) -> (records, embeddings or None, track records - exactly ``runTracked``'s -, QUALITY_DTYPE [n * max_faces]
        or None - exactly ``runQuality``'s).  The finished tracks wait in the book: ``book.drain``."""
        frames = np.ascontiguousarray(frames, np.uint8)
        n = frames.shape[0]
        if frames.shape[1:] != (self.det.frameHeight, self.det.frameWidth, 3):
            raise ValueError("runSighted: frames must be [n, frameHeight, frameWidth, 3]")
        ids = _stream_ids(stream_ids, n)
        res = np.zeros(n * self.max_faces, RESULT_DTYPE)
        emb = np.zeros((n * self.max_faces, 512), np.float32) if want_embeds else None
        trk = np.zeros((n, self.max_faces), TRACK_DTYPE)
        qual = np.zeros(n * self.max_faces, QUALITY_DTYPE) if want_quality else None
        _check(lib.frt_pipeline_run_sighted(self._h, tracker._h, book._h, _quality_options(quality), _ptr(frames), n, _ptr(ids), _ptr(res), _ptr(trk),
                                            _ptr(qual), _ptr(emb)))
        return res, emb, trk, qual

    def runQuality(self, frames, options=None, want_embeds=True, want_crops=False):
        """``run`` that also scores every face slot on the pipeline stream (frt_pipeline_run_quality) -> (records, embeddings or None -
        exactly ``run``'s -, QUALITY_DTYPE [n * max_faces], an unused or empty-ROI slot all zero[, u8 crops [n * max_faces, 112, 112, 3]])."""
        frames = np.ascontiguousarray(frames, np.uint8)
        n = frames.shape[0]
        if frames.shape[1:] != (self.det.frameHeight, self.det.frameWidth, 3):
            raise ValueError("runQuality: frames must be [n, frameHeight, frameWidth, 3]")
        res = np.zeros(n * self.max_faces, RESULT_DTYPE)
        emb = np.zeros((n * self.max_faces, 512), np.float32) if want_embeds else None
        qual = np.zeros(n * self.max_faces, QUALITY_DTYPE)
        crops = np.zeros((n * self.max_faces, 112, 112, 3), np.uint8) if want_crops else None
        _check(lib.frt_pipeline_run_quality(self._h, _ptr(frames), n, _quality_options(options), _ptr(res), _ptr(qual), _ptr(emb), _ptr(crops)))
        return (res, emb, qual, crops) if want_crops else (res, emb, qual)

    def enrolImages(self, classNames, images, labels=None, quality=None, want_quality=False):
        """/insert/face for whole photos: detect, require exactly one face, embed, and append the accepted photos' rows to the live gallery as
        ONE edit, device to device.  ``labels``: one int per image for a labelled gallery.  Returns (status [n] of FRT_ENROL_*, first new
        row index, embeddings [n_enrolled, 512] - exactly the rows added, faces [n] records with the match against the gallery as it was
        before the call).  The recogniser's ``classNames`` / ``classCount`` grow by the accepted names only.
        ``quality`` (a QualityOptions) or ``want_quality`` takes the gated route (frt_pipeline_enrol_images_gated): a photo whose one face
        carries a quality flag comes back FRT_ENROL_LOW_QUALITY and adds no row, and with ``want_quality`` the face's QUALITY_DTYPE record
        [n] is returned as a fifth value."""
        arr, keep = _face_images(images)
        names = list(classNames)
        n = len(keep)
        if len(names) != n:
            raise ValueError("enrolImages: %d names for %d images" % (len(names), n))
        l = None
        if labels is not None:
            l = np.ascontiguousarray(labels, np.int32).reshape(-1)
            if l.size != n:
                raise ValueError("enrolImages: one label per image")
        mm = self.rec.matmul
        if not self._match:  # (refused before the recogniser's matcher is touched)
            raise FrtError(FRT_ERR_INVALID, "enrolImages: the pipeline has no matcher")
        if mm.k == 0:  # never loaded: an empty gallery of this width first
            mm.galleryBegin(0, self.rec.outputDim)
            mm.galleryCommit()
        status = np.zeros(n, np.int32)
        faces = np.zeros(n, RESULT_DTYPE)
        embeds = np.zeros((n, 512), np.float32)
        first, count = _i(0), _i(0)
        qual = np.zeros(n, QUALITY_DTYPE) if want_quality else None
        if quality is not None or want_quality:
            _check(lib.frt_pipeline_enrol_images_gated(self._h, arr, n, _ptr(l), _quality_options(quality), _ptr(status), _ptr(faces), _ptr(qual),
                                                       _ptr(embeds), ctypes.byref(first), ctypes.byref(count)))
        else:
            _check(lib.frt_pipeline_enrol_images(self._h, arr, n, _ptr(l), _ptr(status), _ptr(faces), _ptr(embeds), ctypes.byref(first), ctypes.byref(count)))
        mm._edited()
        self.rec.classNames = list(self.rec.classNames) + [nm for nm, st in zip(names, status) if st == FRT_ENROL_OK]
        self.rec.classCount = len(self.rec.classNames)
        out = (status, first.value, embeds[:count.value].copy(), faces)
        return out + (qual,) if want_quality else out

    def submit(self, frames, results, embeds=None, crops=None):
        """Asynchronous host boundary: queue one batch (``frames`` u8 [n, H, W, 3], ``results`` a RESULT_DTYPE array of
        n*max_faces records, optional ``embeds`` float32 [n*max_faces, 512], optional ``crops`` u8 [n*max_faces, 112, 112, 3] for the
        faces' BGR crops (frt_pipeline_submit_crops); all C-contiguous, ideally pinned) and return a ticket for :meth:`wait`.  The
        arrays must stay alive and untouched until then."""
        if not (frames.flags.c_contiguous and frames.dtype == np.uint8):
            raise ValueError("frames must be a C-contiguous uint8 array")
        n = frames.shape[0]
        if results.dtype != RESULT_DTYPE or results.size < n * self.max_faces or not results.flags.c_contiguous:
            raise ValueError("results must be a C-contiguous RESULT_DTYPE array of n*max_faces records")
        if embeds is not None and (embeds.dtype != np.float32 or embeds.size < n * self.max_faces * 512 or not embeds.flags.c_contiguous):
            raise ValueError("embeds must be a C-contiguous float32 [n*max_faces, 512] array")
        if crops is not None and (crops.dtype != np.uint8 or crops.size < n * self.max_faces * 112 * 112 * 3 or not crops.flags.c_contiguous):
            raise ValueError("crops must be a C-contiguous uint8 [n*max_faces, 112, 112, 3] array")
        t = ctypes.c_long(-1)
        if crops is None:
            _check(lib.frt_pipeline_submit(self._h, _ptr(frames), n, _ptr(results), _ptr(embeds), ctypes.byref(t)))
        else:
            _check(lib.frt_pipeline_submit_crops(self._h, _ptr(frames), n, _ptr(results), _ptr(embeds), _ptr(crops), ctypes.byref(t)))
        return int(t.value)

    def wait(self, ticket):
        _check(lib.frt_pipeline_wait(self._h, int(ticket)))

    def run_dev(self, frames_ptr, n_frames, results_ptr, embeds_ptr=None, ready_event=None):
        """Asynchronous; arguments are raw device addresses (e.g. ``torch.Tensor.data_ptr()``).  ``ready_event``: raw hipEvent_t the
        producer of the frames recorded (``torch.cuda.Event.cuda_event``) - the stages wait for it on the device."""
        if ready_event:
            _check(lib.frt_pipeline_run_dev_after(self._h, _vp(frames_ptr), int(n_frames), _vp(results_ptr), _vp(embeds_ptr) if embeds_ptr else None,
                                                  _vp(ready_event)))
        else:
            _check(lib.frt_pipeline_run_dev(self._h, _vp(frames_ptr), int(n_frames), _vp(results_ptr), _vp(embeds_ptr) if embeds_ptr else None))

    def set_input_sync(self, enable):
        """Safe mode: order every run_dev call behind the work already queued on the pipeline stream (see include/frt.h)."""
        _check(lib.frt_pipeline_set_input_sync(self._h, 1 if enable else 0))

    def check_overlap(self):
        """-> (ratio, warning): ratio ~1 = the stage streams (and the caller's) run side by side, ~n = n of them share a hardware queue;
        warning = the library's message when ratio > 1.5, else ''."""
        r = ctypes.c_float(0)
        _check(lib.frt_pipeline_check_overlap(self._h, ctypes.byref(r)))
        return float(r.value), lib.frt_last_error().decode(errors="replace")

    def sync(self):
        _check(lib.frt_pipeline_sync(self._h))

    def set_overlap(self, enable):
        """Two-stream software pipelining of consecutive calls (detector of call b+1 under embed/match of call b)."""
        _check(lib.frt_pipeline_set_overlap(self._h, 1 if enable else 0))

    def set_graph(self, enable):
        """hipGraph replay of repeated calls (default on)."""
        _check(lib.frt_pipeline_set_graph(self._h, 1 if enable else 0))

    def set_pairing(self, enable):
        """frt_pipeline_set_pairing: -1 (the default) adaptive - submit() calls share a recogniser pass with the next call's only while the
        recogniser is busy anyway; -2 the same for run_dev calls too; 0 / False off; True / 2, 3, 4: always groups of that many consecutive
        calls (results complete when the group is, or at a flush)."""
        _check(lib.frt_pipeline_set_pairing(self._h, int(enable)))

    def merge_stats(self):
        """-> (calls that carried several submit tickets, tickets they carried): adaptive merging at the host boundary."""
        a, b = ctypes.c_long(0), ctypes.c_long(0)
        _check(lib.frt_pipeline_merge_stats(self._h, ctypes.byref(a), ctypes.byref(b)))
        return int(a.value), int(b.value)

    def graph_stats(self):
        """-> (stage graphs captured, stage graphs replayed) since the pipeline was created (set_graph)."""
        a, b = ctypes.c_long(0), ctypes.c_long(0)
        _check(lib.frt_pipeline_graph_stats(self._h, ctypes.byref(a), ctypes.byref(b)))
        return int(a.value), int(b.value)

    def pairing_stats(self):
        """-> (recogniser passes that served two calls, passes that served one)."""
        a, b = ctypes.c_long(0), ctypes.c_long(0)
        _check(lib.frt_pipeline_pairing_stats(self._h, ctypes.byref(a), ctypes.byref(b)))
        return int(a.value), int(b.value)

    def set_align(self, enable):
        """Optional 5-point aligned crop instead of the reference's bbox crop (needs a detector blob with LandmarkHead)."""
        _check(lib.frt_pipeline_set_align(self._h, 1 if enable else 0))

    def set_stream(self, hip_stream):
        """``hip_stream``: raw hipStream_t value (e.g. ``torch.cuda.current_stream().cuda_stream``) or None."""
        _check(lib.frt_pipeline_set_stream(self._h, _vp(hip_stream) if hip_stream else None))

    def close(self):
        if self._h:
            lib.frt_pipeline_destroy(self._h)
            self._h = _vp()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ----------------------------------------------------------------------------------------------------------------------
# JPEG frame ingest / reply step (src/app.cpp:296, 328-340)
# ----------------------------------------------------------------------------------------------------------------------
def jpeg_info(data):
    b = np.frombuffer(bytes(data), np.uint8)
    w, h, c = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
    _check(lib.frt_jpeg_info(_ptr(b), b.size, ctypes.byref(w), ctypes.byref(h), ctypes.byref(c)))
    return w.value, h.value, c.value


def jpeg_read_coefficients(data):
    """Host half of the decoder: -> (geometry dict, coef int16 [total_blocks, 64] natural order, not dequantised)."""
    b = np.frombuffer(bytes(data), np.uint8)
    g = np.zeros(219, np.int32)
    _check(lib.frt_jpeg_read_coefficients(_ptr(b), b.size, None, 0, _ptr(g)))
    coef = np.zeros((int(g[26]), 64), np.int16)
    _check(lib.frt_jpeg_read_coefficients(_ptr(b), b.size, _ptr(coef), coef.shape[0], _ptr(g)))
    comps = [dict(zip(("h", "v", "bw", "bh", "dw", "dh", "block0"), (int(x) for x in g[5 + 7 * i:12 + 7 * i]))) for i in range(int(g[2]))]
    geo = dict(width=int(g[0]), height=int(g[1]), ncomp=int(g[2]), hmax=int(g[3]), vmax=int(g[4]), comps=comps,
               q=[g[27 + 64 * i:27 + 64 * (i + 1)].astype(np.int32).copy() for i in range(int(g[2]))])
    return geo, coef


def jpeg_write_jfif(quality, width, height, coef_zigzag):
    c = np.ascontiguousarray(coef_zigzag, np.int16)
    out = np.zeros(c.size * 3 + 4096, np.uint8)
    n = ctypes.c_size_t(0)
    _check(lib.frt_jpeg_write_jfif(int(quality), int(width), int(height), _ptr(c), _ptr(out), out.size, ctypes.byref(n)))
    return out[:n.value].tobytes()


def base64_encode(data):
    b = np.frombuffer(bytes(data), np.uint8)
    need = lib.frt_base64_encode(_ptr(b) if b.size else None, b.size, None, 0)
    out = ctypes.create_string_buffer(need)
    lib.frt_base64_encode(_ptr(b) if b.size else None, b.size, out, need)
    return out.value.decode()


class JpegCodec:
    """``cv::imdecode`` in front of the hot path and ``cv::imencode('.jpg')`` behind it: Huffman coding on host threads, transforms on the device."""

    def __init__(self, max_images=32, max_width=1920, max_height=1088, n_threads=0, device=0):
        self._h = _vp()
        self.max_images = int(max_images)
        _check(lib.frt_jpeg_decoder_create(self.max_images, int(max_width), int(max_height), int(n_threads), device, ctypes.byref(self._h)))

    def decode(self, data):
        """bytes -> u8 BGR [h, w, 3] at the image's own size."""
        w, h, _ = jpeg_info(data)
        b = np.frombuffer(bytes(data), np.uint8)
        out = np.zeros((h, w, 3), np.uint8)
        _check(lib.frt_jpeg_decode(self._h, _ptr(b), b.size, _ptr(out), out.size, None, None))
        return out

    def decode_batch_dev(self, blobs, frames_ptr, out_h, out_w, hip_stream=None):
        """list of bytes -> device frames [n][out_h][out_w][3] at raw address ``frames_ptr`` (asynchronous on ``hip_stream``)."""
        keep = [np.frombuffer(bytes(b), np.uint8) for b in blobs]
        n = len(keep)
        ptrs = (ctypes.c_void_p * n)(*[k.ctypes.data for k in keep])
        sizes = (ctypes.c_size_t * n)(*[k.size for k in keep])
        _check(lib.frt_jpeg_decode_batch_dev(self._h, ptrs, sizes, n, _vp(frames_ptr), int(out_h), int(out_w), _vp(hip_stream) if hip_stream else None))

    def encode(self, images, quality=95, device_ptr=None, shape=None, ready_event=None):
        """u8 BGR [n, rows, cols, 3] (host array, or raw device address + ``shape``) -> list of JFIF byte strings.  ``ready_event``: raw
        hipEvent_t recorded behind the producer of a device input (the codec's stream waits for it on the device)."""
        if device_ptr is None:
            a = np.ascontiguousarray(images, np.uint8)
            if a.ndim == 3:
                a = a[None]
            n, rows, cols = a.shape[:3]
            src, dev = _ptr(a), 0
        else:
            n, rows, cols = shape
            src, dev = _vp(device_ptr), 1
        stride = rows * cols * 3 + 4096
        out = np.zeros((n, stride), np.uint8)
        sizes = (ctypes.c_size_t * n)()
        _check(lib.frt_jpeg_encode_batch_after(self._h, src, dev, n, rows, cols, int(quality), _ptr(out), stride, sizes,
                                               _vp(ready_event) if ready_event else None))
        return [out[i, :sizes[i]].tobytes() for i in range(n)]

    def close(self):
        if self._h:
            lib.frt_jpeg_decoder_destroy(self._h)
            self._h = _vp()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def profile_enable(kind):
    _check(lib.frt_profile_enable(int(kind)))


def profile_collect(cap=65536):
    names = ctypes.create_string_buffer(cap * 24)
    ms = np.zeros(cap, np.float64)
    work = np.zeros(cap, np.float64)
    n = lib.frt_profile_collect(names, len(names), _ptr(ms), _ptr(work), cap)
    labels = names.value.decode().split("\n")[:n]
    return labels, ms[:n].copy(), work[:n].copy()
