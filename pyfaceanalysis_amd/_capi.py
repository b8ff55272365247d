"""ctypes binding of include/higsfa.h (the drop-in boundary).  No fallback: if the native
library is missing this module raises at first use."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

HG_U8, HG_F32, HG_F64 = 0, 1, 2
HG_OK = 0
HG_ERR_ARG, HG_ERR_FORMAT, HG_ERR_DIM, HG_ERR_DEVICE, HG_ERR_NOMEM, HG_ERR_STATE = -1, -2, -3, -4, -5, -6
HG_PLAN_GENERIC, HG_PLAN_FUSED = 0, 1
HG_FILTER_NEAREST, HG_FILTER_BILINEAR, HG_FILTER_BICUBIC = 0, 2, 3      # enum hg_filter: PIL's own codes (Image.NEAREST / BILINEAR / BICUBIC)
# enum hg_resample: PIL's codes again, but a DIFFERENT operation (Image.resize, not Image.transform): frames.resize, the cascade's prescale
HG_RESAMPLE_NEAREST, HG_RESAMPLE_LANCZOS, HG_RESAMPLE_BILINEAR, HG_RESAMPLE_BICUBIC, HG_RESAMPLE_BOX, HG_RESAMPLE_HAMMING = 0, 1, 2, 3, 4, 5
HG_FRAME_L, HG_FRAME_RGB, HG_FRAME_BGR, HG_FRAME_RGBA, HG_FRAME_BGRA = 0, 1, 2, 3, 4      # frame formats (pyfaceanalysis_amd/frames.py)
HG_MAX_STACK_FRAMES = 1024      # frames in one call of the stack entries (include/higsfa.h)
HG_MAX_STREAM_WINDOWS = 8192    # 9 * n_streams * max_faces of a stream set (include/higsfa.h)

# HIGSFA_LIB: another build of the same library (same-box A/B of two commits, tools/build_ref_lib.sh) — never a different backend
_LIB_PATH = os.environ.get("HIGSFA_LIB") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "libhigsfa.so")
# the only entries an older library selected with HIGSFA_LIB may lack (lib() below): the window filters, the step lanes, the colour frames, the multi-face tracker, the resize, the frame stacks, the stream set, the frame lists, estimation over a frame list
_ENTRIES_SINCE_FILTERS = ("hg_patcher_extract_filter_device", "hg_patcher_extract_filter", "hg_cascade_set_interpolation", "hg_eyes_set_interpolation")
_ENTRIES_SINCE_LANES = ("hg_flow_set_lanes", "hg_flow_lanes", "hg_flow_step_lane_device", "hg_flow_lane_done_event", "hg_flow_lane_join",
                        "hg_flow_check_errors", "hg_lane_stream_id", "hg_event_synchronize")
_ENTRIES_SINCE_COLOR = ("hg_frame_to_gray_device", "hg_frame_to_gray_host", "hg_patcher_extract_format_device", "hg_cascade_set_frame_format")
_ENTRIES_SINCE_MULTI_TRACKING = ("hg_cascade_tracked_grid_multi_device", "hg_tracker_create_multi", "hg_tracker_step_frame_multi_device")
_ENTRIES_SINCE_RESIZE = ("hg_frame_resize_host", "hg_patcher_resize_device", "hg_cascade_set_prescale_filter")
_ENTRIES_SINCE_NORMALIZE = ("hg_normalize_geometry_host", "hg_normalize_faces_host", "hg_patcher_normalize_device")
_ENTRIES_SINCE_ESTIMATION = ("hg_estimator_create", "hg_estimator_free", "hg_estimator_patches_device", "hg_estimator_estimate_device")
_ENTRIES_SINCE_FRAME_STACKS = ("hg_patcher_extract_frames_device", "hg_cascade_detect_frames_device", "hg_cascade_detect_faces_frames_device")
_ENTRIES_SINCE_ESTIMATE_FRAMES = ("hg_patcher_normalize_frames_device", "hg_estimator_estimate_frames_device")
_ENTRIES_SINCE_STREAM_SET = ("hg_stream_tracker_create", "hg_stream_tracker_free", "hg_stream_tracker_reset", "hg_stream_tracker_step_frames_device",
                             "hg_cascade_tracked_grid_streams_device")
_ENTRIES_SINCE_FRAME_LISTS = ("hg_patcher_extract_frame_list_device", "hg_cascade_detect_frame_list_device", "hg_cascade_detect_faces_frame_list_device")
_ENTRIES_SINCE_ESTIMATE_FRAME_LIST = ("hg_patcher_normalize_frame_list_device", "hg_estimator_estimate_frame_list_device")
_lib = None


class HgInfo(C.Structure):
    _fields_ = [("input_dim", C.c_int64), ("output_dim", C.c_int64), ("n_top_nodes", C.c_int32),
                ("plan_kind", C.c_int32), ("n_stages", C.c_int32), ("device", C.c_int32),
                ("weight_bytes", C.c_int64), ("flops_per_row", C.c_int64),
                ("padded_flops_per_row", C.c_int64), ("workspace_bytes", C.c_int64)]


class HgCascadeConsts(C.Structure):
    _fields_ = [(n, C.c_double) for n in (
        "regression_width", "regression_height", "desired_sampling", "tolerance_posxy_deviation", "tolerance_scale_deviation",
        "tolerance_angle_deviation", "max_scale_radio", "min_scale_radio", "net_Dang", "cut_off_face")]


class HgCascadeLevel(C.Structure):      # hg_cascade_level: one pyramid level of the first-stage grid (face_analysis.py:630-652)
    _fields_ = [("nx", C.c_int32), ("ny", C.c_int32)] + [(n, C.c_double) for n in ("x_stop", "y_stop", "patch_w", "patch_h", "max_dx", "max_dy", "base_side")]


class HgFrameRef(C.Structure):          # hg_frame_ref: one grey frame of a list (hg_patcher_extract_frame_list_device)
    _fields_ = [("frame_dev", C.c_void_p), ("frame_h", C.c_int32), ("frame_w", C.c_int32), ("ld", C.c_int64)]


class HgCascadeFrame(C.Structure):      # hg_cascade_frame: one frame of a list with its prescaled size and level table
    _fields_ = [("frame_dev", C.c_void_p), ("frame_h", C.c_int32), ("frame_w", C.c_int32), ("ld", C.c_int64), ("prescale_w", C.c_int32),
                ("prescale_h", C.c_int32), ("levels", C.POINTER(HgCascadeLevel)), ("n_levels", C.c_int32)]


class HgCascadeStage(C.Structure):
    _fields_ = [("type", C.c_int32), ("serial", C.c_int32), ("flow", C.c_void_p), ("classifier", C.c_void_p)]


class HgEyeConsts(C.Structure):         # hg_eye_consts (include/higsfa.h)
    _fields_ = [(n, C.c_double) for n in ("eye_regression_width", "eye_regression_height", "face_sampling", "eye_sampling", "tolerance",
                                          "target_mean", "target_std")] + [(n, C.c_int32) for n in ("eye_w", "eye_h", "n_features", "reserved")]


class HgTrackedConsts(C.Structure):     # hg_tracked_consts (include/higsfa.h)
    _fields_ = [(n, C.c_double) for n in ("subimage_width", "subimage_height", "regression_width", "regression_height", "net_Dx", "net_Dy")]


class HgNormConsts(C.Structure):        # hg_norm_consts (include/higsfa.h)
    _fields_ = [(n, C.c_int32) for n in ("out_w", "out_h", "method", "rotate")]


class HgEstimatorConsts(C.Structure):   # hg_estimator_consts (include/higsfa.h)
    _fields_ = ([(n, C.c_int32) for n in ("crop_w", "crop_h", "method", "rotate", "patch_w", "patch_h", "filter", "clip")] + [("box", C.c_double * 4)] +
                [(n, C.c_double) for n in ("target_mean", "target_std")] + [(n, C.c_int32) for n in ("n_features", "reserved")])


# hg_norm_geom as a numpy record (include/higsfa.h): 144 bytes, no padding
NORM_GEOM_DTYPE = np.dtype([("crop_x0", np.int32), ("crop_y0", np.int32), ("W", np.int32), ("H", np.int32), ("angle", np.float64),
                            ("shift", np.float64, (2,)), ("m", np.float64, (6,)), ("box", np.float64, (4,)), ("rotated", np.int32),
                            ("status", np.int32), ("rect", np.int32, (4,))])
HG_NORM_AREA, HG_NORM_AREAZ = 0, 1

HG_STAGE = {"Disc": 0, "PosX": 1, "PosY": 2, "PAng": 3, "Scale": 4}


class NativeLibraryMissing(ImportError):
    pass


def lib():
    """Load libhigsfa.so (built by ``python -m pyfaceanalysis_amd.build``).

    Load order with PyTorch: the torch wheel bundles its own ROCm runtime (torch/lib/libamdhip64.so, librocblas.so,
    librocsolver.so); loaded first, it is the one runtime everything binds to.  The other way round the system
    runtime owns the GPU and a later ``import torch`` reports "No HIP GPUs are available".  So when torch is installed
    it is imported here, before the library (HIGSFA_NO_TORCH=1 skips this for torch-free processes)."""
    global _lib
    if _lib is not None:
        return _lib
    import sys
    if "torch" not in sys.modules and not os.environ.get("HIGSFA_NO_TORCH"):
        import importlib.util
        if importlib.util.find_spec("torch") is not None:
            import torch  # noqa: F401
    if not os.path.exists(_LIB_PATH):
        raise NativeLibraryMissing(
            "%s not found: the HIP library is the only execution path of this package; build it "
            "with `python -m pyfaceanalysis_amd.build` (or __graft_entry__.build())" % _LIB_PATH)
    L = C.CDLL(_LIB_PATH)
    vp, i64, i32, sz = C.c_void_p, C.c_int64, C.c_int, C.c_size_t
    sigs = {
        "hg_version": (C.c_int, []),
        "hg_last_error": (C.c_char_p, []),
        "hg_device_count": (C.c_int, [C.POINTER(C.c_int)]),
        "hg_flow_load": (C.c_int, [vp, sz, i32, C.POINTER(vp)]),
        "hg_flow_free": (None, [vp]),
        "hg_flow_info": (C.c_int, [vp, C.POINTER(HgInfo)]),
        "hg_flow_describe": (C.c_int, [vp, C.c_char_p, sz, C.POINTER(sz)]),
        "hg_flow_to_device": (C.c_int, [vp, i32]),
        "hg_flow_reserve": (C.c_int, [vp, i64]),
        "hg_flow_execute": (C.c_int, [vp, vp, i32, i64, i64, vp, i32, i64, i64]),
        "hg_flow_execute_sharded": (C.c_int, [vp, vp, i32, i64, i64, vp, i32, i64, i64, C.POINTER(C.c_int), i32]),
        "hg_flow_execute_device": (C.c_int, [vp, vp, i32, i64, i64, vp, i32, i64, i64, vp]),
        "hg_flow_set_lanes": (C.c_int, [vp, i32]),
        "hg_flow_lanes": (C.c_int, [vp, C.POINTER(C.c_int)]),
        "hg_flow_step_lane_device": (C.c_int, [vp, i32, vp, i32, i64, i64, vp, i32, i64, i64, vp]),
        "hg_flow_lane_done_event": (C.c_int, [vp, i32, C.POINTER(vp)]),
        "hg_flow_lane_join": (C.c_int, [vp, i32, vp]),
        "hg_flow_check_errors": (C.c_int, [vp]),
        "hg_lane_stream_id": (C.c_int, [i32, i32, C.POINTER(C.c_uint64)]),
        "hg_event_create": (C.c_int, [C.POINTER(vp)]),
        "hg_event_create_on": (C.c_int, [C.POINTER(vp), C.c_int, C.c_int]),
        "hg_event_destroy": (None, [vp]),
        "hg_event_record": (C.c_int, [vp, vp]),
        "hg_stream_wait_event": (C.c_int, [vp, vp]),
        "hg_event_query": (C.c_int, [vp]),
        "hg_event_synchronize": (C.c_int, [vp]),
        "hg_flow_host_transport": (C.c_int, [vp, C.POINTER(C.c_int)]),
        "hg_host_pack_probe": (C.c_int, [vp, i32, i64, i64, i64, i32, C.POINTER(C.c_double)]),
        "hg_host_store_probe": (C.c_int, [i32, sz, i32, C.POINTER(C.c_double), C.POINTER(C.c_int)]),
        "hg_host_dma_probe": (C.c_int, [i32, sz, i32, C.POINTER(C.c_double)]),
        "hg_flow_set_profiling": (C.c_int, [vp, i32]),
        "hg_flow_stage_times": (C.c_int, [vp, C.POINTER(C.c_double), C.POINTER(i64), i32, C.POINTER(i32)]),
        "hg_flow_stage_name": (C.c_int, [vp, i32, C.c_char_p, sz]),
        "hg_flow_reset_profile": (C.c_int, [vp]),
        "hg_gauss_create": (C.c_int, [C.c_int32, C.c_int32, vp, vp, vp, vp, vp, i32, C.POINTER(vp)]),
        "hg_gauss_free": (None, [vp]),
        "hg_gauss_regression_device": (C.c_int, [vp, vp, i32, i64, i64, vp, vp, vp]),
        "hg_gauss_regression": (C.c_int, [vp, vp, i32, i64, i64, vp, vp]),
        "hg_gauss_regression_multi_device": (C.c_int, [C.POINTER(vp), i32, vp, i32, i64, i64, vp, i64, vp]),
        "hg_patcher_create": (C.c_int, [i32, C.POINTER(vp)]),
        "hg_patcher_free": (None, [vp]),
        "hg_patcher_extract_device": (C.c_int, [vp, vp, i32, i32, i32, i64, vp, i64, i32, i32, vp, i32, i64, vp]),
        "hg_patcher_extract_keyed_device": (C.c_int, [vp, C.c_uint64, vp, i32, i32, i32, i64, vp, i64, i32, i32, vp, i32, i64, vp]),
        "hg_patcher_extract": (C.c_int, [vp, vp, i32, i32, i32, i64, vp, i64, i32, i32, vp, i32, i64]),
        "hg_patcher_extract_rotate_device": (C.c_int, [vp, vp, i32, i32, i32, i64, vp, vp, i64, i32, i32, vp, i32, i64, vp]),
        "hg_patcher_extract_rotate": (C.c_int, [vp, vp, i32, i32, i32, i64, vp, vp, i64, i32, i32, vp, i32, i64]),
        "hg_patcher_extract_filter_device": (C.c_int, [vp, i32, vp, i32, i32, i32, i64, vp, vp, i64, i32, i32, vp, i32, i64, vp]),
        "hg_patcher_extract_filter": (C.c_int, [vp, i32, vp, i32, i32, i32, i64, vp, vp, i64, i32, i32, vp, i32, i64]),
        "hg_cascade_set_interpolation": (C.c_int, [vp, vp, i32]),
        "hg_frame_to_gray_device": (C.c_int, [i32, vp, i32, i32, i32, i64, vp, i64, vp]),
        "hg_frame_to_gray_host": (C.c_int, [vp, i32, i32, i32, i64, vp, i64]),
        "hg_patcher_extract_format_device": (C.c_int, [vp, i32, vp, i32, i32, i64, vp, i64, i32, i32, vp, i32, i64, vp]),
        "hg_cascade_set_frame_format": (C.c_int, [vp, i32]),
        "hg_frame_resize_host": (C.c_int, [i32, vp, i32, i32, i32, i64, i32, vp, i32, i32, i64]),
        "hg_patcher_resize_device": (C.c_int, [vp, i32, i32, vp, i32, i32, i32, i64, i32, vp, i32, i32, i64, vp]),
        "hg_cascade_set_prescale_filter": (C.c_int, [vp, i32]),
        "hg_normalize_geometry_host": (C.c_int, [vp, i64, i32, i32, C.POINTER(HgNormConsts), vp]),
        "hg_normalize_faces_host": (C.c_int, [vp, i32, i32, i64, vp, i64, i32, i32, vp, i64]),
        "hg_patcher_normalize_device": (C.c_int, [vp, i32, vp, i32, i32, i64, vp, i64, i32, i32, vp, i64, vp]),
        "hg_eyes_set_interpolation": (C.c_int, [vp, i32]),
        "hg_estimator_create": (C.c_int, [vp, vp, vp, vp, C.POINTER(HgEstimatorConsts), vp, i32, C.POINTER(vp)]),
        "hg_estimator_free": (None, [vp]),
        "hg_estimator_patches_device": (C.c_int, [vp, i32, vp, i64, i64, vp, i64, vp]),
        "hg_estimator_estimate_device": (C.c_int, [vp, i32, vp, i32, i32, i64, vp, i64, vp, i64, vp, vp, vp]),
        "hg_patcher_normalize_frames_device": (C.c_int, [vp, i32, vp, i32, i64, i32, i32, i64, vp, vp, i64, i32, i32, vp, i64, vp]),
        "hg_estimator_estimate_frames_device": (C.c_int, [vp, i32, vp, i32, i64, i32, i32, i64, vp, vp, i64, vp, i64, vp, vp, vp]),
        "hg_patcher_normalize_frame_list_device": (C.c_int, [vp, i32, C.POINTER(HgFrameRef), i32, vp, vp, i64, i32, i32, vp, i64, vp]),
        "hg_estimator_estimate_frame_list_device": (C.c_int, [vp, i32, C.POINTER(HgFrameRef), i32, vp, vp, i64, vp, i64, vp, vp, vp]),
        "hg_cascade_update_device": (C.c_int, [i32, i32, C.POINTER(HgCascadeConsts), i64, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
        "hg_cascade_compact_device": (C.c_int, [i32, vp, i64, vp, vp, vp]),
        "hg_gather_rows_device": (C.c_int, [i32, vp, vp, i64, vp, vp, i64, vp]),
        "hg_cascade_create": (C.c_int, [C.POINTER(HgCascadeStage), i32, i32, i32, i32, C.POINTER(HgCascadeConsts), vp, i32, i32, C.POINTER(vp)]),
        "hg_cascade_free": (None, [vp]),
        "hg_cascade_detect_device": (C.c_int, [vp, vp, i32, i32, i64, vp, vp, i64, vp, vp, vp, vp, i64, C.POINTER(i64), vp, C.POINTER(i64), vp]),
        "hg_cascade_detect_levels_device": (C.c_int, [vp, vp, i32, i32, i64, C.POINTER(HgCascadeLevel), i32, vp, vp, vp, vp, i64, C.POINTER(i64), vp, C.POINTER(i64), vp]),
        "hg_cascade_detect_frame_device": (C.c_int, [vp, vp, i32, i32, i64, i32, i32, C.POINTER(HgCascadeLevel), i32, vp, vp, vp, vp, i64, C.POINTER(i64), vp, C.POINTER(i64), vp]),
        "hg_cascade_grid_device": (C.c_int, [i32, C.POINTER(HgCascadeLevel), i32, vp, vp, i64, C.POINTER(i64), vp]),
        "hg_eyes_create": (C.c_int, [vp, vp, vp, vp, C.POINTER(HgEyeConsts), i32, C.POINTER(vp)]),
        "hg_eyes_free": (None, [vp]),
        "hg_eyes_locate_device": (C.c_int, [vp, vp, i32, i32, i64, vp, vp, i64, vp, vp, vp, vp, vp]),
        "hg_eyes_boxes_device": (C.c_int, [vp, vp, vp, i64, vp, vp, vp]),
        "hg_purge_detections_device": (C.c_int, [i32, vp, i64, vp, vp, vp]),
        "hg_cascade_detect_faces_frame_device": (C.c_int, [vp, vp, vp, i32, i32, i64, i32, i32, C.POINTER(HgCascadeLevel), i32, vp, i64, C.POINTER(i64),
                                                           C.POINTER(i64), vp, C.POINTER(i64), vp]),
        "hg_patcher_extract_frames_device": (C.c_int, [vp, i32, vp, i32, i64, i32, i32, i64, vp, vp, vp, i64, i32, i32, vp, i32, i64, vp]),
        "hg_cascade_detect_frames_device": (C.c_int, [vp, vp, i32, i64, i32, i32, i64, i32, i32, C.POINTER(HgCascadeLevel), i32, vp, vp, vp, vp, i64, vp, vp,
                                                      C.POINTER(i64), vp]),
        "hg_cascade_detect_faces_frames_device": (C.c_int, [vp, vp, vp, i32, i64, i32, i32, i64, i32, i32, C.POINTER(HgCascadeLevel), i32, vp, i64, vp, vp, vp,
                                                            C.POINTER(i64), vp]),
        "hg_patcher_extract_frame_list_device": (C.c_int, [vp, i32, C.POINTER(HgFrameRef), i32, vp, vp, vp, i64, i32, i32, vp, i32, i64, vp]),
        "hg_cascade_detect_frame_list_device": (C.c_int, [vp, C.POINTER(HgCascadeFrame), i32, vp, vp, vp, vp, i64, vp, vp, C.POINTER(i64), vp]),
        "hg_cascade_detect_faces_frame_list_device": (C.c_int, [vp, vp, C.POINTER(HgCascadeFrame), i32, vp, i64, vp, vp, vp, C.POINTER(i64), vp]),
        "hg_cascade_tracked_grid_device": (C.c_int, [i32, C.POINTER(HgTrackedConsts), vp, vp, vp, vp]),
        "hg_tracker_create": (C.c_int, [vp, vp, C.POINTER(HgTrackedConsts), C.POINTER(vp)]),
        "hg_tracker_free": (None, [vp]),
        "hg_tracker_reset": (C.c_int, [vp]),
        "hg_tracker_step_frame_device": (C.c_int, [vp, vp, i32, i32, i64, i32, i32, C.POINTER(HgCascadeLevel), i32, vp, i64, C.POINTER(i64),
                                                   C.POINTER(i64), vp, C.POINTER(i64), C.POINTER(C.c_int), vp]),
        "hg_cascade_tracked_grid_multi_device": (C.c_int, [i32, C.POINTER(HgTrackedConsts), vp, i32, vp, vp, vp]),
        "hg_tracker_create_multi": (C.c_int, [vp, vp, C.POINTER(HgTrackedConsts), i32, i32, C.POINTER(vp)]),
        "hg_tracker_step_frame_multi_device": (C.c_int, [vp, vp, i32, i32, i64, i32, i32, C.POINTER(HgCascadeLevel), i32, vp, i64, C.POINTER(i64),
                                                         C.POINTER(i64), vp, C.POINTER(i64), C.POINTER(C.c_int), vp, C.POINTER(C.c_int), vp]),
        "hg_stream_tracker_create": (C.c_int, [vp, vp, C.POINTER(HgTrackedConsts), i32, i32, i32, C.POINTER(vp)]),
        "hg_stream_tracker_free": (None, [vp]),
        "hg_stream_tracker_reset": (C.c_int, [vp, i32]),
        "hg_stream_tracker_step_frames_device": (C.c_int, [vp, vp, i32, i64, i32, i32, i64, i32, i32, C.POINTER(HgCascadeLevel), i32, vp, i64, vp, vp, vp, vp, vp,
                                                           C.POINTER(i64), vp]),
        "hg_cascade_tracked_grid_streams_device": (C.c_int, [i32, C.POINTER(HgTrackedConsts), vp, vp, i32, i32, vp, vp, vp]),
        "hg_sfa_train_layer": (C.c_int, [vp, i32, i32, i64, i64, vp, C.c_int32, C.c_int32, i32, vp, vp, vp, vp]),
        "hg_pca_train_layer": (C.c_int, [vp, i32, i32, i64, i64, vp, C.c_int32, C.c_int32, i32, vp, vp, vp, vp]),
        "hg_train_apply_device": (C.c_int, [vp, i32, i64, i64, vp, C.c_int32, C.c_int32, vp, vp, C.c_int32, C.c_int32, vp, vp, vp, i64, i32]),
    }
    for name, (res, args) in sigs.items():
        try:
            fn = getattr(L, name)
        except AttributeError:
            # an A/B run on the library of an older commit (HIGSFA_LIB, tools/build_ref_lib.sh) may lack the newest entries, and only
            # those: calling one raises AttributeError there; any other missing symbol is a broken build and fails here
            if name in (_ENTRIES_SINCE_FILTERS + _ENTRIES_SINCE_LANES + _ENTRIES_SINCE_COLOR + _ENTRIES_SINCE_MULTI_TRACKING + _ENTRIES_SINCE_RESIZE +
                        _ENTRIES_SINCE_NORMALIZE + _ENTRIES_SINCE_ESTIMATION + _ENTRIES_SINCE_FRAME_STACKS +
                        _ENTRIES_SINCE_ESTIMATE_FRAMES + _ENTRIES_SINCE_STREAM_SET + _ENTRIES_SINCE_FRAME_LISTS +
                        _ENTRIES_SINCE_ESTIMATE_FRAME_LIST) and os.environ.get("HIGSFA_LIB"):
                continue
            raise
        fn.restype = res
        fn.argtypes = args
    _lib = L
    return L


EXPORTED_SYMBOLS = (
    "hg_version", "hg_last_error", "hg_device_count", "hg_flow_load", "hg_flow_free", "hg_flow_info",
    "hg_flow_describe", "hg_flow_to_device", "hg_flow_reserve", "hg_flow_execute", "hg_flow_execute_sharded",
    "hg_flow_execute_device", "hg_event_create", "hg_event_create_on", "hg_event_destroy", "hg_event_record", "hg_stream_wait_event", "hg_event_query", "hg_flow_host_transport", "hg_host_pack_probe", "hg_host_store_probe", "hg_host_dma_probe", "hg_flow_set_profiling", "hg_flow_stage_times", "hg_flow_stage_name",
    "hg_flow_reset_profile", "hg_gauss_create", "hg_gauss_free", "hg_gauss_regression_device",
    "hg_gauss_regression", "hg_patcher_create", "hg_patcher_free", "hg_patcher_extract_device",
    "hg_patcher_extract_keyed_device", "hg_patcher_extract", "hg_patcher_extract_rotate_device", "hg_patcher_extract_rotate", "hg_cascade_update_device",
    "hg_cascade_compact_device", "hg_gather_rows_device", "hg_cascade_create", "hg_cascade_free", "hg_cascade_detect_device",
    "hg_cascade_detect_levels_device", "hg_cascade_detect_frame_device", "hg_cascade_grid_device", "hg_gauss_regression_multi_device",
    "hg_sfa_train_layer", "hg_pca_train_layer", "hg_train_apply_device",
    "hg_eyes_create", "hg_eyes_free", "hg_eyes_locate_device", "hg_eyes_boxes_device", "hg_purge_detections_device", "hg_cascade_detect_faces_frame_device",
    "hg_cascade_tracked_grid_device", "hg_tracker_create", "hg_tracker_free", "hg_tracker_reset", "hg_tracker_step_frame_device",
    "hg_patcher_extract_filter_device", "hg_patcher_extract_filter", "hg_cascade_set_interpolation", "hg_eyes_set_interpolation",
    "hg_flow_set_lanes", "hg_flow_lanes", "hg_flow_step_lane_device", "hg_flow_lane_done_event", "hg_flow_lane_join", "hg_flow_check_errors",
    "hg_lane_stream_id", "hg_event_synchronize",
    "hg_frame_to_gray_device", "hg_frame_to_gray_host", "hg_patcher_extract_format_device", "hg_cascade_set_frame_format",
    "hg_cascade_tracked_grid_multi_device", "hg_tracker_create_multi", "hg_tracker_step_frame_multi_device",
    "hg_frame_resize_host", "hg_patcher_resize_device", "hg_cascade_set_prescale_filter",
    "hg_normalize_geometry_host", "hg_normalize_faces_host", "hg_patcher_normalize_device",
    "hg_estimator_create", "hg_estimator_free", "hg_estimator_patches_device", "hg_estimator_estimate_device",
    "hg_patcher_extract_frames_device", "hg_cascade_detect_frames_device", "hg_cascade_detect_faces_frames_device",
    "hg_patcher_normalize_frames_device", "hg_estimator_estimate_frames_device",
    "hg_stream_tracker_create", "hg_stream_tracker_free", "hg_stream_tracker_reset", "hg_stream_tracker_step_frames_device",
    "hg_cascade_tracked_grid_streams_device",
    "hg_patcher_extract_frame_list_device", "hg_cascade_detect_frame_list_device", "hg_cascade_detect_faces_frame_list_device",
    "hg_patcher_normalize_frame_list_device", "hg_estimator_estimate_frame_list_device",
)

_EXC = {HG_ERR_ARG: ValueError, HG_ERR_FORMAT: ValueError, HG_ERR_DIM: ValueError,
        HG_ERR_DEVICE: RuntimeError, HG_ERR_NOMEM: MemoryError, HG_ERR_STATE: RuntimeError}


class NodeException(ValueError):
    """Counterpart of mdp.NodeException (dimension mismatches raise this in MDP)."""


def check(rc):
    if rc == HG_OK:
        return
    msg = lib().hg_last_error().decode("utf-8", "replace")
    if rc == HG_ERR_DIM:
        raise NodeException(msg)
    raise _EXC.get(rc, RuntimeError)("higsfa: " + msg)


def filter_code(f):
    """An interpolation filter as enum hg_filter; PIL's Image.NEAREST / BILINEAR / BICUBIC (ints or IntEnum members) pass straight through."""
    try:
        code = int(f)
    except (TypeError, ValueError):
        code = None
    if code not in (HG_FILTER_NEAREST, HG_FILTER_BILINEAR, HG_FILTER_BICUBIC) or isinstance(f, (bool, float)):
        raise ValueError("unknown interpolation filter %r (0 NEAREST, 2 BILINEAR, 3 BICUBIC)" % (f,))
    return code


def np_dtype_code(dt):
    dt = np.dtype(dt)
    if dt == np.uint8:
        return HG_U8
    if dt == np.float32:
        return HG_F32
    if dt == np.float64:
        return HG_F64
    return None
