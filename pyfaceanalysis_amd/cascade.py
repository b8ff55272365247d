"""The detection cascade around the hot call, resident on one GPU (BASELINE.json configs[2]).

The reference runs, per image, per pyramid level and per cascade stage (FaceDetectUpdated.py:592-766):

    subimages_arr = load_network_subimages(...)                      :686   extract (PIL, host)
    sl = networks[k].execute(subimages_arr, benchmark=benchmark)     :699   THE HOT CALL
    reg_out = classifiers[k].regression(sl[:, 0:d], avg_labels)      :719
    update_current_subimage_coordinates / identify_patches_to_discard :728-735 (face_analysis.py:803-887)
    boolean-mask compaction of every per-candidate array              :739-759

``DeviceCascade`` runs the same loop inside the library (``hg_cascade_detect_device``, include/higsfa.h: rotated window
extraction -> ``hg_flow_execute_device`` -> Gaussian regression -> one fused update / discard / compaction kernel per stage)
on one stream: no per-candidate array ever visits the host; the host reads one integer after each Disc stage (the survivor
count, which shrinks a lot there and sizes the next launches).  All pyramid levels run as ONE batch of candidates, as the
reference's author notes is possible (:599), each candidate carrying its level's constants.  torch is used for the frame
tensor and the stream only.  (The single steps are also exported one by one — ``hg_cascade_update_device``,
``hg_cascade_compact_device``, ``hg_gather_rows_device`` — for callers that drive the loop themselves.)

Stages follow the pipeline grammar (face_analysis.py:437-443): a type with a serial digit ("Disc1", "PosX0", ...), a flow
or None (the stage reuses the previous features, :680-682), a classifier.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import _capi, frames, grid
from .patches import Patcher

CUT_OFFS_FACE = [0.99, 0.95, 0.85, 0.8, 0.7, 0.6, 0.5, 0.45, 0.10, 0.05]      # FaceDetectUpdated.py:98
TOLERANCE_SCALE = TOLERANCE_ANGLE = TOLERANCE_POSXY = 1.1                     # FaceDetectUpdated.py:113-115
DESIRED_SAMPLING = 0.825                                                      # FaceDetectUpdated.py:729


class Stage(object):
    def __init__(self, name, flow, classifier):
        self.name = name
        self.type, self.serial = name[:-1], int(name[-1])
        if self.type not in _capi.HG_STAGE:
            raise ValueError("unknown stage type %r" % name)
        self.flow, self.classifier = flow, classifier


def frame_windows(im_width, im_height, smallest_face, pipeline, subimage_size):
    """All first-stage windows of a frame (grid.frame_boxes) with, per window, the constants of its pyramid level:
    (max_Dx_diff, max_Dy_diff, base_side) — face_analysis.py:651-652, FaceDetectUpdated.py:604-605."""
    p = dict(pipeline)
    p["subimage_width"], p["subimage_height"] = subimage_size
    boxes, level = [], []
    for s, b in grid.frame_boxes(im_width, im_height, smallest_face, pipeline=p):
        pw, ph = p["subimage_width"] * s, p["subimage_height"] * s
        boxes.append(b)
        level.append(np.tile([p["net_Dx"] * pw / p["regression_width"], p["net_Dy"] * ph / p["regression_height"],
                              math.sqrt(pw ** 2 + ph ** 2)], (len(b), 1)))
    return np.concatenate(boxes), np.concatenate(level)


def frame_levels(im_width, im_height, smallest_face, pipeline, subimage_size):
    """The same grid as a table of pyramid levels (``_capi.HgCascadeLevel``) for ``hg_cascade_detect_levels_device``, which
    computes the windows on the device: per level the grid counts and linspace end points of face_analysis.py:640-646, the patch
    size (:630-631) and the level constants (:651-652).  ``frame_windows`` of the same arguments is what the device produces,
    bit for bit (tests/test_cascade.py)."""
    p = dict(pipeline)
    p["subimage_width"], p["subimage_height"] = subimage_size
    svals = grid.sampling_values(im_width, im_height, p["subimage_width"], p["subimage_height"], smallest_face, p["net_mins"], p["net_maxs"])
    arr = (_capi.HgCascadeLevel * max(len(svals), 1))()
    for i, s in enumerate(svals):
        pw, ph = p["subimage_width"] * s, p["subimage_height"] * s
        sep_x = p["net_Dx"] * 2.0 * pw / p["regression_width"]
        sep_y = p["net_Dy"] * 2.0 * ph / p["regression_height"]
        arr[i].nx = int(math.ceil((1 + (im_width - pw) / sep_x) * grid.PATCH_OVERLAP_POSX_POSY))
        arr[i].ny = int(math.ceil((1 + (im_height - ph) / sep_y) * grid.PATCH_OVERLAP_POSX_POSY))
        arr[i].x_stop, arr[i].y_stop = im_width - pw, im_height - ph
        arr[i].patch_w, arr[i].patch_h = pw, ph
        arr[i].max_dx = p["net_Dx"] * pw / p["regression_width"]
        arr[i].max_dy = p["net_Dy"] * ph / p["regression_height"]
        arr[i].base_side = math.sqrt(pw ** 2 + ph ** 2)
    return arr, len(svals), sum(arr[i].nx * arr[i].ny for i in range(len(svals)))


def tracked_windows(box, pipeline, subimage_size):
    """The nine windows of a frame that follows a found face (grid.tracked_boxes; the reference's ``track_single_face`` branch)
    with, per window, (max_Dx_diff, max_Dy_diff, base_side) — the layout ``frame_windows`` returns.  ``box``: (x0, y0, x1, y1) of the
    previous frame's first purged detection, in the coordinates of the prescaled frame.  What k_cascade_init_tracked writes on the
    device, bit for bit (tests/test_tracking_gpu.py).  A (K, 4) array of boxes gives the concatenation of the per-box results, (9 K, 4)
    and (9 K, 3): window 9 s + i is window i of box s, what k_cascade_init_tracked_multi writes (tests/test_multi_tracking_gpu.py)."""
    if np.ndim(box) == 2:
        parts = [tracked_windows(b, pipeline, subimage_size) for b in np.asarray(box, dtype=np.float64)]
        if not parts:
            return np.zeros((0, 4)), np.zeros((0, 3))
        return np.concatenate([b for b, _ in parts]), np.concatenate([lv for _, lv in parts])
    p = dict(pipeline)
    sw, sh = subimage_size
    _, _, pw, ph, max_dx, max_dy = grid.tracked_positions(box, sw, sh, p["regression_width"], p["regression_height"], p["net_Dx"], p["net_Dy"])
    boxes = grid.tracked_boxes(box, sw, sh, p["regression_width"], p["regression_height"], p["net_Dx"], p["net_Dy"])
    return boxes, np.tile([max_dx, max_dy, math.sqrt(pw ** 2 + ph ** 2)], (9, 1))


class DeviceCascade(object):
    def __init__(self, stages, subimage_size, n_features, pipeline=None, device=0, interpolation_formats=None, frame_format="L",
                 prescale_filter="NEAREST"):
        """interpolation_formats: the filter of every stage's extraction, a sequence indexed by the stage's serial like
        ``CUT_OFFS_FACE`` (FaceDetectUpdated.py:125, :671; PIL's codes 0 / 2 / 3); None: NEAREST everywhere.  The prescale is
        not a stage: prescale_filter (``frames.RESAMPLE``: a name or PIL's code) is the filter of ``Image.resize`` in front of every
        frame path — ``detect_frame``, ``detect_faces``, ``prescale`` and a ``FaceTracker`` on this cascade; "NEAREST" is the
        reference's (:551-561), the others are PIL's antialiased resize of the grey frame, bit for bit.  frame_format: the format of the frames ``detect``, ``detect_frame``, ``detect_faces``
        and ``prescale`` are given ("L", "RGB", "BGR", "RGBA", "BGRA": frames.py); a colour frame is converted as PIL's
        ``convert("L")`` does (:541-543) inside the library, and everything behind that reads the grey frame."""
        import torch
        self.torch = torch
        self.frame_format = frames.format_code(frame_format)
        self.prescale_filter = frames.resample_code(prescale_filter)
        self.stages = list(stages)
        self.w, self.h = int(subimage_size[0]), int(subimage_size[1])
        self.k = int(n_features)              # feature columns kept per candidate (>= every classifier's input_dim)
        self.pipeline = dict(grid.FACE_PIPELINE if pipeline is None else pipeline)
        self.device = int(device)
        self.dev = torch.device("cuda", self.device)
        self.patcher = Patcher(self.device)
        self._h = None
        self._levels = {}        # (frame size, smallest_face) -> level table (frame_levels)
        self._prescale = {}      # (frame size, prescaled size) -> (box tensor, output tensor) of the prescale step
        self._frames = {}        # (frame size, smallest_face, prescale size) -> everything detect_frame needs per call
        self._list_bufs = {}     # kind of list call -> (rows, output buffers): one set, grown on demand (_list_plan)
        self._list_pre = None    # the byte buffer of prescale_frame_list's outputs, grown on demand
        for st in self.stages:
            if st.classifier.input_dim > self.k:
                raise ValueError("stage %s: classifier reads %d features, cascade keeps %d" % (st.name, st.classifier.input_dim, self.k))
        self.interpolation_formats = None
        if interpolation_formats is not None:
            self.interpolation_formats = [_capi.filter_code(f) for f in interpolation_formats]
            for st in self.stages:
                if st.serial >= len(self.interpolation_formats):
                    raise ValueError("stage %s: interpolation_formats has %d entries" % (st.name, len(self.interpolation_formats)))

    def _consts(self):
        p = self.pipeline
        c = _capi.HgCascadeConsts()
        c.regression_width, c.regression_height = p["regression_width"], p["regression_height"]
        c.desired_sampling = DESIRED_SAMPLING
        c.tolerance_posxy_deviation, c.tolerance_scale_deviation, c.tolerance_angle_deviation = TOLERANCE_POSXY, TOLERANCE_SCALE, TOLERANCE_ANGLE
        c.max_scale_radio, c.min_scale_radio = p["net_maxs"] / 0.825, p["net_mins"] / 0.825
        c.net_Dang = p["net_Dang"]
        c.cut_off_face = 0.0                 # per stage: cut_offs_face[serial]
        return c

    def _handle(self):
        if self._h is not None:
            return self._h
        L = _capi.lib()
        arr = (_capi.HgCascadeStage * len(self.stages))()
        for i, st in enumerate(self.stages):
            arr[i].type, arr[i].serial = _capi.HG_STAGE[st.type], st.serial
            if st.flow is not None:
                if st.flow.device != self.device or st.flow.output_dtype != np.float32:
                    raise ValueError("stage %s: flow must live on device %d with output_dtype float32" % (st.name, self.device))
                arr[i].flow = st.flow._handle().h
            else:
                arr[i].flow = None
            arr[i].classifier = st.classifier._handle(st.classifier.avg_labels)
        cut = (C.c_double * len(CUT_OFFS_FACE))(*CUT_OFFS_FACE)
        cc = self._consts()
        h = C.c_void_p()
        _capi.check(L.hg_cascade_create(arr, len(self.stages), self.w, self.h, self.k, C.byref(cc), cut, len(CUT_OFFS_FACE), self.device, C.byref(h)))
        self._h = h
        if self.interpolation_formats is not None:
            fmt = (C.c_int32 * len(self.interpolation_formats))(*self.interpolation_formats)
            _capi.check(L.hg_cascade_set_interpolation(h, fmt, len(self.interpolation_formats)))
        if self.frame_format != _capi.HG_FRAME_L:
            _capi.check(L.hg_cascade_set_frame_format(h, self.frame_format))
        if self.prescale_filter != _capi.HG_RESAMPLE_NEAREST:
            _capi.check(L.hg_cascade_set_prescale_filter(h, self.prescale_filter))
        return h

    def set_prescale_filter(self, prescale_filter):
        """Change the prescale's filter from the next frame on (hg_cascade_set_prescale_filter): between two frames, never during one."""
        code = frames.resample_code(prescale_filter)
        if self._h is not None:
            _capi.check(_capi.lib().hg_cascade_set_prescale_filter(self._h, code))
        self.prescale_filter = code

    def set_frame_format(self, frame_format):
        """Change the format of the frames given from now on (hg_cascade_set_frame_format): between two frames, never during one."""
        code = frames.format_code(frame_format)
        if self._h is not None:
            _capi.check(_capi.lib().hg_cascade_set_frame_format(self._h, code))
        self.frame_format = code

    def _check_frame(self, frame):
        frames.check_color_frame(self.torch, frame, self.frame_format, self.dev)

    def prescale(self, frame, prescale_size=grid.PRESCALE_SIZE):
        """FaceDetectUpdated.py:551-556: shrink so that the larger side is <= prescale_size, ``Image.resize(prescale_filter)``; NEAREST —
        PIL's nearest resize is the EXTENT rule over the whole frame, so the patcher does it (bit-exact vs PIL in the tests).
        A grey frame that needs no shrinking is returned as it is.  Otherwise the returned tensor lives with the cascade, one per
        (frame size, prescaled size): it is valid until the next ``prescale()`` with the same frame size and the same prescaled
        size on this cascade, which writes into it again — a caller that keeps a prescaled frame longer clones it.  A colour frame
        (``frame_format``) always comes back as such a cascade-owned grey tensor, the grey frame the cascade reads: cut from the
        colour frame by the same rule (only the sampled pixels are converted), or, where no shrinking is needed, converted whole."""
        t = self.torch
        self._check_frame(frame)
        fh, fw = int(frame.shape[0]), int(frame.shape[1])
        pw, ph = grid.prescaled_size(fw, fh, prescale_size)
        stream = t.cuda.current_stream(self.dev).cuda_stream
        if (pw, ph) == (fw, fh):
            if self.frame_format == _capi.HG_FRAME_L:
                return frame
            key = (fw, fh, fw, fh)
            if key not in self._prescale:
                self._prescale[key] = (None, t.empty((fh, fw), dtype=t.uint8, device=self.dev))
            return frames.to_gray(frame, self.frame_format, out=self._prescale[key][1])
        key = (fw, fh, pw, ph)
        if key not in self._prescale:      # the box of the whole frame and the output live with the cascade: no per-frame upload / allocation
            self._prescale[key] = (t.tensor([[0.0, 0.0, float(fw), float(fh)]], dtype=t.float64, device=self.dev),
                                   t.empty((ph, pw), dtype=t.uint8, device=self.dev))
        whole, small = self._prescale[key]
        return self._shrink_into(frame, fw, fh, pw, ph, whole, small, stream)

    def _shrink_into(self, frame, fw, fh, pw, ph, whole, small, stream):
        """The shrinking part of ``prescale``: ``frame`` (fw x fh, checked) -> ``small``, a dense (ph, pw) grey uint8 tensor, by the configured
        filter; ``whole``: the box of the whole frame on the device."""
        if self.prescale_filter != _capi.HG_RESAMPLE_NEAREST:      # PIL's antialiased resize of the grey frame (frames.resize)
            return frames.resize(frame, (pw, ph), self.prescale_filter, self.frame_format, out=small, patcher=self.patcher)
        if self.frame_format == _capi.HG_FRAME_L:
            self.patcher.extract_device(frame.data_ptr(), np.uint8, fh, fw, frame.stride(0), whole.data_ptr(), 1, (pw, ph), small.data_ptr(),
                                        np.uint8, pw * ph, stream=stream)
        else:
            _capi.check(_capi.lib().hg_patcher_extract_format_device(
                self.patcher._handle(), self.frame_format, frame.data_ptr(), fh, fw, frame.stride(0), whole.data_ptr(), 1, pw, ph, small.data_ptr(),
                _capi.HG_U8, pw * ph, stream))
        return small

    def prescale_frames(self, stack, prescale_size=grid.PRESCALE_SIZE):
        """``prescale`` for a stack of B same-size frames (``_check_stack``): the (B, ph, pw) grey uint8 stack the rows of
        ``detect_frames`` / ``detect_faces_frames`` refer to — what ``normalize.FaceNormalizer.normalize_frames`` and
        ``analysis.FaceAnalyzer.estimate_faces_frames`` take beside those rows.  Composed here from the per-frame calls: frame f is
        written by the code ``prescale(stack[f])`` runs (the configured filter, grey and colour formats) into slice f of one tensor, so
        its bytes are that call's; B launches, no host wait.  A grey stack that needs no shrinking is returned as it is.  Otherwise the
        tensor is cascade-owned per (B, frame size, prescaled size), with ``prescale``'s lifetime rule: valid until the next
        ``prescale_frames`` with the same key, which writes into it again.  An empty stack returns an empty (0, 0, 0) tensor without
        touching the library."""
        t = self.torch
        stack = self._check_stack(stack)
        if stack is None:
            return t.empty((0, 0, 0), dtype=t.uint8)
        b, fh, fw = int(stack.shape[0]), int(stack.shape[1]), int(stack.shape[2])
        pw, ph = grid.prescaled_size(fw, fh, prescale_size)
        grey = self.frame_format == _capi.HG_FRAME_L
        if (pw, ph) == (fw, fh) and grey:
            return stack
        key = ("stack", b, fw, fh, pw, ph)
        if key not in self._prescale:
            self._prescale[key] = (t.tensor([[0.0, 0.0, float(fw), float(fh)]], dtype=t.float64, device=self.dev),
                                   t.empty((b, ph, pw), dtype=t.uint8, device=self.dev))
        whole, small = self._prescale[key]
        stream = t.cuda.current_stream(self.dev).cuda_stream
        for f in range(b):
            if (pw, ph) == (fw, fh):
                frames.to_gray(stack[f], self.frame_format, out=small[f])
            else:
                self._shrink_into(stack[f], fw, fh, pw, ph, whole, small[f], stream)
        return small

    def detect(self, frame, smallest_face=0.2, windows=None):
        """frame: (H, W) uint8 torch tensor on this device ((H, W, C) for a colour ``frame_format``).  Returns a dict of host arrays:
        coords (n, 4), angles (n), orig_index (n), confidence (n), counts (survivors after every stage, -1 where the count stayed on
        the device), rows_executed."""
        t, L = self.torch, _capi.lib()
        if self.frame_format != _capi.HG_FRAME_L:
            self._check_frame(frame)
        elif frame.dtype != t.uint8 or frame.device != self.dev or frame.stride(1) != 1:
            raise ValueError("frame must be a uint8 tensor on %s with contiguous rows" % (self.dev,))
        fh, fw = int(frame.shape[0]), int(frame.shape[1])
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        counts = np.zeros(len(self.stages), dtype=np.int32)
        n_out, rows = C.c_int64(), C.c_int64()
        stream = C.c_void_p(t.cuda.current_stream(self.dev).cuda_stream)
        if windows is None:
            # the frame's own grid: the windows are computed on the device from the table of pyramid levels (face_analysis.py:630-669)
            key = (fw, fh, float(smallest_face))
            if key not in self._levels:
                self._levels[key] = frame_levels(fw, fh, smallest_face, self.pipeline, (self.w, self.h))
            levels, n_levels, n0 = self._levels[key]
            coords, angles = np.empty((n0, 4)), np.empty(n0)
            oidx, conf = np.empty(n0, dtype=np.int32), np.empty(n0)
            _capi.check(L.hg_cascade_detect_levels_device(
                self._handle(), C.c_void_p(frame.data_ptr()), fh, fw, frame.stride(0), levels, n_levels, vp(coords), vp(angles), vp(oidx),
                vp(conf), n0, C.byref(n_out), vp(counts), C.byref(rows), stream))
        else:
            boxes, level = windows
            boxes = np.ascontiguousarray(boxes, dtype=np.float64)
            level = np.ascontiguousarray(level, dtype=np.float64)
            n0 = len(boxes)
            coords, angles = np.empty((n0, 4)), np.empty(n0)
            oidx, conf = np.empty(n0, dtype=np.int32), np.empty(n0)
            _capi.check(L.hg_cascade_detect_device(
                self._handle(), C.c_void_p(frame.data_ptr()), fh, fw, frame.stride(0), vp(boxes), vp(level), n0, vp(coords), vp(angles), vp(oidx),
                vp(conf), n0, C.byref(n_out), vp(counts), C.byref(rows), stream))
        n = n_out.value
        return dict(coords=coords[:n].copy(), angles=angles[:n].copy(), orig_index=oidx[:n].astype(np.int64), confidence=conf[:n].copy(),
                    counts=[int(c) for c in counts], rows_executed=int(rows.value), n_windows=n0)

    def detect_frame(self, frame, smallest_face=0.2, prescale_size=grid.PRESCALE_SIZE):
        """prescale + detect as ONE host call (hg_cascade_detect_frame_device): what the reference does per image between loading
        it and writing its detections (FaceDetectUpdated.py:551-561 prescale, :589-600 grid, :665-766 stage loop).  Everything that
        depends only on the frame size — prescaled size, level table, output buffers — is computed once and kept; the frame itself
        is checked on every call (the library is handed its raw pointer)."""
        t, L = self.torch, _capi.lib()
        self._check_frame(frame)
        fh, fw = int(frame.shape[0]), int(frame.shape[1])
        key = (fw, fh, float(smallest_face), int(prescale_size or 0))
        plan = self._frames.get(key)
        if plan is None:
            pw, ph = grid.prescaled_size(fw, fh, prescale_size) if prescale_size else (fw, fh)
            pre = (pw, ph) if (pw, ph) != (fw, fh) else (0, 0)
            levels, n_levels, n0 = frame_levels(pw, ph, smallest_face, self.pipeline, (self.w, self.h))
            bufs = (np.empty((n0, 4)), np.empty(n0), np.empty(n0, dtype=np.int32), np.empty(n0), np.zeros(len(self.stages), dtype=np.int32))
            plan = self._frames[key] = (pre, levels, n_levels, n0, bufs, [b.ctypes.data_as(C.c_void_p) for b in bufs], C.c_int64(), C.c_int64())
        pre, levels, n_levels, n0, (coords, angles, oidx, conf, counts), ptr, n_out, rows = plan
        _capi.check(L.hg_cascade_detect_frame_device(
            self._handle(), frame.data_ptr(), fh, fw, frame.stride(0), pre[0], pre[1], levels, n_levels, ptr[0], ptr[1], ptr[2], ptr[3], n0,
            C.byref(n_out), ptr[4], C.byref(rows), t.cuda.current_stream(self.dev).cuda_stream))
        n = n_out.value
        return dict(coords=coords[:n].copy(), angles=angles[:n].copy(), orig_index=oidx[:n].astype(np.int64), confidence=conf[:n].copy(),
                    counts=counts.tolist(), rows_executed=rows.value, n_windows=n0)

    def detect_faces(self, frame, eyes, smallest_face=0.2, prescale_size=grid.PRESCALE_SIZE):
        """detect_frame, then the eye step (``eyes``: an ``eyes.EyeLocator`` on this device) on the survivors, on the frame the cascade
        read, the discard of the too-far faces, one row per face and the purge — as ONE host call
        (hg_cascade_detect_faces_frame_device; FaceDetectUpdated.py:947-1041, :1180).  Returns faces (m, 10) = (x0, y0, x1, y1, angle,
        eyeL_x, eyeL_y, eyeR_x, eyeR_y, confidence), n_before_purge, counts, rows_executed, n_windows.  The frame is checked on every
        call; everything that depends only on the frame size is computed once and kept."""
        t, L = self.torch, _capi.lib()
        self._check_frame(frame)
        if eyes.device != self.device:
            raise ValueError("eye locator on device %d, cascade on device %d" % (eyes.device, self.device))
        fh, fw = int(frame.shape[0]), int(frame.shape[1])
        key = ("faces", fw, fh, float(smallest_face), int(prescale_size or 0))
        plan = self._frames.get(key)
        if plan is None:
            pw, ph = grid.prescaled_size(fw, fh, prescale_size) if prescale_size else (fw, fh)
            pre = (pw, ph) if (pw, ph) != (fw, fh) else (0, 0)
            levels, n_levels, n0 = frame_levels(pw, ph, smallest_face, self.pipeline, (self.w, self.h))
            rows, counts = np.empty((n0 + 1, 10)), np.zeros(len(self.stages), dtype=np.int32)      # the purge may keep n + 1 rows
            plan = self._frames[key] = (pre, levels, n_levels, n0, rows, counts, C.c_int64(), C.c_int64(), C.c_int64())
        pre, levels, n_levels, n0, rows, counts, n_out, n_before, n_rows = plan
        _capi.check(L.hg_cascade_detect_faces_frame_device(
            self._handle(), eyes._handle(), frame.data_ptr(), fh, fw, frame.stride(0), pre[0], pre[1], levels, n_levels,
            rows.ctypes.data_as(C.c_void_p), len(rows), C.byref(n_out), C.byref(n_before), counts.ctypes.data_as(C.c_void_p), C.byref(n_rows),
            t.cuda.current_stream(self.dev).cuda_stream))
        return dict(faces=rows[:n_out.value].copy(), n_before_purge=n_before.value, counts=counts.tolist(), rows_executed=n_rows.value,
                    n_windows=n0)

    def _check_stack(self, stack):
        """A stack of same-size frames as one tensor, or ValueError; None for an empty stack.  (B, H, W) uint8, (B, H, W, C) for a colour
        ``frame_format``; rows contiguous (pixels packed), ``stride(1)`` at least a row's bytes — a broadcast view has 0 and is refused
        as ``ld < frame_w`` is — and ``stride(0)`` at least a frame's reach, (H - 1) stride(1) + W C: the frames may be every second
        frame of a larger stack or crops of larger frames.  A list or tuple of same-shaped tensors is stacked (``torch.stack``).
        Shape, dtype and strides are checked before the device, which is checked before the library is touched."""
        t = self.torch
        c = frames.CHANNELS[self.frame_format]
        color = self.frame_format != _capi.HG_FRAME_L
        shape = "(B, H, W, %d)" % c if color else "(B, H, W)"
        if isinstance(stack, (list, tuple)):
            if len(stack) == 0:
                return None
            if any(not isinstance(f, t.Tensor) or f.shape != stack[0].shape or f.dtype != stack[0].dtype or f.device != stack[0].device for f in stack):
                raise ValueError("a list of frames must hold tensors of one shape, dtype and device (frames of different sizes do not share a call)")
            stack = t.stack(list(stack))
        if not isinstance(stack, t.Tensor) or stack.dim() != (4 if color else 3) or stack.dtype != t.uint8 or (color and stack.shape[3] != c):
            raise ValueError("a stack of frames must be a %s uint8 tensor" % shape)
        b, fh, fw = int(stack.shape[0]), int(stack.shape[1]), int(stack.shape[2])
        if b == 0:
            return None
        if fh == 0 or fw == 0:
            raise ValueError("a stack of empty frames")
        if b > _capi.HG_MAX_STACK_FRAMES:
            raise ValueError("%d frames in a stack, at most %d" % (b, _capi.HG_MAX_STACK_FRAMES))
        if (color and (stack.stride(3) != 1 or stack.stride(2) != c)) or (not color and stack.stride(2) != 1):
            raise ValueError("the frames of a stack must have contiguous rows (packed pixels), got strides %s" % (tuple(stack.stride()),))
        if fh > 1 and stack.stride(1) < fw * c:
            raise ValueError("rows %d bytes apart hold %d bytes: a broadcast or overlapping view is not a frame" % (stack.stride(1), fw * c))
        ld = stack.stride(1) if fh > 1 else fw * c
        if b > 1 and stack.stride(0) < (fh - 1) * ld + fw * c:
            raise ValueError("frames %d bytes apart reach over %d bytes: a broadcast or overlapping view is not a stack" %
                             (stack.stride(0), (fh - 1) * ld + fw * c))
        if stack.device != self.dev:
            raise ValueError("the stack must live on %s" % (self.dev,))
        return stack

    def _stack_plan(self, what, stack, smallest_face, prescale_size):
        """Everything a stack call needs that depends on (B, frame size, smallest_face, prescale size) alone, computed once and kept like
        detect_frame's plans, and the geometry of this stack."""
        b, fh, fw = int(stack.shape[0]), int(stack.shape[1]), int(stack.shape[2])
        c = frames.CHANNELS[self.frame_format]
        key = (what, b, fw, fh, float(smallest_face), int(prescale_size or 0))
        plan = self._frames.get(key)
        if plan is None:
            pw, ph = grid.prescaled_size(fw, fh, prescale_size) if prescale_size else (fw, fh)
            pre = (pw, ph) if (pw, ph) != (fw, fh) else (0, 0)
            levels, n_levels, n0 = frame_levels(pw, ph, smallest_face, self.pipeline, (self.w, self.h))
            first, counts = np.zeros(b + 1, dtype=np.int32), np.zeros(len(self.stages), dtype=np.int32)
            if what == "stack":
                bufs = (np.empty((b * n0, 4)), np.empty(b * n0), np.empty(b * n0, dtype=np.int32), np.empty(b * n0))
            else:
                bufs = (np.empty((b * (n0 + 1), 10)), np.zeros(b, dtype=np.int32))      # the purge may keep n + 1 rows of every frame
            plan = self._frames[key] = (pre, levels, n_levels, n0, bufs, first, counts, C.c_int64())
        ld = stack.stride(1) if fh > 1 else fw * c
        stride = stack.stride(0) if b > 1 else (fh - 1) * ld + fw * c
        return plan, (b, fh, fw, ld, stride)

    def detect_frames(self, stack, smallest_face=0.2, prescale_size=grid.PRESCALE_SIZE):
        """``detect_frame`` for a stack of B same-size frames as ONE pooled pass (hg_cascade_detect_frames_device): the windows of all
        frames are one batch of candidates through the stage loop.  stack: see ``_check_stack``.  Returns ``frames``, a list of B dicts
        with coords, angles, orig_index, confidence — array for array what ``detect_frame`` returns for that frame — and the pooled
        counts (the sum of the per-frame counts, -1 where those are -1), rows_executed and n_windows (B times one frame's).  An empty
        stack returns an empty list without touching the library."""
        t = self.torch
        stack = self._check_stack(stack)
        if stack is None:
            return dict(frames=[], counts=[0] * len(self.stages), rows_executed=0, n_windows=0)
        (pre, levels, n_levels, n0, bufs, first, counts, rows), (b, fh, fw, ld, stride) = self._stack_plan("stack", stack, smallest_face, prescale_size)
        coords, angles, oidx, conf = bufs
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        _capi.check(_capi.lib().hg_cascade_detect_frames_device(
            self._handle(), stack.data_ptr(), b, stride, fh, fw, ld, pre[0], pre[1], levels, n_levels, vp(coords), vp(angles), vp(oidx), vp(conf), b * n0,
            vp(first), vp(counts), C.byref(rows), t.cuda.current_stream(self.dev).cuda_stream))
        out = []
        for f in range(b):
            lo, hi = int(first[f]), int(first[f + 1])
            out.append(dict(coords=coords[lo:hi].copy(), angles=angles[lo:hi].copy(), orig_index=oidx[lo:hi].astype(np.int64),
                            confidence=conf[lo:hi].copy()))
        return dict(frames=out, counts=counts.tolist(), rows_executed=rows.value, n_windows=b * n0)

    def detect_faces_frames(self, stack, eyes, smallest_face=0.2, prescale_size=grid.PRESCALE_SIZE):
        """``detect_faces`` for a stack of B same-size frames (hg_cascade_detect_faces_frames_device): the pooled stage loop, the eye step
        on all survivors as one batch, the purge per frame.  Returns ``faces``, a list of B (m_b, 10) arrays — what ``detect_faces``
        returns for that frame — ``n_before_purge``, a list of B, and the pooled counts, rows_executed, n_windows."""
        t = self.torch
        if eyes.device != self.device:
            raise ValueError("eye locator on device %d, cascade on device %d" % (eyes.device, self.device))
        stack = self._check_stack(stack)
        if stack is None:
            return dict(faces=[], n_before_purge=[], counts=[0] * len(self.stages), rows_executed=0, n_windows=0)
        (pre, levels, n_levels, n0, bufs, first, counts, n_rows), (b, fh, fw, ld, stride) = self._stack_plan("stack faces", stack, smallest_face, prescale_size)
        rows, before = bufs
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        _capi.check(_capi.lib().hg_cascade_detect_faces_frames_device(
            self._handle(), eyes._handle(), stack.data_ptr(), b, stride, fh, fw, ld, pre[0], pre[1], levels, n_levels, vp(rows), len(rows), vp(first),
            vp(before), vp(counts), C.byref(n_rows), t.cuda.current_stream(self.dev).cuda_stream))
        return dict(faces=[rows[int(first[f]):int(first[f + 1])].copy() for f in range(b)], n_before_purge=before.tolist(), counts=counts.tolist(),
                    rows_executed=n_rows.value, n_windows=b * n0)

    def _check_list(self, frame_list):
        """A list (or tuple) of frames of ANY sizes, or ValueError; None for an empty list.  Every frame is checked as ``_check_frame``
        checks one — (H, W) uint8, (H, W, C) for a colour ``frame_format``, packed pixels — and, as ``_check_stack`` does, refused when
        it is empty or its rows are fewer bytes apart than they hold (a broadcast view).  Shapes, dtypes and strides are checked
        before the device, which is checked before the library is touched."""
        t = self.torch
        if not isinstance(frame_list, (list, tuple)):
            raise ValueError("a list of frames must be a list or tuple of tensors (a stack of same-size frames: detect_frames)")
        if len(frame_list) == 0:
            return None
        if len(frame_list) > _capi.HG_MAX_STACK_FRAMES:
            raise ValueError("%d frames in a list, at most %d" % (len(frame_list), _capi.HG_MAX_STACK_FRAMES))
        c = frames.CHANNELS[self.frame_format]
        for i, f in enumerate(frame_list):
            if not isinstance(f, t.Tensor):
                raise ValueError("frame %d of the list is not a tensor" % i)
            try:
                frames.check_color_frame(t, f, self.frame_format, f.device)
            except ValueError as e:
                raise ValueError("frame %d of the list: %s" % (i, e))
            fh, fw = int(f.shape[0]), int(f.shape[1])
            if fh == 0 or fw == 0:
                raise ValueError("frame %d of the list is empty" % i)
            if fh > 1 and f.stride(0) < fw * c:
                raise ValueError("frame %d of the list: rows %d bytes apart hold %d bytes: a broadcast or overlapping view is not a frame" %
                                 (i, f.stride(0), fw * c))
        for i, f in enumerate(frame_list):
            if f.device != self.dev:
                raise ValueError("frame %d of the list must live on %s" % (i, self.dev))
        return list(frame_list)

    def _list_plan(self, what, frame_list, smallest_face, prescale_size):
        """The descriptor array of this list (hg_cascade_frame, assembled per call), the window count of every frame, and output buffers.
        What depends on a frame's size alone — prescaled size, level table — is kept per distinct size, as detect_frame's plans are."""
        c = frames.CHANNELS[self.frame_format]
        arr = (_capi.HgCascadeFrame * len(frame_list))()
        n0s = []
        for i, f in enumerate(frame_list):
            fh, fw = int(f.shape[0]), int(f.shape[1])
            key = ("list", fw, fh, float(smallest_face), int(prescale_size or 0))
            plan = self._frames.get(key)
            if plan is None:
                pw, ph = grid.prescaled_size(fw, fh, prescale_size) if prescale_size else (fw, fh)
                pre = (pw, ph) if (pw, ph) != (fw, fh) else (0, 0)
                plan = self._frames[key] = (pre,) + tuple(frame_levels(pw, ph, smallest_face, self.pipeline, (self.w, self.h)))
            pre, levels, n_levels, n0 = plan
            a = arr[i]
            a.frame_dev, a.frame_h, a.frame_w, a.ld = f.data_ptr(), fh, fw, (f.stride(0) if fh > 1 else fw * c)
            a.prescale_w, a.prescale_h = pre
            a.levels, a.n_levels = C.cast(levels, C.POINTER(_capi.HgCascadeLevel)), n_levels
            n0s.append(n0)
        b, total = len(frame_list), sum(n0s)
        # ONE set of output buffers per kind of call, grown on demand (nearly every list of a folder of photographs has another length and
        # window count: a set per (b, total) would stay with the cascade for ever)
        rows, bufs = self._list_bufs.get(what, (0, None))
        if bufs is None or rows < total + b or len(bufs[1]) < b + 1:
            rows = max(total + b, 2 * rows)
            nb = max(b, 2 * (len(bufs[1]) - 1) if bufs else 0)
            first, counts = np.zeros(nb + 1, dtype=np.int32), np.zeros(len(self.stages), dtype=np.int32)
            if what == "list bufs":
                out = (np.empty((rows, 4)), np.empty(rows), np.empty(rows, dtype=np.int32), np.empty(rows))
            else:
                out = (np.empty((rows, 10)), np.zeros(nb, dtype=np.int32))      # the purge may keep n + 1 rows of every frame
            bufs = (out, first, counts, C.c_int64())
            self._list_bufs[what] = (rows, bufs)
        return arr, total, bufs

    def prescale_frame_list(self, frame_list, prescale_size=grid.PRESCALE_SIZE):
        """``prescale`` for a list of frames of DIFFERENT sizes (``_check_list``): the list of grey uint8 frames the rows of
        ``detect_frame_list`` / ``detect_faces_frame_list`` refer to — what ``normalize.FaceNormalizer.normalize_frame_list`` and
        ``analysis.FaceAnalyzer.estimate_faces_frame_list`` take beside those rows.  Composed here from the per-frame calls: frame f is
        written by the code ``prescale(frame_list[f])`` runs (the configured filter, grey and colour formats), so its bytes are that
        call's; B launches, no host wait.  NOT ``prescale``'s tensors, which are one per (frame size, prescaled size) — two frames of one
        size would come back as the same tensor: the outputs are (ph, pw) views at 256-byte-aligned offsets of ONE cascade-owned byte
        buffer, grown on demand, valid until the next ``prescale_frame_list`` on this cascade (a caller that keeps them longer clones
        them).  A grey frame that needs no shrinking is returned as it is.  An empty list returns ``[]`` without touching the library."""
        t = self.torch
        frame_list = self._check_list(frame_list)
        if frame_list is None:
            return []
        grey = self.frame_format == _capi.HG_FRAME_L
        plan, total = [], 0
        for f in frame_list:
            fh, fw = int(f.shape[0]), int(f.shape[1])
            pw, ph = grid.prescaled_size(fw, fh, prescale_size)
            if (pw, ph) == (fw, fh) and grey:
                plan.append(None)
                continue
            plan.append((fw, fh, pw, ph, total))
            total += (pw * ph + 255) & ~255
        stream = t.cuda.current_stream(self.dev)
        buf = self._list_pre
        if total and (buf is None or buf.numel() < total):
            # a launch enqueued on this stream may still write the old buffer: it goes back to the allocator only behind that work (the
            # views handed out earlier keep it alive as long as the caller holds them)
            if buf is not None:
                buf.record_stream(stream)
            buf = self._list_pre = t.empty(max(total, 2 * (0 if buf is None else buf.numel())), dtype=t.uint8, device=self.dev)
        out = []
        for f, p in zip(frame_list, plan):
            if p is None:
                out.append(f)
                continue
            fw, fh, pw, ph, at = p
            small = buf[at:at + pw * ph].view(ph, pw)
            if (pw, ph) == (fw, fh):
                frames.to_gray(f, self.frame_format, out=small)
            else:
                key = ("whole", fw, fh)
                if key not in self._prescale:      # the box of the whole frame lives with the cascade, one per frame size
                    self._prescale[key] = t.tensor([[0.0, 0.0, float(fw), float(fh)]], dtype=t.float64, device=self.dev)
                self._shrink_into(f, fw, fh, pw, ph, self._prescale[key], small, stream.cuda_stream)
            out.append(small)
        return out

    def detect_frame_list(self, frame_list, smallest_face=0.2, prescale_size=grid.PRESCALE_SIZE):
        """``detect_frame`` for a list of frames of DIFFERENT sizes as ONE pooled pass (hg_cascade_detect_frame_list_device): every frame is
        prescaled to its own size and has its own grid, and the concatenated grids are one batch of candidates through the stage loop.
        frame_list: see ``_check_list`` (shapes and row strides may differ; frames of one size are ``detect_frames``'s case).  Returns
        what ``detect_frames`` returns: ``frames``, a list of dicts — array for array what ``detect_frame`` returns for that frame — and
        the pooled counts, rows_executed and n_windows (the sum over the frames).  An empty list returns an empty result without
        touching the library."""
        t = self.torch
        frame_list = self._check_list(frame_list)
        if frame_list is None:
            return dict(frames=[], counts=[0] * len(self.stages), rows_executed=0, n_windows=0)
        arr, total, ((coords, angles, oidx, conf), first, counts, rows) = self._list_plan("list bufs", frame_list, smallest_face, prescale_size)
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        _capi.check(_capi.lib().hg_cascade_detect_frame_list_device(
            self._handle(), arr, len(frame_list), vp(coords), vp(angles), vp(oidx), vp(conf), total, vp(first), vp(counts), C.byref(rows),
            t.cuda.current_stream(self.dev).cuda_stream))
        out = []
        for f in range(len(frame_list)):
            lo, hi = int(first[f]), int(first[f + 1])
            out.append(dict(coords=coords[lo:hi].copy(), angles=angles[lo:hi].copy(), orig_index=oidx[lo:hi].astype(np.int64),
                            confidence=conf[lo:hi].copy()))
        return dict(frames=out, counts=counts.tolist(), rows_executed=rows.value, n_windows=total)

    def detect_faces_frame_list(self, frame_list, eyes, smallest_face=0.2, prescale_size=grid.PRESCALE_SIZE):
        """``detect_faces`` for a list of frames of different sizes (hg_cascade_detect_faces_frame_list_device): the pooled stage loop, the
        eye step on all survivors as one batch — every eye patch cut from its face's own prescaled frame — and the purge per frame.
        Returns what ``detect_faces_frames`` returns: ``faces``, a list of (m_b, 10) arrays, ``n_before_purge``, a list, and the pooled
        counts, rows_executed, n_windows."""
        t = self.torch
        if eyes.device != self.device:
            raise ValueError("eye locator on device %d, cascade on device %d" % (eyes.device, self.device))
        frame_list = self._check_list(frame_list)
        if frame_list is None:
            return dict(faces=[], n_before_purge=[], counts=[0] * len(self.stages), rows_executed=0, n_windows=0)
        arr, total, ((rows, before), first, counts, n_rows) = self._list_plan("list faces bufs", frame_list, smallest_face, prescale_size)
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        _capi.check(_capi.lib().hg_cascade_detect_faces_frame_list_device(
            self._handle(), eyes._handle(), arr, len(frame_list), vp(rows), len(rows), vp(first), vp(before), vp(counts), C.byref(n_rows),
            t.cuda.current_stream(self.dev).cuda_stream))
        return dict(faces=[rows[int(first[f]):int(first[f + 1])].copy() for f in range(len(frame_list))], n_before_purge=before[:len(frame_list)].tolist(),
                    counts=counts.tolist(), rows_executed=n_rows.value, n_windows=total)

    def close(self):
        if self._h is not None:
            _capi.lib().hg_cascade_free(self._h)
            self._h = None
        self.patcher.close()
