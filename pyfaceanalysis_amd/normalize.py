"""Pose-normalised face crops: ``face_normalization_tools.normalize_image`` on the device (include/higsfa.h, "normalize_image").

What the reference does with the rows of ``detect_faces`` / ``FaceTracker`` next: ``save_pose_normalized_face_detections``
(face_analysis.py:983-1013) makes 256 x 192 crops from the approximate eyes of every surviving box, ``estimate_age_race_gender``
(face_analysis.py:1170-1222) 256 x 260 crops from the located eyes of every purged face — the image age, race and gender estimation
starts from.  Both call ``normalize_image`` in one configuration, the one restated here: ``centering_mode="mid_eyes_inferred-mouth"``,
``rotation_mode`` "EyeLineRotation" or "noRotation", ``integer_rotation_center=True``, ``allow_random_background=False``,
``convert_format="L"``, the mouth inferred from the eyes, ``normalization_method`` "eyes_inferred-mouth_area" or
"eyes_inferred-mouth_areaZ", any ``out_size``.  Everything else is refused with a ValueError that names it.

The geometry is computed per face on the host in float64 (hg_normalize_geometry_host: the reference's operation order and the libm
Python's ``math`` uses); the pixels are PIL's, bit for bit — ``crop.rotate(angle, BICUBIC)`` of the zero-padded crop around the face,
then ``transform(out_size, EXTENT, box, BICUBIC)`` — computed on the device for the few thousand rotated pixels the cut reads
(hg_patcher_normalize_device), or on the host (``normalize_host``).  Frames are grey uint8; a colour frame goes through
``frames.to_gray`` first.

EYE COORDINATES ARE IN THE COORDINATES OF THE FRAME PASSED IN.  The rows of ``detect_faces`` refer to the frame the cascade read —
the prescaled one — so the caller passes that frame (``DeviceCascade.prescale(frame)``, or ``frames.resize(frame, size, "NEAREST")``)
with ``faces[:, 5:9]``.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _capi

assert _capi.NORM_GEOM_DTYPE.itemsize == 144

METHODS = {"eyes_inferred-mouth_area": _capi.HG_NORM_AREA, "eyes_inferred-mouth_areaZ": _capi.HG_NORM_AREAZ}
ROTATION_MODES = {"EyeLineRotation": True, "noRotation": False}
# the two callers of the reference: (out_size, normalization_method), face_analysis.py:1172-1179 and :986-995
PRESETS = {"age": ((256, 260), "eyes_inferred-mouth_areaZ"), "pose": ((256, 192), "eyes_inferred-mouth_area")}
STATUS = {0: "ok", 1: "left eye right of the right eye", 2: "a coordinate is not finite", 3: "the eyes coincide", 4: "the centre is beyond 2^20"}
# the stack calls' own status (``normalize_frames``, ``FaceAnalyzer.estimate_frames``): the face's frame index lies outside the stack.  It
# is Python's: the geometry knows no frames, hg_norm_geom.status stays 0 for such a face and the library treats it like a refused one.
STATUS_FRAME_RANGE = 5
STATUS[STATUS_FRAME_RANGE] = "the frame index is outside the stack"      # (or outside the list: ``normalize_frame_list``, ``estimate_frame_list``)


def check_configuration(normalization_method="eyes_inferred-mouth_area", centering_mode="mid_eyes_inferred-mouth", rotation_mode="EyeLineRotation",
                        integer_rotation_center=True, allow_random_background=False, convert_format="L"):
    """``normalize_image``'s keyword arguments -> (method code, rotate) for the configuration this build restates, or a ValueError naming
    the argument that is not offered."""
    if normalization_method not in METHODS:
        raise ValueError("normalization_method %r is not offered (one of %s; \"eyes_mouth_area\" needs a real mouth)" % (normalization_method, ", ".join(METHODS)))
    if centering_mode != "mid_eyes_inferred-mouth":
        raise ValueError("centering_mode %r is not offered (only \"mid_eyes_inferred-mouth\")" % (centering_mode,))
    if rotation_mode not in ROTATION_MODES:
        raise ValueError("rotation_mode %r is not offered (\"EyeLineRotation\" or \"noRotation\")" % (rotation_mode,))
    if not integer_rotation_center:
        raise ValueError("integer_rotation_center=False is not offered")
    if allow_random_background:
        raise ValueError("allow_random_background=True is not offered")
    if convert_format != "L":
        raise ValueError("convert_format %r is not offered (only \"L\")" % (convert_format,))
    return METHODS[normalization_method], ROTATION_MODES[rotation_mode]


def _consts(out_size, method, rotate):
    if isinstance(method, str):
        if method not in METHODS:
            raise ValueError("normalization_method %r is not offered (one of %s; \"eyes_mouth_area\" needs a real mouth)" % (method, ", ".join(METHODS)))
        method = METHODS[method]
    ow, oh = int(out_size[0]), int(out_size[1])
    if not (1 <= ow <= 4096 and 1 <= oh <= 4096):
        raise ValueError("out_size must be (width, height) with 1 .. 4096 pixels each, got %r" % (out_size,))
    c = _capi.HgNormConsts()
    c.out_w, c.out_h, c.method, c.rotate = ow, oh, int(method), 1 if rotate else 0
    return c


def _eyes(eyes):
    e = np.asarray(eyes, dtype=np.float64)
    if e.ndim > 2 or (e.ndim == 2 and e.shape[1] != 4) or e.size % 4:
        raise ValueError("eyes must be (n, 4): left eye x, left eye y, right eye x, right eye y")
    return np.ascontiguousarray(e.reshape(-1, 4))


def geometry(eyes, frame_size, out_size=(256, 192), method="eyes_inferred-mouth_area", rotate=True):
    """The geometry of ``normalize_image`` per face (hg_normalize_geometry_host): a record array of ``_capi.NORM_GEOM_DTYPE`` —
    ``crop_x0, crop_y0, W, H, angle, shift, m, box, rotated, status, rect``.  ``frame_size``: (width, height), PIL's order."""
    e = _eyes(eyes)
    c = _consts(out_size, method, rotate)
    g = np.zeros(e.shape[0], dtype=_capi.NORM_GEOM_DTYPE)
    _capi.check(_capi.lib().hg_normalize_geometry_host(e.ctypes.data_as(C.c_void_p), e.shape[0], int(frame_size[0]), int(frame_size[1]), C.byref(c),
                                                       g.ctypes.data_as(C.c_void_p)))
    return g


def _check_geoms(geoms):
    g = np.ascontiguousarray(geoms)
    if g.dtype != _capi.NORM_GEOM_DTYPE or g.ndim != 1:
        raise ValueError("geoms must be the 1-d record array geometry() returns")
    return g


def normalize_host(frame, eyes=None, out_size=(256, 192), method="eyes_inferred-mouth_area", rotate=True, geoms=None):
    """The host twin (hg_normalize_faces_host: plain C++, no device): ``frame`` an (H, W) uint8 array whose rows may be any number of
    bytes >= W apart (a crop view of a larger frame is fine).  Returns (images (n, out_h, out_w) uint8, status (n,) int32).  ``geoms``:
    the records of ``geometry`` for this frame size and ``out_size`` instead of ``eyes``."""
    a = np.asarray(frame)
    if a.dtype != np.uint8 or a.ndim != 2 or a.shape[0] == 0 or a.shape[1] == 0:
        raise ValueError("frame must be a non-empty (H, W) uint8 array (grey; colour frames go through frames.to_gray_host first)")
    if (a.shape[1] > 1 and a.strides[1] != 1) or (a.shape[0] > 1 and a.strides[0] < a.shape[1]):
        a = np.ascontiguousarray(a)
    h, w = a.shape
    g = geometry(eyes, (w, h), out_size, method, rotate) if geoms is None else _check_geoms(geoms)
    ow, oh = int(out_size[0]), int(out_size[1])
    out = np.zeros((g.shape[0], oh, ow), dtype=np.uint8)
    _capi.check(_capi.lib().hg_normalize_faces_host(a.ctypes.data_as(C.c_void_p), h, w, a.strides[0] if h > 1 else w, g.ctypes.data_as(C.c_void_p),
                                                    g.shape[0], ow, oh, out.ctypes.data_as(C.c_void_p), ow * oh))
    return out, g["status"].astype(np.int32)


def approximate_eye_coords(boxes, angles=None):
    """The eye coordinates ``compute_approximate_eye_boxes_coordinates(box, face_sampling=0.825, eye_sampling=2.3719, rot_angle=angle)``
    returns first (face_analysis.py:87-122), for every box: (n, 4) left eye x, left eye y, right eye x, right eye y — what
    ``save_pose_normalized_face_detections`` feeds to ``normalize_image``.  numpy, the reference's operation order."""
    b = np.asarray(boxes, dtype=np.float64).reshape(-1, 4)
    x0, y0, x1, y1 = b[:, 0], b[:, 1], b[:, 2], b[:, 3]
    rot_angle = np.zeros(b.shape[0]) if angles is None else np.asarray(angles, dtype=np.float64).reshape(-1)
    if rot_angle.shape[0] != b.shape[0]:
        raise ValueError("angles must have one entry per box")
    fc_x = (x0 + x1) / 2.0
    fc_y = (y0 + y1) / 2.0
    eye_dx = (37.0 / 2.0) * (np.abs(x1 - x0) / 64.0) / (2 * 0.825)
    eye_dy = (42.0 / 2.0) * (np.abs(y1 - y0) / 64.0) / (2 * 0.825)
    rad = rot_angle * np.pi / 180
    eye_right_dx_rotated = eye_dx * np.cos(rad) - eye_dy * np.sin(rad)
    eye_right_dy_rotated = eye_dy * np.cos(rad) + eye_dx * np.sin(rad)
    eye_left_dx_rotated = (-1 * eye_dx) * np.cos(rad) - eye_dy * np.sin(rad)
    eye_left_dy_rotated = eye_dy * np.cos(rad) + (-1 * eye_dx) * np.sin(rad)
    eye_left_x = fc_x + 1 * eye_left_dx_rotated
    eye_right_x = fc_x + 1 * eye_right_dx_rotated
    eye_left_y = fc_y - eye_left_dy_rotated
    eye_right_y = fc_y - eye_right_dy_rotated
    return np.stack([eye_left_x, eye_left_y, eye_right_x, eye_right_y], axis=1)


def check_grey_stack(t, stack, device, what):
    """A stack of same-size grey frames for ``what`` ("normalize_frames", "estimate_frames") as one tensor, or ValueError; None for an
    empty stack.  The rules of ``DeviceCascade._check_stack`` for grey frames: (B, H, W) uint8, rows contiguous, ``stride(1) >= W`` (a
    broadcast view is refused), ``stride(0) >= (H - 1) stride(1) + W`` — every second frame of a larger stack or crops of larger frames
    are fine — at most ``HG_MAX_STACK_FRAMES`` frames; a list or tuple of same-shaped tensors is stacked.  Shape, dtype and strides are
    checked before the device.  ``device``: the index the stack must live on."""
    if isinstance(stack, (list, tuple)):
        if len(stack) == 0:
            return None
        if any(not isinstance(f, t.Tensor) or f.shape != stack[0].shape or f.dtype != stack[0].dtype or f.device != stack[0].device for f in stack):
            raise ValueError("a list of frames must hold tensors of one shape, dtype and device (frames of different sizes do not share a call)")
        stack = t.stack(list(stack))
    if not isinstance(stack, t.Tensor):
        raise ValueError("%s takes a device tensor" % what)
    if stack.dtype != t.uint8 or stack.dim() != 3:
        raise ValueError("the stack must be (B, H, W) grey uint8 (a float stack is not offered; a colour stack goes through DeviceCascade.prescale_frames first)")
    b, h, w = (int(v) for v in stack.shape)
    if b == 0:
        return None
    if h == 0 or w == 0:
        raise ValueError("a stack of empty frames")
    if b > _capi.HG_MAX_STACK_FRAMES:
        raise ValueError("%d frames in a stack, at most %d" % (b, _capi.HG_MAX_STACK_FRAMES))
    if stack.stride(2) != 1:
        raise ValueError("the frames of a stack must have contiguous rows, got strides %s" % (tuple(stack.stride()),))
    if h > 1 and stack.stride(1) < w:
        raise ValueError("rows %d bytes apart hold %d bytes: a broadcast or overlapping view is not a frame" % (stack.stride(1), w))
    ld = stack.stride(1) if h > 1 else w
    if b > 1 and stack.stride(0) < (h - 1) * ld + w:
        raise ValueError("frames %d bytes apart reach over %d bytes: a broadcast or overlapping view is not a stack" % (stack.stride(0), (h - 1) * ld + w))
    if device is not None:
        check_stack_device(stack, device, what)
    return stack


def check_stack_device(stack, device, what):
    """The last refusal before the library: the stack (None: an empty one) lives on device ``device``."""
    if stack is None:
        return
    if not stack.is_cuda:
        raise ValueError("%s takes a device tensor" % what)
    if (stack.device.index or 0) != device:
        raise ValueError("the stack is on %s, not on device %d" % (stack.device, device))


def stack_layout(stack):
    """(B, H, W, ld, frame_stride) of a checked stack, as the stack entries take them (bytes; one frame: the bound itself)."""
    b, h, w = (int(v) for v in stack.shape)
    ld = stack.stride(1) if h > 1 else w
    return b, h, w, ld, (stack.stride(0) if b > 1 else (h - 1) * ld + w)


def check_face_frame(face_frame, n):
    """``face_frame`` as the (n,) int32 array the stack entries read: one frame index per face, an integer dtype.  An index the stack does
    not hold is no error here (the face gets ``STATUS_FRAME_RANGE``); one beyond int32 becomes -1."""
    if face_frame is None:
        raise ValueError("face_frame is required: one frame index per face")
    f = np.asarray(face_frame)
    if f.size == 0:
        f = f.astype(np.int64)
    if f.dtype.kind not in "iu" or f.ndim != 1 or f.shape[0] != n:
        raise ValueError("face_frame must be (n,) integers, one frame index per face (n = %d), got dtype %s, shape %s" % (n, f.dtype, f.shape))
    f = (np.minimum(f, np.uint64(1 << 31)) if f.dtype == np.uint64 else f).astype(np.int64)
    return np.ascontiguousarray(np.where((f < -(1 << 31)) | (f >= (1 << 31)), -1, f).astype(np.int32))


def check_grey_list(t, frame_list, what):
    """A list (or tuple) of grey frames of ANY sizes for ``what`` ("normalize_frame_list", "estimate_frame_list"), or ValueError naming the
    frame; None for an empty list.  The rules of ``DeviceCascade._check_list`` for grey frames: every frame an (H, W) uint8 tensor, not
    empty, rows contiguous and ``stride(0) >= W`` (a broadcast view is refused), at most ``HG_MAX_STACK_FRAMES`` frames; the tensors may be
    separate allocations or views of one buffer, and one tensor may be listed twice.  Shapes, dtypes and strides only: the device is
    ``check_list_device``'s, the last refusal before the library."""
    if not isinstance(frame_list, (list, tuple)):
        raise ValueError("%s takes a list or tuple of (H, W) grey uint8 device tensors (a stack of same-size frames goes through the _frames call)" % what)
    if len(frame_list) == 0:
        return None
    if len(frame_list) > _capi.HG_MAX_STACK_FRAMES:
        raise ValueError("%d frames in a list, at most %d" % (len(frame_list), _capi.HG_MAX_STACK_FRAMES))
    for i, f in enumerate(frame_list):
        if not isinstance(f, t.Tensor):
            raise ValueError("frame %d of the list is not a tensor" % i)
        if f.dtype != t.uint8 or f.dim() != 2:
            raise ValueError("frame %d of the list must be (H, W) grey uint8 (a float frame is not offered; a colour frame goes through "
                             "DeviceCascade.prescale_frame_list first)" % i)
        h, w = int(f.shape[0]), int(f.shape[1])
        if h == 0 or w == 0:
            raise ValueError("frame %d of the list is empty" % i)
        if w > 1 and f.stride(1) != 1:
            raise ValueError("frame %d of the list must have contiguous rows, got strides %s" % (i, tuple(f.stride())))
        if h > 1 and f.stride(0) < w:
            raise ValueError("frame %d of the list: rows %d bytes apart hold %d bytes: a broadcast or overlapping view is not a frame" % (i, f.stride(0), w))
    return list(frame_list)


def check_list_device(frame_list, device, what):
    """The last refusal before the library: every frame of the list (None: an empty one) lives on device ``device``."""
    for i, f in enumerate(frame_list or ()):
        if not f.is_cuda:
            raise ValueError("%s takes device tensors (frame %d of the list is on the host)" % (what, i))
        if (f.device.index or 0) != device:
            raise ValueError("frame %d of the list is on %s, not on device %d" % (i, f.device, device))


def list_sizes(frame_list):
    """[(width, height)] of a checked list (None: [])."""
    return [(int(f.shape[1]), int(f.shape[0])) for f in (frame_list or ())]


def list_refs(frame_list):
    """The ``hg_frame_ref`` array of a checked list of grey frames (ld in bytes; one row: the width)."""
    arr = (_capi.HgFrameRef * len(frame_list))()
    for a, f in zip(arr, frame_list):
        h, w = int(f.shape[0]), int(f.shape[1])
        a.frame_dev, a.frame_h, a.frame_w, a.ld = f.data_ptr(), h, w, (f.stride(0) if h > 1 else w)
    return arr


class FaceNormalizer(object):
    """``normalize_image`` for the faces of one frame, on the device.  ``preset``: "age" — (256, 260), areaZ, the crops
    ``estimate_age_race_gender`` makes (face_analysis.py:1172-1179) — or "pose" — (256, 192), area, those of
    ``save_pose_normalized_face_detections`` (:986-995); ``out_size`` / ``method`` override either part.  ``rotate``: True
    "EyeLineRotation", False "noRotation".  ``patcher``: a ``patches.Patcher`` to share (one stream per patcher); None: its own."""

    def __init__(self, device=0, preset="age", out_size=None, method=None, rotate=True, patcher=None):
        from .patches import Patcher
        if preset not in PRESETS:
            raise ValueError("unknown preset %r (one of %s)" % (preset, ", ".join(PRESETS)))
        size, meth = PRESETS[preset]
        self.out_size = tuple(int(v) for v in (out_size if out_size is not None else size))
        self.method = method if method is not None else meth
        self.rotate = bool(rotate)
        _consts(self.out_size, self.method, self.rotate)      # refuses what is not offered now, not at the first frame
        self.device = int(device)
        self._own = patcher is None
        self._patcher = Patcher(self.device) if patcher is None else patcher

    def geometry(self, eyes, frame_size):
        """The records of every face for a frame of ``frame_size`` = (width, height)."""
        return geometry(eyes, frame_size, self.out_size, self.method, self.rotate)

    def normalize(self, frame, eyes=None, geoms=None, out=None, flags=0):
        """``frame``: an (H, W) uint8 device tensor with contiguous rows, any row pitch (a pitched buffer, a crop of a larger frame);
        ``eyes``: (n, 4) in that frame's coordinates (or ``geoms`` from ``geometry`` for that frame size).  Enqueued on the current
        stream of the frame's device, no host wait.  Returns (images, status): images an (n, out_h, out_w) uint8 device tensor (``out``
        if given: that shape, each image contiguous, ``stride(0) >= out_w * out_h``), all zero for a face whose status is not 0; status
        an int32 ndarray (``STATUS``).  ``flags`` is for tests and A/B runs (1: every face staged, 2: every face tap by tap; same bytes)."""
        import torch as t
        from .eyes import check_frame
        if not isinstance(frame, t.Tensor) or not frame.is_cuda:
            raise ValueError("normalize takes a device tensor (normalize_host takes a host array)")
        if frame.dtype != t.uint8:
            raise ValueError("frame must be grey uint8 (a float frame is not offered; a colour frame goes through frames.to_gray first)")
        check_frame(t, frame, frame.device)
        h, w = int(frame.shape[0]), int(frame.shape[1])
        if h == 0 or w == 0:
            raise ValueError("frame must not be empty")
        if (frame.device.index or 0) != self.device:
            raise ValueError("frame is on %s, the normalizer on device %d" % (frame.device, self.device))
        g = self.geometry(eyes, (w, h)) if geoms is None else _check_geoms(geoms)
        n = int(g.shape[0])
        ow, oh = self.out_size
        if out is None:
            out = t.empty((n, oh, ow), dtype=t.uint8, device=frame.device)
        elif (not isinstance(out, t.Tensor) or out.dtype != t.uint8 or out.device != frame.device or tuple(out.shape) != (n, oh, ow)
              or (ow > 1 and out.stride(2) != 1) or (oh > 1 and out.stride(1) != ow) or (n > 1 and out.stride(0) < ow * oh)):
            raise ValueError("out must be a (%d, %d, %d) uint8 tensor on %s whose images are contiguous" % (n, oh, ow, frame.device))
        if n:
            _capi.check(_capi.lib().hg_patcher_normalize_device(
                self._patcher._handle(), int(flags), frame.data_ptr(), h, w, frame.stride(0) if h > 1 else w, g.ctypes.data_as(C.c_void_p), n, ow, oh,
                out.data_ptr(), out.stride(0) if n > 1 else ow * oh, t.cuda.current_stream(frame.device).cuda_stream))
        return out, g["status"].astype(np.int32)

    def normalize_frames(self, stack, eyes=None, face_frame=None, geoms=None, out=None, flags=0):
        """``normalize`` for faces spread over a stack of B same-size frames, ONE call (hg_patcher_normalize_frames_device): ``stack`` a
        (B, H, W) grey uint8 device tensor (``check_grey_stack``; the prescaled stack the rows of ``detect_faces_frames`` refer to is
        ``DeviceCascade.prescale_frames(stack)``), ``eyes`` (n, 4) in the coordinates of each face's own frame (or ``geoms`` from
        ``geometry`` for the frame size), ``face_frame`` (n,) integers: the frame of every face, in any order.  Returns (images, status) as
        ``normalize`` does; face i's image is, byte for byte, ``normalize(stack[face_frame[i]], eyes[i:i + 1])``'s.  A face whose frame
        index is outside [0, B) gets an all-zero image and status ``STATUS_FRAME_RANGE``; it is no error.  An empty stack or n = 0
        touches no library entry."""
        import torch as t
        dev = stack.device if isinstance(stack, t.Tensor) else t.device("cuda", self.device)      # (an empty stack's images live where it does)
        stack = check_grey_stack(t, stack, None, "normalize_frames")      # layout first, then the faces, then the device
        ow, oh = self.out_size
        if geoms is not None:
            g = _check_geoms(geoms)
        else:
            e = _eyes(eyes)
            g = self.geometry(e, (int(stack.shape[2]), int(stack.shape[1]))) if stack is not None and len(e) else np.zeros(len(e), dtype=_capi.NORM_GEOM_DTYPE)
        n = int(g.shape[0])
        ff = check_face_frame(face_frame, n)
        check_stack_device(stack, self.device, "normalize_frames")
        b = 0 if stack is None else int(stack.shape[0])
        status = np.where((ff < 0) | (ff >= b), STATUS_FRAME_RANGE, g["status"]).astype(np.int32)
        if stack is not None:
            dev = stack.device
        if out is None:
            out = t.empty((n, oh, ow), dtype=t.uint8, device=dev) if b else t.zeros((n, oh, ow), dtype=t.uint8, device=dev)
        elif (not isinstance(out, t.Tensor) or out.dtype != t.uint8 or out.device != dev or tuple(out.shape) != (n, oh, ow)
              or (ow > 1 and out.stride(2) != 1) or (oh > 1 and out.stride(1) != ow) or (n > 1 and out.stride(0) < ow * oh)):
            raise ValueError("out must be a (%d, %d, %d) uint8 tensor on %s whose images are contiguous" % (n, oh, ow, dev))
        elif not b:
            out.zero_()
        if n and b:
            b, h, w, ld, stride = stack_layout(stack)
            _capi.check(_capi.lib().hg_patcher_normalize_frames_device(
                self._patcher._handle(), int(flags), stack.data_ptr(), b, stride, h, w, ld, g.ctypes.data_as(C.c_void_p), ff.ctypes.data_as(C.c_void_p), n,
                ow, oh, out.data_ptr(), out.stride(0) if n > 1 else ow * oh, t.cuda.current_stream(stack.device).cuda_stream))
        return out, status

    def list_geometry(self, sizes, eyes, face_frame):
        """The records of faces spread over frames of DIFFERENT sizes: ``sizes`` a list of (width, height), ``face_frame`` (n,) the frame
        of every face, in any order.  Record i is ``geometry(eyes[i], sizes[face_frame[i]])``, computed per frame on the host and
        scattered back into the faces' order; a face whose index lies outside the list gets a zeroed record.  Returns (geoms, face_frame
        as the checked int32 array)."""
        e = _eyes(eyes)
        ff = check_face_frame(face_frame, len(e))
        g = np.zeros(len(e), dtype=_capi.NORM_GEOM_DTYPE)
        for f in np.unique(ff[(ff >= 0) & (ff < len(sizes))]):
            idx = np.flatnonzero(ff == f)
            g[idx] = self.geometry(e[idx], sizes[int(f)])
        return g, ff

    def normalize_frame_list(self, frame_list, eyes=None, face_frame=None, geoms=None, out=None, flags=0):
        """``normalize`` for faces spread over a list of B frames of DIFFERENT sizes, ONE call (hg_patcher_normalize_frame_list_device):
        ``frame_list`` a list of (H, W) grey uint8 device tensors with contiguous rows, any row pitch, separate allocations or views of
        one buffer (``check_grey_list``; the prescaled frames the rows of ``detect_faces_frame_list`` refer to are
        ``DeviceCascade.prescale_frame_list(frame_list)``); ``eyes`` (n, 4) in the coordinates of each face's own frame, ``face_frame``
        (n,) integers: the frame of every face, in any order.  ``geoms`` instead of ``eyes``: taken as given — record i must be
        ``geometry`` for the size of face i's OWN frame (``list_geometry``).  Returns (images, status) as ``normalize_frames`` does, ``out``
        as there; face i's image is, byte for byte, ``normalize(frame_list[face_frame[i]], eyes[i:i + 1])``'s.  A face whose frame index
        is outside [0, B) gets an all-zero image and status ``STATUS_FRAME_RANGE``; it is no error.  Enqueued on the current stream, no
        host wait.  An empty list or n = 0 touches no library entry."""
        import torch as t
        frame_list = check_grey_list(t, frame_list, "normalize_frame_list")      # layout first, then the faces, then the device
        b = 0 if frame_list is None else len(frame_list)
        ow, oh = self.out_size
        if geoms is not None:
            g = _check_geoms(geoms)
            ff = check_face_frame(face_frame, int(g.shape[0]))
        else:
            g, ff = self.list_geometry(list_sizes(frame_list), eyes, face_frame)
        n = int(g.shape[0])
        check_list_device(frame_list, self.device, "normalize_frame_list")
        status = np.where((ff < 0) | (ff >= b), STATUS_FRAME_RANGE, g["status"]).astype(np.int32)
        # (an empty list has no tensor to say where its all-zero images live: where ``out`` does, else on the normalizer's device)
        dev = frame_list[0].device if b else out.device if isinstance(out, t.Tensor) else t.device("cuda", self.device)
        if out is None:
            out = t.empty((n, oh, ow), dtype=t.uint8, device=dev) if b else t.zeros((n, oh, ow), dtype=t.uint8, device=dev)
        elif (not isinstance(out, t.Tensor) or out.dtype != t.uint8 or out.device != dev or tuple(out.shape) != (n, oh, ow)
              or (ow > 1 and out.stride(2) != 1) or (oh > 1 and out.stride(1) != ow) or (n > 1 and out.stride(0) < ow * oh)):
            raise ValueError("out must be a (%d, %d, %d) uint8 tensor on %s whose images are contiguous" % (n, oh, ow, dev))
        elif not b:
            out.zero_()
        if n and b:
            refs = list_refs(frame_list)
            _capi.check(_capi.lib().hg_patcher_normalize_frame_list_device(
                self._patcher._handle(), int(flags), refs, b, g.ctypes.data_as(C.c_void_p), ff.ctypes.data_as(C.c_void_p), n, ow, oh, out.data_ptr(),
                out.stride(0) if n > 1 else ow * oh, t.cuda.current_stream(dev).cuda_stream))
        return out, status

    def close(self):
        """Frees the patcher it owns; the caller makes sure the device has finished with it (as for ``Patcher.close``)."""
        if self._own and self._patcher is not None:
            self._patcher.close()
        self._patcher = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
