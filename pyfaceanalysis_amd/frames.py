"""Frame formats: packed colour frames and PIL's "L" conversion, on the device and on the host.

A camera or a video decoder delivers packed colour pixels; the reference converts them before anything else
(``images = [im.convert("L")]``, FaceDetectUpdated.py:541-543; its file branch loads with ``image_format="L"``, :533).  PIL's rule is
integer and per pixel,

    L = (R * 19595 + G * 38470 + B * 7471 + 0x8000) >> 16

and the fourth byte of RGBA / RGBX is ignored; ``to_gray`` (hg_frame_to_gray_device) and ``to_gray_host`` (hg_frame_to_gray_host) give
PIL's bytes, every 24-bit colour included (tests/test_color_frames_*.py).  A colour frame is an (H, W, C) uint8 tensor whose pixels
are packed (``stride(2) == 1``, ``stride(1) == C``) and whose rows are at least W * C bytes apart — a crop of a larger frame is one;
a grey frame is the (H, W) uint8 tensor with contiguous rows every entry has always read.  ``DeviceCascade(frame_format=...)``,
``FaceTracker`` and ``EyeLocator.locate(frame_format=...)`` take colour frames directly.

``resize`` / ``resize_host`` are Pillow's ``Image.resize((w, h), filter)`` for these frames (hg_patcher_resize_device,
hg_frame_resize_host; include/higsfa.h): the antialiased alternative to the NEAREST prescale.  Their filters (``RESAMPLE``) carry PIL's
codes like the window filters do, but name another operation — ``Image.resize`` is a separable convolution whose support grows with the
shrink factor, ``Image.transform(EXTENT, filter)`` samples a fixed neighbourhood.  ``DeviceCascade(prescale_filter=...)`` puts one in
front of every frame path.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _capi

FORMATS = {"L": _capi.HG_FRAME_L, "RGB": _capi.HG_FRAME_RGB, "BGR": _capi.HG_FRAME_BGR, "RGBA": _capi.HG_FRAME_RGBA, "BGRA": _capi.HG_FRAME_BGRA}
CHANNELS = {_capi.HG_FRAME_L: 1, _capi.HG_FRAME_RGB: 3, _capi.HG_FRAME_BGR: 3, _capi.HG_FRAME_RGBA: 4, _capi.HG_FRAME_BGRA: 4}
# enum hg_resample: the filters of Image.resize (PIL's own codes; Image.Resampling members pass as ints)
RESAMPLE = {"NEAREST": _capi.HG_RESAMPLE_NEAREST, "LANCZOS": _capi.HG_RESAMPLE_LANCZOS, "BILINEAR": _capi.HG_RESAMPLE_BILINEAR,
            "BICUBIC": _capi.HG_RESAMPLE_BICUBIC, "BOX": _capi.HG_RESAMPLE_BOX, "HAMMING": _capi.HG_RESAMPLE_HAMMING}
RESAMPLE_NAMES = {v: k for k, v in RESAMPLE.items()}


def resample_code(f):
    """A resize filter name ("NEAREST", "LANCZOS", "BILINEAR", "BICUBIC", "BOX", "HAMMING") or PIL's code -> enum hg_resample."""
    if isinstance(f, str):
        if f.upper() not in RESAMPLE:
            raise ValueError("unknown resize filter %r (one of %s)" % (f, ", ".join(RESAMPLE)))
        return RESAMPLE[f.upper()]
    if isinstance(f, (bool, float)) or not isinstance(f, (int, np.integer)) or int(f) not in RESAMPLE_NAMES:
        raise ValueError("unknown resize filter %r (one of %s)" % (f, ", ".join(RESAMPLE)))
    return int(f)


def format_code(frame_format):
    """A format name ("L", "RGB", "BGR", "RGBA", "BGRA"; RGBX / BGRX frames pass as RGBA / BGRA) or an HG_FRAME_* code -> the code."""
    if isinstance(frame_format, str):
        if frame_format not in FORMATS:
            raise ValueError("unknown frame format %r (one of %s)" % (frame_format, ", ".join(FORMATS)))
        return FORMATS[frame_format]
    if isinstance(frame_format, bool) or not isinstance(frame_format, (int, np.integer)) or int(frame_format) not in CHANNELS:
        raise ValueError("unknown frame format %r (one of %s)" % (frame_format, ", ".join(FORMATS)))
    return int(frame_format)


def check_color_frame(t, frame, frame_format, dev):
    """``frame`` is a frame of ``frame_format`` on ``dev`` (a torch.device; ``t`` the torch module) or ValueError.  Returns the format's
    code.  "L": what ``eyes.check_frame`` accepts; a colour format: (H, W, C) uint8, C the format's, packed pixels, rows >= W * C apart."""
    code = format_code(frame_format)
    if code == _capi.HG_FRAME_L:
        from .eyes import check_frame
        check_frame(t, frame, dev)
        return code
    c = CHANNELS[code]
    if not isinstance(frame, t.Tensor) or frame.dim() != 3 or frame.dtype != t.uint8 or frame.device != dev:
        raise ValueError("a colour frame must be a 3-d (H, W, %d) uint8 tensor on %s" % (c, dev))
    if frame.shape[2] != c:
        raise ValueError("frame has %d channels, the format has %d" % (frame.shape[2], c))
    if frame.stride(2) != 1 or frame.stride(1) != c or frame.stride(0) < frame.shape[1] * c:
        raise ValueError("a colour frame must have packed pixels (strides (>= W * %d, %d, 1)), got %s" % (c, c, tuple(frame.stride())))
    return code


def to_gray(frame, frame_format, out=None):
    """PIL's ``convert("L")`` of a device frame (hg_frame_to_gray_device), enqueued on the current stream of its device.  ``out``: an
    (H, W) uint8 tensor on the same device with contiguous rows (a view of a larger buffer is fine) that does not overlap ``frame``;
    None: a new dense tensor.  "L" copies the frame.  Returns ``out``."""
    import torch as t
    if not isinstance(frame, t.Tensor) or not frame.is_cuda:
        raise ValueError("to_gray takes a device tensor (to_gray_host converts a host array)")
    code = check_color_frame(t, frame, frame_format, frame.device)
    h, w = int(frame.shape[0]), int(frame.shape[1])
    if out is None:
        out = t.empty((h, w), dtype=t.uint8, device=frame.device)
    elif (not isinstance(out, t.Tensor) or out.dim() != 2 or out.dtype != t.uint8 or out.device != frame.device or tuple(out.shape) != (h, w)
          or (w > 1 and out.stride(1) != 1) or (h > 1 and out.stride(0) < w)):
        raise ValueError("out must be a (%d, %d) uint8 tensor on %s with contiguous rows" % (h, w, frame.device))
    if h == 0 or w == 0:
        return out
    _capi.check(_capi.lib().hg_frame_to_gray_device(frame.device.index or 0, frame.data_ptr(), code, h, w, frame.stride(0), out.data_ptr(),
                                                    out.stride(0) if h > 1 else w, t.cuda.current_stream(frame.device).cuda_stream))
    return out


def to_gray_host(frame, frame_format):
    """The same conversion of a host array (hg_frame_to_gray_host: plain C++, no device): (H, W, C) uint8 -> (H, W) uint8; "L": a copy
    of the (H, W) array."""
    code = format_code(frame_format)
    c = CHANNELS[code]
    a = np.asarray(frame)
    if a.dtype != np.uint8 or a.ndim != (2 if code == _capi.HG_FRAME_L else 3) or (a.ndim == 3 and a.shape[2] != c):
        raise ValueError("frame must be a uint8 array of shape %s" % ("(H, W)" if code == _capi.HG_FRAME_L else "(H, W, %d)" % c))
    h, w = a.shape[:2]
    packed = a.strides[1] == c and (a.ndim == 2 or a.strides[2] == 1) and a.strides[0] >= w * c
    if not packed:
        a = np.ascontiguousarray(a)
    out = np.empty((h, w), dtype=np.uint8)
    if h and w:
        _capi.check(_capi.lib().hg_frame_to_gray_host(a.ctypes.data_as(C.c_void_p), code, h, w, a.strides[0], out.ctypes.data_as(C.c_void_p), w))
    return out


def _out_format(code, out_format):
    oc = format_code(out_format or "L")
    if oc != _capi.HG_FRAME_L and oc != code:
        raise ValueError("out_format is \"L\" or the frame's own format")
    return oc


def resize(frame, size, filter="BILINEAR", frame_format="L", out_format=None, out=None, patcher=None, flags=0):
    """Pillow's ``Image.resize(size, filter)`` of a device frame (hg_patcher_resize_device), enqueued on the current stream of its device:
    bit for bit PIL's bytes (tests/test_resample_gpu.py).  ``size``: (width, height), PIL's order.  ``out_format``: None / "L" — a grey
    (H, W) image, a colour frame converted as ``convert("L")`` first (the reference's order) — or the frame's own colour format — an
    (H, W, C) image resampled band by band (four-byte formats as RGBX: all four bytes).  "NEAREST" with grey output is the cascade's
    NEAREST prescale; with colour output it is refused.  ``out``: a tensor of that shape on the same device with packed pixels and rows
    at least a row's bytes apart, not overlapping ``frame``; None: a new dense tensor.  ``patcher``: the ``patches.Patcher`` that keeps
    the tables and the intermediate image between calls (one stream per patcher); None: a temporary one, freed after the device has
    finished.  ``flags`` is for tests and A/B runs only (1: two launches, 2: one launch where eligible; same bytes).  Returns ``out``."""
    import torch as t
    from .patches import Patcher
    if not isinstance(frame, t.Tensor) or not frame.is_cuda:
        raise ValueError("resize takes a device tensor (resize_host resizes a host array)")
    code = check_color_frame(t, frame, frame_format, frame.device)
    oc = _out_format(code, out_format)
    fcode = resample_code(filter)
    ow, oh = int(size[0]), int(size[1])
    if ow <= 0 or oh <= 0 or frame.shape[0] == 0 or frame.shape[1] == 0:
        raise ValueError("resize: sizes must be positive")
    h, w = int(frame.shape[0]), int(frame.shape[1])
    c = CHANNELS[oc]
    shape = (oh, ow) if oc == _capi.HG_FRAME_L else (oh, ow, c)
    if out is None:
        out = t.empty(shape, dtype=t.uint8, device=frame.device)
    elif (not isinstance(out, t.Tensor) or out.dtype != t.uint8 or out.device != frame.device or tuple(out.shape) != shape
          or (out.dim() == 3 and (out.stride(2) != 1 or out.stride(1) != c)) or (out.dim() == 2 and ow > 1 and out.stride(1) != 1)
          or (oh > 1 and out.stride(0) < ow * c)):
        raise ValueError("out must be a %s uint8 tensor on %s with packed pixels" % (shape, frame.device))
    own = patcher is None
    if own:
        patcher = Patcher(frame.device.index or 0)
    try:
        _capi.check(_capi.lib().hg_patcher_resize_device(
            patcher._handle(), fcode, int(flags), frame.data_ptr(), code, h, w, frame.stride(0) if h > 1 else w * CHANNELS[code], oc, out.data_ptr(), oh, ow,
            out.stride(0) if oh > 1 else ow * c, t.cuda.current_stream(frame.device).cuda_stream))
    finally:
        if own:
            t.cuda.current_stream(frame.device).synchronize()
            patcher.close()
    return out


def resize_host(frame, size, filter="BILINEAR", frame_format="L", out_format=None):
    """The same rule on a host array (hg_frame_resize_host: plain C++, no device): (H, W) or (H, W, C) uint8 -> (h, w) or (h, w, C)."""
    code = format_code(frame_format)
    oc = _out_format(code, out_format)
    fcode = resample_code(filter)
    c = CHANNELS[code]
    a = np.asarray(frame)
    if a.dtype != np.uint8 or a.ndim != (2 if code == _capi.HG_FRAME_L else 3) or (a.ndim == 3 and a.shape[2] != c):
        raise ValueError("frame must be a uint8 array of shape %s" % ("(H, W)" if code == _capi.HG_FRAME_L else "(H, W, %d)" % c))
    h, w = a.shape[:2]
    ow, oh = int(size[0]), int(size[1])
    if ow <= 0 or oh <= 0 or h == 0 or w == 0:
        raise ValueError("resize: sizes must be positive")
    packed = a.strides[1] == c and (a.ndim == 2 or a.strides[2] == 1) and a.strides[0] >= w * c
    if not packed:
        a = np.ascontiguousarray(a)
    oc_n = CHANNELS[oc]
    out = np.empty((oh, ow) if oc == _capi.HG_FRAME_L else (oh, ow, oc_n), dtype=np.uint8)
    _capi.check(_capi.lib().hg_frame_resize_host(fcode, a.ctypes.data_as(C.c_void_p), code, h, w, a.strides[0], oc, out.ctypes.data_as(C.c_void_p), oh, ow,
                                                 ow * oc_n))
    return out
