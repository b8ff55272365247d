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
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _capi

FORMATS = {"L": _capi.HG_FRAME_L, "RGB": _capi.HG_FRAME_RGB, "BGR": _capi.HG_FRAME_BGR, "RGBA": _capi.HG_FRAME_RGBA, "BGRA": _capi.HG_FRAME_BGRA}
CHANNELS = {_capi.HG_FRAME_L: 1, _capi.HG_FRAME_RGB: 3, _capi.HG_FRAME_BGR: 3, _capi.HG_FRAME_RGBA: 4, _capi.HG_FRAME_BGRA: 4}


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
