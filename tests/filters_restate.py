"""numpy restatement of the BILINEAR / BICUBIC window rule (include/higsfa.h, hg_patcher_extract_filter_device): PIL's
ImagingGenericTransform with affine_transform and bilinear_filter8 / bicubic_filter8 (Geometry.c) for mode "L" images, every operation
in float64 and rounded on its own, and the matrix ``Image.rotate`` builds.  tests/test_filters_host.py pins it to PIL itself; the GPU
tests use it where an expectation is composed from several steps (eye patches)."""
import math

import numpy as np

BILINEAR, BICUBIC = 2, 3


def _bicubic(v1, v2, v3, v4, d):
    p1 = v2
    p2 = -v1 + v3
    p3 = 2 * (v1 - v2) + v3 - v4
    p4 = -v1 + v2 - v3 + v4
    return p1 + d * (p2 + d * (p3 + d * p4))


def affine(img, a, size, filt):
    """``Image.fromarray(img).transform(size, AFFINE, a, filt)`` for a (H, W) uint8 array: (h, w) uint8."""
    if filt not in (BILINEAR, BICUBIC):
        raise ValueError("filter %r is not restated here" % (filt,))
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim == 2
    H, W = img.shape
    w, h = size
    f = img.astype(np.float64)
    xin = (np.arange(w) + 0.5)[None, :]
    yin = (np.arange(h) + 0.5)[:, None]
    xs = a[0] * xin + a[1] * yin + a[2]
    ys = a[3] * xin + a[4] * yin + a[5]
    outside = (xs < 0) | (xs >= W) | (ys < 0) | (ys >= H)
    xs = np.where(outside, 0.5, xs) - 0.5
    ys = np.where(outside, 0.5, ys) - 0.5
    x, y = np.floor(xs).astype(np.int64), np.floor(ys).astype(np.int64)
    dx, dy = xs - x, ys - y
    cx = lambda v: np.clip(v, 0, W - 1)
    cy = lambda v: np.clip(v, 0, H - 1)
    if filt == BILINEAR:
        x0, x1 = cx(x), cx(x + 1)
        row = lambda yy: f[yy, x0] + (f[yy, x1] - f[yy, x0]) * dx
        v1 = row(cy(y))
        v2 = np.where(y + 1 < H, row(cy(y + 1)), v1)
        out = np.trunc(v1 + (v2 - v1) * dy)
    else:
        x0, x1, x2, x3 = cx(x - 1), cx(x), cx(x + 1), cx(x + 2)
        row = lambda yy: _bicubic(f[yy, x0], f[yy, x1], f[yy, x2], f[yy, x3], dx)
        r1 = row(cy(y - 1))
        r2 = np.where((y >= 0) & (y < H), row(cy(y)), r1)
        r3 = np.where((y + 1 >= 0) & (y + 1 < H), row(cy(y + 1)), r2)
        r4 = np.where((y + 2 >= 0) & (y + 2 < H), row(cy(y + 2)), r3)
        v = _bicubic(r1, r2, r3, r4, dy)
        out = np.where(v <= 0, 0.0, np.where(v >= 255, 255.0, np.trunc(v)))
    out = np.where(outside, 0.0, out)
    return out.astype(np.uint8)


def extent(img, box, size, filt):
    """``transform(size, EXTENT, box, filt)``."""
    x0, y0, x1, y1 = (float(v) for v in box)
    w, h = size
    return affine(img, ((x1 - x0) / w, 0.0, x0, 0.0, (y1 - y0) / h, y0), size, filt)


def rotate_matrix(angle, center):
    """The matrix of ``Image.rotate(angle, center=center)`` (no expand, no translate)."""
    angle = -math.radians(angle % 360.0)
    m = [round(math.cos(angle), 15), round(math.sin(angle), 15), 0.0, round(-math.sin(angle), 15), round(math.cos(angle), 15), 0.0]
    x, y = -center[0], -center[1]
    m[2], m[5] = m[0] * x + m[1] * y + m[2], m[3] * x + m[4] * y + m[5]
    m[2] += center[0]
    m[5] += center[1]
    return m


def rotate(img, angle, center, filt):
    """``Image.rotate(angle, filt, center=center)``: same size as the frame, 0 where the rotation reads outside it."""
    return affine(img, rotate_matrix(angle, center), (img.shape[1], img.shape[0]), filt)


def window(img, box, delta_ang, size, filt):
    """One window by the build's composition: the frame rotated about the box centre with ``filt``, then the EXTENT cut with ``filt``;
    ``delta_ang % 360 == 0``: the cut from the frame itself.  Flat (w * h) uint8."""
    if float(delta_ang) % 360.0 != 0.0:
        b = [float(v) for v in box]
        img = rotate(img, float(delta_ang), ((b[0] + b[2]) / 2.0, (b[1] + b[3]) / 2.0), filt)
    return extent(img, box, size, filt).reshape(-1)


def windows(img, boxes, delta_angs, size, filt):
    return np.stack([window(img, b, a, size, filt) for b, a in zip(boxes, delta_angs)]) if len(boxes) else np.zeros((0, size[0] * size[1]), np.uint8)
