"""Shapes, frames and PIL's ``Image.resize`` called as the reference, shared by tests/test_resample_host.py and tests/test_resample_gpu.py.
A shape is (w, h, out_w, out_h), PIL's order."""
import numpy as np

from tests import color_cases as CC

FILTERS = ("BOX", "BILINEAR", "HAMMING", "BICUBIC", "LANCZOS")
CODES = {"NEAREST": 0, "LANCZOS": 1, "BILINEAR": 2, "BICUBIC": 3, "BOX": 4, "HAMMING": 5}      # PIL's own (Image.Resampling)
SHAPES = [
    (37, 23, 16, 9),
    (64, 48, 33, 48),          # no vertical pass
    (50, 40, 50, 17),          # no horizontal pass
    (19, 31, 40, 50),          # upscale: the filter is not stretched
    (200, 113, 104, 58),
    (129, 7, 3, 5),
    (5, 5, 1, 1),
    (300, 2, 77, 2),
    (480, 270, 250, 140),
]
# the device kernels' edges: one column and one row past a 64 x 16 tile (the fused kernel's tile, hg_resample.hip); a source narrower than
# 8 bytes; an output width that is not a multiple of 4 (written with an odd destination stride by the test)
GPU_SHAPES = SHAPES + [(130, 70, 65, 17), (5, 9, 3, 4), (90, 61, 43, 29)]
WIDE_KERNEL = (300, 40, 7, 40)      # LANCZOS: ksize 261
# Image.resize resizes the height of a very tall image first (h > 100 w and the height shrinks): another intermediate, other bytes;
# and a shape just as steep that does not meet that rule (on the device: 480 intermediate rows per tile, two launches)
TALL, STEEP = (8, 3000, 4, 100), (40, 3000, 20, 100)
KINDS = ("noise", "binary")


def gray_frame(w, h, kind, seed=0):
    a = np.random.default_rng(9000 + seed + 7 * w + 13 * h).integers(0, 256, (h, w), dtype=np.uint8)
    return a if kind == "noise" else ((a > 127) * np.uint8(255)).astype(np.uint8)


def color_frame(w, h, fmt, seed=0):
    return CC.noise_frame(h, w, fmt, 9100 + seed + 7 * w + 13 * h)


def pil_resize(arr, size, filt):
    """PIL's resize of a grey (H, W) or colour (H, W, 3 as "RGB" / 4 as "RGBX") uint8 array; ``size`` = (w, h)."""
    from PIL import Image
    a = np.ascontiguousarray(arr)
    if a.ndim == 2:
        im = Image.fromarray(a, "L")
    elif a.shape[2] == 3:
        im = Image.fromarray(a, "RGB")
    else:
        im = Image.frombuffer("RGBX", (a.shape[1], a.shape[0]), a.tobytes(), "raw", "RGBX", 0, 1)
    return np.asarray(im.resize(tuple(size), CODES[filt]))


def pil_gray_resize(arr, fmt, size, filt):
    """``convert("L")`` first, then the resize: the reference's order (FaceDetectUpdated.py:543, :556)."""
    return pil_resize(CC.pil_gray(arr, fmt), size, filt)
