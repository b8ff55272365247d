"""Colour frames shared by tests/test_color_frames_host.py and tests/test_color_frames_gpu.py, and PIL's ``convert("L")`` called here
as the reference: RGB / RGBA frames directly, BGR / BGRA frames on the channel-swapped array."""
import numpy as np

COLOR_FORMATS = ("RGB", "BGR", "RGBA", "BGRA")
BPP = {"L": 1, "RGB": 3, "BGR": 3, "RGBA": 4, "BGRA": 4}
SWAPPED = {"RGB": False, "BGR": True, "RGBA": False, "BGRA": True}


def pil_gray(arr, fmt):
    """PIL's grey of an (H, W, C) frame of format ``fmt``."""
    from PIL import Image
    a = np.ascontiguousarray(arr)
    if SWAPPED[fmt]:
        a = a.copy()
        a[..., 0], a[..., 2] = arr[..., 2], arr[..., 0]
    return np.array(Image.fromarray(a, "RGB" if a.shape[2] == 3 else "RGBA").convert("L"))


def as_format(rgb, fmt, seed=0):
    """An (H, W, 3) RGB array as a frame of ``fmt``: channels swapped for BGR / BGRA, a seeded noise byte as the fourth channel."""
    out = rgb[..., ::-1] if SWAPPED[fmt] else rgb
    if BPP[fmt] == 4:
        x = np.random.default_rng(7300 + seed).integers(0, 256, rgb.shape[:2] + (1,), dtype=np.uint8)
        out = np.concatenate([out, x], axis=2)
    return np.ascontiguousarray(out)


def noise_frame(h, w, fmt, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, BPP[fmt]), dtype=np.uint8)


_ALL = {}


def all_colors():
    """(rgb, grey): the 4096 x 4096 RGB frame that holds every 24-bit colour once and PIL's grey of it, made once (read only)."""
    if not _ALL:
        from PIL import Image
        idx = np.arange(1 << 24, dtype=np.uint32).reshape(4096, 4096)
        rgb = np.stack([idx & 255, (idx >> 8) & 255, idx >> 16], axis=2).astype(np.uint8)
        assert len(np.unique(idx)) == 1 << 24
        _ALL["rgb"], _ALL["gray"] = rgb, np.asarray(Image.fromarray(rgb, "RGB").convert("L"))
    return _ALL["rgb"], _ALL["gray"]


def color_twin(gray, seed):
    """(rgb, fell_back): an RGB frame that PIL converts to ``gray``.  R and B are the grey value plus seeded offsets in [-60, 60],
    clipped; G is the smallest value for which L = (R*19595 + G*38470 + B*7471 + 0x8000) >> 16 gives the grey value; a pixel that has
    no such G is (g, g, g)."""
    g = gray.astype(np.int64)
    off = np.random.default_rng(seed).integers(-60, 61, gray.shape + (2,))
    r, b = np.clip(g + off[..., 0], 0, 255), np.clip(g + off[..., 1], 0, 255)
    base = r * 19595 + b * 7471 + 0x8000
    gg = np.maximum((g << 16) - base + 38469, 0) // 38470                  # smallest G with base + G*38470 >= g << 16
    ok = (gg <= 255) & (((base + gg * 38470) >> 16) == g)
    rgb = np.where(ok[..., None], np.stack([r, gg, b], axis=2), g[..., None]).astype(np.uint8)
    return rgb, ~ok


# ---- layouts of a colour frame inside a larger byte buffer ---------------------------------------------------------------------------
COLOR_LAYOUTS = ("dense", "pad1", "roi")


def color_layout_geometry(name, h, w, bpp):
    """(buffer rows, row stride in bytes, first row, first byte in the row) of a layout whose view is the frame."""
    if name == "dense":
        return h, w * bpp, 0, 0
    if name == "pad1":                               # rows one byte further apart than they are long: rows at every byte alignment
        return h, w * bpp + 1, 0, 0
    if name == "roi":                                # a crop of a larger colour frame: 3 rows and 13 pixels in, foreign pixels on all sides
        return h + 5, (w + 24) * bpp, 3, 13 * bpp
    raise KeyError(name)


def host_color_layout(arr, name, seed):
    """(byte buffer (rows, ld_bytes), byte offset of the frame): the buffer is seeded noise and holds ``arr`` at the layout's place."""
    h, w, bpp = arr.shape
    rows, ldb, y0, xb = color_layout_geometry(name, h, w, bpp)
    buf = np.random.default_rng(seed).integers(1, 256, (rows, ldb)).astype(np.uint8)
    buf[y0:y0 + h, xb:xb + w * bpp] = arr.reshape(h, w * bpp)
    return buf, y0 * ldb + xb


class ColorLayout(object):
    """A colour frame on the device inside a layout's buffer: ``view`` is the (H, W, C) tensor handed to the code under test."""

    def __init__(self, arr, name, seed=9201):
        import torch
        self.name, self.arr = name, arr
        self.buf, off = host_color_layout(arr, name, seed)
        self.dev = torch.from_numpy(self.buf).cuda()
        h, w, bpp = arr.shape
        self.ld_bytes = self.buf.shape[1]
        self.view = torch.as_strided(self.dev, (h, w, bpp), (self.ld_bytes, bpp, 1), off)
        assert np.array_equal(self.view.cpu().numpy(), arr)

    def assert_untouched(self):
        assert np.array_equal(self.dev.cpu().numpy(), self.buf), (self.name, "the source buffer changed")

    def __repr__(self):
        return self.name
