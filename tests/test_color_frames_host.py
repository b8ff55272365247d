"""CPU: PIL's "L" conversion on the host (hg_frame_to_gray_host, frames.to_gray_host) against ``Image.convert("L")`` called here —
every 24-bit colour, the four colour formats on pitched sources and outputs, ``array_equal`` throughout — the refusals of the entry,
and the format table and the frame checker of pyfaceanalysis_amd/frames.py as far as they can be reached without a device."""
import ctypes as C

import numpy as np
import pytest

from pyfaceanalysis_amd import _capi, frames
from tests import color_cases as CC


def vp(a):
    return a.ctypes.data_as(C.c_void_p)


def test_every_color_on_the_host(native_lib):
    rgb, want = CC.all_colors()
    got = np.zeros((4096, 4096), dtype=np.uint8)
    assert native_lib.hg_frame_to_gray_host(vp(rgb), _capi.HG_FRAME_RGB, 4096, 4096, 4096 * 3, vp(got), 4096) == _capi.HG_OK
    assert np.array_equal(got, want)
    assert np.array_equal(frames.to_gray_host(rgb, "RGB"), want)
    # the rule itself, as the header states it
    r, g, b = (rgb[..., i].astype(np.uint32) for i in range(3))
    assert np.array_equal(want, ((r * 19595 + g * 38470 + b * 7471 + 0x8000) >> 16).astype(np.uint8))


@pytest.mark.parametrize("fmt", ("BGR", "RGBA", "BGRA", "RGB"))
def test_formats_on_pitched_buffers(native_lib, fmt):
    h, w, bpp = 64, 67, CC.BPP[fmt]
    arr = CC.noise_frame(h, w, fmt, 7101)
    want = CC.pil_gray(arr, fmt)
    ldb = w * bpp + 1 if (w * bpp) % 2 == 0 else w * bpp + 2      # odd: rows at every byte alignment
    assert ldb % 2 == 1
    src = np.random.default_rng(7102).integers(1, 256, (h, ldb)).astype(np.uint8)
    src[:, :w * bpp] = arr.reshape(h, w * bpp)
    before = src.copy()
    dst = np.full((h, w + 1), 7, dtype=np.uint8)
    assert native_lib.hg_frame_to_gray_host(vp(src), frames.FORMATS[fmt], h, w, ldb, vp(dst), w + 1) == _capi.HG_OK
    assert np.array_equal(dst[:, :w], want) and np.all(dst[:, w] == 7)
    assert np.array_equal(src, before)
    assert np.array_equal(frames.to_gray_host(arr, fmt), want)
    # a view that is not packed (every other column) goes through a dense copy
    assert np.array_equal(frames.to_gray_host(arr[:, ::2], fmt), want[:, ::2])
    if bpp == 4:      # the fourth byte is ignored
        other = arr.copy()
        other[..., 3] ^= 0xff
        assert np.array_equal(frames.to_gray_host(other, fmt), want)
    assert not np.array_equal(CC.pil_gray(arr[..., [2, 1, 0] + [3] * (bpp - 3)], fmt), want)      # the channel order matters on this frame


def test_gray_format_is_a_pitched_copy(native_lib):
    g = np.random.default_rng(7103).integers(0, 256, (9, 13), dtype=np.uint8)
    wide = np.full((9, 20), 3, dtype=np.uint8)
    wide[:, :13] = g
    dst = np.full((9, 14), 7, dtype=np.uint8)
    assert native_lib.hg_frame_to_gray_host(vp(wide), _capi.HG_FRAME_L, 9, 13, 20, vp(dst), 14) == _capi.HG_OK
    assert np.array_equal(dst[:, :13], g) and np.all(dst[:, 13] == 7)
    assert np.array_equal(frames.to_gray_host(g, "L"), g)


def test_refusals_leave_the_output_alone(native_lib):
    L = native_lib
    h, w = 5, 6
    arr = CC.noise_frame(h, w, "RGB", 7104)
    want = CC.pil_gray(arr, "RGB")
    dst = np.full((h, w), 9, dtype=np.uint8)
    RGB, RGBA = _capi.HG_FRAME_RGB, _capi.HG_FRAME_RGBA
    bad = [
        (vp(arr), 5, h, w, w * 3, vp(dst), w),           # unknown formats
        (vp(arr), -1, h, w, w * 3, vp(dst), w),
        (vp(arr), RGB, h, w, w * 3 - 1, vp(dst), w),     # row stride below the row's bytes
        (vp(arr), RGBA, h, w, w * 3, vp(dst), w),        # ... of a four-byte format
        (vp(arr), RGB, h, w, 0, vp(dst), w),
        (vp(arr), RGB, h, w, w * 3, vp(dst), w - 1),     # output rows overlap
        (None, RGB, h, w, w * 3, vp(dst), w),            # null pointers
        (vp(arr), RGB, h, w, w * 3, None, w),
        (vp(arr), RGB, 0, w, w * 3, vp(dst), w),         # empty and negative sizes
        (vp(arr), RGB, h, -1, w * 3, vp(dst), w),
    ]
    for args in bad:
        assert L.hg_frame_to_gray_host(*args) == _capi.HG_ERR_ARG, args[1:5]
        assert L.hg_last_error() and np.all(dst == 9)
        assert L.hg_frame_to_gray_host(vp(arr), RGB, h, w, w * 3, vp(dst), w) == _capi.HG_OK and np.array_equal(dst, want)
        dst[:] = 9
    for a, fmt in ((arr, "L"), (arr[..., 0], "RGB"), (arr, "RGBA"), (arr.astype(np.float32), "RGB")):
        with pytest.raises(ValueError):
            frames.to_gray_host(a, fmt)


def test_format_table():
    assert frames.FORMATS == {"L": 0, "RGB": 1, "BGR": 2, "RGBA": 3, "BGRA": 4}
    assert (_capi.HG_FRAME_L, _capi.HG_FRAME_RGB, _capi.HG_FRAME_BGR, _capi.HG_FRAME_RGBA, _capi.HG_FRAME_BGRA) == (0, 1, 2, 3, 4)
    assert [frames.CHANNELS[frames.FORMATS[n]] for n in ("L", "RGB", "BGR", "RGBA", "BGRA")] == [1, 3, 3, 4, 4]
    for name, code in frames.FORMATS.items():
        assert frames.format_code(name) == code and frames.format_code(code) == code
    for bad in ("rgb", "YUV", 5, -1, True, 1.0, None):
        with pytest.raises(ValueError):
            frames.format_code(bad)
    # the header's table is this one
    import os
    import re
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "higsfa.h")).read()
    assert {m[0]: int(m[1]) for m in re.findall(r"#define HG_FRAME_([A-Z]+)\s+(\d+)", text)} == frames.FORMATS


def test_frame_checker_without_a_device():
    import torch
    cpu = torch.device("cpu")
    rgb = torch.zeros((6, 8, 3), dtype=torch.uint8)
    rgba = torch.zeros((6, 8, 4), dtype=torch.uint8)
    gray = torch.zeros((6, 8), dtype=torch.uint8)
    assert frames.check_color_frame(torch, rgb, "RGB", cpu) == 1 and frames.check_color_frame(torch, rgb, "BGR", cpu) == 2
    assert frames.check_color_frame(torch, rgba, "RGBA", cpu) == 3 and frames.check_color_frame(torch, rgba, 4, cpu) == 4
    assert frames.check_color_frame(torch, gray, "L", cpu) == 0
    assert frames.check_color_frame(torch, rgba[1:5, 2:7], "BGRA", cpu) == 4              # a crop of a larger frame is a frame
    refused = [
        (rgb, "L"),                          # a 3-d frame as grey
        (gray, "RGB"),                       # a 2-d frame as colour
        (rgb, "RGBA"), (rgba, "BGR"),        # wrong channel count
        (rgba[..., :3], "RGB"),              # pixels not packed: four bytes apart
        (rgb[:, ::2], "RGB"),                # every other pixel
        (rgb.permute(1, 0, 2), "RGB"),       # transposed: rows closer than a row's bytes
        (rgb.to(torch.float32), "RGB"),
        (rgb.numpy(), "RGB"),                # not a tensor
        (rgb, "XYZ"),
    ]
    for frame, fmt in refused:
        with pytest.raises(ValueError):
            frames.check_color_frame(torch, frame, fmt, cpu)
    with pytest.raises(ValueError):
        frames.check_color_frame(torch, rgb, "RGB", torch.device("cuda", 0))           # on another device
    with pytest.raises(ValueError):
        frames.to_gray(rgb, "RGB")                                                      # the device entry takes device tensors
    from pyfaceanalysis_amd.cascade import DeviceCascade
    with pytest.raises(ValueError):
        DeviceCascade([], (16, 16), 10, frame_format="XYZ")
    assert DeviceCascade([], (16, 16), 10, frame_format="BGRA").frame_format == 4 and DeviceCascade([], (16, 16), 10).frame_format == 0


def test_color_twin_construction():
    """The twin the GPU tests feed the cascade (tests/color_cases.py): PIL converts it back to the grey frame, few pixels fell back to
    (g, g, g), and a swap of R and B changes PIL's grey for most pixels — a wrong channel order cannot pass for the right one."""
    gray = np.random.default_rng(28).integers(0, 256, (120, 160), dtype=np.uint8)       # the 160 x 120 frame of tests/test_filters_gpu.py
    rgb, fell_back = CC.color_twin(gray, 2801)
    assert np.array_equal(CC.pil_gray(rgb, "RGB"), gray)
    assert fell_back.mean() <= 0.10
    assert (CC.pil_gray(rgb, "BGR") != gray).mean() >= 0.50
