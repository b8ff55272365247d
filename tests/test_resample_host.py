"""CPU: PIL's ``Image.resize`` with a filter on the host (hg_frame_resize_host, csrc/hg_resample.cpp) against PIL called here,
``array_equal``: five filters, noise and 0 / 255 images, grey and colour sources, grey and colour output, pitched buffers, and what the
entry refuses.  The stand-alone driver tests/resample_driver.cpp runs the same unit under AddressSanitizer and UBSan as a program."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from pyfaceanalysis_amd import _capi, build, frames
from tests import color_cases as CC
from tests import resample_cases as RC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("shape", RC.SHAPES + [RC.TALL, RC.STEEP], ids=lambda s: "%dx%d-%dx%d" % s)
def test_gray_equals_pil(native_lib, shape):
    w, h, ow, oh = shape
    for kind in RC.KINDS:
        img = RC.gray_frame(w, h, kind)
        for filt in RC.FILTERS:
            got = frames.resize_host(img, (ow, oh), filt)
            assert got.shape == (oh, ow) and np.array_equal(got, RC.pil_resize(img, (ow, oh), filt)), (shape, kind, filt)
    # NEAREST is the rule of the prescale as it has always been
    img = RC.gray_frame(w, h, "noise")
    assert np.array_equal(frames.resize_host(img, (ow, oh), "NEAREST"), RC.pil_resize(img, (ow, oh), "NEAREST")), shape


def test_resize_is_not_the_window_filter(native_lib):
    """The figure the header quotes: on a 192 x 108 -> 100 x 56 noise image Image.resize(BILINEAR) and Image.transform(EXTENT, BILINEAR)
    differ nearly everywhere, and the host entry is the former."""
    from PIL import Image
    img = np.random.default_rng(5).integers(0, 256, (108, 192), dtype=np.uint8)
    a = np.asarray(Image.fromarray(img).resize((100, 56), Image.BILINEAR))
    b = np.asarray(Image.fromarray(img).transform((100, 56), Image.EXTENT, (0, 0, 192, 108), Image.BILINEAR))
    assert (a != b).sum() > 5000
    assert np.array_equal(frames.resize_host(img, (100, 56), "BILINEAR"), a)


@pytest.mark.parametrize("fmt", CC.COLOR_FORMATS)
def test_color_source_gray_output_equals_convert_then_resize(native_lib, fmt):
    for shape in RC.SHAPES + [RC.TALL]:
        w, h, ow, oh = shape
        arr = RC.color_frame(w, h, fmt)
        for filt in RC.FILTERS:
            assert np.array_equal(frames.resize_host(arr, (ow, oh), filt, fmt), RC.pil_gray_resize(arr, fmt, (ow, oh), filt)), (shape, fmt, filt)
    # the order matters, so the test can tell: resize first, convert afterwards gives other bytes
    arr = RC.color_frame(37, 23, "RGB")
    other = CC.pil_gray(RC.pil_resize(arr, (16, 9), "BILINEAR"), "RGB")
    assert (other != RC.pil_gray_resize(arr, "RGB", (16, 9), "BILINEAR")).sum() > 0


@pytest.mark.parametrize("fmt", CC.COLOR_FORMATS)
def test_color_output_equals_pil_band_for_band(native_lib, fmt):
    for shape in RC.SHAPES + [RC.TALL]:
        w, h, ow, oh = shape
        arr = RC.color_frame(w, h, fmt)
        for filt in RC.FILTERS:
            got = frames.resize_host(arr, (ow, oh), filt, fmt, fmt)
            assert got.shape == (oh, ow, CC.BPP[fmt]) and np.array_equal(got, RC.pil_resize(arr, (ow, oh), filt)), (shape, fmt, filt)


def _raw(filt, src, fmt, h, w, ld, ofmt, dst, oh, ow, dld):
    p = lambda a: a if a is None or isinstance(a, int) else a.ctypes.data_as(C.c_void_p)
    return _capi.lib().hg_frame_resize_host(filt, p(src), fmt, h, w, ld, ofmt, p(dst), oh, ow, dld)


@pytest.mark.parametrize("fmt,ofmt", [("L", "L"), ("RGB", "L"), ("BGRA", "L"), ("RGB", "RGB"), ("RGBA", "RGBA")])
def test_pitched_source_and_destination(native_lib, fmt, ofmt):
    w, h, ow, oh = 37, 23, 16, 9
    arr = RC.color_frame(w, h, fmt) if fmt != "L" else RC.gray_frame(w, h, "noise")[:, :, None]
    bpp, obpp = CC.BPP[fmt], CC.BPP[ofmt]
    want = frames.resize_host(arr if fmt != "L" else arr[:, :, 0], (ow, oh), "BICUBIC", fmt, ofmt).reshape(oh, ow * obpp)
    for layout in CC.COLOR_LAYOUTS:                       # dense, rows one byte further apart (odd ld), a crop of a larger frame
        buf, off = CC.host_color_layout(arr, layout, 31)
        keep = buf.copy()
        dld = ow * obpp + 3                               # odd for every output here
        dst = np.full(5 + oh * dld + 5, 7, dtype=np.uint8)
        src = buf.reshape(-1)[off:]
        rc = _raw(3, src, frames.FORMATS[fmt], h, w, buf.shape[1], frames.FORMATS[ofmt], dst[5:], oh, ow, dld)
        assert rc == _capi.HG_OK, native_lib.hg_last_error()
        rows = dst[5:5 + oh * dld].reshape(oh, dld)
        assert np.array_equal(rows[:, :ow * obpp], want), (fmt, ofmt, layout)
        assert np.all(rows[:-1, ow * obpp:] == 7) and np.all(dst[:5] == 7) and np.all(dst[5 + (oh - 1) * dld + ow * obpp:] == 7), "guard bytes changed"
        assert np.array_equal(buf, keep), "the source changed"


def test_refusals_without_a_device(native_lib):
    src = np.zeros((8, 30), dtype=np.uint8)
    dst = np.full((8, 30), 7, dtype=np.uint8)
    L, RGB = 0, 1
    ok = (2, src, L, 8, 10, 30, L, dst, 4, 5, 30)
    assert _raw(*ok) == _capi.HG_OK
    dst[:] = 7

    def with_(**kw):
        names = ("filt", "src", "fmt", "h", "w", "ld", "ofmt", "dst", "oh", "ow", "dld")
        a = dict(zip(names, ok))
        a.update(kw)
        return tuple(a[n] for n in names)
    refused = {
        "unknown filter code 6": with_(filt=6), "unknown filter code -1": with_(filt=-1),
        "h <= 0": with_(h=0), "w <= 0": with_(w=-3), "out_h <= 0": with_(oh=0), "out_w <= 0": with_(ow=0),
        "ld below w": with_(ld=9), "ld below w * 3": with_(fmt=RGB, ld=29), "dst_ld below out_w": with_(dld=4),
        "dst_ld below out_w * 3": with_(fmt=RGB, ofmt=RGB, dld=14),
        "NEAREST with colour output": with_(filt=0, fmt=RGB, ofmt=RGB),
        "null source": with_(src=None), "null destination": with_(dst=None),
        "unknown source format": with_(fmt=5), "out_format neither L nor the source's": with_(fmt=RGB, ofmt=2),
        "colour output from a grey source": with_(ofmt=RGB),
        "overlap": with_(dst=src),
    }
    for what, args in refused.items():
        assert _raw(*args) == _capi.HG_ERR_ARG, what
        assert len(native_lib.hg_last_error()) > 10, what
        assert np.all(dst == 7), (what, "wrote before refusing")
    # tables beyond the stated cap: refused, nothing allocated (3 -> 2^23 pixels with BOX: 12 bytes of k and 8 of bounds per pixel)
    big = np.full(1 << 23, 7, dtype=np.uint8)
    assert _raw(4, src, L, 1, 3, 3, L, big, 1, 1 << 23, 1 << 23) == _capi.HG_ERR_ARG and b"HG_RESAMPLE_MAX_TABLE_BYTES" in native_lib.hg_last_error()
    assert np.all(big == 7)
    for bad in ("CUBIC", 6, -1, True, 2.0, None):
        with pytest.raises(ValueError):
            frames.resample_code(bad)
    with pytest.raises(ValueError):
        frames.resize_host(src, (5, 4), "BILINEAR", "L", "RGB")
    with pytest.raises(ValueError):
        frames.resize_host(np.zeros((4, 4, 3), np.uint8), (2, 2), "NEAREST", "RGB", "RGB")


def test_filter_table_and_cascade_argument():
    import re
    assert frames.RESAMPLE == RC.CODES
    from PIL import Image
    for name, code in frames.RESAMPLE.items():
        assert int(getattr(Image.Resampling, name)) == code and frames.resample_code(name) == code and frames.resample_code(code) == code
        assert frames.resample_code(getattr(Image.Resampling, name)) == code and frames.RESAMPLE_NAMES[code] == name
    text = open(os.path.join(ROOT, "include", "higsfa.h")).read()
    assert {m[0]: int(m[1]) for m in re.findall(r"HG_RESAMPLE_([A-Z]+) = (\d)", text)} == frames.RESAMPLE
    from pyfaceanalysis_amd.cascade import DeviceCascade
    assert DeviceCascade([], (16, 16), 10).prescale_filter == 0
    dc = DeviceCascade([], (16, 16), 10, prescale_filter="BICUBIC")
    assert dc.prescale_filter == 3
    dc.set_prescale_filter(Image.LANCZOS)
    assert dc.prescale_filter == 1
    with pytest.raises(ValueError):
        DeviceCascade([], (16, 16), 10, prescale_filter="CUBIC")
    assert _capi.lib().hg_cascade_set_prescale_filter(None, 2) == _capi.HG_ERR_ARG


def test_coefficient_unit_under_sanitizers(tmp_path):
    """tests/resample_driver.cpp with csrc/hg_resample.cpp, built with -fsanitize=address,undefined and run as a program: the shape list,
    every filter and format pair, pitched buffers with guard bytes, and an extreme shrink (3000 -> 1, LANCZOS: 18001 taps)."""
    exe = str(tmp_path / "resample_driver")
    cmd = [build.CXX, "-O1", "-g", "-std=c++17", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           os.path.join(ROOT, "tests", "resample_driver.cpp"), os.path.join(build.CSRC, "hg_resample.cpp"), "-o", exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode(errors="replace")[-3000:]
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    out = r.stdout.decode(errors="replace")
    assert r.returncode == 0 and "resample_driver: ok" in out, out[-3000:]
