"""CPU: the host side of ``tracking.StreamSetTracker`` / ``hg_stream_tracker``.  The five new C entries are declared, exported and
bound; every refusal that is decided on numbers comes as HG_ERR_ARG before a handle, a data pointer or a device is looked at (zeroed host
memory stands in for the handles), and the call after each refusal still works; ``StreamSetTracker`` refuses the same numbers at
construction and a bad stack — shape, dtype, strides, length, device — at ``step`` without creating a handle.  (``n_frames != n_streams``
needs a live handle: tests/test_stream_set_gpu.py.)"""
import ctypes as C
import os
import re

import numpy as np
import pytest

from pyfaceanalysis_amd import _capi
from tests import stream_set_cases as SC

HERE = os.path.dirname(os.path.abspath(__file__))
NEW_ENTRIES = ("hg_stream_tracker_create", "hg_stream_tracker_free", "hg_stream_tracker_reset", "hg_stream_tracker_step_frames_device",
               "hg_cascade_tracked_grid_streams_device")
ARG = _capi.HG_ERR_ARG


def consts():
    tc = _capi.HgTrackedConsts()
    tc.subimage_width = tc.subimage_height = 64.0
    tc.regression_width = tc.regression_height = 128.0
    tc.net_Dx, tc.net_Dy = 40.0, 20.0
    return tc


@pytest.fixture()
def dummy():
    buf = C.create_string_buffer(1 << 16)
    return C.cast(buf, C.c_void_p), buf


def test_cases_are_consistent():
    SC.assert_cases_consistent()
    assert _capi.HG_MAX_STREAM_WINDOWS == SC.MAX_STREAM_WINDOWS and _capi.HG_MAX_STACK_FRAMES == SC.MAX_STACK_FRAMES


def test_new_entries_declared_and_exported(native_lib):
    text = open(os.path.join(os.path.dirname(HERE), "include", "higsfa.h")).read()
    assert re.search(r"#define\s+HG_MAX_STREAM_WINDOWS\s+%d\b" % SC.MAX_STREAM_WINDOWS, text)
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(hg_[a-z_0-9]+)\s*\(", text))
    for name in NEW_ENTRIES:
        assert name in declared, name
        assert hasattr(native_lib, name) and getattr(native_lib, name).argtypes is not None, name
        assert name in _capi.EXPORTED_SYMBOLS, name


def test_create_refusals_need_no_device(native_lib):
    """The numbers are refused before any handle is looked at (none exists here); in range, the null handles are what is refused — the
    call after every refusal, so each shows that the one before left the library working."""
    tc = consts()
    for b, k, r, word in SC.BAD_SETS:
        h = C.c_void_p(1)
        rc = native_lib.hg_stream_tracker_create(None, None, C.byref(tc), b, k, r, C.byref(h))
        assert rc == ARG and not h.value, (b, k, r)
        assert word in native_lib.hg_last_error().decode(), (b, k, r, native_lib.hg_last_error())
        h = C.c_void_p(1)
        assert native_lib.hg_stream_tracker_create(None, None, C.byref(tc), 4, 8, 0, C.byref(h)) == ARG and not h.value
        assert "null" in native_lib.hg_last_error().decode(), (b, k, r)
    for b, k, r in SC.GOOD_SETS:
        h = C.c_void_p(1)
        assert native_lib.hg_stream_tracker_create(None, None, C.byref(tc), b, k, r, C.byref(h)) == ARG and not h.value
        assert "null" in native_lib.hg_last_error().decode(), (b, k, r)
    assert native_lib.hg_stream_tracker_create(None, None, C.byref(tc), 2, 2, 0, None) == ARG
    assert native_lib.hg_stream_tracker_reset(None, -1) == ARG
    native_lib.hg_stream_tracker_free(None)


def _levels():
    arr = (_capi.HgCascadeLevel * 1)()
    arr[0].nx, arr[0].ny = 3, 2
    arr[0].patch_w = arr[0].patch_h = 64.0
    return arr


def test_step_refusals_need_no_device(native_lib, dummy):
    """The frame numbers of a step are refused before the handle is looked at: with a null handle and with zeroed memory in its place.
    Nothing is written: stream_first keeps its bytes."""
    p, _keep = dummy
    lv = _levels()
    first = (C.c_int32 * 8)(*([77] * 8))
    rows = (C.c_double * 640)()
    n_rows = C.c_int64(-5)
    ok = dict(t=None, frames=p, n_frames=3, stride=130 * 144 + 97, h=131, w=97, ld=144, pre=(0, 0), out_cap=16)
    bad = dict(no_frames=(dict(n_frames=0), "frames in a stack"), negative_frames=(dict(n_frames=-4), "frames in a stack"),
               too_many_frames=(dict(n_frames=SC.MAX_STACK_FRAMES + 1), "frames in a stack"), ld_below_width=(dict(ld=96, stride=1 << 20), "geometry"),
               ld_zero=(dict(ld=0, stride=1 << 20), "geometry"), zero_height=(dict(h=0), "geometry"), zero_width=(dict(w=0), "geometry"),
               stride_below_bound=(dict(stride=130 * 144 + 96), "apart"), stride_zero=(dict(stride=0), "apart"), negative_cap=(dict(out_cap=-1), "capacity"))

    def call(a):
        return native_lib.hg_stream_tracker_step_frames_device(a["t"], a["frames"], a["n_frames"], a["stride"], a["h"], a["w"], a["ld"], a["pre"][0], a["pre"][1],
                                                               lv, 1, rows, a["out_cap"], C.cast(first, C.c_void_p), None, None, None, None, C.byref(n_rows), None)

    for handle in (None, p):
        for name, (kw, word) in bad.items():
            a = dict(ok, t=handle)
            a.update(kw)
            assert call(a) == ARG, (name, native_lib.hg_last_error())
            assert word in native_lib.hg_last_error().decode(), (name, native_lib.hg_last_error())
            assert list(first) == [77] * 8 and n_rows.value == -5, name
            assert call(dict(ok)) == ARG and "null" in native_lib.hg_last_error().decode(), name      # good numbers: the null handle is what is refused
    # a handle without streams (zeroed memory): any frame count differs from its n_streams = 0
    assert call(dict(ok, t=p)) == ARG and "streams" in native_lib.hg_last_error().decode()
    assert list(first) == [77] * 8


def test_grid_streams_refusals_need_no_device(native_lib, dummy):
    p, _keep = dummy
    tc = consts()
    f = native_lib.hg_cascade_tracked_grid_streams_device
    for b, k in ((0, 1), (-1, 1), (SC.MAX_STACK_FRAMES + 1, 1), (1, 0), (1, 65)):
        assert f(0, C.byref(tc), p, p, b, k, p, p, None) == ARG, (b, k)
    for args in ((None, p, p, p, p), (C.byref(tc), None, p, p, p), (C.byref(tc), p, None, p, p), (C.byref(tc), p, p, None, p), (C.byref(tc), p, p, p, None)):
        assert f(0, args[0], args[1], args[2], 2, 2, args[3], args[4], None) == ARG
    for bad in (float("nan"), float("inf"), 0.0, -40.0):
        tc.net_Dx = bad
        assert f(0, C.byref(tc), p, p, 2, 2, p, p, None) == ARG, bad


def _cascade(frame_format="L"):
    from pyfaceanalysis_amd.cascade import DeviceCascade
    return DeviceCascade([], (64, 64), 20, frame_format=frame_format)


class _Eyes(object):
    device = 0


def test_python_constructor_refusals():
    from pyfaceanalysis_amd.tracking import StreamSetTracker
    dc = _cascade()
    for b, k, r, word in SC.BAD_SETS:
        with pytest.raises(ValueError, match=word):
            StreamSetTracker(dc, _Eyes(), b, max_faces=k, rescan_every=r)
    for b, k, r in SC.GOOD_SETS:
        tr = StreamSetTracker(dc, _Eyes(), b, max_faces=k, rescan_every=r)
        assert tr.n_streams == b and tr.max_faces == k and tr.rescan_every == r and tr._h is None
        assert all(tr.tracked_faces(s).shape == (0, 4) for s in (0, b - 1, -1))
        with pytest.raises(IndexError):
            tr.tracked_faces(b)

    class Other(object):
        device = 1
    with pytest.raises(ValueError, match="device"):
        StreamSetTracker(dc, Other(), 2)


def test_python_stack_refusals():
    """Shape, dtype, strides and length are refused before the device, the device before the library: no handle is ever created."""
    import torch
    from pyfaceanalysis_amd.tracking import StreamSetTracker
    dc = _cascade()
    tr = StreamSetTracker(dc, _Eyes(), 3, max_faces=2)
    z = torch.zeros((3, 13, 17), dtype=torch.uint8)
    bad = {"2-d": z[0], "4-d": z[None], "float": z.float(), "int8": z.to(torch.int8), "not a tensor": np.zeros((3, 13, 17), np.uint8),
           "transposed rows": z.transpose(1, 2), "every second column": z[:, :, ::2], "broadcast frames": z[:1].expand(3, 13, 17),
           "broadcast rows": z[:, :1].expand(3, 13, 17), "overlapping frames": torch.as_strided(z, (3, 13, 17), (17, 17, 1)), "empty frames": z[:, :0],
           "list of two sizes": [z[0], z[0], z[0, :5]], "empty stack": z[:0], "empty list": []}
    for name, s in bad.items():
        with pytest.raises(ValueError):
            tr.step(s)
    for name, s in {"two frames": z[:2], "four frames": torch.zeros((4, 13, 17), dtype=torch.uint8), "a list of two": [z[0], z[1]]}.items():
        with pytest.raises(ValueError, match="for a set of 3 streams"):
            tr.step(s)
    with pytest.raises(ValueError, match="must live on"):      # a good stack on the wrong device: the last refusal before the library
        tr.step(z)
    with pytest.raises(ValueError, match="must live on"):
        tr.step(torch.zeros((6, 13, 40), dtype=torch.uint8)[::2, :, 3:20])
    assert tr._h is None and dc._h is None and dc.patcher._h is None, "no handle was created: the library was not touched"
    tr.reset()
    tr.reset(1)
    with pytest.raises(IndexError):
        tr.reset(3)
    tr.close()
    with pytest.raises(RuntimeError, match="closed"):
        tr.step(z)
    rgb = StreamSetTracker(_cascade("RGB"), _Eyes(), 2)
    for s in (torch.zeros((2, 5, 7), dtype=torch.uint8), torch.zeros((2, 5, 7, 4), dtype=torch.uint8), torch.zeros((3, 5, 7, 3), dtype=torch.uint8)):
        with pytest.raises(ValueError):
            rgb.step(s)
    with pytest.raises(ValueError, match="must live on"):
        rgb.step(torch.zeros((2, 5, 7, 3), dtype=torch.uint8))
