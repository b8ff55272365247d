"""CPU: the frame-stack entries (hg_patcher_extract_frames_device, hg_cascade_detect_frames_device,
hg_cascade_detect_faces_frames_device) are declared and exported, refuse bad arguments before they look at a handle, a data pointer or a
device, and ``DeviceCascade.detect_frames`` / ``detect_faces_frames`` refuse bad stacks and return empty lists for an empty one without
touching the library (no GPU needed: the tensors are host tensors, refused for their device only after shape, dtype and strides)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from pyfaceanalysis_amd import _capi
from tests import frame_batch_cases as BC

HERE = os.path.dirname(os.path.abspath(__file__))
NEW_ENTRIES = ("hg_patcher_extract_frames_device", "hg_cascade_detect_frames_device", "hg_cascade_detect_faces_frames_device")
ARG = _capi.HG_ERR_ARG


def test_new_entries_declared_and_exported(native_lib):
    text = open(os.path.join(os.path.dirname(HERE), "include", "higsfa.h")).read()
    assert re.search(r"#define\s+HG_MAX_STACK_FRAMES\s+%d\b" % _capi.HG_MAX_STACK_FRAMES, text)
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(hg_[a-z_0-9]+)\s*\(", text))
    for name in NEW_ENTRIES:
        assert name in declared, name
        assert hasattr(native_lib, name), name
        assert name in _capi.EXPORTED_SYMBOLS, name


@pytest.fixture()
def dummy():
    """Zeroed host memory in the role of a handle or a data pointer: a refusal must come before anything behind it is used."""
    buf = C.create_string_buffer(1 << 16)
    return C.cast(buf, C.c_void_p), buf


def _patcher_args(ptr, **kw):
    p = ptr
    a = dict(p=p, filter=0, frames=p, n_frames=3, stride=(BC.H - 1) * BC.LD + BC.W, h=BC.H, w=BC.W, ld=BC.LD, boxes=p, angs=None, rows=p, n=5,
             ow=8, oh=8, out=p, dtype=_capi.HG_U8, ldo=64)
    a.update(kw)
    return (a["p"], a["filter"], a["frames"], a["n_frames"], a["stride"], a["h"], a["w"], a["ld"], a["boxes"], a["angs"], a["rows"], a["n"], a["ow"],
            a["oh"], a["out"], a["dtype"], a["ldo"], None)


def test_patcher_frames_refusals_need_no_device(native_lib, dummy):
    p, _keep = dummy
    f = native_lib.hg_patcher_extract_frames_device
    bound = (BC.H - 1) * BC.LD + BC.W
    bad = dict(null_handle=dict(p=None), null_frames=dict(frames=None), null_boxes=dict(boxes=None), null_rows=dict(rows=None), null_out=dict(out=None),
               no_frames=dict(n_frames=0), negative_frames=dict(n_frames=-2), stride_below_bound=dict(stride=bound - 1), stride_zero=dict(stride=0),
               ld_below_width=dict(ld=BC.W - 1, stride=1 << 20), ld_zero=dict(ld=0, stride=1 << 20), negative_n=dict(n=-1), filter_1=dict(filter=1),
               filter_7=dict(filter=7), out_dtype=dict(dtype=9), ldo=dict(ldo=63), out_size=dict(ow=0))
    for name, kw in bad.items():
        assert f(*_patcher_args(p, **kw)) == ARG, name
    for filt in (0, 2, 3):                                     # n == 0: HG_OK for every filter, the handle is not looked at
        assert f(*_patcher_args(p, n=0, filter=filt)) == _capi.HG_OK, filt
    assert f(*_patcher_args(p, n=0, stride=bound)) == _capi.HG_OK       # the bound itself is a valid stride
    assert f(*_patcher_args(p, n=0, stride=bound - 1)) == ARG           # ... and the refusals come before n == 0


def _levels(nx=3, ny=2, n=1):
    arr = (_capi.HgCascadeLevel * n)()
    for i in range(n):
        arr[i].nx, arr[i].ny = nx, ny
        arr[i].patch_w = arr[i].patch_h = 64.0
    return arr


def _cascade_call(native_lib, faces, c, e, frames, n_frames, stride, h, w, ld, pre, levels, n_levels, first, out_cap=16):
    rows = C.c_int64()
    buf = (C.c_double * 640)()
    first_p = C.cast(first, C.c_void_p) if first is not None else None
    if faces:
        return native_lib.hg_cascade_detect_faces_frames_device(c, e, frames, n_frames, stride, h, w, ld, pre[0], pre[1], levels, n_levels, buf, out_cap, first_p,
                                                                None, None, C.byref(rows), None)
    return native_lib.hg_cascade_detect_frames_device(c, frames, n_frames, stride, h, w, ld, pre[0], pre[1], levels, n_levels, buf, None, None, None, out_cap,
                                                      first_p, None, C.byref(rows), None)


@pytest.mark.parametrize("faces", (False, True))
def test_cascade_frames_refusals_need_no_device(native_lib, dummy, faces):
    """Every refusal is HG_ERR_ARG (never HG_ERR_DEVICE: there is no device here) and leaves frame_first as it was."""
    p, _keep = dummy
    lv = _levels()
    first = (C.c_int32 * 8)(*([77] * 8))
    ok = dict(c=p, e=p, frames=p, n_frames=3, stride=130 * 144 + 97, h=131, w=97, ld=144, pre=(0, 0), levels=lv, n_levels=1, first=first)
    bound_levels = _levels(nx=1 << 12, ny=1 << 12)            # 2^24 windows a frame: 3 frames exceed 2^31 / 64, one frame does not
    bad = dict(null_cascade=dict(c=None), no_frames=dict(n_frames=0), negative_frames=dict(n_frames=-1),
               too_many_frames=dict(n_frames=_capi.HG_MAX_STACK_FRAMES + 1), too_many_windows=dict(levels=bound_levels),
               no_levels=dict(n_levels=0), ld_below_width=dict(ld=96, stride=1 << 20), zero_height=dict(h=0), stride_below_bound=dict(stride=130 * 144 + 96),
               null_frames=dict(frames=None), null_frame_first=dict(first=None), half_a_prescale=dict(pre=(50, 0)), negative_cap=dict(out_cap=-1))
    if faces:
        bad["null_eyes"] = dict(e=None)
    for name, kw in bad.items():
        a = dict(ok)
        a.update(kw)
        assert _cascade_call(native_lib, faces, **a) == ARG, (name, native_lib.hg_last_error())
        assert list(first) == [77] * 8, name


def _cascade(frame_format="L"):
    from pyfaceanalysis_amd.cascade import DeviceCascade
    return DeviceCascade([], (64, 64), 20, frame_format=frame_format)


class _Eyes(object):
    device = 0


@pytest.mark.parametrize("method", ("detect_frames", "detect_faces_frames"))
def test_python_stack_refusals_and_empty_stack(method):
    import torch
    dc = _cascade()
    call = (lambda s: dc.detect_frames(s)) if method == "detect_frames" else (lambda s: dc.detect_faces_frames(s, _Eyes()))
    z = torch.zeros((3, 13, 17), dtype=torch.uint8)
    bad = {"2-d": z[0], "4-d": z[None], "float": z.float(), "int8": z.to(torch.int8), "not a tensor": np.zeros((3, 13, 17), np.uint8),
           "transposed rows": z.transpose(1, 2), "every second column": z[:, :, ::2], "broadcast frames": z[:1].expand(3, 13, 17),
           "broadcast rows": z[:, :1].expand(3, 13, 17), "overlapping frames": torch.as_strided(z, (3, 13, 17), (17, 17, 1)),
           "empty frames": z[:, :0], "list of two sizes": [z[0], z[0, :5]], "list of two dtypes": [z[0], z[0].float()],
           "too many frames": torch.zeros((_capi.HG_MAX_STACK_FRAMES + 1, 1, 1), dtype=torch.uint8)}
    for name, s in bad.items():
        with pytest.raises(ValueError):
            call(s)
    with pytest.raises(ValueError, match="must live on"):      # a good layout on the wrong device: the last refusal before the library
        call(z)
    with pytest.raises(ValueError, match="must live on"):
        call(torch.zeros((6, 13, 40), dtype=torch.uint8)[::2, :, 3:20])
    for empty in ([], (), z[:0]):
        got = call(empty)
        assert got["counts"] == [] and got["rows_executed"] == 0 and got["n_windows"] == 0
        if method == "detect_frames":
            assert got["frames"] == []
        else:
            assert got["faces"] == [] and got["n_before_purge"] == []
    assert dc._h is None and dc.patcher._h is None, "no handle was created: the library was not touched"


def test_python_colour_stack_refusals():
    import torch
    dc = _cascade("RGB")
    z = torch.zeros((2, 5, 7, 3), dtype=torch.uint8)
    for s in (z[0], z[..., :2], torch.zeros((2, 5, 7, 4), dtype=torch.uint8), z[:, :, ::2], z.permute(0, 1, 3, 2), z[:, :1].expand(2, 5, 7, 3)):
        with pytest.raises(ValueError):
            dc.detect_frames(s)
    with pytest.raises(ValueError, match="must live on"):
        dc.detect_frames(z)
    assert dc.detect_frames(z[:0])["frames"] == []
    with pytest.raises(ValueError):
        _cascade().detect_frames(z)          # a colour stack given to a grey cascade


def test_patcher_case_geometry():
    """The premises of the GPU patcher test (tests/frame_batch_cases.py), pinned without a device."""
    buf, offsets = BC.stack_buffer()
    boxes, angles, row_frame = BC.windows()
    assert BC.FRAME_STRIDE % BC.LD != 0 and BC.FRAME_STRIDE >= (BC.H - 1) * BC.LD + BC.W
    inside = np.zeros(len(buf), dtype=bool)
    for off in offsets:
        np.lib.stride_tricks.as_strided(inside[off:], shape=(BC.H, BC.W), strides=(BC.LD, 1))[...] = True
    assert (buf[~inside] == 255).all() and inside.sum() == BC.N_FRAMES * BC.H * BC.W and (~inside[:offsets[0]]).all()
    assert boxes.shape == (BC.N_ROWS, 4) and set(row_frame) == {-1, 0, 1, 2, 3, 8}
    x0, y0, x1, y1 = boxes.T
    assert ((x0 >= 0) & (y0 >= 0) & (x1 <= BC.W) & (y1 <= BC.H)).sum() >= 15                  # inside
    assert (x0 < 0).any() and (y0 < 0).any() and (x1 > BC.W).any() and (y1 > BC.H).any()      # over every edge
    assert ((x0 >= BC.W) | (y1 <= 0)).sum() >= 5                                              # wholly outside
    assert {0.0, 90.0, -90.0, 180.0, 22.5, -22.5} <= set(angles)
