"""CPU: the frame-list entries (hg_patcher_extract_frame_list_device, hg_cascade_detect_frame_list_device,
hg_cascade_detect_faces_frame_list_device) are declared and exported, refuse a bad frame anywhere in the list before they look at a
handle, a data pointer or a device — naming the frame — and ``DeviceCascade.detect_frame_list`` / ``detect_faces_frame_list`` refuse bad
lists and return the empty result for an empty one without touching the library.  The premises of tests/test_frame_list_gpu.py that need
no device are pinned here through ``frame_levels`` / ``grid``."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from pyfaceanalysis_amd import _capi, grid
from tests import frame_batch_cases as BC
from tests import frame_list_cases as LC

HERE = os.path.dirname(os.path.abspath(__file__))
NEW_ENTRIES = ("hg_patcher_extract_frame_list_device", "hg_cascade_detect_frame_list_device", "hg_cascade_detect_faces_frame_list_device")
ARG = _capi.HG_ERR_ARG
POSITIONS = (0, 1, 2)      # the bad frame FIRST, in the MIDDLE and LAST of a list of three


def test_new_entries_declared_and_exported(native_lib):
    text = open(os.path.join(os.path.dirname(HERE), "include", "higsfa.h")).read()
    assert "typedef struct hg_frame_ref" in text and "typedef struct hg_cascade_frame" in text
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(hg_[a-z_0-9]+)\s*\(", text))
    for name in NEW_ENTRIES:
        assert name in declared, name
        assert hasattr(native_lib, name), name
        assert name in _capi.EXPORTED_SYMBOLS, name
    assert C.sizeof(_capi.HgFrameRef) == 24 and C.sizeof(_capi.HgCascadeFrame) == 48


@pytest.fixture()
def dummy():
    """Zeroed host memory in the role of a handle or a data pointer: a refusal must come before anything behind it is used."""
    buf = C.create_string_buffer(1 << 16)
    return C.cast(buf, C.c_void_p), buf


GOOD = ((131, 97, 144), (61, 40, 40), (5, 7, 9))      # (frame_h, frame_w, ld)


def _refs(p, bad_at=None, **kw):
    arr = (_capi.HgFrameRef * 3)()
    for i, (h, w, ld) in enumerate(GOOD):
        arr[i].frame_dev, arr[i].frame_h, arr[i].frame_w, arr[i].ld = p.value, h, w, ld
    for k, v in kw.items():
        setattr(arr[bad_at], k, v)
    return arr


def _patcher_call(lib, p0, refs0, **kw):
    a = dict(p=p0, filter=0, refs=refs0, n_frames=3, boxes=p0, angs=None, rows=p0, n=5, ow=8, oh=8, out=p0, dtype=_capi.HG_U8, ldo=64)
    a.update(kw)
    return lib.hg_patcher_extract_frame_list_device(a["p"], a["filter"], a["refs"], a["n_frames"], a["boxes"], a["angs"], a["rows"], a["n"], a["ow"], a["oh"],
                                                    a["out"], a["dtype"], a["ldo"], None)


def test_patcher_list_refusals_need_no_device(native_lib, dummy):
    p, _keep = dummy
    good = _refs(p)
    bad = dict(null_handle=dict(p=None), null_frames=dict(refs=None), null_boxes=dict(boxes=None), null_rows=dict(rows=None), null_out=dict(out=None),
               no_frames=dict(n_frames=0), negative_frames=dict(n_frames=-2), too_many_frames=dict(n_frames=_capi.HG_MAX_STACK_FRAMES + 1),
               negative_n=dict(n=-1), filter_1=dict(filter=1), filter_7=dict(filter=7), out_dtype=dict(dtype=9), ldo=dict(ldo=63), out_size=dict(ow=0))
    for name, kw in bad.items():
        assert _patcher_call(native_lib, p, good, **kw) == ARG, name
    per_frame = dict(zero_height=dict(frame_h=0), negative_width=dict(frame_w=-3), ld_below_width=dict(ld=3), ld_zero=dict(ld=0), null_frame=dict(frame_dev=None))
    for name, kw in per_frame.items():
        for at in POSITIONS:
            for n in (5, 0):                                   # the refusals come before n == 0
                assert _patcher_call(native_lib, p, _refs(p, at, **kw), n=n) == ARG, (name, at)
                assert ("frame %d " % at) in native_lib.hg_last_error().decode(), (name, at, native_lib.hg_last_error())
    for at in POSITIONS:                                       # a rotated NEAREST call on a frame of 32768 pixels or more per side
        huge = _refs(p, at, frame_w=32768, ld=32768)
        assert _patcher_call(native_lib, p, huge, angs=p) == ARG and ("frame %d " % at) in native_lib.hg_last_error().decode(), at
        assert _patcher_call(native_lib, p, huge, angs=p, n=0, filter=2) == _capi.HG_OK      # ... and on that call only
    for filt in (0, 2, 3):                                     # n == 0: HG_OK for every filter, the handle is not looked at
        assert _patcher_call(native_lib, p, good, n=0, filter=filt) == _capi.HG_OK, filt


def _levels(nx=3, ny=2, n=1):
    arr = (_capi.HgCascadeLevel * n)()
    for i in range(n):
        arr[i].nx, arr[i].ny = nx, ny
        arr[i].patch_w = arr[i].patch_h = 64.0
    return arr


def _cframes(p, lv, bad_at=None, **kw):
    arr = (_capi.HgCascadeFrame * 3)()
    for i, (h, w, ld) in enumerate(GOOD):
        a = arr[i]
        a.frame_dev, a.frame_h, a.frame_w, a.ld, a.prescale_w, a.prescale_h = p.value, h, w, ld, 0, 0
        a.levels, a.n_levels = C.cast(lv, C.POINTER(_capi.HgCascadeLevel)), 1
    for k, v in kw.items():
        setattr(arr[bad_at], k, v)
    return arr


def _cascade_call(lib, faces, c, e, frames, n_frames, first, out_cap=16):
    rows = C.c_int64(-5)
    buf = (C.c_double * 640)(*([-3.0] * 640))
    first_p = C.cast(first, C.c_void_p) if first is not None else None
    if faces:
        rc = lib.hg_cascade_detect_faces_frame_list_device(c, e, frames, n_frames, buf, out_cap, first_p, None, None, C.byref(rows), None)
    else:
        rc = lib.hg_cascade_detect_frame_list_device(c, frames, n_frames, buf, None, None, None, out_cap, first_p, None, C.byref(rows), None)
    assert rows.value == -5 and all(v == -3.0 for v in buf), "output sentinels untouched"
    return rc


@pytest.mark.parametrize("faces", (False, True))
def test_cascade_list_refusals_need_no_device(native_lib, dummy, faces):
    """Every refusal is HG_ERR_ARG (never HG_ERR_DEVICE: there is no device here), leaves the outputs as they were and, for a bad frame,
    names it — FIRST, in the MIDDLE and LAST of a list of three."""
    p, _keep = dummy
    lv = _levels()
    first = (C.c_int32 * 8)(*([77] * 8))
    good = _cframes(p, lv)
    ok = dict(c=p, e=p, frames=good, n_frames=3, first=first)
    bad = dict(null_cascade=dict(c=None), null_list=dict(frames=None), no_frames=dict(n_frames=0), negative_frames=dict(n_frames=-1),
               too_many_frames=dict(n_frames=_capi.HG_MAX_STACK_FRAMES + 1), null_frame_first=dict(first=None), negative_cap=dict(out_cap=-1))
    if faces:
        bad["null_eyes"] = dict(e=None)
    for name, kw in bad.items():
        a = dict(ok)
        a.update(kw)
        assert _cascade_call(native_lib, faces, **a) == ARG, (name, native_lib.hg_last_error())
        assert list(first) == [77] * 8, name
    bound_levels = _levels(nx=1 << 12, ny=1 << 12)            # 2^24 windows: with two more frames of 6 windows the total is still below 2^31 / 64 = 2^25 ...
    two_bound = _levels(nx=1 << 12, ny=1 << 13)               # ... 2^25 windows in one frame is refused as that frame's grid, 2^24 + 2^24 + 6 as the total
    no_lv = C.POINTER(_capi.HgCascadeLevel)()
    per_frame = dict(zero_height=dict(frame_h=0), zero_width=dict(frame_w=0), ld_below_width=dict(ld=3), null_frame=dict(frame_dev=None),
                     null_levels=dict(levels=no_lv), no_levels=dict(n_levels=0), too_many_levels=dict(n_levels=33), half_a_prescale=dict(prescale_w=50),
                     bad_grid=dict(levels=C.cast(_levels(nx=0), C.POINTER(_capi.HgCascadeLevel))),
                     one_grid_too_large=dict(levels=C.cast(two_bound, C.POINTER(_capi.HgCascadeLevel))))
    for name, kw in per_frame.items():
        for at in POSITIONS:
            a = dict(ok)
            a["frames"] = _cframes(p, lv, at, **kw)
            assert _cascade_call(native_lib, faces, **a) == ARG, (name, at, native_lib.hg_last_error())
            assert ("frame %d " % at) in native_lib.hg_last_error().decode(), (name, at, native_lib.hg_last_error())
            assert list(first) == [77] * 8, (name, at)
    if faces:      # a NEAREST eye step (a zeroed handle reads as one) cuts rotated NEAREST windows: a frame of 32768 pixels or more per side is refused
        for at in POSITIONS:      # ... by the size the grid is laid over: the same frame behind a prescale is not
            a = dict(ok)
            a["frames"] = _cframes(p, lv, at, frame_w=40000, ld=40000)
            assert _cascade_call(native_lib, faces, **a) == ARG and ("frame %d " % at) in native_lib.hg_last_error().decode(), at
            assert "32768" in native_lib.hg_last_error().decode() and list(first) == [77] * 8
    total = _cframes(p, lv)                                    # the TOTAL above the bound: no single frame is
    for at in (0, 2):
        total[at].levels = C.cast(bound_levels, C.POINTER(_capi.HgCascadeLevel))
    a = dict(ok)
    a["frames"] = total
    assert _cascade_call(native_lib, faces, **a) == ARG and "too many windows" in native_lib.hg_last_error().decode()
    assert list(first) == [77] * 8


def _cascade(frame_format="L"):
    from pyfaceanalysis_amd.cascade import DeviceCascade
    return DeviceCascade([], (64, 64), 20, frame_format=frame_format)


class _Eyes(object):
    device = 0


@pytest.mark.parametrize("method", ("detect_frame_list", "detect_faces_frame_list"))
def test_python_list_refusals_and_empty_list(method):
    import torch
    dc = _cascade()
    call = (lambda s: dc.detect_frame_list(s)) if method == "detect_frame_list" else (lambda s: dc.detect_faces_frame_list(s, _Eyes()))
    a, b = torch.zeros((13, 17), dtype=torch.uint8), torch.zeros((5, 40), dtype=torch.uint8)
    bad = {"not a list": a, "a stack tensor": torch.zeros((2, 13, 17), dtype=torch.uint8), "not a tensor": [a, np.zeros((13, 17), np.uint8), b],
           "float": [a, b.float()], "int8": [a.to(torch.int8), b], "3-d": [a, b[None]], "1-d": [a[0], b], "every second column": [a, b[:, ::2]],
           "transposed": [a.t(), b], "broadcast rows": [a, b[:1].expand(5, 40)], "empty frame": [a, b[:, :0], a], "no rows": [a[:0], b],
           "too many frames": [a] * (_capi.HG_MAX_STACK_FRAMES + 1), "a colour frame": [a, torch.zeros((5, 7, 3), dtype=torch.uint8)]}
    for name, s in bad.items():
        with pytest.raises(ValueError):
            call(s)
    for good in ([a, b], (b, a, torch.zeros((9, 60), dtype=torch.uint8)[:, 3:40])):      # two sizes and strides: accepted up to the device check
        with pytest.raises(ValueError, match="must live on"):
            call(good)
    for empty in ([], ()):
        got = call(empty)
        assert got["counts"] == [] and got["rows_executed"] == 0 and got["n_windows"] == 0
        if method == "detect_frame_list":
            assert got["frames"] == []
        else:
            assert got["faces"] == [] and got["n_before_purge"] == []
    assert dc._h is None and dc.patcher._h is None, "no handle was created: the library was not touched"
    with pytest.raises(ValueError):      # detect_frames keeps refusing two sizes: the list entries are new names on purpose
        dc.detect_frames([a, b])


def test_python_colour_list_refusals():
    import torch
    dc = _cascade("RGB")
    z, y = torch.zeros((5, 7, 3), dtype=torch.uint8), torch.zeros((4, 9, 3), dtype=torch.uint8)
    for s in ([z, y[..., :2]], [z[:, :, 0], y], [z, torch.zeros((4, 9, 4), dtype=torch.uint8)], [z[:, ::2], y], [z.permute(0, 2, 1), y],
              [z, y[:1].expand(4, 9, 3)]):
        with pytest.raises(ValueError):
            dc.detect_frame_list(s)
    with pytest.raises(ValueError, match="must live on"):
        dc.detect_frame_list([z, y])
    assert dc.detect_frame_list([])["frames"] == [] and dc._h is None


def _facts(size, prescale_size=grid.PRESCALE_SIZE):
    """(prescaled size, level table as bytes, window count) of a frame size with the tests' smallest_face and sub-image size."""
    from pyfaceanalysis_amd.cascade import frame_levels
    pw, ph = grid.prescaled_size(size[0], size[1], prescale_size)
    levels, n_levels, n0 = frame_levels(pw, ph, 0.1, grid.FACE_PIPELINE, (64, 64))
    return (pw, ph), bytes(levels)[:n_levels * C.sizeof(_capi.HgCascadeLevel)], n0


def test_cascade_case_premises():
    """What tests/test_frame_list_gpu.py takes for granted about its lists, pinned without a device."""
    n = lambda size: _facts(size)[2]
    assert (n(BC.SMALL), n(BC.MEDIUM), n(BC.LONG)) == (397, 1308, 5148)
    counts = [n(size) for size, _seed in LC.CHUNKED]
    first = np.cumsum([0] + counts)
    assert sum(counts) == LC.CHUNKED_TOTAL > 8192 and 8192 not in first
    a, b = (_facts(s) for s in LC.SHARED_GRID)
    assert LC.SHARED_GRID[0] != LC.SHARED_GRID[1] and a == b, "two sizes, one grid after the prescale"
    c, d = (_facts(s) for s in LC.EQUAL_COUNT)
    assert c[2] == d[2] and (c[0], c[1]) != (d[0], d[1]), "equal window counts, different grids"
    assert {size for size, _ in LC.TABLES} == set(LC.SHARED_GRID) | set(LC.EQUAL_COUNT)
    many = [_facts(size) for size in LC.MANY_GRIDS]
    assert len({(m[0], m[1]) for m in many}) == len(many) == 6 > 4, "more distinct level tables than the keyed ring has slots"
    assert max(w * h for (w, h), _ in LC.MIXED + LC.CHUNKED) == 2000 * 300


def test_patcher_case_geometry():
    """The premises of the GPU patcher test (tests/frame_list_cases.py), pinned without a device."""
    buf, offsets = LC.patch_buffer()
    boxes, angles, row_frame = LC.patch_windows()
    inside = np.zeros(len(buf), dtype=bool)
    for (w, h, ld, _s), off in zip(LC.PATCH_FRAMES, offsets):
        assert ld >= w
        np.lib.stride_tricks.as_strided(inside[off:], shape=(h, w), strides=(ld, 1))[...] = True
    assert (buf[~inside] == 255).all() and inside.sum() == sum(w * h for w, h, _l, _s in LC.PATCH_FRAMES) and (~inside[:offsets[0]]).all()
    assert len({(w, h) for w, h, _l, _s in LC.PATCH_FRAMES}) == 3 and len({ld for _w, _h, ld, _s in LC.PATCH_FRAMES}) == 3
    assert min(w for w, _h, _l, _s in LC.PATCH_FRAMES) < 8 and LC.PATCH_FRAMES[0][2] == 9
    assert boxes.shape == (LC.N_ROWS, 4) and set(row_frame) == {-1, 0, 1, 2, 3, 8}
    for f, (w, h, _l, _s) in enumerate(LC.PATCH_FRAMES):      # every frame meets every kind of window, in ITS coordinates
        x0, y0, x1, y1 = boxes[row_frame == f].T
        assert ((x0 >= 0) & (y0 >= 0) & (x1 <= w) & (y1 <= h)).sum() >= 3, f
        assert (x0 < 0).any() and (y0 < 0).any() and (x1 > w).any() and (y1 > h).any(), f
        assert ((x0 >= w) | (y1 <= 0)).sum() >= 1, f
    assert {0.0, 90.0, -90.0, 180.0, 22.5, -22.5} <= set(angles)
