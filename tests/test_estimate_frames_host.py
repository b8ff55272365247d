"""CPU: the stack entries of pose normalisation and estimation (hg_patcher_normalize_frames_device,
hg_estimator_estimate_frames_device) are declared and exported and refuse bad arguments with HG_ERR_ARG before they look behind a handle
or a data pointer or at a device (zeroed host memory stands in for all of them); ``normalize_frames`` / ``estimate_frames`` /
``estimate_faces_frames`` / ``prescale_frames`` refuse bad stacks and face lists and answer an empty stack or n = 0 without touching the
library (host tensors: refused for their device only after shape, dtype, strides and the faces)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from pyfaceanalysis_amd import _capi, analysis as A, normalize as N
from tests import estimate_frames_cases as EC
from tests import normalize_cases as NC

HERE = os.path.dirname(os.path.abspath(__file__))
NEW_ENTRIES = ("hg_patcher_normalize_frames_device", "hg_estimator_estimate_frames_device")
ARG, OK = _capi.HG_ERR_ARG, _capi.HG_OK
FW, FH, LD = 97, 61, 101
BOUND = (FH - 1) * LD + FW
SIZE = (32, 24)


def test_new_entries_declared_and_exported(native_lib):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(os.path.dirname(HERE), "include", "higsfa.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(hg_[a-z_0-9]+)\s*\(", text))
    for name in NEW_ENTRIES:
        assert name in declared and hasattr(native_lib, name) and name in _capi.EXPORTED_SYMBOLS, name


@pytest.fixture()
def dummy():
    """Zeroed host memory in the role of a handle or a device pointer: a refusal must come before anything behind it is used."""
    buf = C.create_string_buffer(1 << 16)
    return C.cast(buf, C.c_void_p), buf


def geoms(n=2, frame_size=(FW, FH)):
    return N.geometry([NC.eye_sets(*frame_size)[i % 9][1] for i in range(n)], frame_size, SIZE, NC.AREA)


def _calls(native_lib, p, g, ff):
    """(normalise call, estimate call) with keyword overrides of one good argument set."""
    base = dict(h=p, flags=0, frames=p, n_frames=3, stride=BOUND, fh=FH, fw=FW, ld=LD, g=g.ctypes.data_as(C.c_void_p), ff=ff.ctypes.data_as(C.c_void_p), n=len(g),
                ow=SIZE[0], oh=SIZE[1], out=p, ldo=SIZE[0] * SIZE[1], out_stride=len(g))

    def norm(**kw):
        a = dict(base, **kw)
        return native_lib.hg_patcher_normalize_frames_device(a["h"], a["flags"], a["frames"], a["n_frames"], a["stride"], a["fh"], a["fw"], a["ld"], a["g"], a["ff"],
                                                             a["n"], a["ow"], a["oh"], a["out"], a["ldo"], None)

    def est(**kw):
        a = dict(base, **kw)
        return native_lib.hg_estimator_estimate_frames_device(a["h"], a["flags"], a["frames"], a["n_frames"], a["stride"], a["fh"], a["fw"], a["ld"], a["g"], a["ff"],
                                                              a["n"], a["out"], a["out_stride"], None, None, None)
    return norm, est


def test_refusals_need_no_device(native_lib, dummy):
    p, _keep = dummy
    g, ff = geoms(), np.array([0, 2], dtype=np.int32)
    norm, est = _calls(native_lib, p, g, ff)
    other = geoms(2, (FW + 3, FH)).ctypes.data_as(C.c_void_p)      # geoms built for another frame size
    common = dict(null_handle=dict(h=None), null_frames=dict(frames=None), null_geoms=dict(g=None), null_face_frame=dict(ff=None), null_out=dict(out=None),
                  no_frames=dict(n_frames=0), negative_frames=dict(n_frames=-1), too_many_frames=dict(n_frames=_capi.HG_MAX_STACK_FRAMES + 1),
                  stride_below_bound=dict(stride=BOUND - 1), stride_zero=dict(stride=0), ld_below_width=dict(ld=FW - 1, stride=1 << 20), zero_height=dict(fh=0),
                  negative_n=dict(n=-1), flags_3=dict(flags=3), flags_4=dict(flags=4), flags_negative=dict(flags=-1), other_frame_size=dict(g=other))
    for name, kw in common.items():
        assert norm(**kw) == ARG, (name, native_lib.hg_last_error())
        assert est(**kw) == ARG, (name, native_lib.hg_last_error())
    for name, kw in dict(out_w=dict(ow=0), out_h=dict(oh=4097), ldo=dict(ldo=SIZE[0] * SIZE[1] - 1)).items():
        assert norm(**kw) == ARG, name
    assert est(out_stride=1) == ARG
    # n == 0 is HG_OK (no pointer is needed then), the bound itself is a valid stride, the largest stack is one; refusals come before n == 0
    for call in (norm, est):
        assert call(n=0) == OK and call(n=0, frames=None, g=None, ff=None, out=None) == OK
        assert call(n=0, stride=BOUND) == OK and call(n=0, stride=BOUND - 1) == ARG
        assert call(n=0, n_frames=_capi.HG_MAX_STACK_FRAMES) == OK and call(n=0, n_frames=_capi.HG_MAX_STACK_FRAMES + 1) == ARG
        assert call(n=0, fh=1, stride=FW) == OK and call(n=0, fh=1, stride=FW - 1) == ARG
        assert call(n=0, ld=1 << 62, stride=(1 << 63) - 1) == ARG      # (frame_h - 1) ld overflows int64: still decided right
        assert call(n=0, flags=1) == OK and call(n=0, flags=3) == ARG


def _stacks(torch):
    z = torch.zeros((3, 13, 17), dtype=torch.uint8)
    return z, {"2-d": z[0], "4-d": z[None], "float": z.float(), "int8": z.to(torch.int8), "not a tensor": np.zeros((3, 13, 17), np.uint8),
               "colour": torch.zeros((3, 13, 17, 3), dtype=torch.uint8), "transposed rows": z.transpose(1, 2), "every second column": z[:, :, ::2],
               "broadcast frames": z[:1].expand(3, 13, 17), "broadcast rows": z[:, :1].expand(3, 13, 17),
               "overlapping frames": torch.as_strided(z, (3, 13, 17), (17, 17, 1)), "empty frames": z[:, :0], "list of two sizes": [z[0], z[0, :5]],
               "too many frames": torch.zeros((_capi.HG_MAX_STACK_FRAMES + 1, 1, 1), dtype=torch.uint8)}


class _Flow(object):
    device, output_dtype, input_dim, output_dim = 0, np.float32, 64, 5


class _Clf(object):
    input_dim, avg_labels = 5, [-1.0, 1.0]


def _objects():
    fa = A.FaceAnalyzer(_Flow(), gender=_Clf(), contrast=(128.0, 48.0), patch_size=(8, 8))
    return fa, fa._norm


def test_python_stack_refusals():
    import torch
    fa, fn = _objects()
    z, bad = _stacks(torch)
    eyes = np.array([NC.eye_sets(17, 13)[0][1]] * 2)
    calls = {"normalize_frames": lambda s: fn.normalize_frames(s, eyes, [0, 1]), "estimate_frames": lambda s: fa.estimate_frames(s, eyes, [0, 1]),
             "estimate_faces_frames": lambda s: fa.estimate_faces_frames(s, [np.zeros((0, 10))] * 3)}
    for what, call in calls.items():
        for name, s in bad.items():
            with pytest.raises(ValueError):
                call(s)
        for name in ("float", "colour"):      # the message style of estimate: what is not offered and where such a stack goes first
            with pytest.raises(ValueError, match="float stack is not offered; a colour stack goes through"):
                call(bad[name])
        with pytest.raises(ValueError, match="device tensor"):      # a good layout on the host: the last refusal before the library
            call(z)
        with pytest.raises(ValueError, match="device tensor"):
            call(torch.zeros((6, 13, 40), dtype=torch.uint8)[::2, :, 3:20])
    assert fa._h is None and fn._patcher._h is None, "no handle was created"


def test_python_face_refusals():
    import torch
    fa, fn = _objects()
    z = torch.zeros((3, 13, 17), dtype=torch.uint8)
    eyes = np.array([NC.eye_sets(17, 13)[0][1]] * 2)
    for call in (lambda e, f: fn.normalize_frames(z, e, f), lambda e, f: fa.estimate_frames(z, e, f)):
        for name, f in {"missing": None, "too short": [0], "too long": [0, 1, 2], "float": np.array([0.0, 1.0]), "bool": np.array([True, False]),
                        "2-d": np.zeros((2, 1), dtype=np.int32), "strings": ["0", "1"]}.items():
            with pytest.raises(ValueError, match="face_frame"):
                call(eyes, f)
        with pytest.raises(ValueError, match="eyes"):
            call(np.zeros((2, 3)), [0, 1])
        for f in ([0, 1], np.array([2, -1], dtype=np.int64), np.array([0, 7], dtype=np.uint8)):      # good faces: refused for the device, last
            with pytest.raises(ValueError, match="device tensor"):
                call(eyes, f)
    for faces in ([], [np.zeros((0, 10))] * 2, [np.zeros((0, 10))] * 4, np.zeros((3, 10)), None):
        with pytest.raises(ValueError, match="one per frame"):
            fa.estimate_faces_frames(z, faces)
    with pytest.raises(ValueError):
        fa.estimate_faces_frames(z, [np.zeros((1, 9))] * 3)
    assert list(N.check_face_frame(np.array([0, 2 ** 40, -2 ** 40, 2 ** 31 - 1], dtype=np.int64), 4)) == [0, -1, -1, 2 ** 31 - 1]
    assert list(N.check_face_frame(np.array([3, 2 ** 63], dtype=np.uint64), 2)) == [3, -1]
    assert fa._h is None and fn._patcher._h is None


def test_empty_stack_and_no_faces_touch_no_library_entry(monkeypatch):
    import torch
    fa, fn = _objects()
    monkeypatch.setattr(_capi, "lib", lambda: pytest.fail("the library was touched"))
    z = torch.zeros((3, 13, 17), dtype=torch.uint8)
    for empty in ([], z[:0]):
        res = fa.estimate_frames(empty, np.zeros((0, 4)), [])
        assert sorted(res) == ["gender", "gender_confidence", "gender_label", "status"]
        assert res["gender"].shape == (0,) and res["gender"].dtype == np.float64 and res["status"].dtype == np.int32 and res["gender_label"] == []
        assert fa.estimate_faces_frames(empty, []) == []
        with pytest.raises(ValueError, match="one per frame"):
            fa.estimate_faces_frames(empty, [np.zeros((0, 10))])
        # faces on a stack without frames: every index is outside it
        res = fa.estimate_frames(empty, np.array([NC.eye_sets(17, 13)[0][1]] * 2), [0, 1], return_intermediates=True)
        assert list(res["status"]) == [EC.STATUS_FRAME_RANGE] * 2 and np.isnan(res["gender"]).all() and res["gender_label"] == [None, None]
        assert res["patches"].shape == (2, 64) and res["features"].shape == (2, 5)
    img, status = fn.normalize_frames(z[:0], np.zeros((0, 4)), [])
    assert tuple(img.shape) == (0, 260, 256) and img.dtype == torch.uint8 and status.shape == (0,) and status.dtype == np.int32
    # n = 0 on a stack with frames: refused for its device only (a host tensor), after the faces
    with pytest.raises(ValueError, match="device tensor"):
        fa.estimate_frames(z, np.zeros((0, 4)), [])
    assert N.STATUS[N.STATUS_FRAME_RANGE] and N.STATUS_FRAME_RANGE == EC.STATUS_FRAME_RANGE


def test_prescale_frames_refusals_and_empty_stack():
    import torch
    from pyfaceanalysis_amd.cascade import DeviceCascade
    dc = DeviceCascade([], (64, 64), 20)
    z, bad = _stacks(torch)
    for name, s in bad.items():
        with pytest.raises(ValueError):
            dc.prescale_frames(s)
    with pytest.raises(ValueError, match="must live on"):
        dc.prescale_frames(z)
    for empty in ([], z[:0]):
        assert tuple(dc.prescale_frames(empty).shape) == (0, 0, 0)
    rgb = DeviceCascade([], (64, 64), 20, frame_format="RGB")
    with pytest.raises(ValueError):
        rgb.prescale_frames(z)
    with pytest.raises(ValueError, match="must live on"):
        rgb.prescale_frames(torch.zeros((2, 5, 7, 3), dtype=torch.uint8))
    assert dc._h is None and dc.patcher._h is None and rgb.patcher._h is None


def test_case_premises():
    """The premises of the GPU tests' cases, pinned without a device."""
    eyes, ff = EC.spread_faces()
    assert set(ff) == {0, 1, 2} and len(eyes) == len(ff) == 3 * 19
    e2, f2, want = EC.with_bad_rows(eyes, ff, 3)
    assert sorted(want.values()) == [1, 2, 5, 5, 5] and sorted(int(f2[r]) for r, c in want.items() if c == 5) == [-1, 3, 8]
    e, f = EC.est_faces()
    assert len(e) == 9 and (np.diff(f) < 0).any()
    g = N.geometry(eyes, EC.FRAME, (17, 13), NC.AREAZ)
    np_ = g["rect"][:, 2].astype(np.int64) * g["rect"][:, 3]
    assert (np_ > 16 * 17 * 13).any() and ((np_ > 0) & (np_ <= 16 * 17 * 13)).any(), "one call holds staged faces and tap-by-tap faces"
