"""CPU: the frame-list entries of pose normalisation and estimation (hg_patcher_normalize_frame_list_device,
hg_estimator_estimate_frame_list_device) are declared and exported and refuse bad arguments with HG_ERR_ARG before they look behind a
handle or a data pointer or at a device (zeroed host memory stands in for all of them), naming the frame where one frame is the reason;
``normalize_frame_list`` / ``estimate_frame_list`` / ``estimate_faces_frame_list`` / ``prescale_frame_list`` refuse bad lists and face
lists and answer an empty list without loading the library; the geometry of faces on frames of different sizes is each face's own
frame's; tests/estimate_frame_list_driver.cpp runs the host-only argument check as a program, plain and under ASan / UBSan."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from pyfaceanalysis_amd import _capi, analysis as A, build, normalize as N
from tests import estimate_frame_list_cases as LE
from tests import normalize_cases as NC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ("hg_patcher_normalize_frame_list_device", "hg_estimator_estimate_frame_list_device")
ARG, OK = _capi.HG_ERR_ARG, _capi.HG_OK
GOOD = ((131, 97, 144), (61, 40, 40), (5, 7, 9))      # (frame_h, frame_w, ld)
SIZE = (32, 24)
POSITIONS = (0, 1, 2)      # the bad frame FIRST, in the MIDDLE and LAST of a list of three


def test_new_entries_declared_and_exported(native_lib):
    text = open(os.path.join(ROOT, "include", "higsfa.h")).read()
    assert "OWN FRAME" in text, "the header says what size the geoms are computed for"
    declared = set(re.findall(r"\b(hg_[a-z_0-9]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))
    for name in NEW_ENTRIES:
        assert name in declared and hasattr(native_lib, name) and name in _capi.EXPORTED_SYMBOLS, name
    assert len(declared) == len(_capi.EXPORTED_SYMBOLS) == 105


@pytest.fixture()
def dummy():
    """Zeroed host memory in the role of a handle or a device pointer: a refusal must come before anything behind it is used."""
    buf = C.create_string_buffer(1 << 16)
    return C.cast(buf, C.c_void_p), buf


def _refs(p, bad_at=None, **kw):
    arr = (_capi.HgFrameRef * 3)()
    for i, (h, w, ld) in enumerate(GOOD):
        arr[i].frame_dev, arr[i].frame_h, arr[i].frame_w, arr[i].ld = p.value, h, w, ld
    for k, v in kw.items():
        setattr(arr[bad_at], k, v)
    return arr


def _geoms(ff):
    """One good face per entry of ff, made for that frame's size."""
    g = np.zeros(len(ff), dtype=_capi.NORM_GEOM_DTYPE)
    for i, f in enumerate(ff):
        h, w, _ld = GOOD[f]
        g[i] = N.geometry([NC.eye_sets(w, h)[i % 9][1]], (w, h), SIZE, NC.AREA)[0]
    return g


def _calls(native_lib, p, g, ff):
    """(normalise call, estimate call) with keyword overrides of one good argument set."""
    base = dict(h=p, flags=0, refs=_refs(p), n_frames=3, g=g.ctypes.data_as(C.c_void_p), ff=ff.ctypes.data_as(C.c_void_p), n=len(g), ow=SIZE[0], oh=SIZE[1], out=p,
                ldo=SIZE[0] * SIZE[1], out_stride=len(g))

    def norm(**kw):
        a = dict(base, **kw)
        return native_lib.hg_patcher_normalize_frame_list_device(a["h"], a["flags"], a["refs"], a["n_frames"], a["g"], a["ff"], a["n"], a["ow"], a["oh"], a["out"],
                                                                 a["ldo"], None)

    def est(**kw):
        a = dict(base, **kw)
        return native_lib.hg_estimator_estimate_frame_list_device(a["h"], a["flags"], a["refs"], a["n_frames"], a["g"], a["ff"], a["n"], a["out"], a["out_stride"],
                                                                  None, None, None)
    return norm, est


def test_refusals_need_no_device(native_lib, dummy):
    p, _keep = dummy
    ff = np.array([2, 0, 1, 0], dtype=np.int32)
    g = _geoms(ff)
    norm, est = _calls(native_lib, p, g, ff)
    moved = np.array([2, 1, 1, 0], dtype=np.int32)      # face 1's geom was built for frame 0's size
    common = dict(null_handle=dict(h=None), null_list=dict(refs=None), null_geoms=dict(g=None), null_face_frame=dict(ff=None), null_out=dict(out=None),
                  no_frames=dict(n_frames=0), negative_frames=dict(n_frames=-1), too_many_frames=dict(n_frames=_capi.HG_MAX_STACK_FRAMES + 1),
                  negative_n=dict(n=-1), flags_3=dict(flags=3), flags_4=dict(flags=4), flags_negative=dict(flags=-1),
                  another_frames_size=dict(ff=moved.ctypes.data_as(C.c_void_p)))
    for name, kw in common.items():
        assert norm(**kw) == ARG, (name, native_lib.hg_last_error())
        assert est(**kw) == ARG, (name, native_lib.hg_last_error())
    assert norm(ff=moved.ctypes.data_as(C.c_void_p)) == ARG and b"another frame size" in native_lib.hg_last_error()
    for name, kw in dict(out_w=dict(ow=0), out_h=dict(oh=4097), ldo=dict(ldo=SIZE[0] * SIZE[1] - 1)).items():
        assert norm(**kw) == ARG, name
    assert est(out_stride=len(g) - 1) == ARG
    # a bad frame FIRST, in the MIDDLE and LAST: the message names it, and the refusal comes before n == 0
    per_frame = dict(null_frame=dict(frame_dev=None), zero_height=dict(frame_h=0), ld_below_width=dict(ld=3), negative_width=dict(frame_w=-3),
                     too_wide=dict(frame_w=(1 << 24) + 1, ld=1 << 25))
    for name, kw in per_frame.items():
        for at in POSITIONS:
            for call in (norm, est):
                for n in (len(g), 0):
                    assert call(refs=_refs(p, at, **kw), n=n) == ARG, (name, at)
                    assert ("frame %d " % at) in native_lib.hg_last_error().decode(), (name, at, native_lib.hg_last_error())
    # n == 0 is HG_OK (no data pointer is needed then), the largest list is one, an index outside the list is no error for the check
    many = (_capi.HgFrameRef * (_capi.HG_MAX_STACK_FRAMES + 1))()
    for a in many:
        a.frame_dev, a.frame_h, a.frame_w, a.ld = p.value, 5, 7, 9
    for call in (norm, est):
        assert call(n=0) == OK and call(n=0, g=None, ff=None, out=None) == OK
        assert call(n=0, refs=many, n_frames=_capi.HG_MAX_STACK_FRAMES) == OK and call(n=0, refs=many, n_frames=_capi.HG_MAX_STACK_FRAMES + 1) == ARG
        assert call(n=0, flags=1) == OK and call(n=0, flags=3) == ARG and call(n=0, refs=None) == ARG


def _lists(torch):
    a, b = torch.zeros((13, 17), dtype=torch.uint8), torch.zeros((5, 40), dtype=torch.uint8)
    return (a, b), {"not a list": a, "a stack tensor": torch.zeros((2, 13, 17), dtype=torch.uint8), "not a tensor": [a, np.zeros((13, 17), np.uint8), b],
                    "float": [a, b.float()], "int8": [a.to(torch.int8), b], "3-d": [a, b[None]], "1-d": [a[0], b], "every second column": [a, b[:, ::2]],
                    "transposed": [a.t(), b], "broadcast rows": [a, b[:1].expand(5, 40)], "empty frame": [a, b[:, :0], a], "no rows": [a[:0], b],
                    "too many frames": [a] * (_capi.HG_MAX_STACK_FRAMES + 1), "a colour frame": [a, torch.zeros((5, 7, 3), dtype=torch.uint8)]}


class _Flow(object):
    device, output_dtype, input_dim, output_dim = 0, np.float32, 64, 5


class _Clf(object):
    input_dim, avg_labels = 5, [-1.0, 1.0]


def _objects():
    fa = A.FaceAnalyzer(_Flow(), gender=_Clf(), contrast=(128.0, 48.0), patch_size=(8, 8))
    return fa, fa._norm


def test_python_list_refusals():
    import torch
    fa, fn = _objects()
    (a, b), bad = _lists(torch)
    eyes = np.array([NC.eye_sets(17, 13)[0][1]] * 2)
    calls = {"normalize_frame_list": lambda s: fn.normalize_frame_list(s, eyes, [0, 1]), "estimate_frame_list": lambda s: fa.estimate_frame_list(s, eyes, [0, 1]),
             "estimate_faces_frame_list": lambda s: fa.estimate_faces_frame_list(s, [np.zeros((0, 10))] * (len(s) if isinstance(s, list) else 2))}
    for what, call in calls.items():
        for name, s in bad.items():
            with pytest.raises(ValueError):
                call(s)
        for name in ("not a tensor", "float", "a colour frame", "every second column", "empty frame"):      # the message names the frame
            with pytest.raises(ValueError, match="frame [12] of the list"):
                call(bad[name])
        with pytest.raises(ValueError, match="float frame is not offered; a colour frame goes through"):
            call(bad["float"])
        for good in ([a, b], [b, a, torch.zeros((9, 60), dtype=torch.uint8)[:, 3:40]], [a, a]):      # good layouts on the host: the last refusal before the library
            with pytest.raises(ValueError, match="device tensors"):
                call(good)
    assert fa._h is None and fn._patcher._h is None, "no handle was created"


def test_python_face_refusals():
    import torch
    fa, fn = _objects()
    frames = [torch.zeros((13, 17), dtype=torch.uint8), torch.zeros((5, 40), dtype=torch.uint8), torch.zeros((9, 9), dtype=torch.uint8)]
    eyes = np.array([NC.eye_sets(17, 13)[0][1]] * 2)
    for call in (lambda e, f: fn.normalize_frame_list(frames, e, f), lambda e, f: fa.estimate_frame_list(frames, e, f)):
        for name, f in {"missing": None, "too short": [0], "too long": [0, 1, 2], "float": np.array([0.0, 1.0]), "bool": np.array([True, False]),
                        "2-d": np.zeros((2, 1), dtype=np.int32), "strings": ["0", "1"]}.items():
            with pytest.raises(ValueError, match="face_frame"):
                call(eyes, f)
        with pytest.raises(ValueError, match="eyes"):
            call(np.zeros((2, 3)), [0, 1])
        for f in ([0, 1], np.array([2, -1], dtype=np.int64), np.array([0, 7], dtype=np.uint8)):      # good faces: refused for the device, last
            with pytest.raises(ValueError, match="device tensors"):
                call(eyes, f)
    g = fn.geometry(eyes, (17, 13))
    with pytest.raises(ValueError, match="face_frame"):
        fn.normalize_frame_list(frames, geoms=g, face_frame=[0])
    with pytest.raises(ValueError, match="geoms"):
        fa.estimate_frame_list(frames, geoms=np.zeros(2), face_frame=[0, 1])
    for faces in ([], [np.zeros((0, 10))] * 2, [np.zeros((0, 10))] * 4, np.zeros((3, 10)), None):
        with pytest.raises(ValueError, match="one per frame"):
            fa.estimate_faces_frame_list(frames, faces)
    with pytest.raises(ValueError):
        fa.estimate_faces_frame_list(frames, [np.zeros((1, 9))] * 3)
    assert fa._h is None and fn._patcher._h is None


def test_empty_list_never_loads_the_library(monkeypatch):
    import torch
    fa, fn = _objects()
    monkeypatch.setattr(_capi, "lib", lambda: pytest.fail("the library was touched"))
    monkeypatch.setattr(_capi, "_lib", None)
    for empty in ([], ()):
        res = fa.estimate_frame_list(empty, np.zeros((0, 4)), [])
        assert sorted(res) == ["gender", "gender_confidence", "gender_label", "status"]
        assert res["gender"].shape == (0,) and res["gender"].dtype == np.float64 and res["status"].dtype == np.int32 and res["gender_label"] == []
        assert fa.estimate_faces_frame_list(empty, []) == []
        with pytest.raises(ValueError, match="one per frame"):
            fa.estimate_faces_frame_list(empty, [np.zeros((0, 10))])
        # faces on a list without frames: every index is outside it
        res = fa.estimate_frame_list(empty, np.array([NC.eye_sets(17, 13)[0][1]] * 3), [0, 1, -1], return_intermediates=True)
        assert list(res["status"]) == [N.STATUS_FRAME_RANGE] * 3 and np.isnan(res["gender"]).all() and np.isnan(res["gender_confidence"]).all()
        assert res["gender_label"] == [None] * 3 and res["patches"].shape == (3, 64) and res["features"].shape == (3, 5)
        out = torch.full((2, 260, 256), 7, dtype=torch.uint8)      # (the images of an empty list live where ``out`` does)
        img, status = fn.normalize_frame_list(empty, np.array([NC.eye_sets(17, 13)[0][1]] * 2), [0, 5], out=out)
        assert img is out and not img.any() and list(status) == [N.STATUS_FRAME_RANGE] * 2 and status.dtype == np.int32
    from pyfaceanalysis_amd.cascade import DeviceCascade
    for fmt in ("L", "RGB"):
        dc = DeviceCascade([], (64, 64), 20, frame_format=fmt)
        assert dc.prescale_frame_list([]) == [] and dc.prescale_frame_list(()) == []
        assert dc._h is None and dc.patcher._h is None and dc._list_pre is None
    assert _capi._lib is None, "the native library was never loaded"
    assert N.STATUS_FRAME_RANGE == LE.STATUS_FRAME_RANGE and N.STATUS[N.STATUS_FRAME_RANGE]


def test_frame_index_outside_a_host_list_is_refused_for_the_device_only():
    """On a list with frames the faces are checked first, an index outside it is no error, and the host tensors are refused last."""
    import torch
    fa, fn = _objects()
    frames = [torch.zeros((13, 17), dtype=torch.uint8), torch.zeros((5, 40), dtype=torch.uint8)]
    with pytest.raises(ValueError, match="device tensors"):
        fa.estimate_frame_list(frames, np.array([NC.eye_sets(17, 13)[0][1]] * 2), [0, 9])
    with pytest.raises(ValueError, match="device tensors"):
        fa.estimate_frame_list(frames, np.zeros((0, 4)), [])


def test_prescale_frame_list_refusals():
    import torch
    from pyfaceanalysis_amd.cascade import DeviceCascade
    dc = DeviceCascade([], (64, 64), 20)
    (a, b), bad = _lists(torch)
    for name, s in bad.items():
        with pytest.raises(ValueError):
            dc.prescale_frame_list(s)
    with pytest.raises(ValueError, match="must live on"):
        dc.prescale_frame_list([a, b])
    rgb = DeviceCascade([], (64, 64), 20, frame_format="RGB")
    with pytest.raises(ValueError):
        rgb.prescale_frame_list([a, b])
    with pytest.raises(ValueError, match="must live on"):
        rgb.prescale_frame_list([torch.zeros((5, 7, 3), dtype=torch.uint8), torch.zeros((4, 9, 3), dtype=torch.uint8)])
    assert dc._h is None and dc.patcher._h is None and rgb.patcher._h is None and dc._list_pre is None


def test_geometry_scatter(native_lib):
    """The geoms of interleaved faces on three sizes equal, field for field, ``geometry(eyes[i], that frame's size)``; with frame 0's size
    for every face they differ (the premise: the case can tell)."""
    fn = N.FaceNormalizer(0, preset="pose", out_size=(17, 13), method="eyes_inferred-mouth_areaZ")
    eyes, ff = LE.spread_faces()
    eyes, ff, bad = LE.with_bad_rows(eyes, ff, LE.N_FRAMES)
    g, ffc = fn.list_geometry(LE.SIZES, eyes, ff)
    assert ffc.dtype == np.int32 and np.array_equal(ffc, ff) and g.dtype == _capi.NORM_GEOM_DTYPE and len(g) == len(eyes)
    zero = np.zeros(1, dtype=_capi.NORM_GEOM_DTYPE)[0]
    border = {tuple(e) for f in (1, 2) for e in LE.border_eyes(*LE.SIZES[f])}
    told_apart, border_told_apart = 0, 0
    for i in range(len(eyes)):
        inside = 0 <= ff[i] < LE.N_FRAMES
        want = fn.geometry(eyes[i:i + 1], LE.SIZES[ff[i]])[0] if inside else zero
        for k in NC.GEOM_FIELDS:
            assert np.array_equal(g[i][k], want[k], equal_nan=True), (i, k)
        if inside and ff[i] != 0 and want["status"] == 0:
            planted = fn.geometry(eyes[i:i + 1], LE.SIZES[0])[0]
            differs = any(not np.array_equal(planted[k], want[k], equal_nan=True) for k in NC.GEOM_FIELDS)
            told_apart += differs
            border_told_apart += differs and tuple(eyes[i]) in border
    refused = {r: c for r, c in bad.items() if c != LE.STATUS_FRAME_RANGE}
    assert {r: int(g["status"][r]) for r in refused} == refused
    assert told_apart >= 10 and border_told_apart >= 1, "a variant using frame 0's size for every face is told apart, on a border face too"
    fn.close()


def test_case_premises(native_lib):
    """The premises of the GPU tests' cases, pinned without a device."""
    eyes, ff = LE.spread_faces()
    assert set(ff) == {0, 1, 2} and len(eyes) == len(ff) == 3 * (LE.N_NAMED + 10) and len(set(LE.SIZES)) == 3 and LE.SIZES[0] == (7, 5)
    fn = N.FaceNormalizer(0, preset="pose", out_size=(17, 13), method="eyes_inferred-mouth_areaZ")
    g, _ = fn.list_geometry(LE.SIZES, eyes, ff)
    staged, taps = LE.modes(g, (17, 13))
    assert taps.sum() >= 4 and staged.sum() >= 10, "one call holds staged faces and tap-by-tap faces"
    assert set(ff[taps]) == {1, 2} and set(ff[staged]) == {0, 1, 2}, "tap-by-tap faces on two frames, staged ones on all three"
    fn.close()
    for size, method in NC.SMALL_OUT_SIZES:      # unrotated, the rectangle a cut reads is the crop's own: over every edge of the two larger frames
        flat = N.FaceNormalizer(0, preset="pose", out_size=size, method="eyes_inferred-mouth_areaZ" if method == NC.AREAZ else "eyes_inferred-mouth_area", rotate=False)
        over = LE.overhang(flat.list_geometry(LE.SIZES, eyes, ff)[0], ff)
        assert over[1] == (True,) * 4 and over[2] == (True,) * 4 and any(over[0]), (size, over)
        flat.close()
    e, f = LE.est_faces()
    assert len(e) == 9 and len(set(LE.EST_SIZES)) == 3
    e2, f2, want = LE.with_bad_rows(eyes, ff, 3)
    assert sorted(want.values()) == [1, 2, 5, 5, 5] and sorted(int(f2[r]) for r, c in want.items() if c == 5) == [-1, 3, 8]


def _run(cmd, **kw):
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, **kw)
    return r.returncode, r.stdout.decode(errors="replace")


@pytest.mark.skipif(shutil.which(build.CXX) is None, reason="needs the host compiler")
def test_list_check_driver_plain_and_under_asan_ubsan(tmp_path):
    """tests/estimate_frame_list_driver.cpp with csrc/hg_normalize.cpp: its own main, no library preloaded."""
    base = [build.CXX, "-O1", "-g", "-std=c++17", "-Wall", "-ffp-contract=off", "-I" + build.CSRC]
    src = [os.path.join(ROOT, "tests", "estimate_frame_list_driver.cpp"), os.path.join(build.CSRC, "hg_normalize.cpp")]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    # the driver itself must compile and pass as a plain build: a compile error is a failure, never a skip
    plain = str(tmp_path / "estimate_frame_list_driver_plain")
    rc, out = _run(base + src + ["-o", plain])
    assert rc == 0, out[-3000:]
    rc, out = _run([plain], timeout=300)
    assert rc == 0 and "estimate_frame_list_driver: ok" in out, out[-3000:]
    # only a missing sanitizer runtime is a reason to skip: asked of a trivial program, not of the driver
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    rc, out = _run([build.CXX] + san + [str(probe), "-o", str(tmp_path / "probe")])
    if rc != 0:
        pytest.skip("no sanitizer runtime here: " + out[-300:])
    exe = str(tmp_path / "estimate_frame_list_driver")
    rc, out = _run(base + san + src + ["-o", exe])
    assert rc == 0, out[-3000:]
    rc, out = _run([exe], timeout=300, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert rc == 0 and "runtime error" not in out and "AddressSanitizer" not in out and "estimate_frame_list_driver: ok" in out, out[-3000:]
