"""CPU: pose-normalised face crops on the host (hg_normalize_geometry_host, hg_normalize_faces_host; csrc/hg_normalize.cpp).  The
geometry against the reference's lines transcribed to Python (tests/normalize_cases.py::geometry_restate), field for field with ``==``;
the pixels against PIL itself composed as the reference composes it (``pil_normalize``), ``array_equal``.  The stand-alone driver
tests/normalize_driver.cpp runs the same unit under AddressSanitizer and UBSan as a program."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from pyfaceanalysis_amd import _capi, build, normalize as N
from tests import eyes_restate as ER
from tests import filters_restate as FR
from tests import normalize_cases as NC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = NC.small_cases() + NC.large_cases()


def assert_geom_equal(got, want, what):
    """Every field with ==: the host unit and Python's math share one libm, so the trig-derived fields agree to the last bit too."""
    for k in NC.GEOM_FIELDS:
        assert np.array_equal(np.asarray(got[k]), np.asarray(want[k])), (what, k, got[k], want[k])


def test_geometry_equals_restatement_on_cases(native_lib):
    for name, fs, e, size, method in CASES:
        for rotate in (True, False):
            g = N.geometry([e], fs, size, method, rotate)
            assert g.shape == (1,) and g["status"][0] == 0
            assert_geom_equal(g[0], NC.geometry_restate(e, fs, size, method, rotate), (name, rotate))


@pytest.mark.parametrize("fs", NC.FRAME_SIZES + [NC.LARGE_FRAME])
def test_geometry_equals_restatement_on_random_eyes(native_lib, fs):
    E = NC.random_eyes(300, fs)
    assert len(E) > 250
    for (size, method), rotate in zip(NC.OUT_SIZES, (True, True, False, True)):
        g = N.geometry(E, fs, size, method, rotate)
        for i, e in enumerate(E):
            assert_geom_equal(g[i], NC.geometry_restate(e, fs, size, method, rotate), (fs, i, size))
        ok = g[g["status"] == 0]
        assert len(ok) > 200 and np.all(ok["W"] & 1) and np.all(ok["H"] & 1)


def test_square_crop_at_exactly_ninety_degrees(native_lib):
    """The 65 x 65 frame: the crop is the frame, square, and the eye line is exactly +-90 degrees — Image.rotate's transpose shortcut."""
    for (name, e), want in zip(NC.SQUARE_EYES, (90.0, -90.0)):
        g = N.geometry([e], NC.SQUARE_FRAME, (32, 24))[0]
        assert (g["W"], g["H"], g["crop_x0"], g["crop_y0"], g["angle"]) == (65, 65, 0, 0, want), (name, g)
    g = N.geometry([NC.eye_sets(97, 61)[0][1]], (97, 61), (32, 24))[0]
    assert g["angle"] == 0.0 and g["rotated"] == 0 and list(g["m"]) == [1.0, 0.0, 0.0, 0.0, 1.0, 0.0]


REFUSED = [((5.0, 5.0, 4.0, 5.0), 1), ((np.nan, 1.0, 2.0, 3.0), 2), ((1.0, np.inf, 2.0, 3.0), 2), ((7.0, 7.0, 7.0, 7.0), 3),
           ((-1e9, -1.135e9, 1e9, -1.135e9 + 3e6), 4), ((-1e200, 0.0, 1e200, 0.0), 2)]


def test_refused_faces_in_the_middle_of_a_batch(native_lib):
    fs, size, method = (97, 61), (32, 24), NC.AREA
    frame = NC.noise_frame(*fs)
    good = [e for _, e in NC.eye_sets(*fs)]
    eyes = good[:3] + [e for e, _ in REFUSED] + good[3:6]
    img, status = N.normalize_host(frame, eyes, size, method)
    assert status.dtype == np.int32 and list(status) == [0, 0, 0] + [s for _, s in REFUSED] + [0, 0, 0]
    g = N.geometry(eyes, fs, size, method)
    for i, e in enumerate(eyes):
        assert_geom_equal(g[i], NC.geometry_restate(e, fs, size, method), i)
        if status[i]:
            assert not img[i].any()
            blank = g[i:i + 1].copy()
            blank["status"] = 0
            assert not any(blank.tobytes())      # everything but the status is zero
        else:
            assert np.array_equal(img[i], N.normalize_host(frame, [e], size, method)[0][0])      # neighbours untouched
            assert np.array_equal(img[i], NC.pil_normalize(frame, g[i], size))


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_pixels_equal_pil(native_lib, case):
    name, fs, e, size, method = case
    frame = NC.noise_frame(*fs)
    g = N.geometry([e], fs, size, method)
    want = NC.pil_normalize(frame, g[0], size)
    img, status = N.normalize_host(frame, [e], size, method)
    assert img.shape == (1, size[1], size[0]) and img.dtype == np.uint8 and status[0] == 0
    assert np.array_equal(img[0], want)
    if fs != NC.LARGE_FRAME:
        assert want.any() or "corners" in name      # (all but the corner faces, whose centre lies outside the frame, show some of it)
        for view in (NC.pitched(frame), NC.crop_view(frame)):
            assert not view.flags["C_CONTIGUOUS"]
            assert np.array_equal(N.normalize_host(view, [e], size, method)[0][0], want)
        unrot = N.normalize_host(frame, [e], size, method, rotate=False)[0][0]
        assert np.array_equal(unrot, NC.pil_normalize(frame, N.geometry([e], fs, size, method, False)[0], size))


def test_both_host_paths_are_taken(native_lib):
    """The case list has faces on both sides of the work-equality bound (rect pixels against 16 out_w out_h)."""
    taps = set()
    for name, fs, e, size, method in CASES:
        r = N.geometry([e], fs, size, method)[0]["rect"]
        if int(r[2]) * int(r[3]) > 16 * size[0] * size[1]:
            taps.add(name)
    # the face with eyes 330 pixels apart, wherever the crop is large enough to hold more than 16 rotated pixels per output pixel
    assert {"97x61-wider-17x13", "160x120-wider-32x24", "160x120-wider-17x13"} <= taps, taps
    assert not any("level" in n or "one-pixel" in n or "at-the-bound" in n for n in taps), taps
    r = N.geometry([NC.AT_THE_BOUND[2]], *NC.AT_THE_BOUND[1:2], NC.AT_THE_BOUND[3], NC.AT_THE_BOUND[4])[0]["rect"]
    assert (int(r[2]), int(r[3])) == (68, 52) and 68 * 52 == 16 * 17 * 13      # exactly at the bound: still staged


def test_the_composition_matters(native_lib):
    """Rotating the FRAME about the face centre and cutting the box from it (the window rule of the patcher, filters_restate.window) is not
    normalize_image: on a tilted face near the border the zero padding is part of the crop here (its zeros enter the taps of the rotation),
    and pixels outside the frame are simply absent there.  The test can tell the two apart."""
    differing = 0
    for fs in NC.FRAME_SIZES[:2]:
        frame = NC.noise_frame(*fs)
        for name, e in NC.eye_sets(*fs):
            if not name.startswith(("tilt", "corners")):
                continue
            size, method = (32, 24), NC.AREA
            g = N.geometry([e], fs, size, method)[0]
            ours = N.normalize_host(frame, [e], size, method)[0][0]
            assert np.array_equal(ours, NC.pil_normalize(frame, g, size))
            box = np.asarray(g["box"]) + np.array([g["crop_x0"], g["crop_y0"], g["crop_x0"], g["crop_y0"]], dtype=np.float64)
            other = FR.window(frame, box, float(g["angle"]), size, FR.BICUBIC).reshape(size[1], size[0])
            differing += int(not np.array_equal(ours, other))
    assert differing >= 1


def test_approximate_eye_coords_equal_the_restated_reference(native_lib):
    rng = np.random.default_rng(11)
    x0, y0 = rng.uniform(-50, 900, 64), rng.uniform(-50, 500, 64)
    side = rng.uniform(20, 300, 64)
    boxes = np.stack([x0, y0, x0 + side, y0 + side * rng.uniform(0.8, 1.2, 64)], axis=1)
    angles = rng.uniform(-45, 45, 64)
    angles[::5] = 0.0
    got = N.approximate_eye_coords(boxes, angles)
    want = np.array([ER.eye_boxes(b, a)[0] for b, a in zip(boxes, angles)])
    assert got.shape == (64, 4) and np.array_equal(got, want)
    assert np.array_equal(N.approximate_eye_coords(boxes[:3]), np.array([ER.eye_boxes(b, 0.0)[0] for b in boxes[:3]]))
    assert np.all(got[:, 0] < got[:, 2])
    # what save_pose_normalized_face_detections does with them: the pose preset on those eyes
    frame = NC.noise_frame(160, 120)
    e = N.approximate_eye_coords([[40.0, 20.0, 110.0, 90.0]], [12.5])
    img, status = N.normalize_host(frame, e, *N.PRESETS["pose"])
    assert status[0] == 0 and np.array_equal(img[0], NC.pil_normalize(frame, N.geometry(e, (160, 120), *N.PRESETS["pose"])[0], (256, 192)))


def test_configurations_not_offered_are_refused_by_name(native_lib):
    assert N.check_configuration() == (_capi.HG_NORM_AREA, True)
    assert N.check_configuration("eyes_inferred-mouth_areaZ", rotation_mode="noRotation") == (_capi.HG_NORM_AREAZ, False)
    for kw, word in ((dict(normalization_method="eyes_mouth_area"), "eyes_mouth_area"), (dict(centering_mode="eyeL"), "eyeL"),
                     (dict(centering_mode="noFace"), "noFace"), (dict(centering_mode="mid_eyes_mouth"), "mid_eyes_mouth"),
                     (dict(rotation_mode="Random"), "Random"), (dict(integer_rotation_center=False), "integer_rotation_center"),
                     (dict(allow_random_background=True), "allow_random_background"), (dict(convert_format="RGB"), "RGB")):
        with pytest.raises(ValueError, match=word):
            N.check_configuration(**kw)
    with pytest.raises(ValueError, match="eyes_mouth_area"):
        N.geometry([[1, 2, 3, 4]], (10, 10), method="eyes_mouth_area")
    with pytest.raises(ValueError, match="preset"):
        N.FaceNormalizer(preset="gender")
    with pytest.raises(ValueError):
        N.geometry([[1, 2, 3]], (10, 10))
    with pytest.raises(ValueError):
        N.geometry([[1, 2, 3, 4]], (10, 10), out_size=(0, 4))
    with pytest.raises(ValueError):
        N.normalize_host(np.zeros((4, 4), np.float32), [[1, 2, 3, 4]])
    with pytest.raises(ValueError):
        N.normalize_host(np.zeros((4, 4, 3), np.uint8), [[1, 2, 3, 4]])
    fn = N.FaceNormalizer(preset="age")
    assert fn.out_size == (256, 260) and fn.method == "eyes_inferred-mouth_areaZ"
    fn = N.FaceNormalizer(preset="pose", out_size=(64, 48))
    assert fn.out_size == (64, 48) and fn.method == "eyes_inferred-mouth_area"


def test_c_entries_refuse_bad_arguments(native_lib):
    L = native_lib
    frame = NC.noise_frame(16, 12)
    g = N.geometry([[4.0, 5.0, 9.0, 6.0]], (16, 12), (8, 6))
    out = np.full((1, 48), 7, np.uint8)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    call = lambda **kw: L.hg_normalize_faces_host(*[dict(dict(frame=p(frame), h=12, w=16, ld=16, g=p(g), n=1, ow=8, oh=6, out=p(out), ldo=48), **kw)[k]
                                                    for k in ("frame", "h", "w", "ld", "g", "n", "ow", "oh", "out", "ldo")])
    assert call() == _capi.HG_OK and out.any() and np.array_equal(out.reshape(6, 8), NC.pil_normalize(frame, g[0], (8, 6)))
    out[:] = 7
    for kw in (dict(frame=None), dict(g=None), dict(out=None), dict(h=0), dict(w=-1), dict(ld=15), dict(ldo=47), dict(ow=0), dict(oh=4097), dict(n=-1),
               dict(w=15, ld=16), dict(h=20)):      # (the last two: a geom whose crop size belongs to another frame size)
        assert call(**kw) == _capi.HG_ERR_ARG, kw
        assert L.hg_last_error()
    assert np.all(out == 7)
    assert call(n=0) == _capi.HG_OK and np.all(out == 7)
    c = _capi.HgNormConsts(8, 6, 0, 1)
    e = np.array([[4.0, 5.0, 9.0, 6.0]])
    assert L.hg_normalize_geometry_host(p(e), 1, 16, 12, C.byref(c), p(g)) == _capi.HG_OK
    assert L.hg_normalize_geometry_host(p(e), 1, 16, 12, None, p(g)) == _capi.HG_ERR_ARG
    assert L.hg_normalize_geometry_host(None, 1, 16, 12, C.byref(c), p(g)) == _capi.HG_ERR_ARG
    assert L.hg_normalize_geometry_host(p(e), 1, 0, 12, C.byref(c), p(g)) == _capi.HG_ERR_ARG
    assert L.hg_normalize_geometry_host(p(e), 1, 16, 12, C.byref(_capi.HgNormConsts(8, 6, 2, 1)), p(g)) == _capi.HG_ERR_ARG
    assert L.hg_normalize_geometry_host(p(e), 0, 16, 12, C.byref(c), None) == _capi.HG_OK


def test_device_kernels_have_no_contracted_fma(tmp_path):
    """hg_normalize.hip claims PIL's doubles, one rounding per operation: compiled to gfx950 assembly with the build's flags and again
    with -ffp-contract=off, its kernels hold the same number of float64 fused multiply-adds (tests/test_fp_contract.py)."""
    from tests.test_fp_contract import _fma_counts, _kernels
    counts = {}
    for tag, extra in (("built", []), ("off", ["-ffp-contract=off"])):
        out = tmp_path / (tag + ".s")
        cmd = [build.HIPCC] + build.FLAGS + ["-x", "hip", "--cuda-device-only", "-S"] + extra + [os.path.join(build.CSRC, "hg_normalize.hip"), "-o", str(out)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
        assert r.returncode == 0, r.stdout.decode(errors="replace")[-2000:]
        counts[tag] = _fma_counts(str(out))
    for name in ("k_norm_rect", "k_norm_cut<"):
        built, off = _kernels(counts["built"], name), _kernels(counts["off"], name)
        assert built and set(built) == set(off), (name, sorted(counts["built"]))
        assert built == off, (name, built, off)      # (the ones that remain are the division's own sequence in the cut's (hi - lo) / n)


def test_host_unit_under_sanitizers(tmp_path):
    """tests/normalize_driver.cpp with csrc/hg_normalize.cpp, built with -fsanitize=address,undefined and run as a program: faces all
    around exact-size frames, pitched rows and images with guard bytes, refused faces, both paths, the refusals."""
    exe = str(tmp_path / "normalize_driver")
    cmd = [build.CXX, "-O1", "-g", "-std=c++17", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           os.path.join(ROOT, "tests", "normalize_driver.cpp"), os.path.join(build.CSRC, "hg_normalize.cpp"), "-o", exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode(errors="replace")[-3000:]
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    out = r.stdout.decode(errors="replace")
    assert r.returncode == 0 and "normalize_driver: ok" in out, out[-3000:]
