"""GPU: colour frames — PIL's "L" conversion on the device (hg_frame_to_gray_device), windows cut straight from a colour frame
(hg_patcher_extract_format_device), and the cascade, the tracker and the eye step fed RGB / BGR(A) frames (hg_cascade_set_frame_format).

PIL called here is the reference for every pixel (``array_equal``; BGR / BGRA: PIL on the channel-swapped array), and the cascade on a
colour frame must give, array for array, what the grey cascade gives on the frame PIL converts it to.  Small shapes: three-row frames
of 1 .. 65 pixels for the conversion (every ``w % 4`` tail, one thread and several threads per row), the 53 x 37 frame of
tests/filters_cases.py for the windows, the 160 x 120 frame and the T5L-16 cascade of tests/test_filters_gpu.py."""
import ctypes as C

import numpy as np
import pytest

from pyfaceanalysis_amd import _capi, frames, grid
from tests import color_cases as CC
from tests import filters_cases as FC
from tests.test_filters_gpu import SF, SUB, K, Rig, assert_same_detection, composed_faces

pytestmark = pytest.mark.gpu

WIDTHS = (1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 63, 64, 65)
DT = {np.uint8: _capi.HG_U8, np.float32: _capi.HG_F32}
FILTERS = [3] * 10                # as test_detect_faces_and_tracked_frame_bicubic, which establishes a face on this frame
TWIN_SEED = 2801


@pytest.fixture(scope="module")
def pt(native_lib):
    from pyfaceanalysis_amd.patches import Patcher
    p = Patcher()
    yield p
    p.close()


@pytest.fixture(scope="module")
def rig(native_lib, nets, pt):
    r = Rig(nets, pt)
    yield r
    r.close()


def stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


# ---- 1. to_gray against PIL --------------------------------------------------------------------------------------------------------
class Dst(object):
    """An (h, w) output view inside a buffer of 7s: dense (4-aligned rows: one packed store per four pixels), rows w + 1 apart, or a
    dense view that starts 3 bytes off alignment (byte stores)."""

    def __init__(self, name, h, w):
        import torch
        self.name = name
        ld, off = (w + 1, 0) if name == "ld+1" else (w, 3 if name == "off3" else 0)
        self.buf = torch.full((off + h * ld + 5,), 7, dtype=torch.uint8, device="cuda")
        self.view = torch.as_strided(self.buf, (h, w), (ld, 1), off)
        self.mask = np.ones(self.buf.shape[0], dtype=bool)
        idx = off + np.arange(h)[:, None] * ld + np.arange(w)[None, :]
        self.mask[idx.reshape(-1)] = False
        assert (self.view.data_ptr() % 4 == 0) == (name != "off3")

    def check(self, want, what):
        assert np.array_equal(self.view.cpu().numpy(), want), (what, self.name)
        assert np.all(self.buf.cpu().numpy()[self.mask] == 7), (what, self.name, "bytes outside the output view changed")


@pytest.mark.parametrize("fmt", CC.COLOR_FORMATS)
def test_to_gray_small_shapes_equal_pil(native_lib, fmt):
    h = 3
    for w in WIDTHS:
        arr = CC.noise_frame(h, w, fmt, 7200 + w)
        want = CC.pil_gray(arr, fmt)
        for lname in CC.COLOR_LAYOUTS:
            lay = CC.ColorLayout(arr, lname)
            for dname in ("dense", "ld+1", "off3"):
                dst = Dst(dname, h, w)
                assert frames.to_gray(lay.view, fmt, out=dst.view) is dst.view
                dst.check(want, (fmt, w, lname))
                lay.assert_untouched()
            assert np.array_equal(frames.to_gray(lay.view, fmt).cpu().numpy(), want)      # out=None: a new dense tensor


def test_to_gray_gray_format_is_a_pitched_copy(native_lib):
    import torch
    g = np.random.default_rng(7210).integers(0, 256, (5, 13), dtype=np.uint8)
    wide = torch.full((5, 20), 3, dtype=torch.uint8, device="cuda")
    wide[:, :13] = torch.from_numpy(g).cuda()
    for dname in ("dense", "ld+1", "off3"):
        dst = Dst(dname, 5, 13)
        frames.to_gray(wide[:, :13], "L", out=dst.view)
        dst.check(g, "L")


@pytest.mark.parametrize("fmt,shape", [("RGB", (70000, 3)), ("BGRA", (3, 70000)), ("BGR", (3, 70000)), ("RGBA", (70000, 3)), ("RGB", (524300, 3))])
def test_to_gray_beyond_the_grid_limits(native_lib, fmt, shape):
    """70000 rows and 70000 columns: more rows / more pixels of a row than one dimension of a grid of one-row workgroups holds.  The
    launcher gives a narrow frame eight rows per workgroup, so its grid takes further trips in y only beyond 65535 * 8 = 524280 rows:
    the 524300-row frame (1.6 M pixels) is the smallest that reaches that path."""
    import torch
    arr = CC.noise_frame(shape[0], shape[1], fmt, 7220)
    got = frames.to_gray(torch.from_numpy(arr).cuda(), fmt)
    assert np.array_equal(got.cpu().numpy(), CC.pil_gray(arr, fmt))


# ---- 2. every colour ---------------------------------------------------------------------------------------------------------------
def test_every_color_on_the_device(native_lib):
    import torch
    rgb, want = CC.all_colors()
    got = frames.to_gray(torch.from_numpy(rgb).cuda(), "RGB")
    assert np.array_equal(got.cpu().numpy(), want)
    del got
    bgra = CC.as_format(rgb, "BGRA", seed=1)                # R and B swapped, the fourth byte noise
    assert bgra.shape == (4096, 4096, 4) and len(np.unique(bgra[::16, ::16, 3])) > 200
    got = frames.to_gray(torch.from_numpy(bgra).cuda(), "BGRA")
    assert np.array_equal(got.cpu().numpy(), want)


# ---- 3. the format gather and the prescale -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", CC.COLOR_FORMATS)
def test_format_gather_equals_gather_of_the_converted_frame(pt, fmt):
    import torch
    L = _capi.lib()
    boxes = FC.boxes()
    bdev = torch.from_numpy(boxes).cuda()
    n = len(boxes)
    arr = CC.noise_frame(FC.FRAME_H, FC.FRAME_W, fmt, 7230)
    gray = CC.pil_gray(arr, fmt)
    gdev = torch.from_numpy(gray).cuda()
    lays = [CC.ColorLayout(arr, name) for name in CC.COLOR_LAYOUTS]
    for size in ((37, 21), (48, 5), (16, 12)):
        row = size[0] * size[1]
        pil = FC.pil_windows(gray, boxes, np.zeros(n), size, 0)
        assert pil[:14].any(axis=1).all() and not pil[14:16].any()          # inside / over the edges: pixels; outside: none
        for dt, tdt in ((np.uint8, torch.uint8), (np.float32, torch.float32)):
            want = torch.full((n, row), 5, dtype=tdt, device="cuda")
            assert L.hg_patcher_extract_device(pt._handle(), gdev.data_ptr(), _capi.HG_U8, FC.FRAME_H, FC.FRAME_W, FC.FRAME_W, bdev.data_ptr(), n, size[0],
                                               size[1], want.data_ptr(), DT[dt], row, stream()) == _capi.HG_OK
            assert np.array_equal(want.cpu().numpy(), pil.astype(dt))
            for lay in lays:
                got = torch.full((n, row), 9, dtype=tdt, device="cuda")
                rc = L.hg_patcher_extract_format_device(pt._handle(), frames.FORMATS[fmt], lay.view.data_ptr(), FC.FRAME_H, FC.FRAME_W, lay.ld_bytes,
                                                        bdev.data_ptr(), n, size[0], size[1], got.data_ptr(), DT[dt], row, stream())
                assert rc == _capi.HG_OK
                assert torch.equal(got, want), (fmt, size, dt, lay)
                lay.assert_untouched()
    # HG_FRAME_L through the same entry is hg_patcher_extract_device
    got = torch.full((n, 192), 9, dtype=torch.uint8, device="cuda")
    assert L.hg_patcher_extract_format_device(pt._handle(), _capi.HG_FRAME_L, gdev.data_ptr(), FC.FRAME_H, FC.FRAME_W, FC.FRAME_W, bdev.data_ptr(), n, 16, 12,
                                              got.data_ptr(), _capi.HG_U8, 192, stream()) == _capi.HG_OK
    assert np.array_equal(got.cpu().numpy(), FC.pil_windows(gray, boxes, np.zeros(n), (16, 12), 0))


def color_cascade(rig, fmt, formats=FILTERS):
    from pyfaceanalysis_amd.cascade import DeviceCascade
    dc = DeviceCascade(rig.stages, SUB, K, rig.pipe, interpolation_formats=formats, frame_format=fmt)
    rig.open.append(dc)
    return dc


def test_prescale_of_color_frames_equals_pil(rig):
    import torch
    from PIL import Image
    dc = color_cascade(rig, "RGB")
    rgb = CC.noise_frame(1080, 1920, "RGB", 7240)
    assert grid.prescaled_size(1920, 1080) == (1000, 562)
    want = np.asarray(Image.fromarray(rgb, "RGB").convert("L").resize((1000, 562), Image.NEAREST))
    fdev = torch.from_numpy(rgb).cuda()
    for _ in range(2):
        small = dc.prescale(fdev)
        assert tuple(small.shape) == (562, 1000) and np.array_equal(small.cpu().numpy(), want)
    for fmt in ("RGB", "BGRA"):
        arr = CC.noise_frame(37, 53, fmt, 7241)
        pw, ph = grid.prescaled_size(53, 37, 24)
        assert (pw, ph) != (53, 37)
        want = np.asarray(Image.fromarray(CC.pil_gray(arr, fmt), "L").resize((pw, ph), Image.NEAREST))
        if fmt == "RGB":
            assert np.array_equal(want, np.asarray(Image.fromarray(arr, "RGB").convert("L").resize((pw, ph), Image.NEAREST)))
        dcf = color_cascade(rig, fmt)
        for name in CC.COLOR_LAYOUTS:
            lay = CC.ColorLayout(arr, name)
            assert np.array_equal(dcf.prescale(lay.view, prescale_size=24).cpu().numpy(), want), (fmt, name)
            lay.assert_untouched()
        # no shrinking needed: the converted frame, in a tensor of the cascade's
        whole = dcf.prescale(CC.ColorLayout(arr, "roi").view)
        assert tuple(whole.shape) == (37, 53) and np.array_equal(whole.cpu().numpy(), CC.pil_gray(arr, fmt))


# ---- 4. the cascade on colour equals the cascade on grey -----------------------------------------------------------------------------
class Answers(object):
    """What the grey cascade gives on rig.fdev: detect, detect_frame, detect_faces and two tracker steps."""

    def __init__(self, rig):
        from pyfaceanalysis_amd.tracking import FaceTracker
        self.dc, self.loc = rig.cascade(FILTERS), rig.locator(3)
        self.detect = self.dc.detect(rig.fdev, smallest_face=SF)
        self.explicit = self.dc.detect(rig.fdev, smallest_face=SF, windows=(rig.boxes, rig.level))
        self.frame = self.dc.detect_frame(rig.fdev, smallest_face=SF)
        self.faces = self.dc.detect_faces(rig.fdev, self.loc, smallest_face=SF)
        tr = FaceTracker(self.dc, self.loc, smallest_face=SF)
        try:
            self.steps = [tr.step(rig.fdev), tr.step(rig.fdev)]
        finally:
            tr.close()


@pytest.fixture(scope="module")
def answers(rig):
    a = Answers(rig)
    # the comparisons below cannot pass on nothing: a face, found by both paths, and a tracked second step
    want, n_before = composed_faces(a.dc, a.loc, rig.fdev, a.frame)
    assert len(a.frame["coords"]) >= 1 and len(want) >= 1 and np.array_equal(a.faces["faces"], want) and a.faces["n_before_purge"] == n_before
    assert a.steps[0]["tracked"] is False and a.steps[1]["tracked"] is True
    return a


@pytest.fixture(scope="module")
def twin(rig):
    """The colour twin of the rig's frame, with what makes it a fair test asserted."""
    rgb, fell_back = CC.color_twin(rig.frame, TWIN_SEED)
    assert np.array_equal(CC.pil_gray(rgb, "RGB"), rig.frame)
    swapped_differs = (CC.pil_gray(rgb, "BGR") != rig.frame).mean()
    print("colour twin: %.1f %% of the pixels fell back to (g, g, g); a swap of R and B changes %.1f %% of PIL's grey" % (100 * fell_back.mean(), 100 * swapped_differs))
    assert fell_back.mean() <= 0.10
    assert swapped_differs >= 0.50
    return rgb


def assert_same_faces(got, want, what):
    assert got["faces"].shape == want["faces"].shape and np.array_equal(got["faces"], want["faces"]), what
    for key in ("n_before_purge", "counts", "rows_executed"):
        assert got[key] == want[key], (what, key)
    if "tracked" in want:
        assert got["tracked"] is want["tracked"] and got["n_windows"] == want["n_windows"], what


def run_all(dc, loc, frame, rig):
    from pyfaceanalysis_amd.tracking import FaceTracker
    out = dict(detect=dc.detect(frame, smallest_face=SF), explicit=dc.detect(frame, smallest_face=SF, windows=(rig.boxes, rig.level)),
               frame=dc.detect_frame(frame, smallest_face=SF), faces=dc.detect_faces(frame, loc, smallest_face=SF))
    tr = FaceTracker(dc, loc, smallest_face=SF)
    try:
        out["steps"] = [tr.step(frame), tr.step(frame)]
    finally:
        tr.close()
    return out


def assert_all_equal(got, a, what):
    for key in ("detect", "explicit", "frame"):
        assert_same_detection(got[key], getattr(a, key), (what, key))
        assert got[key]["counts"] == getattr(a, key)["counts"] and got[key]["rows_executed"] == getattr(a, key)["rows_executed"], (what, key)
    assert_same_faces(got["faces"], a.faces, (what, "detect_faces"))
    for i in range(2):
        assert_same_faces(got["steps"][i], a.steps[i], (what, "step", i))


@pytest.mark.parametrize("fmt", ("RGB", "BGRA"))
def test_cascade_on_color_equals_cascade_on_gray(rig, answers, twin, fmt):
    dc = color_cascade(rig, fmt)
    arr = CC.as_format(twin, fmt, seed=2)
    assert np.array_equal(CC.pil_gray(arr, fmt), rig.frame)
    for name in ("dense", "roi"):
        lay = CC.ColorLayout(arr, name)
        assert_all_equal(run_all(dc, answers.loc, lay.view, rig), answers, (fmt, name))
        lay.assert_untouched()
        assert np.array_equal(dc.prescale(lay.view).cpu().numpy(), rig.frame)          # the grey frame the cascade read


# ---- 5. the same through the prescale ------------------------------------------------------------------------------------------------
def embedded(twin, k, fmt, seed):
    """A (120 k, 160 k) colour noise frame whose pixels [1::k, 1::k] are the twin: PIL's NEAREST resize to 160 x 120 picks exactly those."""
    from PIL import Image
    big = CC.noise_frame(120 * k, 160 * k, "RGB", seed)
    big[1::k, 1::k] = twin
    assert np.array_equal(np.asarray(Image.fromarray(big, "RGB").convert("L").resize((160, 120), Image.NEAREST)), CC.pil_gray(twin, "RGB"))
    return CC.as_format(big, fmt, seed=seed)


@pytest.mark.parametrize("fmt", ("RGB", "BGRA"))
def test_cascade_on_color_through_the_prescale(rig, answers, twin, fmt):
    import torch
    from pyfaceanalysis_amd.tracking import FaceTracker
    dev = {k: torch.from_numpy(embedded(twin, k, fmt, 7250 + k)).cuda() for k in (2, 3)}
    dev[1] = torch.from_numpy(CC.as_format(twin, fmt, seed=3)).cuda()
    dc = color_cascade(rig, fmt)
    for k in (2, 3):
        assert_same_faces(dc.detect_faces(dev[k], answers.loc, smallest_face=SF, prescale_size=160), answers.faces, (fmt, k))
        assert_same_detection(dc.detect_frame(dev[k], smallest_face=SF, prescale_size=160), answers.frame, (fmt, k))
        assert np.array_equal(dc.prescale(dev[k], prescale_size=160).cpu().numpy(), rig.frame)
        tr = FaceTracker(dc, answers.loc, smallest_face=SF, prescale_size=160)
        try:
            for i in range(2):
                assert_same_faces(tr.step(dev[k]), answers.steps[i], (fmt, k, "step", i))
        finally:
            tr.close()
    # six frames through ONE cascade: the prescale buffer is reused and grown, the converted-frame buffer used and bypassed; every frame
    # against a cascade created for it alone
    one = color_cascade(rig, fmt)
    for i, k in enumerate((2, 3, 1, 3, 2, 1)):
        fresh = color_cascade(rig, fmt)
        got = one.detect_faces(dev[k], answers.loc, smallest_face=SF, prescale_size=160)
        assert_same_faces(got, fresh.detect_faces(dev[k], answers.loc, smallest_face=SF, prescale_size=160), (fmt, "frame", i, k))
        assert_same_faces(got, answers.faces, (fmt, "frame", i, k, "grey"))
        rig.open.remove(fresh)
        fresh.close()


# ---- 6. the format changes between frames ---------------------------------------------------------------------------------------------
def test_set_frame_format_between_frames(rig, answers, twin):
    import torch
    dc = rig.cascade(FILTERS)
    rgb = torch.from_numpy(twin).cuda()
    other = np.random.default_rng(7260).integers(0, 256, (120, 160), dtype=np.uint8)      # a second grey frame: another answer
    odev = torch.from_numpy(other).cuda()
    want_other = answers.dc.detect_frame(odev, smallest_face=SF)
    assert not np.array_equal(want_other["coords"], answers.frame["coords"])
    assert_same_detection(dc.detect_frame(rig.fdev, smallest_face=SF), answers.frame, "grey, before")
    dc.set_frame_format("RGB")
    assert_same_detection(dc.detect_frame(rgb, smallest_face=SF), answers.frame, "RGB")
    assert_same_faces(dc.detect_faces(rgb, answers.loc, smallest_face=SF), answers.faces, "RGB faces")
    with pytest.raises(ValueError):
        dc.detect_frame(rig.fdev, smallest_face=SF)                 # a grey frame now
    dc.set_frame_format("L")
    assert_same_detection(dc.detect_frame(odev, smallest_face=SF), want_other, "grey, after")
    assert_same_detection(dc.detect_frame(rig.fdev, smallest_face=SF), answers.frame, "grey, after")
    with pytest.raises(ValueError):
        dc.detect_frame(rgb, smallest_face=SF)


# ---- 7. the eye step -------------------------------------------------------------------------------------------------------------------
def test_eye_locator_on_a_color_frame(rig, twin):
    import torch
    loc = rig.locator(3)
    nz = np.flatnonzero(np.abs(rig.face_angles) > 1.0)[:4]
    boxes, angles = rig.face_boxes[nz], rig.face_angles[nz]
    want = loc.locate(rig.fdev, boxes, angles, return_patches=True)
    assert want["patches"].shape == (8, 256) and want["patches"].any()
    for fmt, name in (("RGB", "dense"), ("RGB", "roi"), ("BGRA", "pad1")):
        lay = CC.ColorLayout(CC.as_format(twin, fmt, seed=4), name)
        got = loc.locate(lay.view, boxes, angles, return_patches=True, frame_format=fmt)
        for key in ("patches", "eye_coords", "too_far", "reg"):
            assert np.array_equal(got[key], want[key]), (fmt, name, key)
        lay.assert_untouched()
    with pytest.raises(ValueError):
        loc.locate(rig.fdev, boxes, angles, frame_format="RGB")
    with pytest.raises(ValueError):
        loc.locate(torch.from_numpy(twin).cuda(), boxes, angles)


# ---- 8. refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handles_usable(rig, pt, answers, twin):
    import torch
    from pyfaceanalysis_amd.cascade import frame_levels
    L = _capi.lib()
    RGB, RGBA = _capi.HG_FRAME_RGB, _capi.HG_FRAME_RGBA
    h, w = 5, 6
    arr = CC.noise_frame(h, w, "RGB", 7270)
    want = CC.pil_gray(arr, "RGB")
    src = torch.from_numpy(arr).cuda()
    dst = torch.full((h, w), 9, dtype=torch.uint8, device="cuda")
    sp, dp = src.data_ptr(), dst.data_ptr()
    for args in ((0, sp, 5, h, w, w * 3, dp, w), (0, sp, -1, h, w, w * 3, dp, w), (0, sp, RGB, h, w, w * 3 - 1, dp, w), (0, sp, RGBA, h, w, w * 3, dp, w),
                 (0, sp, RGB, h, w, w * 3, dp, w - 1), (0, None, RGB, h, w, w * 3, dp, w), (0, sp, RGB, h, w, w * 3, None, w), (0, sp, RGB, 0, w, w * 3, dp, w),
                 (0, sp, RGB, h, 0, w * 3, dp, w)):
        assert L.hg_frame_to_gray_device(*args, stream()) == _capi.HG_ERR_ARG, args
        torch.cuda.synchronize()
        assert bool((dst == 9).all())
        assert L.hg_frame_to_gray_device(0, sp, RGB, h, w, w * 3, dp, w, stream()) == _capi.HG_OK
        assert np.array_equal(dst.cpu().numpy(), want)
        dst.fill_(9)
    # the format gather
    boxes = torch.tensor([[0.0, 0.0, float(w), float(h)]], dtype=torch.float64, device="cuda")
    out = torch.full((1, w * h), 9, dtype=torch.uint8, device="cuda")

    def gather(fmt, ld):
        return L.hg_patcher_extract_format_device(pt._handle(), fmt, sp, h, w, ld, boxes.data_ptr(), 1, w, h, out.data_ptr(), _capi.HG_U8, w * h, stream())
    for fmt, ld in ((7, w * 3), (RGB, w * 3 - 1), (RGBA, w * 4 - 1)):
        assert gather(fmt, ld) == _capi.HG_ERR_ARG
        torch.cuda.synchronize()
        assert bool((out == 9).all())
        assert gather(RGB, w * 3) == _capi.HG_OK and np.array_equal(out.cpu().numpy().reshape(h, w), want)
        out.fill_(9)
    # the cascade: an unknown format changes nothing; a colour frame whose rows are closer than their bytes is refused by every entry
    dc = color_cascade(rig, "RGB")
    rgb = torch.from_numpy(twin).cuda()
    assert_same_detection(dc.detect_frame(rgb, smallest_face=SF), answers.frame, "before")
    for bad in (5, -1):
        assert L.hg_cascade_set_frame_format(dc._handle(), bad) == _capi.HG_ERR_ARG
        with pytest.raises(ValueError):
            dc.set_frame_format(bad)
    assert L.hg_cascade_set_frame_format(None, RGB) == _capi.HG_ERR_ARG
    levels, n_levels, n0 = frame_levels(160, 120, SF, rig.pipe, SUB)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    coords, angles, oidx, conf = np.full((n0, 4), -3.0), np.empty(n0), np.empty(n0, dtype=np.int32), np.empty(n0)
    counts, n_out, rows = np.zeros(len(rig.stages), dtype=np.int32), C.c_int64(), C.c_int64()
    for ld, pre in ((160 * 3 - 1, (0, 0)), (160, (0, 0)), (160 * 3 - 1, (80, 60))):
        rc = L.hg_cascade_detect_frame_device(dc._handle(), rgb.data_ptr(), 120, 160, ld, pre[0], pre[1], levels, n_levels, vp(coords), vp(angles), vp(oidx), vp(conf), n0,
                                              C.byref(n_out), vp(counts), C.byref(rows), stream())
        assert rc == _capi.HG_ERR_ARG and np.all(coords == -3.0), (ld, pre)
        rc = L.hg_cascade_detect_levels_device(dc._handle(), rgb.data_ptr(), 120, 160, ld, levels, n_levels, vp(coords), vp(angles), vp(oidx), vp(conf), n0,
                                               C.byref(n_out), vp(counts), C.byref(rows), stream())
        assert rc == _capi.HG_ERR_ARG and np.all(coords == -3.0), (ld, pre)
        assert_same_detection(dc.detect_frame(rgb, smallest_face=SF), answers.frame, ("after", ld))
    # the Python checker on device tensors
    gray_dc = answers.dc
    for cascade, frame in ((dc, rig.fdev), (gray_dc, rgb), (dc, rgb[:, :, :2]), (dc, torch.from_numpy(CC.as_format(twin, "RGBA")).cuda()), (dc, rgb[:, ::2])):
        for call in (lambda: cascade.detect(frame, smallest_face=SF), lambda: cascade.detect_frame(frame, smallest_face=SF),
                     lambda: cascade.detect_faces(frame, answers.loc, smallest_face=SF), lambda: cascade.prescale(frame)):
            with pytest.raises(ValueError):
                call()
    bad_out = torch.empty((120, 161), dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError):
        frames.to_gray(rgb, "RGB", out=bad_out)
    assert_same_detection(dc.detect_frame(rgb, smallest_face=SF), answers.frame, "at the end")
