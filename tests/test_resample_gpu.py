"""GPU: PIL's ``Image.resize`` with a filter on the device (hg_patcher_resize_device, csrc/hg_resample.hip) and as the cascade's
prescale (hg_cascade_set_prescale_filter).  PIL called here is the reference for every byte (``array_equal``); the cascade with a
prescale filter must give, array for array, what the same cascade gives on the frame PIL resized.

Small shapes: the host test's list plus the kernels' edges — 130 x 70 -> 65 x 17 is one column and one row past the fused kernel's
64 x 16 tile; 300 x 40 -> 7 x 40 with LANCZOS has 261 taps; 40 x 3000 -> 20 x 100 needs 480 intermediate rows per tile, more than the
fused kernel holds, so both passes run as two launches; 8 x 3000 -> 4 x 100 is an image so tall that PIL resizes its height first;
5 x 9 is a source narrower than 8 bytes; 90 x 61 -> 43 x 29 is an output width that is no multiple of 4.  ``flags`` 1 forces the two
launches and 2 the fused kernel wherever it is eligible, so both are compared on every kind of source whatever the default is.
The cascade runs on 320 x 180 frames prescaled to 160 x 90 with 16 x 16 windows and the T5L-16 network."""
import numpy as np
import pytest

from pyfaceanalysis_amd import _capi, frames, grid
from tests import color_cases as CC
from tests import eyes_restate as ER
from tests import resample_cases as RC

pytestmark = pytest.mark.gpu

CONTRAST = (128.0, 48.0)          # as tests/test_eyes_gpu.py
SUB, K, SF = (16, 16), 10, 0.3    # as tests/test_filters_gpu.py
IDS = lambda s: "%dx%d-%dx%d" % s


@pytest.fixture(scope="module")
def pt(native_lib):
    from pyfaceanalysis_amd.patches import Patcher
    p = Patcher()
    yield p
    p.close()


def dev(a):
    import torch
    return torch.from_numpy(np.array(a, copy=True)).cuda()


class Dst(object):
    """An (h, w) or (h, w, c) output view inside a buffer of 7s: rows ``ld`` bytes apart, starting ``off`` bytes into the buffer."""

    def __init__(self, h, w, c, ld, off):
        import torch
        self.buf = torch.full((off + h * ld + 5,), 7, dtype=torch.uint8, device="cuda")
        self.view = torch.as_strided(self.buf, (h, w) if c == 1 else (h, w, c), (ld, 1) if c == 1 else (ld, c, 1), off)
        self.mask = np.ones(self.buf.shape[0], dtype=bool)
        self.mask[(off + np.arange(h)[:, None] * ld + np.arange(w * c)[None, :]).reshape(-1)] = False

    def check(self, want, what):
        assert np.array_equal(self.view.cpu().numpy(), want), what
        assert np.all(self.buf.cpu().numpy()[self.mask] == 7), (what, "bytes outside the output view changed")


# ---- 1. the matrix against PIL ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", RC.GPU_SHAPES + [RC.TALL, RC.STEEP], ids=IDS)
def test_gray_equals_pil(pt, shape):
    w, h, ow, oh = shape
    for kind in RC.KINDS:
        img = RC.gray_frame(w, h, kind)
        d = dev(img)
        for filt in RC.FILTERS:
            got = frames.resize(d, (ow, oh), filt, patcher=pt)
            assert tuple(got.shape) == (oh, ow) and np.array_equal(got.cpu().numpy(), RC.pil_resize(img, (ow, oh), filt)), (shape, kind, filt)
        assert np.array_equal(d.cpu().numpy(), img)


def test_wide_kernel(pt):
    w, h, ow, oh = RC.WIDE_KERNEL
    img = RC.gray_frame(w, h, "noise")
    want = RC.pil_resize(img, (ow, oh), "LANCZOS")
    for flags in (0, 1, 2):
        assert np.array_equal(frames.resize(dev(img), (ow, oh), "LANCZOS", patcher=pt, flags=flags).cpu().numpy(), want), flags


@pytest.mark.parametrize("ld_extra,off", [(0, 0), (2, 0), (0, 3), (1, 1)])
def test_output_width_not_a_multiple_of_four_and_odd_destination_strides(pt, ld_extra, off):
    w, h, ow, oh = 90, 61, 43, 29
    img = RC.gray_frame(w, h, "noise")
    for filt in ("BILINEAR", "LANCZOS"):
        want = RC.pil_resize(img, (ow, oh), filt)
        for flags in (0, 1, 2):
            dst = Dst(oh, ow, 1, ow + ld_extra, off)
            assert frames.resize(dev(img), (ow, oh), filt, out=dst.view, patcher=pt, flags=flags) is dst.view
            dst.check(want, (filt, flags))
    rgb = RC.color_frame(w, h, "RGB")
    for flags in (0, 1, 2):                               # a colour source
        dst = Dst(oh, ow, 1, ow + ld_extra, off)
        frames.resize(dev(rgb), (ow, oh), "BICUBIC", "RGB", out=dst.view, patcher=pt, flags=flags)
        dst.check(RC.pil_gray_resize(rgb, "RGB", (ow, oh), "BICUBIC"), ("RGB", flags))
    # one pass only, straight into the pitched destination
    for size in ((43, 61), (90, 29)):
        dst = Dst(size[1], size[0], 1, size[0] + ld_extra, off)
        frames.resize(dev(img), size, "BICUBIC", out=dst.view, patcher=pt)
        dst.check(RC.pil_resize(img, size, "BICUBIC"), size)


# ---- 2. one launch (flags 2) against two (flags 1) against the default ------------------------------------------------------------------
@pytest.mark.parametrize("shape", [s for s in RC.GPU_SHAPES if s[0] != s[2] and s[1] != s[3]], ids=IDS)
def test_one_launch_and_two_launches_give_the_same_bytes(pt, shape):
    w, h, ow, oh = shape
    img, rgb = RC.gray_frame(w, h, "noise"), RC.color_frame(w, h, "RGB")
    cases = [(img, "L", "L"), (rgb, "RGB", "L"), (rgb, "RGB", "RGB")]
    for filt in RC.FILTERS:
        for arr, fmt, ofmt in cases:
            got = [frames.resize(dev(arr), (ow, oh), filt, fmt, ofmt, patcher=pt, flags=f).cpu().numpy() for f in (2, 1, 0)]
            assert np.array_equal(got[0], got[1]) and np.array_equal(got[0], got[2]), (shape, filt, fmt, ofmt)


# ---- 3. crops of larger frames, colour formats --------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", CC.COLOR_FORMATS)
@pytest.mark.parametrize("shape", [(37, 23, 16, 9), (130, 70, 65, 17), (64, 48, 33, 48), (50, 40, 50, 17), (5, 9, 3, 4), RC.TALL, RC.STEEP], ids=IDS)
def test_color_frames_in_every_layout(pt, fmt, shape):
    w, h, ow, oh = shape
    arr = RC.color_frame(w, h, fmt)
    for filt in ("BILINEAR", "BICUBIC", "LANCZOS"):
        want_gray, want_color = RC.pil_gray_resize(arr, fmt, (ow, oh), filt), RC.pil_resize(arr, (ow, oh), filt)
        for name in CC.COLOR_LAYOUTS:
            lay = CC.ColorLayout(arr, name)
            for flags in (0, 1, 2):
                assert np.array_equal(frames.resize(lay.view, (ow, oh), filt, fmt, patcher=pt, flags=flags).cpu().numpy(), want_gray), (fmt, filt, name, flags)
                got = frames.resize(lay.view, (ow, oh), filt, fmt, fmt, patcher=pt, flags=flags)
                assert tuple(got.shape) == (oh, ow, CC.BPP[fmt]) and np.array_equal(got.cpu().numpy(), want_color), (fmt, filt, name, flags)
            lay.assert_untouched()
    # colour output into a pitched destination that starts at an odd byte
    c = CC.BPP[fmt]
    dst = Dst(oh, ow, c, ow * c + 3, 1)
    frames.resize(CC.ColorLayout(arr, "roi").view, (ow, oh), "HAMMING", fmt, fmt, out=dst.view, patcher=pt)
    dst.check(RC.pil_resize(arr, (ow, oh), "HAMMING"), (fmt, "pitched colour output"))


def test_gray_crop_at_an_odd_byte(pt):
    w, h, ow, oh = 37, 23, 16, 9
    img = RC.gray_frame(w, h, "noise")
    big = np.random.default_rng(3).integers(1, 256, (h + 4, w + 20), dtype=np.uint8)
    big[2:2 + h, 7:7 + w] = img
    d = dev(big)
    view = d[2:2 + h, 7:7 + w]
    assert view.data_ptr() % 2 == 1 and view.stride(0) != w
    for filt in RC.FILTERS:
        for flags in (0, 1, 2):
            assert np.array_equal(frames.resize(view, (ow, oh), filt, patcher=pt, flags=flags).cpu().numpy(), RC.pil_resize(img, (ow, oh), filt)), (filt, flags)
    assert np.array_equal(d.cpu().numpy(), big)


# ---- NEAREST: the prescale's gather; refusals -------------------------------------------------------------------------------------
def test_nearest_is_the_gather_and_refusals_leave_the_patcher_usable(pt):
    w, h, ow, oh = 200, 113, 104, 58
    img, rgb = RC.gray_frame(w, h, "noise"), RC.color_frame(w, h, "BGR")
    want = RC.pil_resize(img, (ow, oh), "NEAREST")
    assert np.array_equal(frames.resize(dev(img), (ow, oh), "NEAREST", patcher=pt).cpu().numpy(), want)
    dst = Dst(oh, ow, 1, ow + 3, 1)
    frames.resize(dev(img), (ow, oh), "NEAREST", out=dst.view, patcher=pt)
    dst.check(want, "NEAREST, pitched destination")
    assert np.array_equal(frames.resize(dev(rgb), (ow, oh), 0, "BGR", patcher=pt).cpu().numpy(), RC.pil_gray_resize(rgb, "BGR", (ow, oh), "NEAREST"))
    d = dev(img)
    L = _capi.lib()
    import torch
    out = torch.full((oh, ow), 7, dtype=torch.uint8, device="cuda")
    call = lambda **kw: L.hg_patcher_resize_device(*[dict(dict(p=pt._handle(), filt=2, flags=0, src=d.data_ptr(), fmt=0, h=h, w=w, ld=w, ofmt=0, dst=out.data_ptr(), oh=oh,
                                                            ow=ow, dld=ow, st=None), **kw)[k] for k in ("p", "filt", "flags", "src", "fmt", "h", "w", "ld", "ofmt", "dst", "oh", "ow", "dld", "st")])
    refused = dict(filt=6, flags=4, fmt=7, ofmt=1, ld=w - 1, dld=ow - 1, h=0, ow=0, src=None, dst=None, p=None)
    for k, v in refused.items():
        assert call(**{k: v}) == _capi.HG_ERR_ARG and len(L.hg_last_error()) > 10, k
    assert call(flags=3) == _capi.HG_ERR_ARG                                                       # both paths forced at once
    assert call(dst=d.data_ptr() + 5) == _capi.HG_ERR_ARG                                          # overlap
    assert call(filt=0, src=dev(rgb).data_ptr(), fmt=2, ld=3 * w, ofmt=2, dld=3 * ow) == _capi.HG_ERR_ARG      # NEAREST with colour output
    torch.cuda.synchronize()
    assert np.all(out.cpu().numpy() == 7)
    assert call() == _capi.HG_OK
    assert np.array_equal(out.cpu().numpy(), RC.pil_resize(img, (ow, oh), "BILINEAR"))
    with pytest.raises(ValueError):
        frames.resize(dev(rgb), (ow, oh), "NEAREST", "BGR", "BGR", patcher=pt)
    with pytest.raises(ValueError):
        frames.resize(img, (ow, oh))                                                                # a host array


# ---- 4. the table cache -------------------------------------------------------------------------------------------------------------
def test_table_cache_in_rotation():
    """Three sizes in rotation through one patcher, then the first size again, three rounds: the first with one filter (six axes, all
    kept), the others with a filter per size that changes with the round (sixteen axes in all through the eight table slots: tables are
    replaced and built again); every result against a patcher of its own and against PIL."""
    from pyfaceanalysis_amd.patches import Patcher
    shapes = [(200, 113, 104, 58), (37, 23, 16, 9), (130, 70, 65, 17)]
    imgs = [RC.gray_frame(s[0], s[1], "noise") for s in shapes]
    one = Patcher()
    try:
        for rnd in range(3):
            for i in (0, 1, 2, 0):
                w, h, ow, oh = shapes[i]
                filt = RC.FILTERS[(rnd + i) % 5] if rnd else "BILINEAR"
                for flags in (0, 1, 2):
                    got = frames.resize(dev(imgs[i]), (ow, oh), filt, patcher=one, flags=flags).cpu().numpy()
                    fresh = frames.resize(dev(imgs[i]), (ow, oh), filt, flags=flags).cpu().numpy()
                    assert np.array_equal(got, fresh) and np.array_equal(got, RC.pil_resize(imgs[i], (ow, oh), filt)), (rnd, i, filt, flags)
    finally:
        one.close()


# ---- 5. / 6. the cascade's prescale ---------------------------------------------------------------------------------------------------
class Rig(object):
    """A synthetic 17-stage face cascade and eye stages (pyfaceanalysis_amd/synth_cascade.py) on one T5L-16 network, calibrated on the
    BILINEAR 160 x 90 prescale of a 320 x 180 noise frame; four frames of a stream (the first frame and three seeded variations)."""

    def __init__(self, nets, pt):
        from pyfaceanalysis_amd import synth_cascade
        from pyfaceanalysis_amd.cascade import frame_windows
        from pyfaceanalysis_amd.flow import Flow
        self.pipe = dict(grid.FACE_PIPELINE)
        nodes = nets("T5L-16")
        self.flow, self.eye_flow = Flow(nodes, output_dtype=np.float32), Flow(nodes, output_dtype=np.float32)
        rng = np.random.default_rng(41)
        base = rng.integers(0, 256, (180, 320), dtype=np.uint8)
        self.stream = [base]
        for k in range(3):
            f = base.copy()
            ys, xs = rng.integers(0, 180, 400), rng.integers(0, 320, 400)
            f[ys, xs] = rng.integers(0, 256, 400)
            self.stream.append(f)
        assert grid.prescaled_size(320, 180, 160) == (160, 90)
        calib = RC.pil_resize(base, (160, 90), "BILINEAR")
        boxes, _ = frame_windows(160, 90, SF, self.pipe, SUB)
        feats = self.flow.execute(pt.extract(calib, boxes, SUB, dtype=np.uint8))
        self.stages = synth_cascade.build_face_cascade(self.flow, feats, self.pipe, keep_fraction=0.7)
        face_boxes = boxes[rng.choice(len(boxes), 60, replace=False)].copy()
        face_angles = rng.uniform(-22.5, 22.5, 60)
        u8 = pt.extract(calib, ER.all_eye_boxes(face_boxes, face_angles), SUB, dtype=np.uint8, delta_angs=-np.concatenate([face_angles] * 2))
        _, self.clf_x, _, self.clf_y = synth_cascade.build_eye_stages(self.eye_flow, self.eye_flow.execute(ER.contrast(u8, *CONTRAST)))
        self.open = []

    def cascade(self, **kw):
        from pyfaceanalysis_amd.cascade import DeviceCascade
        dc = DeviceCascade(self.stages, SUB, K, self.pipe, **kw)
        self.open.append(dc)
        return dc

    def locator(self):
        from pyfaceanalysis_amd.eyes import EyeLocator
        loc = EyeLocator(self.eye_flow, self.clf_x, self.eye_flow, self.clf_y, contrast=CONTRAST, eye_size=SUB, regression_size=(16.0, 16.0))
        self.open.append(loc)
        return loc

    def close(self):
        for o in self.open:
            o.close()
        self.eye_flow.close()
        self.flow.close()


@pytest.fixture(scope="module")
def rig(native_lib, nets, pt):
    r = Rig(nets, pt)
    yield r
    r.close()


def same_detection(got, ref, what):
    for key in ("orig_index", "coords", "angles", "confidence"):
        assert np.array_equal(got[key], ref[key]), (what, key)
    assert got["counts"] == ref["counts"] and got["rows_executed"] == ref["rows_executed"] and got["n_windows"] == ref["n_windows"], what


def same_faces(got, ref, what):
    assert got["faces"].shape == ref["faces"].shape and np.array_equal(got["faces"], ref["faces"]), what
    for key in ("n_before_purge", "counts", "rows_executed", "n_windows"):
        assert got[key] == ref[key], (what, key)
    if "tracked" in ref:
        assert got["tracked"] is ref["tracked"], what


@pytest.mark.parametrize("filt", ("BILINEAR", "BICUBIC"))
def test_cascade_with_a_prescale_filter_equals_the_cascade_on_pils_frame(rig, filt):
    from pyfaceanalysis_amd.tracking import FaceTracker
    dc, loc = rig.cascade(prescale_filter=filt), rig.locator()
    assert dc.prescale_filter == RC.CODES[filt]
    big = [dev(f) for f in rig.stream]
    small_host = [RC.pil_resize(f, (160, 90), filt) for f in rig.stream]
    small = [dev(f) for f in small_host]
    assert np.array_equal(dc.prescale(big[0], prescale_size=160).cpu().numpy(), small_host[0])
    ref = dc.detect_frame(small[0], smallest_face=SF, prescale_size=None)
    for _ in range(2):                                        # the second call uploads and allocates nothing
        same_detection(dc.detect_frame(big[0], smallest_face=SF, prescale_size=160), ref, (filt, "detect_frame"))
    ref_faces = dc.detect_faces(small[0], loc, smallest_face=SF, prescale_size=None)
    same_faces(dc.detect_faces(big[0], loc, smallest_face=SF, prescale_size=160), ref_faces, (filt, "detect_faces"))
    print("%s: counts %s, %d survivors, %d faces" % (filt, ref["counts"], len(ref["coords"]), len(ref_faces["faces"])))
    assert ref["counts"][0] > 0, "the comparison ran on nothing"
    ta, tb = FaceTracker(dc, loc, smallest_face=SF, prescale_size=160), FaceTracker(dc, loc, smallest_face=SF, prescale_size=None)
    try:
        flags = []
        for i in range(4):
            a, b = ta.step(big[i]), tb.step(small[i])
            same_faces(a, b, (filt, "tracker step", i))
            flags.append(a["tracked"])
        print("%s: tracked steps %s" % (filt, flags))
        if filt == "BILINEAR":      # (the frames are seeded and the arithmetic is exact: these comparisons did not run on nothing)
            assert len(ref["coords"]) >= 1 and len(ref_faces["faces"]) >= 1 and any(flags)
    finally:
        ta.close()
        tb.close()
    # an RGB frame through the filter: convert("L") first, so the grey PIL frame's result
    rgb, _ = CC.color_twin(rig.stream[0], 5100)
    assert np.array_equal(CC.pil_gray(rgb, "RGB"), rig.stream[0])
    dcc = rig.cascade(prescale_filter=filt, frame_format="RGB")
    lay = CC.ColorLayout(rgb, "roi")
    same_detection(dcc.detect_frame(lay.view, smallest_face=SF, prescale_size=160), ref, (filt, "RGB detect_frame"))
    same_faces(dcc.detect_faces(lay.view, loc, smallest_face=SF, prescale_size=160), ref_faces, (filt, "RGB detect_faces"))
    assert np.array_equal(dcc.prescale(lay.view, prescale_size=160).cpu().numpy(), small_host[0])
    lay.assert_untouched()


def test_default_is_nearest_and_switching_back_restores_it(rig):
    never, dc = rig.cascade(), rig.cascade()
    assert never.prescale_filter == 0 and dc.prescale_filter == 0
    big = dev(rig.stream[0])
    want = RC.pil_resize(rig.stream[0], (160, 90), "NEAREST")
    ref = never.detect_frame(big, smallest_face=SF, prescale_size=160)
    assert np.array_equal(never.prescale(big, prescale_size=160).cpu().numpy(), want)
    same_detection(dc.detect_frame(big, smallest_face=SF, prescale_size=160), ref, "before the switch")
    dc.set_prescale_filter("BICUBIC")
    bic = RC.pil_resize(rig.stream[0], (160, 90), "BICUBIC")
    assert (bic != want).mean() > 0.5
    same_detection(dc.detect_frame(big, smallest_face=SF, prescale_size=160), dc.detect_frame(dev(bic), smallest_face=SF, prescale_size=None), "BICUBIC")
    assert np.array_equal(dc.prescale(big, prescale_size=160).cpu().numpy(), bic)
    dc.set_prescale_filter("NEAREST")
    assert dc.prescale_filter == 0
    same_detection(dc.detect_frame(big, smallest_face=SF, prescale_size=160), ref, "after the switch back")
    assert np.array_equal(dc.prescale(big, prescale_size=160).cpu().numpy(), want)
    with pytest.raises(ValueError):
        dc.set_prescale_filter(9)
    assert _capi.lib().hg_cascade_set_prescale_filter(dc._handle(), 9) == _capi.HG_ERR_ARG
    same_detection(dc.detect_frame(big, smallest_face=SF, prescale_size=160), ref, "after a refused code")
