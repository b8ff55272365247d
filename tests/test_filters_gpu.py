"""GPU: BILINEAR / BICUBIC window sampling (hg_patcher_extract_filter*, hg_cascade_set_interpolation, hg_eyes_set_interpolation) —
every window against PIL called here (``array_equal``), the cascade, the eye step and a tracked frame against their composed steps
with the same filters.  Small shapes: a 53 x 37 frame for the windows, a 160 x 120 frame, 16 x 16 sub-images and the T5L-16 network
for the cascade and the eyes."""
import ctypes as C

import numpy as np
import pytest

from oracle import cascade_restate as CR
from pyfaceanalysis_amd import _capi, grid
from tests import eyes_restate as ER
from tests import filters_cases as FC

pytestmark = pytest.mark.gpu

CONTRAST = (128.0, 48.0)          # as tests/test_eyes_gpu.py
SUB = (16, 16)
K = 10                            # T5L-16 has 10 outputs
SF = 0.3
FRAME_SEED = 28                   # the 160 x 120 frame; test_cascade_* asserts that rotated windows with survivors take part
FORMATS = [0, 2, 3, 3, 3, 3, 3, 3, 3, 3]
DT = {np.uint8: _capi.HG_U8, np.float32: _capi.HG_F32, np.float64: _capi.HG_F64}


@pytest.fixture(scope="module")
def pt(native_lib):
    from pyfaceanalysis_amd.patches import Patcher
    p = Patcher()
    yield p
    p.close()


# ---- 1. unrotated windows ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(16, 12), (64, 64), (128, 128)])
@pytest.mark.parametrize("filt", FC.FILTERS)
def test_unrotated_windows_equal_pil(pt, filt, size):
    frame, boxes = FC.frame(), FC.boxes()
    want = FC.pil_windows(frame, boxes, np.zeros(len(boxes)), size, filt)
    assert want[:14].any(axis=1).all() and not want[14:16].any()
    for dt in (np.uint8, np.float32, np.float64):
        got = pt.extract(frame, boxes, size, dtype=dt, interpolation=filt)
        assert got.dtype == dt and np.array_equal(got, want.astype(dt)), (dt, np.argwhere(got != want)[:4])
    # delta_angs given but zero (or a multiple of 360): the unrotated rule through the rotated kernel
    got = pt.extract(frame, boxes, size, dtype=np.uint8, delta_angs=np.where(np.arange(len(boxes)) % 2, 0.0, -720.0), interpolation=filt)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("filt", FC.FILTERS)
def test_row_stride_and_device_entry_twice(pt, filt):
    import torch
    frame, boxes = FC.frame(), FC.boxes()
    size = (16, 12)
    want = FC.pil_windows(frame, boxes, np.zeros(len(boxes)), size, filt)
    # host entry, frame rows 64 apart and output rows 200 apart
    wide = np.full((FC.FRAME_H, 64), 201, dtype=np.uint8)
    wide[:, :FC.FRAME_W] = frame
    out = np.full((len(boxes), 200), 7, dtype=np.uint8)
    rc = _capi.lib().hg_patcher_extract_filter(pt._handle(), filt, wide.ctypes.data, _capi.HG_U8, FC.FRAME_H, FC.FRAME_W, 64, boxes.ctypes.data, None,
                                               len(boxes), size[0], size[1], out.ctypes.data, _capi.HG_U8, 200)
    assert rc == _capi.HG_OK and np.array_equal(out[:, :192], want) and np.all(out[:, 192:] == 7)
    # device entry, strided frame, the same boxes twice on one patcher: the unkeyed entry rebuilds its tables in place on every call, so
    # this checks that a second call over the first one's buffers is right, not that a table is reused (the keyed reuse is the
    # cascade's: test_cascade_with_filters_equals_the_composed_loop calls detect twice with a BILINEAR first stage)
    fdev = torch.from_numpy(wide).cuda()
    bdev = torch.from_numpy(boxes).cuda()
    for _ in range(2):
        odev = torch.full((len(boxes), 192), 9, dtype=torch.uint8, device="cuda")
        pt.extract_device(fdev.data_ptr(), np.uint8, FC.FRAME_H, FC.FRAME_W, 64, bdev.data_ptr(), len(boxes), size, odev.data_ptr(), np.uint8, 192,
                          stream=torch.cuda.current_stream().cuda_stream, interpolation=filt)
        torch.cuda.synchronize()
        assert np.array_equal(odev.cpu().numpy(), want)


# ---- 2. rotated windows ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("filt", FC.FILTERS)
def test_rotated_windows_equal_pil(pt, filt):
    """Corner boxes (the rotation's zero fill enters the taps; their tiles stage the rotated patch in LDS), two boxes shrunk about 8 x
    (tiles whose taps are sparse: computed tap by tap) and a magnified one; (20, 12) is no multiple of the 16 x 16 tile, (64, 64) has
    several tiles in both directions."""
    frame = FC.frame()
    boxes = np.concatenate([FC.corner_boxes(), FC.boxes()[[0, 7, 17, 20, 23]]])
    zero_fill = 0
    for size in ((16, 12), (20, 12), (64, 64)):
        angs = FC.ANGLES if size != (64, 64) else (17.0, -135.0)
        bb = np.repeat(boxes, len(angs), axis=0)
        aa = np.tile(np.array(angs), len(boxes))
        want = FC.pil_windows(frame, bb, aa, size, filt)
        for dt in ((np.uint8, np.float32, np.float64) if size == (20, 12) else (np.uint8,)):
            got = pt.extract(frame, bb, size, dtype=dt, delta_angs=aa, interpolation=filt)
            bad = np.argwhere(got != want)
            assert np.array_equal(got, want.astype(dt)), (size, dt, len(bad), [(bb[i], aa[i], j) for i, j in bad[:3]])
        zero_fill += int((want[:4 * len(angs)] == 0).sum())
    assert zero_fill > 500


# ---- 3. the clamp ------------------------------------------------------------------------------------------------------------
def test_checkerboard_bicubic(pt):
    board = FC.checkerboard()
    boxes = FC.boxes()[:6]
    for angs in (np.zeros(6), np.array([0.5, 17.0, 45.0, -135.0, 90.0, -0.5])):
        want = FC.pil_windows(board, boxes, angs, (64, 64), 3)
        assert (want == 0).any() and (want == 255).any() and ((want > 0) & (want < 255)).any()
        got = pt.extract(board, boxes, (64, 64), dtype=np.uint8, delta_angs=angs if angs.any() else None, interpolation=3)
        assert np.array_equal(got, want)


# ---- 4. NEAREST through the new entries ---------------------------------------------------------------------------------------
def test_interpolation_zero_is_extract_rotate(pt):
    L = _capi.lib()
    boxes = np.concatenate([FC.boxes(), FC.corner_boxes()])
    angs = np.resize(np.array(FC.ANGLES + (0.0,)), len(boxes))
    for frame in (FC.frame(), FC.frame().astype(np.float32) * 0.5):
        for size, dt in (((16, 12), np.uint8), ((20, 12), np.float64), ((64, 64), np.float32)):
            for a in (None, angs):
                old = np.empty((len(boxes), size[0] * size[1]), dtype=dt)
                rc = L.hg_patcher_extract_rotate(pt._handle(), frame.ctypes.data, DT[frame.dtype.type], frame.shape[0], frame.shape[1], frame.shape[1],
                                                 boxes.ctypes.data, None if a is None else a.ctypes.data, len(boxes), size[0], size[1], old.ctypes.data,
                                                 DT[dt], size[0] * size[1])
                assert rc == _capi.HG_OK
                new = pt.extract(frame, boxes, size, dtype=dt, delta_angs=a, interpolation=0)
                assert np.array_equal(new, old) and old.any()


# ---- 5.-7. cascade, eyes, tracking ------------------------------------------------------------------------------------------
class Rig(object):
    """The synthetic 17-stage face cascade (synth_cascade.build_face_cascade) on one T5L-16 flow and 16 x 16 windows of a 160 x 120
    frame, and eye stages on a second handle of the same network."""

    def __init__(self, nets, pt):
        import torch
        from pyfaceanalysis_amd import synth_cascade
        from pyfaceanalysis_amd.cascade import frame_windows
        from pyfaceanalysis_amd.flow import Flow
        self.pt = pt
        self.pipe = dict(grid.FACE_PIPELINE)
        self.nodes = nets("T5L-16")
        self.flow = Flow(self.nodes, output_dtype=np.float32)
        self.eye_flow = Flow(self.nodes, output_dtype=np.float32)
        rng = np.random.default_rng(FRAME_SEED)
        self.frame = rng.integers(0, 256, (120, 160), dtype=np.uint8)
        self.fdev = torch.from_numpy(self.frame).cuda()
        self.boxes, self.level = frame_windows(160, 120, SF, self.pipe, SUB)
        feats = self.flow.execute(pt.extract(self.frame, self.boxes, SUB, dtype=np.uint8))
        self.stages = synth_cascade.build_face_cascade(self.flow, feats, self.pipe, keep_fraction=0.7)
        self.face_boxes = self.boxes[rng.choice(len(self.boxes), 60, replace=False)].copy()
        self.face_angles = rng.uniform(-22.5, 22.5, 60)
        eb = ER.all_eye_boxes(self.face_boxes, self.face_angles)
        u8 = pt.extract(self.frame, eb, SUB, dtype=np.uint8, delta_angs=-np.concatenate([self.face_angles] * 2), interpolation=3)
        _, self.clf_x, _, self.clf_y = synth_cascade.build_eye_stages(self.eye_flow, self.eye_flow.execute(ER.contrast(u8, *CONTRAST)))
        self.open = []

    def cascade(self, formats):
        from pyfaceanalysis_amd.cascade import DeviceCascade
        dc = DeviceCascade(self.stages, SUB, K, self.pipe, interpolation_formats=formats)
        self.open.append(dc)
        return dc

    def locator(self, interpolation):
        from pyfaceanalysis_amd.eyes import EyeLocator
        loc = EyeLocator(self.eye_flow, self.clf_x, self.eye_flow, self.clf_y, contrast=CONTRAST, eye_size=SUB, regression_size=(16.0, 16.0),
                         interpolation=interpolation)
        self.open.append(loc)
        return loc

    def composed_loop(self, formats):
        """The stage loop on the host: Patcher.extract with the stage's filter, flow.execute, the device regression, the restated glue.
        Also returns, per extracting stage, (stage index, filter, rows, rows cut with a non-zero angle)."""
        stages = self.stages
        names = [s.name for s in stages]
        extracting = [k for k, s in enumerate(stages) if s.flow is not None and not (k > 0 and stages[k - 1].type == "Disc")]
        todo, seen = list(extracting), []

        def extract(coords, dang):
            k = todo.pop(0)
            f = 0 if formats is None else formats[stages[k].serial]
            seen.append((k, f, len(coords), int(np.count_nonzero(dang))))
            return self.pt.extract(self.frame, coords, SUB, dtype=np.uint8, delta_angs=dang, interpolation=f) if len(coords) else np.zeros((0, 256), np.uint8)

        def execute(k, subs):
            return stages[k].flow.execute(subs)

        def regress(k, sl):
            return stages[k].classifier.regression(np.ascontiguousarray(sl[:, :stages[k].classifier.input_dim]))
        ref = CR.run_cascade(names, [s.flow is not None for s in stages], self.boxes, self.level, self.pipe, extract, execute, regress)
        assert not todo
        return ref, seen

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


def assert_same_detection(got, ref, what):
    assert np.array_equal(got["orig_index"], ref["orig_index"]), what
    assert np.array_equal(got["coords"], ref["coords"]) and np.array_equal(got["angles"], ref["angles"]), what
    assert np.array_equal(got["confidence"], ref["confidence"]), what


def test_cascade_with_filters_equals_the_composed_loop(rig):
    dc = rig.cascade(FORMATS)
    ref, seen = rig.composed_loop(FORMATS)
    print("extracting stages (stage, filter, rows, rotated rows):", seen, "counts:", ref["counts"])
    # Disc1 cuts BILINEAR windows of the grid; a stage behind PAng0 cuts BICUBIC windows, at least three of them rotated, and at least
    # three candidates survive it: the comparison cannot pass on an empty set
    assert seen[0][:2] == (0, 2) and seen[0][2] == len(rig.boxes)
    rotated = [(k, f, n, nz) for k, f, n, nz in seen[1:] if f == 3 and nz >= 3 and ref["counts"][k] >= 3]
    assert rotated, seen
    for _ in range(2):                      # the second call reuses the first stage's keyed coordinate tables
        got = dc.detect(rig.fdev, smallest_face=SF)
        assert_same_detection(got, ref, "grid on the device")
        known = [i for i, c in enumerate(got["counts"]) if c >= 0]
        assert [i for i in known if rig.stages[i].type == "Disc"] == [i for i, s in enumerate(rig.stages) if s.type == "Disc"]
        assert [got["counts"][i] for i in known] == [ref["counts"][i] for i in known], (got["counts"], ref["counts"])
    assert len(ref["coords"]) >= 1 and np.abs(ref["angles"]).max() > 0
    explicit = dc.detect(rig.fdev, smallest_face=SF, windows=(rig.boxes, rig.level))      # unkeyed first stage
    assert_same_detection(explicit, ref, "windows from the host")
    # the filters matter here: NEAREST everywhere is another answer
    plain_ref, _ = rig.composed_loop(None)
    assert plain_ref["counts"] != ref["counts"] or not np.array_equal(plain_ref["coords"], ref["coords"])


def test_cascade_without_setter_equals_all_nearest(rig):
    unset, zeros = rig.cascade(None), rig.cascade([0] * 10)
    ref, _ = rig.composed_loop(None)
    a, b = unset.detect(rig.fdev, smallest_face=SF), zeros.detect(rig.fdev, smallest_face=SF)
    assert_same_detection(a, ref, "no setter")
    assert_same_detection(b, a, "all zeros")
    assert a["counts"] == b["counts"] and a["rows_executed"] == b["rows_executed"]


def test_eye_patches_bicubic_equal_pil_and_contrast(rig):
    loc = rig.locator(3)
    nz = np.flatnonzero(np.abs(rig.face_angles) > 1.0)[:4]
    boxes, angles = rig.face_boxes[nz], rig.face_angles[nz]
    assert len(nz) == 4
    out = loc.locate(rig.fdev, boxes, angles, return_patches=True)
    eb = loc.eye_boxes(boxes, angles)
    dang = -np.concatenate([angles, angles])
    u8 = FC.pil_windows(rig.frame, eb, dang, SUB, 3)
    assert out["patches"].shape == (8, 256) and np.array_equal(out["patches"], ER.contrast(u8, *CONTRAST))
    from tests import filters_restate as FR
    assert np.array_equal(FR.windows(rig.frame, eb, dang, SUB, 3), u8)
    # ... and they are not the NEAREST patches
    plain = rig.locator(0).locate(rig.fdev, boxes, angles, return_patches=True)
    assert not np.array_equal(plain["patches"], out["patches"])


def composed_faces(dc, loc, pre, det):
    from pyfaceanalysis_amd import eyes as E
    out = loc.locate(pre, det["coords"], det["angles"])
    rows = E.assemble_rows(det["coords"], det["angles"], det["confidence"], out["eye_coords"], out["too_far"])
    return E.purge_detections(rows), len(rows)


def test_detect_faces_and_tracked_frame_bicubic(rig):
    from pyfaceanalysis_amd.cascade import tracked_windows
    from pyfaceanalysis_amd.tracking import FaceTracker
    dc, loc = rig.cascade([3] * 10), rig.locator(3)
    det = dc.detect_frame(rig.fdev, smallest_face=SF)
    assert dc.prescale(rig.fdev) is rig.fdev                      # 160 x 120 needs no prescale
    want, n_before = composed_faces(dc, loc, rig.fdev, det)
    got = dc.detect_faces(rig.fdev, loc, smallest_face=SF)
    assert len(det["coords"]) >= 1 and len(want) >= 1
    assert got["faces"].shape == want.shape and np.array_equal(got["faces"], want)
    assert got["n_before_purge"] == n_before and got["counts"] == det["counts"]
    tr = FaceTracker(dc, loc, smallest_face=SF)
    try:
        r0 = tr.step(rig.fdev)
        assert r0["tracked"] is False and np.array_equal(r0["faces"], want)
        r1 = tr.step(rig.fdev)
        det9 = dc.detect(rig.fdev, windows=tracked_windows(want[0, :4], rig.pipe, SUB))
        want9, n9 = composed_faces(dc, loc, rig.fdev, det9)
        print("tracked frame: composed counts %s, faces %d" % (det9["counts"], len(want9)))
        assert r1["tracked"] is True and r1["n_windows"] == 9
        assert r1["faces"].shape == want9.shape and np.array_equal(r1["faces"], want9) and r1["n_before_purge"] == n9
    finally:
        tr.close()


# ---- 8. errors -----------------------------------------------------------------------------------------------------------------
def test_bad_filters_are_refused_and_leave_the_handles_usable(rig, pt):
    L = _capi.lib()
    frame, boxes = FC.frame(), FC.boxes()
    size = (16, 12)
    want = FC.pil_windows(frame, boxes, np.zeros(len(boxes)), size, 2)
    out = np.full((len(boxes), 192), 5, dtype=np.uint8)

    def c_call(filt, fr, code):
        return L.hg_patcher_extract_filter(pt._handle(), filt, fr.ctypes.data, code, FC.FRAME_H, FC.FRAME_W, FC.FRAME_W, boxes.ctypes.data, None, len(boxes),
                                           size[0], size[1], out.ctypes.data, _capi.HG_U8, 192)
    f32 = frame.astype(np.float32)
    for filt, fr, code in ((1, frame, _capi.HG_U8), (7, frame, _capi.HG_U8), (2, f32, _capi.HG_F32), (3, f32, _capi.HG_F32)):
        assert c_call(filt, fr, code) == _capi.HG_ERR_ARG and np.all(out == 5), filt
        with pytest.raises(ValueError):
            pt.extract(fr, boxes, size, dtype=np.uint8, interpolation=filt)
        assert c_call(2, frame, _capi.HG_U8) == _capi.HG_OK and np.array_equal(out, want)
        out[:] = 5
    for bad in (None, "bilinear", 2.0, True):
        with pytest.raises(ValueError):
            pt.extract(frame, boxes, size, interpolation=bad)
    # the cascade's setter: a list shorter than a stage's serial, an unknown code; the handle keeps its filters
    from pyfaceanalysis_amd.cascade import DeviceCascade
    from pyfaceanalysis_amd.eyes import EyeLocator
    dc = rig.cascade(FORMATS)
    before = dc.detect(rig.fdev, smallest_face=SF)
    for lst in ([3] * 5, [0, 2, 3, 3, 3, 3, 3, 1, 3, 3], [3] * 9 + [7]):
        arr = (C.c_int32 * len(lst))(*lst)
        assert L.hg_cascade_set_interpolation(dc._handle(), arr, len(lst)) == _capi.HG_ERR_ARG, lst
        with pytest.raises(ValueError):
            DeviceCascade(rig.stages, SUB, K, rig.pipe, interpolation_formats=lst)
        after = dc.detect(rig.fdev, smallest_face=SF)
        assert_same_detection(after, before, lst)
    assert L.hg_cascade_set_interpolation(dc._handle(), None, 10) == _capi.HG_ERR_ARG
    # the eye setter
    loc = rig.locator(3)
    nz = np.flatnonzero(np.abs(rig.face_angles) > 1.0)[:4]
    good = loc.locate(rig.fdev, rig.face_boxes[nz], rig.face_angles[nz], return_patches=True)
    for bad in (1, 7, -1):
        assert L.hg_eyes_set_interpolation(loc._handle(), bad) == _capi.HG_ERR_ARG
        with pytest.raises(ValueError):
            EyeLocator(rig.eye_flow, rig.clf_x, rig.eye_flow, rig.clf_y, contrast=CONTRAST, eye_size=SUB, regression_size=(16.0, 16.0), interpolation=bad)
        again = loc.locate(rig.fdev, rig.face_boxes[nz], rig.face_angles[nz], return_patches=True)
        assert np.array_equal(again["patches"], good["patches"]) and np.array_equal(again["eye_coords"], good["eye_coords"])
