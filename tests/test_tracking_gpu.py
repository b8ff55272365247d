"""GPU: tracking one face across a frame stream (``tracking.FaceTracker``, include/higsfa.h ``hg_tracker``) — the reference's
``track_single_face`` mode.  The nine-window grid against the reference's own outputs (tests/golden/reference_tracking.npz), and a
tracked frame — enqueued as a whole, every launch sized by the bound 9, no survivor count read back — against the COMPOSITION of the
existing public pieces on the same prescaled frame, which polls a count after every Disc stage and sizes its launches by it:

    cascade.detect(pre, windows=tracked_windows(previous faces[0, :4], ...)) -> EyeLocator.locate -> eyes.assemble_rows -> eyes.purge_detections

Every comparison is exact (``array_equal``).  The rig is tests/test_frame_stream_gpu.py's: U11L-64 as face flow and eye flow, 64x64
sub-images, the synthetic 17-stage cascade, frames of box-filtered seeded noise."""
import ctypes as C
import os

import numpy as np
import pytest

from pyfaceanalysis_amd import _capi, grid
from tests.test_frame_stream_gpu import SF, SUB, Rig, noise_frame

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
SIZE_A, SIZE_B = (640, 480), (2000, 300)          # no prescale / prescaled to 1000 x 150; both have faces (test_frame_stream_gpu.py's docstring)
SEED = {SIZE_A: 7100 + 4, SIZE_B: 7100 + 1}       # the frames of that stream's elements 4 and 1


@pytest.fixture(scope="module")
def rig(native_lib, nets):
    r = Rig(nets)
    yield r
    r.close()


def device_frame(size, seed=None):
    import torch
    return torch.from_numpy(noise_frame(size[0], size[1], SEED[size] if seed is None else seed)).cuda()


def composed(rig, fdev, box):
    """The tracked frame through the existing calls: (faces, n_before_purge, the cascade's result)."""
    from pyfaceanalysis_amd import eyes as E
    from pyfaceanalysis_amd.cascade import tracked_windows
    pre = rig.dc.prescale(fdev).clone()
    det = rig.dc.detect(pre, windows=tracked_windows(box, rig.pipe, SUB))
    out = rig.loc.locate(pre, det["coords"], det["angles"])
    rows = E.assemble_rows(det["coords"], det["angles"], det["confidence"], out["eye_coords"], out["too_far"])
    return E.purge_detections(rows), len(rows), det


def tracker_for(rig):
    from pyfaceanalysis_amd.tracking import FaceTracker
    return FaceTracker(rig.dc, rig.loc, smallest_face=SF)


def assert_tracked_step(rig, got, fdev, box, what):
    want, n_before, det = composed(rig, fdev, box)
    assert got["tracked"] is True and got["n_windows"] == 9 and got["counts"] == [-1] * len(rig.stages), what
    assert got["faces"].shape == want.shape and np.array_equal(got["faces"], want), (what, got["faces"], want)
    assert got["n_before_purge"] == n_before, what
    assert got["rows_executed"] == 9 * sum(s.flow is not None for s in rig.stages), what
    return det


def assert_full_step(rig, got, fdev, what):
    want = rig.dc.detect_faces(fdev, rig.loc, smallest_face=SF)
    assert got["tracked"] is False and got["n_windows"] == want["n_windows"] and got["n_windows"] > 9, what
    assert got["faces"].shape == want["faces"].shape and np.array_equal(got["faces"], want["faces"]), what
    assert got["n_before_purge"] == want["n_before_purge"] and got["counts"] == want["counts"] and got["rows_executed"] == want["rows_executed"], what


def test_tracked_grid_equals_the_reference_fixture(native_lib):
    """1. hg_cascade_tracked_grid_device (k_cascade_init_tracked alone) on every box of the fixture: the nine windows and their level
    rows equal the reference's outputs bit for bit, the rows where a fused multiply-add would change the last bit included."""
    import torch
    fx = np.load(os.path.join(HERE, "golden", "reference_tracking.npz"))
    L = _capi.lib()
    p = grid.FACE_PIPELINE
    assert fx["fma_side"].sum() >= 8 and fx["fma_corner"].sum() >= 8
    faces = torch.from_numpy(fx["box"]).cuda()
    n = len(fx["box"])
    boxes = torch.full((n, 9, 4), float("nan"), dtype=torch.float64, device="cuda")
    level = torch.full((n, 9, 3), float("nan"), dtype=torch.float64, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    for i in range(n):
        tc = _capi.HgTrackedConsts()
        tc.subimage_width, tc.subimage_height = float(fx["sub"][i][0]), float(fx["sub"][i][1])
        tc.regression_width, tc.regression_height, tc.net_Dx, tc.net_Dy = p["regression_width"], p["regression_height"], p["net_Dx"], p["net_Dy"]
        _capi.check(L.hg_cascade_tracked_grid_device(0, C.byref(tc), faces[i].data_ptr(), boxes[i].data_ptr(), level[i].data_ptr(), stream))
    boxes, level = boxes.cpu().numpy(), level.cpu().numpy()
    for i in range(n):
        assert np.array_equal(boxes[i], fx["boxes"][i]), (i, fx["kind"][i])
        assert np.array_equal(level[i], np.tile([fx["maxd"][i][0], fx["maxd"][i][1], fx["base_side"][i]], (9, 1))), (i, fx["kind"][i])
    tc.net_Dx = float("nan")
    assert L.hg_cascade_tracked_grid_device(0, C.byref(tc), faces.data_ptr(), boxes.ctypes.data, level.ctypes.data, stream) == _capi.HG_ERR_ARG
    assert L.hg_cascade_tracked_grid_device(0, None, faces.data_ptr(), None, None, stream) == _capi.HG_ERR_ARG


def test_tracked_frame_equals_the_composed_path(rig):
    """2. Frame 0 through the full grid keeps faces; frame 1 (the same picture) is a tracked step — nine windows, every count -1 — and
    its faces are those of the composed path on the same prescaled frame, for both frame sizes (one of them prescaled)."""
    for size in (SIZE_A, SIZE_B):
        fdev = device_frame(size)
        tr = tracker_for(rig)
        try:
            assert tr.tracked_face is None
            r0 = tr.step(fdev)
            assert_full_step(rig, r0, fdev, (size, "frame 0"))
            assert len(r0["faces"]) >= 1 and np.array_equal(tr.tracked_face, r0["faces"][0, :4])
            r1 = tr.step(fdev)
            det = assert_tracked_step(rig, r1, fdev, r0["faces"][0, :4], (size, "frame 1"))
            print("tracked frame on %s: composed counts %s, faces %d" % (size, det["counts"], len(r1["faces"])))
            if len(r1["faces"]):
                assert np.array_equal(tr.tracked_face, r1["faces"][0, :4])
            else:
                assert tr.tracked_face is None
        finally:
            tr.close()


def losing_frame(rig, size, box):
    """A frame of ``size`` on which the composed nine-window path around ``box`` keeps nothing: the first of a constant frame and a
    few noise frames of other seeds (the composed path decides, before the tracker sees the frame)."""
    import torch
    cands = [torch.zeros((size[1], size[0]), dtype=torch.uint8, device="cuda")] + [device_frame(size, 9900 + k) for k in range(8)]
    for k, f in enumerate(cands):
        faces, _, det = composed(rig, f, box)
        if len(faces) == 0:
            return f, k, det
    raise AssertionError("no candidate frame loses the face")


def test_losing_the_face_returns_to_the_full_grid(rig):
    """3. A tracked step on a frame where nothing survives returns normally with no face — the live count is 0 under the bound 9
    through every later stage group, the eye step and the purge — drops the tracked face, and the next step is a full-grid step
    whose faces are ``detect_faces``'s."""
    fdev = device_frame(SIZE_A)
    tr = tracker_for(rig)
    try:
        r0 = tr.step(fdev)
        assert len(r0["faces"]) >= 1
        lost, k, det = losing_frame(rig, SIZE_A, r0["faces"][0, :4])
        print("losing frame: candidate %d, composed counts %s" % (k, det["counts"]))
        r1 = tr.step(lost)
        assert_tracked_step(rig, r1, lost, r0["faces"][0, :4], "the losing frame")
        assert r1["faces"].shape == (0, 10) and r1["n_before_purge"] == 0 and tr.tracked_face is None
        r2 = tr.step(fdev)
        assert_full_step(rig, r2, fdev, "after the loss")
        assert np.array_equal(r2["faces"], r0["faces"])
    finally:
        tr.close()


# the stream of test 4: (size, seed or None for the size's own frame, reset before the step)
STREAM = [(SIZE_A, None, False), (SIZE_A, None, False), (SIZE_A, None, False), (SIZE_A, 9901, False), (SIZE_A, None, False),
          (SIZE_B, None, False), (SIZE_B, None, False), (SIZE_B, None, True), (SIZE_B, None, False), (SIZE_A, None, False),
          (SIZE_A, None, False), (SIZE_A, 9902, False)]


def run_stream(rig, check):
    tr = tracker_for(rig)
    log = []
    try:
        held, held_size = None, None
        for i, (size, seed, reset) in enumerate(STREAM):
            fdev = device_frame(size, seed)
            if reset:
                tr.reset()
                assert tr.tracked_face is None
                held = None
            psize = grid.prescaled_size(*size)
            expect_tracked = held is not None and held_size == psize
            got = tr.step(fdev)
            assert got["tracked"] is expect_tracked, (i, size, got["tracked"], expect_tracked)
            if check:
                if expect_tracked:
                    assert_tracked_step(rig, got, fdev, held, (i, size))
                else:
                    assert_full_step(rig, got, fdev, (i, size))
            held = got["faces"][0, :4].copy() if len(got["faces"]) else None
            held_size = psize
            assert (tr.tracked_face is None) == (held is None) and (held is None or np.array_equal(tr.tracked_face, held)), i
            log.append((got["tracked"], got["faces"].copy(), got["n_before_purge"], got["n_windows"]))
        return log
    finally:
        tr.close()


def test_stream_of_twelve_frames(rig):
    """4. Twelve frames of two sizes through one long-lived tracker, with a size change mid-stream (element 5, and back at element 9),
    one reset (before element 7) and two frames of other content (elements 3 and 11): every tracked frame equals the composed path,
    every full frame ``detect_faces``; the tracked flags follow the rules (a face held, the same prescaled size, no reset); a second
    run through a fresh tracker gives the same bytes."""
    assert len(STREAM) == 12 and len({s for s, _, _ in STREAM}) == 2
    a = run_stream(rig, check=True)
    print("stream:", [(t, len(f), nb, nw) for t, f, nb, nw in a])
    flags = [t for t, _, _, _ in a]
    assert flags[0] is False and flags[1] is True                   # a face found, then followed
    assert flags[5] is False and flags[7] is False and flags[9] is False          # the size changes and the reset
    assert flags[6] is True and flags[8] is True and flags[10] is True
    assert sum(flags) >= 6 and any(t and len(f) for t, f, _, _ in a)
    b = run_stream(rig, check=False)
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert x[0] == y[0] and x[2:] == y[2:] and x[1].shape == y[1].shape and np.array_equal(x[1], y[1]), i


def test_existing_calls_unchanged_by_a_tracker(rig):
    """5. ``detect_faces`` and ``EyeLocator.locate`` on one frame give the same bytes before and after a tracker has run full and
    tracked steps on the same cascade and eye handles (shared workspaces; the nullable device count of the eye kernels)."""
    fdev = device_frame(SIZE_A)
    pre = rig.dc.prescale(fdev).clone()
    before = rig.dc.detect_faces(fdev, rig.loc, smallest_face=SF)
    n = min(40, len(rig.face_boxes))
    small = device_frame((1000, 562), 8600)
    loc_before = rig.loc.locate(small, rig.face_boxes[:n], rig.face_angles[:n], return_patches=True)
    tr = tracker_for(rig)
    try:
        flags = [tr.step(fdev)["tracked"] for _ in range(3)]
        assert flags[0] is False and flags[1] is True
    finally:
        tr.close()
    after = rig.dc.detect_faces(fdev, rig.loc, smallest_face=SF)
    for key in ("faces", "n_before_purge", "counts", "rows_executed", "n_windows"):
        assert np.array_equal(before[key], after[key]), key
    loc_after = rig.loc.locate(small, rig.face_boxes[:n], rig.face_angles[:n], return_patches=True)
    for key in ("eye_coords", "too_far", "reg", "patches"):
        assert np.array_equal(loc_before[key], loc_after[key]), key
    assert np.array_equal(pre.cpu().numpy(), rig.dc.prescale(fdev).cpu().numpy())
