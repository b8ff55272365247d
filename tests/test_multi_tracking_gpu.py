"""GPU: tracking SEVERAL faces across a frame stream (``tracking.FaceTracker(max_faces=K)``, include/higsfa.h
``hg_tracker_create_multi`` / ``hg_tracker_step_frame_multi_device``).  A tracked frame with K held faces is one pooled pass over 9 K
windows under the bound 9 K; rows of the cascade are independent, so its oracle is the COMPOSITION of the existing public calls on the
same prescaled frame, which polls a count after every Disc stage and sizes its launches by it:

    cascade.detect(pre, windows=tracked_windows(held boxes (K, 4))) -> EyeLocator.locate -> eyes.assemble_rows -> eyes.purge_detections

Every comparison is exact (``array_equal``).  The rig, the frames and the sizes are tests/test_tracking_gpu.py's (64x64 sub-images,
640x480 and 2000x300 -> 1000x150).

Frame choice.  Tests 3-7 need a frame on which ``detect_faces`` keeps at least three faces.  With the rig's own calibration
(KEEP / LATER_KEEP = 0.3 / 0.7) the frames test_tracking_gpu.py uses do (``FRAME_SEED``); every test asserts the premise before it
relies on it.  Observed on an MI355X: 640x480 of seed 7104 keeps 8 faces, and the tracked step on its 8 boxes (72 windows, composed
counts 69 / 60 / 45 / 36 / 30 after stages 0 / 5 / 10 / 15 / 16) has 18 faces before the purge and keeps 6, slots 0 5 6 4 2 7;
2000x300 of seed 7101 keeps 7 faces, and the tracked step on its 7 boxes (63 windows, 51 / 42 / 33 / 27 / 24) has 21 before the purge
and keeps 7, slots 2 0 2 1 5 5 6.  Partial loss (test 4): the first candidate, zeros over the region of held face 0, leaves slot 7
alone of 8; all lost (test 5): the constant frame.  Cap 2: 18 windows, 1 face kept.  Rescan with max_faces 4: 36 windows keep 2 faces
(slots 0 2), the 18 windows of those keep 1."""
import ctypes as C

import numpy as np
import pytest

from pyfaceanalysis_amd import _capi, grid
from pyfaceanalysis_amd.cascade import frame_levels, tracked_windows
from tests.test_frame_stream_gpu import SF, SUB, Rig
from tests.test_tracking_gpu import HERE, SEED, SIZE_A, SIZE_B, STREAM, assert_full_step, device_frame

pytestmark = pytest.mark.gpu

FRAME_SEED = dict(SEED)          # {(640, 480): 7104, (2000, 300): 7101}: what ``device_frame(size)`` draws
MIN_FACES = 3
MAX_FACES = 8          # of the trackers below, unless a test is about the cap
VICTIM = 0             # test 4: the held face whose search region is overwritten
MARGIN = 8


@pytest.fixture(scope="module")
def rig(native_lib, nets):
    r = Rig(nets)
    yield r
    r.close()


def tracker_for(rig, **kw):
    from pyfaceanalysis_amd.tracking import FaceTracker
    return FaceTracker(rig.dc, rig.loc, smallest_face=SF, **kw)


def composed(rig, fdev, boxes):
    """The tracked frame of the held ``boxes`` (K, 4) through the existing calls: (faces, n_before_purge, slots derived on the host, the
    cascade's result).  A kept row's slot: the assembled rows it equals byte for byte, their cascade survivors' orig_index // 9 — which
    must agree among themselves."""
    from pyfaceanalysis_amd import eyes as E
    pre = rig.dc.prescale(fdev).clone()
    det = rig.dc.detect(pre, windows=tracked_windows(np.asarray(boxes).reshape(-1, 4), rig.pipe, SUB))
    out = rig.loc.locate(pre, det["coords"], det["angles"])
    rows = E.assemble_rows(det["coords"], det["angles"], det["confidence"], out["eye_coords"], out["too_far"])
    src = det["orig_index"][~np.asarray(out["too_far"], dtype=bool)] // 9          # held face of every assembled row
    assert len(src) == len(rows)
    faces = E.purge_detections(rows)
    slots = []
    for f in faces:
        same = [int(src[r]) for r in range(len(rows)) if rows[r].tobytes() == f.tobytes()]
        assert same and len(set(same)) == 1, ("a kept row matches assembled rows of several held faces", same)
        slots.append(same[0])
    return faces, len(rows), np.array(slots, dtype=np.int32), det


def assert_tracked_step(rig, got, fdev, boxes, what):
    k = len(boxes)
    want, n_before, slots, det = composed(rig, fdev, boxes)
    print("%s: K = %d, composed counts %s, before purge %d, faces %d, slots %s, n_held %s" %
          (what, k, det["counts"], n_before, len(want), slots.tolist(), got.get("n_held")))
    assert got["tracked"] is True and got["n_windows"] == 9 * k and got["counts"] == [-1] * len(rig.stages), what
    assert got["faces"].shape == want.shape and np.array_equal(got["faces"], want), (what, got["faces"], want)
    assert got["n_before_purge"] == n_before, what
    assert got["rows_executed"] == 9 * k * sum(s.flow is not None for s in rig.stages), what
    assert got["slots"].dtype == np.int32 and np.array_equal(got["slots"], slots), (what, got["slots"], slots)
    return want, slots


def carried_of(faces, max_faces):
    cand = faces[:max_faces, :4]
    return cand[np.isfinite(cand).all(axis=1)]


def assert_state(tr, faces, got, what):
    want = carried_of(faces, tr.max_faces)
    assert np.array_equal(tr.tracked_faces, want) and got["n_held"] == len(want), (what, tr.tracked_faces, want)
    assert (tr.tracked_face is None) == (len(want) == 0) and (len(want) == 0 or np.array_equal(tr.tracked_face, want[0])), what


def first_step(rig, tr, fdev, what):
    """Step 0 of a fresh tracker: a full-grid step equal to ``detect_faces``, slots all -1; the premise of tests 3-7."""
    r0 = tr.step(fdev)
    assert_full_step(rig, r0, fdev, what)
    print("%s: detect_faces keeps %d faces" % (what, len(r0["faces"])))
    assert len(r0["faces"]) >= MIN_FACES, (what, "the frame must keep at least three faces", len(r0["faces"]))
    assert np.array_equal(r0["slots"], np.full(len(r0["faces"]), -1, dtype=np.int32)), what
    assert_state(tr, r0["faces"], r0, what)
    return r0


def test_multi_grid_kernel(native_lib):
    """1. hg_cascade_tracked_grid_multi_device: every fixture group (boxes of one sub-image size) in ONE launch equals the reference's
    outputs bit for bit; K boxes in one launch equal K launches of hg_cascade_tracked_grid_device; the refusals."""
    import os

    import torch
    fx = np.load(os.path.join(HERE, "golden", "reference_tracking.npz"))
    L, p = _capi.lib(), grid.FACE_PIPELINE
    stream = torch.cuda.current_stream().cuda_stream
    groups = {}
    for i, s in enumerate(fx["sub"]):
        groups.setdefault((int(s[0]), int(s[1])), []).append(i)
    assert len(groups) >= 3 and max(len(v) for v in groups.values()) > 8          # more than one block of 64 windows
    assert fx["fma_side"].sum() >= 8 and fx["fma_corner"].sum() >= 8
    tc = _capi.HgTrackedConsts()
    for (sw, sh), idx in groups.items():
        k = len(idx)
        tc.subimage_width, tc.subimage_height = float(sw), float(sh)
        tc.regression_width, tc.regression_height, tc.net_Dx, tc.net_Dy = p["regression_width"], p["regression_height"], p["net_Dx"], p["net_Dy"]
        faces = torch.from_numpy(np.ascontiguousarray(fx["box"][idx])).cuda()
        boxes = torch.full((9 * k + 1, 4), float("nan"), dtype=torch.float64, device="cuda")          # one guard row behind each output
        level = torch.full((9 * k + 1, 3), float("nan"), dtype=torch.float64, device="cuda")
        _capi.check(L.hg_cascade_tracked_grid_multi_device(0, C.byref(tc), faces.data_ptr(), k, boxes.data_ptr(), level.data_ptr(), stream))
        one_b = torch.full((k, 9, 4), float("nan"), dtype=torch.float64, device="cuda")
        one_l = torch.full((k, 9, 3), float("nan"), dtype=torch.float64, device="cuda")
        for j in range(k):
            _capi.check(L.hg_cascade_tracked_grid_device(0, C.byref(tc), faces[j].data_ptr(), one_b[j].data_ptr(), one_l[j].data_ptr(), stream))
        boxes, level = boxes.cpu().numpy(), level.cpu().numpy()
        assert np.isnan(boxes[-1]).all() and np.isnan(level[-1]).all(), (sw, sh)
        want_l = np.concatenate([np.tile([fx["maxd"][i][0], fx["maxd"][i][1], fx["base_side"][i]], (9, 1)) for i in idx])
        assert np.array_equal(boxes[:-1], np.concatenate([fx["boxes"][i] for i in idx])), (sw, sh)
        assert np.array_equal(level[:-1], want_l), (sw, sh)
        assert np.array_equal(boxes[:-1], one_b.cpu().numpy().reshape(-1, 4)) and np.array_equal(level[:-1], one_l.cpu().numpy().reshape(-1, 3)), (sw, sh)
    out_b = torch.full((9, 4), 7.0, dtype=torch.float64, device="cuda")
    out_l = torch.full((9, 3), 7.0, dtype=torch.float64, device="cuda")
    args = (faces.data_ptr(), 1, out_b.data_ptr(), out_l.data_ptr(), stream)
    assert L.hg_cascade_tracked_grid_multi_device(0, None, *args) == _capi.HG_ERR_ARG
    assert L.hg_cascade_tracked_grid_multi_device(0, C.byref(tc), None, 1, out_b.data_ptr(), out_l.data_ptr(), stream) == _capi.HG_ERR_ARG
    assert L.hg_cascade_tracked_grid_multi_device(0, C.byref(tc), faces.data_ptr(), 1, None, out_l.data_ptr(), stream) == _capi.HG_ERR_ARG
    assert L.hg_cascade_tracked_grid_multi_device(0, C.byref(tc), faces.data_ptr(), 1, out_b.data_ptr(), None, stream) == _capi.HG_ERR_ARG
    for bad_n in (0, -3):
        assert L.hg_cascade_tracked_grid_multi_device(0, C.byref(tc), faces.data_ptr(), bad_n, out_b.data_ptr(), out_l.data_ptr(), stream) == _capi.HG_ERR_ARG
    for bad in (float("nan"), float("inf"), 0.0, -40.0):
        tc.net_Dx = bad
        assert L.hg_cascade_tracked_grid_multi_device(0, C.byref(tc), *args) == _capi.HG_ERR_ARG, bad
    torch.cuda.synchronize()
    assert (out_b.cpu().numpy() == 7.0).all() and (out_l.cpu().numpy() == 7.0).all()          # a refusal launches nothing


def run_single_stream(rig, make):
    tr = make()
    log = []
    try:
        for size, seed, reset in STREAM:
            if reset:
                tr.reset()
                assert tr.tracked_face is None
            got = tr.step(device_frame(size, seed))
            log.append((got, None if tr.tracked_face is None else tr.tracked_face.copy()))
        return log
    finally:
        tr.close()


def test_max_faces_one_is_the_single_face_tracker(rig):
    """2. test_tracking_gpu.py's twelve-element stream through a tracker created by hg_tracker_create_multi(1, 0) and stepped through
    the new entry, then through today's ``FaceTracker``: flags, faces, counts and the carried box are equal at every step."""
    from pyfaceanalysis_amd.tracking import tracked_consts

    def via_create_multi():
        tr = tracker_for(rig)
        L = _capi.lib()
        L.hg_tracker_free(tr._h)
        tr._h = None
        h, tc = C.c_void_p(), tracked_consts(rig.dc)
        _capi.check(L.hg_tracker_create_multi(rig.dc._handle(), rig.loc._handle(), C.byref(tc), 1, 0, C.byref(h)))
        tr._h, tr._multi = h, True
        return tr

    assert len(STREAM) == 12
    a = run_single_stream(rig, via_create_multi)
    b = run_single_stream(rig, lambda: tracker_for(rig))
    print("stream:", [(x["tracked"], len(x["faces"]), x["n_windows"]) for x, _ in a])
    assert sum(x["tracked"] for x, _ in a) >= 6 and any(x["tracked"] and len(x["faces"]) for x, _ in a)
    for i, ((x, bx), (y, by)) in enumerate(zip(a, b)):
        assert "slots" in x and "n_held" in x and "slots" not in y and "n_held" not in y, i
        assert sorted(y) == ["counts", "faces", "n_before_purge", "n_windows", "rows_executed", "tracked"], i
        assert x["tracked"] is y["tracked"] and x["faces"].shape == y["faces"].shape and np.array_equal(x["faces"], y["faces"]), i
        for key in ("n_before_purge", "n_windows", "counts", "rows_executed"):
            assert x[key] == y[key], (i, key)
        assert (bx is None) == (by is None) and (bx is None or np.array_equal(bx, by)), i
        assert x["n_held"] == (0 if bx is None else 1), i
        assert np.array_equal(x["slots"], np.full(len(x["faces"]), 0 if x["tracked"] else -1, dtype=np.int32)), i


def test_tracked_frame_of_k_faces_equals_the_composed_path(rig):
    """3. Frame 0 through the full grid keeps K >= 3 faces; frame 1 (the same picture) is ONE tracked step over 9 K windows whose
    faces, counts and slots are those of the composed path on the same prescaled frame, for both frame sizes (one prescaled).  At
    least two held faces must be behind the kept rows: otherwise nothing is shown about pooling."""
    assert FRAME_SEED == {SIZE_A: 7104, SIZE_B: 7101}
    for size in (SIZE_A, SIZE_B):
        fdev = device_frame(size)
        tr = tracker_for(rig, max_faces=MAX_FACES)
        try:
            assert tr.tracked_face is None and tr.tracked_faces.shape == (0, 4)
            r0 = first_step(rig, tr, fdev, (size, "frame 0"))
            held = tr.tracked_faces
            assert MIN_FACES <= len(held) <= MAX_FACES
            r1 = tr.step(fdev)
            want, slots = assert_tracked_step(rig, r1, fdev, held, (size, "frame 1"))
            assert len(set(slots.tolist())) >= 2, (size, slots)
            assert_state(tr, r1["faces"], r1, (size, "frame 1"))
        finally:
            tr.close()


def region_of(rig, box, frame_w, frame_h):
    """The search region of one held face: its nine windows (the box and one separation step to either side), MARGIN pixels wider on
    every side, clipped to the frame; (x_lo, y_lo, x_hi, y_hi) as slice bounds."""
    w, _ = tracked_windows(box, rig.pipe, SUB)
    x_lo, y_lo = int(np.floor(w[:, 0].min())) - MARGIN, int(np.floor(w[:, 1].min())) - MARGIN
    x_hi, y_hi = int(np.ceil(w[:, 2].max())) + 1 + MARGIN, int(np.ceil(w[:, 3].max())) + 1 + MARGIN
    return max(x_lo, 0), max(y_lo, 0), min(x_hi, frame_w), min(y_hi, frame_h)


def test_partial_loss(rig):
    """4. The search region of ONE held face overwritten (zeros, then noise of seeds 9900-9903; the first for which the composed path
    keeps some but not all slots): the tracked step equals the composed path, fewer faces are held afterwards, and the following step
    runs 9 * n_held windows and equals ITS composed path with the new boxes."""
    import torch
    fdev = device_frame(SIZE_A)
    tr = tracker_for(rig, max_faces=MAX_FACES)
    try:
        first_step(rig, tr, fdev, "frame 0")
        held = tr.tracked_faces
        k = len(held)
        x_lo, y_lo, x_hi, y_hi = region_of(rig, held[VICTIM], SIZE_A[0], SIZE_A[1])
        assert x_hi - x_lo > 16 and y_hi - y_lo > 16
        fills = [torch.zeros((SIZE_A[1], SIZE_A[0]), dtype=torch.uint8, device="cuda")] + [device_frame(SIZE_A, 9900 + j) for j in range(4)]
        chosen = None
        for j, fill in enumerate(fills):
            cand = fdev.clone()
            cand[y_lo:y_hi, x_lo:x_hi] = fill[y_lo:y_hi, x_lo:x_hi]
            _, _, slots, _ = composed(rig, cand, held)
            print("partial loss: candidate %d keeps slots %s of %d held" % (j, sorted(set(slots.tolist())), k))
            if 0 < len(set(slots.tolist())) < k:
                chosen = cand
                break
        assert chosen is not None, "no candidate overwrite loses some but not all held faces"
        r1 = tr.step(chosen)
        assert_tracked_step(rig, r1, chosen, held, "the overwritten frame")
        assert_state(tr, r1["faces"], r1, "the overwritten frame")
        assert 0 < r1["n_held"] < k, (r1["n_held"], k)
        held1 = tr.tracked_faces
        r2 = tr.step(chosen)
        assert r2["n_windows"] == 9 * r1["n_held"]
        assert_tracked_step(rig, r2, chosen, held1, "the frame after the loss")
        assert_state(tr, r2["faces"], r2, "the frame after the loss")
    finally:
        tr.close()


def test_all_lost_returns_to_the_full_grid(rig):
    """5. A tracked step on a frame where the composed K-face path keeps nothing (a constant frame, else noise of other seeds — the
    composed path decides before the tracker sees the frame) returns no row and holds nothing; the next step is a full-grid step
    equal to ``detect_faces``."""
    import torch
    fdev = device_frame(SIZE_A)
    tr = tracker_for(rig, max_faces=MAX_FACES)
    try:
        r0 = first_step(rig, tr, fdev, "frame 0")
        held = tr.tracked_faces
        cands = [torch.zeros((SIZE_A[1], SIZE_A[0]), dtype=torch.uint8, device="cuda")] + [device_frame(SIZE_A, 9900 + j) for j in range(8)]
        lost = None
        for j, f in enumerate(cands):
            faces, _, _, det = composed(rig, f, held)
            if len(faces) == 0:
                lost = f
                print("all lost: candidate %d, composed counts %s" % (j, det["counts"]))
                break
        assert lost is not None, "no candidate frame loses every held face"
        r1 = tr.step(lost)
        assert_tracked_step(rig, r1, lost, held, "the losing frame")
        assert r1["faces"].shape == (0, 10) and r1["slots"].shape == (0,) and r1["n_held"] == 0
        assert tr.tracked_face is None and tr.tracked_faces.shape == (0, 4)
        r2 = tr.step(fdev)
        assert_full_step(rig, r2, fdev, "after the loss")
        assert np.array_equal(r2["faces"], r0["faces"]) and (r2["slots"] == -1).all() and r2["n_held"] == r0["n_held"]
    finally:
        tr.close()


def test_the_cap(rig):
    """6. max_faces = 2 on a frame with >= 3 faces: the first two rows are carried, the next step has 18 windows and equals the composed
    path on those two boxes."""
    fdev = device_frame(SIZE_A)
    tr = tracker_for(rig, max_faces=2)
    try:
        r0 = first_step(rig, tr, fdev, "frame 0")
        assert np.isfinite(r0["faces"][:2, :4]).all()
        assert np.array_equal(tr.tracked_faces, r0["faces"][:2, :4]) and r0["n_held"] == 2
        r1 = tr.step(fdev)
        assert r1["n_windows"] == 18
        assert_tracked_step(rig, r1, fdev, r0["faces"][:2, :4], "frame 1")
        assert_state(tr, r1["faces"], r1, "frame 1")
        assert r1["n_held"] <= 2
    finally:
        tr.close()


def run_rescan(rig, check):
    fdev = device_frame(SIZE_A)
    tr = tracker_for(rig, max_faces=4, rescan_every=2)
    log = []
    try:
        for i in range(6):
            held = tr.tracked_faces
            got = tr.step(fdev)
            if check:
                if got["tracked"]:
                    assert_tracked_step(rig, got, fdev, held, "step %d" % i)
                else:
                    assert_full_step(rig, got, fdev, "step %d" % i)
                    assert len(got["faces"]) >= MIN_FACES and (got["slots"] == -1).all() and len(got["slots"]) == len(got["faces"]), i
                assert_state(tr, got["faces"], got, "step %d" % i)
            log.append(got)
        return log
    finally:
        tr.close()


def test_rescan(rig):
    """7. rescan_every = 2 over six steps on one frame: full, tracked, tracked, full, tracked, tracked.  Every full step equals
    ``detect_faces`` with slots all -1, every tracked step the composed path."""
    log = run_rescan(rig, check=True)
    assert [g["tracked"] for g in log] == [False, True, True, False, True, True]
    assert all(g["n_held"] > 0 for g in log), "a step that holds nothing would make the next one full for another reason"


def test_shared_handles(rig):
    """8. ``detect_faces``, ``EyeLocator.locate`` and a single-face tracker's first two steps give the same bytes before and after a
    multi tracker has run full and tracked steps on the same cascade and eye handles; the six steps of a second run through a fresh
    multi tracker give the bytes of the first."""
    fdev = device_frame(SIZE_A)
    small = device_frame((1000, 562), 8600)
    n = min(40, len(rig.face_boxes))

    def snapshot():
        faces = rig.dc.detect_faces(fdev, rig.loc, smallest_face=SF)
        loc = rig.loc.locate(small, rig.face_boxes[:n], rig.face_angles[:n], return_patches=True)
        tr = tracker_for(rig)
        try:
            steps = [tr.step(fdev) for _ in range(2)]
        finally:
            tr.close()
        assert steps[0]["tracked"] is False and steps[1]["tracked"] is True
        return faces, loc, steps

    def same(x, y, what):
        for key in sorted(x):
            assert np.array_equal(x[key], y[key]), (what, key)

    before = snapshot()
    a = run_rescan(rig, check=False)
    assert [g["tracked"] for g in a] == [False, True, True, False, True, True] and a[1]["n_windows"] > 9
    after = snapshot()
    same(before[0], after[0], "detect_faces")
    for key in ("eye_coords", "too_far", "reg", "patches"):
        assert np.array_equal(before[1][key], after[1][key]), key
    for i in range(2):
        same(before[2][i], after[2][i], "single-face step %d" % i)
    b = run_rescan(rig, check=False)
    for i, (x, y) in enumerate(zip(a, b)):
        assert sorted(x) == sorted(y)
        same(x, y, "second run, step %d" % i)


def raw_step(rig, tr, fdev, rows, slots, want_held=True):
    """hg_tracker_step_frame_multi_device by hand on ``tr``'s handle: (rc, n_out, used_tracked_grid, n_held)."""
    import torch
    fh, fw = int(fdev.shape[0]), int(fdev.shape[1])
    levels, n_levels, _ = frame_levels(fw, fh, SF, rig.dc.pipeline, (rig.dc.w, rig.dc.h))
    counts = np.zeros(len(rig.stages), dtype=np.int32)
    n_out, n_before, n_rows, used, n_held = C.c_int64(-5), C.c_int64(), C.c_int64(), C.c_int(), C.c_int(-5)
    rc = _capi.lib().hg_tracker_step_frame_multi_device(
        tr._h, fdev.data_ptr(), fh, fw, fdev.stride(0), 0, 0, levels, n_levels, rows.ctypes.data_as(C.c_void_p), len(rows), C.byref(n_out),
        C.byref(n_before), counts.ctypes.data_as(C.c_void_p), C.byref(n_rows), C.byref(used),
        None if slots is None else slots.ctypes.data_as(C.c_void_p), C.byref(n_held) if want_held else None,
        torch.cuda.current_stream().cuda_stream)
    return rc, n_out.value, used.value, n_held.value


def test_refusals_through_the_c_abi(rig):
    """9. out_cap below the kept count is HG_ERR_ARG on a full-grid step and on a tracked step, and the caller's rows and slots keep
    their sentinel bytes; null ``slots`` and ``n_held`` are accepted."""
    assert grid.prescaled_size(*SIZE_A) == SIZE_A          # raw_step passes no prescale
    fdev = device_frame(SIZE_A)
    want = rig.dc.detect_faces(fdev, rig.loc, smallest_face=SF)["faces"]
    assert len(want) >= MIN_FACES
    tr = tracker_for(rig, max_faces=MAX_FACES)
    try:
        small_rows, small_slots = np.full((len(want) - 1, 10), -77.0), np.full(len(want) - 1, -77, dtype=np.int32)
        rc, n_out, used, _ = raw_step(rig, tr, fdev, small_rows, small_slots)
        assert rc == _capi.HG_ERR_ARG and used == 0 and n_out == 0
        assert (small_rows == -77.0).all() and (small_slots == -77).all()
        rows, slots = np.full((9 * MAX_FACES + 1 + len(want), 10), -77.0), np.full(9 * MAX_FACES + 1 + len(want), -77, dtype=np.int32)
        rc, n_out, used, n_held = raw_step(rig, tr, fdev, rows, slots)
        assert rc == _capi.HG_OK and used == 0 and n_out == len(want) and np.array_equal(rows[:n_out], want)
        assert (slots[:n_out] == -1).all() and (slots[n_out:] == -77).all() and (rows[n_out:] == -77.0).all()
        held = carried_of(want, MAX_FACES)
        assert n_held == len(held) >= MIN_FACES
        faces1, _, slots1, _ = composed(rig, fdev, held)
        assert len(faces1) >= 2, "the tracked step must keep rows for its refusal to mean anything"
        small_rows, small_slots = np.full((len(faces1) - 1, 10), -77.0), np.full(len(faces1) - 1, -77, dtype=np.int32)
        rc, n_out, used, n_held1 = raw_step(rig, tr, fdev, small_rows, small_slots)
        assert rc == _capi.HG_ERR_ARG and used == 1 and n_out == 0
        assert (small_rows == -77.0).all() and (small_slots == -77).all()
        held1 = carried_of(faces1, MAX_FACES)
        assert n_held1 == len(held1)          # the hand-over has happened: the next step tracks the new boxes
        if len(held1):
            faces2, _, _, _ = composed(rig, fdev, held1)
            rows[:] = -77.0
            rc, n_out, used, _ = raw_step(rig, tr, fdev, rows, None, want_held=False)
            assert rc == _capi.HG_OK and used == 1 and n_out == len(faces2) and np.array_equal(rows[:n_out], faces2)
            assert (rows[n_out:] == -77.0).all()
    finally:
        tr.close()
