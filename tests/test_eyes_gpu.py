"""GPU: eye localisation and the purge after the face cascade (hg_eyes.hip) against the numpy restatement (tests/eyes_restate.py), on
the synthetic 1920x1080 frame of BASELINE.json configs[2] with the U11L-128 face cascade and U11L-64 eye stages."""
import ctypes as C

import numpy as np
import pytest

from pyfaceanalysis_amd import _capi, grid
from tests import eyes_restate as ER

CONTRAST = (128.0, 48.0)          # the build's contrast targets for these tests (pixel units)


def ulp_close(got, want, scale):
    """|got - want| <= 4 ulp of max(|want|, scale): device cos / sin may differ from libm in the last bit."""
    tol = 4 * np.spacing(np.maximum(np.abs(want), scale))
    return np.all(np.abs(got - want) <= tol)


@pytest.fixture(scope="module")
def setup(native_lib, nets):
    import torch
    from pyfaceanalysis_amd import synth, synth_cascade
    from pyfaceanalysis_amd.cascade import DeviceCascade, frame_windows
    from pyfaceanalysis_amd.eyes import EyeLocator
    from pyfaceanalysis_amd.flow import Flow
    from pyfaceanalysis_amd.patches import Patcher
    rng = np.random.default_rng(synth.INPUT_SEED)
    frame = np.rint(synth._box3(rng.integers(0, 256, (1080, 1920), dtype=np.uint8))).astype(np.uint8)
    pipe = dict(grid.FACE_PIPELINE)
    flow = Flow(nets("U11L-128"), output_dtype=np.float32)
    fdev = torch.from_numpy(frame).cuda()
    boxes, level = frame_windows(1000, 562, 0.1, pipe, (128, 128))
    pt = Patcher()
    stages0 = [synth_cascade.Stage("Disc1", flow, synth_cascade.quantile_classifier(rng.normal(size=(50, 20)), 9, [0.0, 1.0]))]
    dc0 = DeviceCascade(stages0, (128, 128), 20, pipe)
    small_dev = dc0.prescale(fdev)
    small = small_dev.cpu().numpy()
    feats = flow.execute(pt.extract(small, boxes, (128, 128), dtype=np.uint8), n_cols=20)
    # calibrated to leave a handful of survivors on this frame (14 on an MI355X), so that the eye step and the purge have work
    dc = DeviceCascade(synth_cascade.build_face_cascade(flow, feats, pipe, keep_fraction=0.3, later_keep_fraction=0.7), (128, 128), 20, pipe)
    # ~300 faces cut from the grid: angles in +-22.5 plus 0, +-90, 180; a share moved partly outside the frame
    pick = rng.choice(len(boxes), 300, replace=False)
    fboxes = boxes[pick].copy()
    fboxes[:40] -= np.array([60.0, 50.0, 60.0, 50.0])
    fboxes[40:60] += np.array([900.0, 0.0, 900.0, 0.0])
    angles = rng.uniform(-22.5, 22.5, 300)
    angles[::7] = 0.0
    angles[1::23], angles[2::23], angles[3::23] = 90.0, -90.0, 180.0
    # the eye stages, calibrated on features of the restated eye patches of these faces
    eye_flow = Flow(nets("U11L-64"), output_dtype=np.float32)
    eb = ER.all_eye_boxes(fboxes, angles)
    u8 = pt.extract(small, eb, (64, 64), dtype=np.uint8, delta_angs=-np.concatenate([angles, angles]))
    efeats = eye_flow.execute(ER.contrast(u8, *CONTRAST), n_cols=12)
    fx, cx, fy, cy = synth_cascade.build_eye_stages(eye_flow, efeats)
    loc = EyeLocator(fx, cx, fy, cy, contrast=CONTRAST)
    yield dict(frame=frame, fdev=fdev, small=small, small_dev=small_dev, dc=dc, loc=loc, boxes=fboxes, angles=angles, pipe=pipe, flow=flow,
               eye_flow=eye_flow)
    loc.close()
    dc.close()
    dc0.close()
    pt.close()
    eye_flow.close()
    flow.close()


@pytest.mark.gpu
def test_eye_boxes_against_restatement(setup):
    s = setup
    got = s["loc"].eye_boxes(s["boxes"], s["angles"])
    want = ER.all_eye_boxes(s["boxes"], s["angles"])
    zero = np.concatenate([s["angles"] == 0.0] * 2)
    assert zero.sum() >= 60
    assert np.array_equal(got[zero], want[zero])
    scale = np.abs(np.concatenate([s["boxes"]] * 2)).max(axis=1, keepdims=True)
    assert ulp_close(got[~zero], want[~zero], scale[~zero])
    assert (got[:, 0] < 0).any()                                         # some eye boxes reach outside the frame


@pytest.mark.gpu
def test_eye_boxes_against_reference_fixture(setup):
    """hg_eyes_boxes_device against compute_approximate_eye_boxes_coordinates itself (tests/golden/reference_glue.npz): random boxes,
    angles 0, +-90, +-180, +-24.75, tiny, denormal-small and -0.0.  Bit for bit where the angle is zero (cos / sin exact); elsewhere
    within the ulps that device cos / sin may differ from libm by, as above."""
    import os
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_glue.npz"))
    boxes, angles = g["eye_boxes"], g["eye_angles"]
    got = setup["loc"].eye_boxes(boxes, angles)
    want = np.concatenate([g["eye_left"], g["eye_right"]])
    zero = np.concatenate([angles == 0.0] * 2)
    assert zero.sum() >= 8 and np.array_equal(got[zero], want[zero])
    scale = np.abs(np.concatenate([boxes] * 2)).max(axis=1, keepdims=True)
    assert ulp_close(got[~zero], want[~zero], scale[~zero])


@pytest.mark.gpu
def test_patches_bit_exact_against_pil_rule_and_restated_contrast(setup):
    from oracle import pil_restate
    s = setup
    loc = s["loc"]
    out = loc.locate(s["small_dev"], s["boxes"], s["angles"], return_patches=True)
    eb = loc.eye_boxes(s["boxes"], s["angles"])
    dang = -np.concatenate([s["angles"], s["angles"]])
    u8 = pil_restate.extract_subimages_rotate(s["small"], eb, dang, (64, 64))
    want = ER.contrast(u8, *CONTRAST)
    assert out["patches"].shape == (600, 4096) and out["patches"].dtype == np.float32
    assert np.array_equal(out["patches"], want)


@pytest.mark.gpu
def test_eye_coordinates_and_too_far_from_device_regressions(setup):
    s = setup
    loc = s["loc"]
    out = loc.locate(s["small_dev"], s["boxes"], s["angles"])
    eb = loc.eye_boxes(s["boxes"], s["angles"])
    ec, far = ER.shift_eyes(eb, s["angles"], out["reg"])
    assert np.array_equal(out["too_far"], far)
    assert 0 < far.sum() < len(far)                                     # the >= 9 discard removes a visible share, not everything
    scale = np.abs(s["boxes"]).max(axis=1, keepdims=True)
    zero = s["angles"] == 0.0
    assert np.array_equal(out["eye_coords"][zero], ec[zero])
    assert ulp_close(out["eye_coords"], ec, scale)
    assert np.abs(out["reg"]).max() <= 10.5 + 1e-9


@pytest.mark.gpu
def test_batch_independence(setup):
    s = setup
    loc = s["loc"]
    full = loc.locate(s["small_dev"], s["boxes"], s["angles"], return_patches=True)
    for k in (1, 37):
        part = loc.locate(s["small_dev"], s["boxes"][:k], s["angles"][:k], return_patches=True)
        assert np.array_equal(part["eye_coords"], full["eye_coords"][:k]) and np.array_equal(part["too_far"], full["too_far"][:k])
        n = len(s["boxes"])
        assert np.array_equal(part["reg"], np.concatenate([full["reg"][:, :k], full["reg"][:, n:n + k]], axis=1))
        assert np.array_equal(part["patches"], np.concatenate([full["patches"][:k], full["patches"][n:n + k]]))


def purge_cases():
    rng = np.random.default_rng(11)

    def rand_rows(n):
        r = np.zeros((n, 10))
        r[:, 0:4] = rng.uniform(0, 1000, (n, 4))
        r[:, 4] = rng.uniform(-20, 20, n)
        r[:, 5:7] = rng.uniform(0, 1000, (n, 2))
        r[:, 7:9] = r[:, 5:7] + rng.uniform(10, 80, (n, 2))
        r[:, 9] = rng.uniform(0, 1, n)
        return r
    big = rand_rows(4096)
    # planted duplicate clusters: copies moved by less and more than a quarter of the eye distance
    base = big[:200]
    for j, f in enumerate((0.05, 0.15, 0.24, 0.4)):
        d = base.copy()
        dist = np.hypot(d[:, 7] - d[:, 5], d[:, 8] - d[:, 6])
        d[:, 5:9] += (f * dist / np.sqrt(2))[:, None] * np.array([1.0, 0.0, 1.0, 0.0])
        big[200 * (j + 1):200 * (j + 2)] = d
    big[1200:1300, 9] = big[1300:1400, 9]                                # exact ties: same confidence and eye vector
    big[1200:1300, 7:9] = big[1200:1300, 5:7] + (big[1300:1400, 7:9] - big[1300:1400, 5:7])
    big[1400:1420, 7:9] = big[1400:1420, 5:7]                            # zero-area rows
    equal = rand_rows(17)
    equal[:, 7:9] = equal[:, 5:7] + 30.0
    equal[:, 9] = 0.25                                                   # all-equal weights
    zero = rand_rows(3)
    zero[:, 7:9] = zero[:, 5:7]                                          # every eye distance zero: NaN weights, n + 1 rows kept
    return dict(n0=np.zeros((0, 10)), n1=rand_rows(1), n2=rand_rows(2), n17=rand_rows(17), n17_equal=equal, n3_zero=zero, n4096=big)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["n0", "n1", "n2", "n17", "n17_equal", "n3_zero", "n4096"])
def test_purge_on_device_bit_for_bit(native_lib, case):
    from pyfaceanalysis_amd.eyes import purge_detections
    rows = purge_cases()[case]
    got = purge_detections(rows)
    want = ER.purge(rows)
    assert got.shape == want.shape and np.array_equal(got, want)
    if case == "n4096":
        assert len(want) < 4096 - 400
    if case == "n3_zero":
        assert len(want) == 4


@pytest.mark.gpu
def test_whole_call_equals_composed_steps(setup):
    import torch
    from pyfaceanalysis_amd import eyes as E
    s = setup
    dc, loc = s["dc"], s["loc"]

    def composed(fdev):
        det = dc.detect_frame(fdev, smallest_face=0.1)
        small = dc.prescale(fdev)
        out = loc.locate(small, det["coords"], det["angles"])
        rows = E.assemble_rows(det["coords"], det["angles"], det["confidence"], out["eye_coords"], out["too_far"])
        return det, rows, E.purge_detections(rows)
    det, rows, want = composed(s["fdev"])
    got = dc.detect_faces(s["fdev"], loc, smallest_face=0.1)
    assert len(det["coords"]) > 0
    assert got["faces"].shape == want.shape and np.array_equal(got["faces"], want)
    assert got["n_before_purge"] == len(rows) and got["counts"] == det["counts"] and got["rows_executed"] == det["rows_executed"]
    assert got["n_windows"] == 1738
    # another frame of the same size: the plan is reused and the answer is again the composed one
    f2 = torch.from_numpy(np.ascontiguousarray(s["frame"][::-1, ::-1])).cuda()
    _, rows2, want2 = composed(f2)
    got2 = dc.detect_faces(f2, loc, smallest_face=0.1)
    assert np.array_equal(got2["faces"], want2) and got2["n_before_purge"] == len(rows2)
    assert np.array_equal(dc.detect_faces(s["fdev"], loc, smallest_face=0.1)["faces"], want)
    # too small an output buffer: the call fails and writes no row
    m = len(want)
    if m > 0:
        L = _capi.lib()
        levels, n_levels, _ = dc._frames[("faces", 1920, 1080, 0.1, grid.PRESCALE_SIZE)][1:4]
        buf = np.full((m + 4, 10), 7.0)
        a, b, r = C.c_int64(), C.c_int64(), C.c_int64()
        counts = np.zeros(len(dc.stages), dtype=np.int32)
        rc = L.hg_cascade_detect_faces_frame_device(dc._handle(), loc._handle(), s["fdev"].data_ptr(), 1080, 1920, 1920, 1000, 562, levels, n_levels,
                                                    buf.ctypes.data_as(C.c_void_p), m - 1, C.byref(a), C.byref(b), counts.ctypes.data_as(C.c_void_p),
                                                    C.byref(r), torch.cuda.current_stream().cuda_stream)
        assert rc == _capi.HG_ERR_ARG and np.all(buf == 7.0)


@pytest.mark.gpu
def test_frame_without_survivors(setup, nets):
    from pyfaceanalysis_amd import synth_cascade
    from pyfaceanalysis_amd.cascade import DeviceCascade
    s = setup
    rng = np.random.default_rng(3)
    reject_all = synth_cascade.quantile_classifier(rng.normal(size=(50, 20)), 9, [5.0, 6.0])      # every regression >= the cut-off
    dc = DeviceCascade([synth_cascade.Stage("Disc1", s["flow"], reject_all)], (128, 128), 20, s["pipe"])
    got = dc.detect_faces(s["fdev"], s["loc"], smallest_face=0.1)
    assert got["faces"].shape == (0, 10) and got["n_before_purge"] == 0 and got["counts"] == [0]
    dc.close()


@pytest.mark.gpu
def test_bad_frames_after_a_good_one_raise(setup):
    import torch
    s = setup
    dc, loc = s["dc"], s["loc"]
    dc.detect_faces(s["fdev"], loc, smallest_face=0.1)
    with pytest.raises(ValueError):
        dc.detect_faces(s["fdev"].float(), loc, smallest_face=0.1)
    with pytest.raises(ValueError):
        dc.detect_faces(torch.from_numpy(s["frame"]), loc, smallest_face=0.1)
    strided = torch.empty((1920, 1080), dtype=torch.uint8, device=s["fdev"].device).t()
    strided.copy_(s["fdev"])
    assert strided.shape == (1080, 1920) and strided.stride(1) != 1
    with pytest.raises(ValueError):
        dc.detect_faces(strided, loc, smallest_face=0.1)
