"""CPU: the restated eye step and purge against answers worked out by hand from the reference's code, the exact contrast statistics,
and the eye entry points' refusals on the host (no GPU needed)."""
import ctypes as C

import numpy as np
import pytest

from pyfaceanalysis_amd import _capi
from pyfaceanalysis_amd.classifier import GaussianClassifier
from pyfaceanalysis_amd.flow import Flow
from tests import eyes_restate as ER
from tests import helpers


def row(el, er, conf, box=(0.0, 0.0, 100.0, 100.0), angle=0.0):
    return np.array(list(box) + [angle, el[0], el[1], er[0], er[1], conf], dtype=np.float64)


def test_purge_merges_a_duplicate_within_a_quarter_eye_distance():
    a = row((100.0, 100.0), (140.0, 100.0), 0.1)                     # eye distance 40, w = 0.9 * 40
    near = row((108.0, 100.0), (148.0, 100.0), 0.5)                  # moved by 0.2 * 40: error 0.2, not > 0.25 -> merged
    far = row((112.0, 100.0), (152.0, 100.0), 0.5)                   # moved by 0.3 * 40: error 0.3 -> kept
    assert np.array_equal(ER.purge([near, a]), a[None])
    assert np.array_equal(ER.purge([far, a]), np.stack([a, far]))


def test_purge_orders_by_area_weighted_confidence():
    r0 = row((0.0, 0.0), (40.0, 0.0), 0.5)                           # w = 0.5 * 40 = 20
    r1 = row((500.0, 0.0), (700.0, 0.0), 0.8)                        # w = 0.2 * 200 = 40 (least confident, largest)
    r2 = row((0.0, 900.0), (10.0, 900.0), 0.1)                       # w = 0.9 * 10 = 9
    assert np.array_equal(ER.purge([r0, r1, r2]), np.stack([r1, r0, r2]))


def test_purge_exact_ties_follow_the_reversed_stable_order():
    rows = [row((1000.0 * i, 0.0), (1000.0 * i + 40.0, 0.0), 0.5) for i in range(4)]      # equal w, far apart
    assert np.array_equal(ER.purge(rows), np.stack(rows[::-1]))
    w = np.ones(4)
    assert list(np.argsort(w, kind="stable")[::-1]) == [3, 2, 1, 0]


def test_purge_of_zero_and_one_rows_is_a_copy():
    one = row((1.0, 2.0), (3.0, 4.0), 0.5)[None]
    out = ER.purge(one)
    assert np.array_equal(out, one) and out is not one
    assert ER.purge(np.zeros((0, 10))).shape == (0, 10)


def test_purge_zero_eye_distance_follows_numpy():
    # all eye distances zero: w = 0 everywhere, w / w.max() = 0 / 0 = NaN for every row, so the order is the reversed index order;
    # the first kept row against itself: 0 / 0 = NaN never lowers min_d (10000), so it is appended a second time; the other row
    # against it: x / 0 = inf, not < 10000 either -> appended
    r0 = row((10.0, 10.0), (10.0, 10.0), 0.5)
    r1 = row((50.0, 10.0), (50.0, 10.0), 0.2)
    assert np.array_equal(ER.purge([r0, r1]), np.stack([r1, r1, r0]))
    # one zero-distance row among normal ones: its w is 0 (last), its own eye distance is never a divisor of a kept row's error
    r2 = row((0.0, 0.0), (40.0, 0.0), 0.5)
    assert np.array_equal(ER.purge([r0, r2]), np.stack([r2, r0]))
    with np.errstate(invalid="ignore", divide="ignore"):
        assert np.isnan(ER.relative_error_detection(r0[5:9], r0[5:9]))
        assert np.isinf(ER.relative_error_detection(r1[5:9], r0[5:9]))


def test_vectorised_min_error_equals_the_literal_loop():
    rng = np.random.default_rng(2)
    rows = rng.uniform(0, 100, (60, 10))
    rows[::5, 7:9] = rows[::5, 5:7]                                      # zero eye distances
    rows[10:20, 5:9] = rows[0, 5:9] + rng.uniform(0, 3, (10, 4))         # near duplicates
    rows[30:40] = rows[40:50]                                            # exact ties
    assert np.array_equal(ER.purge(rows), ER.purge(rows, literal=True))
    for i in range(len(rows)):
        assert ER.min_error(rows[i, 5:9], rows[:, 5:9]) == ER.literal_min_error(rows[i, 5:9], rows[:, 5:9])


def test_eye_boxes_known_answer_at_zero_angle():
    # a 132 x 132 box at the origin: eye_dx = 18.5 * (132 / 64) / 1.65, eye_dy = 21 * (132 / 64) / 1.65, box side 132 / 105.6 * 75.9008
    eyes, left, right = ER.eye_boxes((0.0, 0.0, 132.0, 132.0), 0.0)
    dx, dy = 18.5 * (132.0 / 64.0) / 1.65, 21.0 * (132.0 / 64.0) / 1.65
    assert np.allclose(eyes, [66.0 - dx, 66.0 - dy, 66.0 + dx, 66.0 - dy], rtol=0, atol=1e-12)
    side = 132.0 / 105.6 * (64 * 2.3719 / 2)
    assert np.allclose(left, [66.0 - dx - side / 2, 66.0 - dy - side / 2, 66.0 - dx + side / 2, 66.0 - dy + side / 2], rtol=0, atol=1e-12)
    assert np.allclose(right[[1, 3]], left[[1, 3]], rtol=0, atol=0)


def test_shift_without_regression_keeps_the_box_centres():
    boxes = np.array([[10.0, 20.0, 150.0, 170.0], [0.0, 0.0, 64.0, 64.0]])
    ang = np.array([0.0, 12.5])
    eb = ER.all_eye_boxes(boxes, ang)
    ec, far = ER.shift_eyes(eb, ang, np.zeros((2, 4)))
    assert not far.any()
    assert np.array_equal(ec[:, :2], (eb[:2, 0:2] + eb[:2, 2:4]) / 2.0) and np.array_equal(ec[:, 2:], (eb[2:, 0:2] + eb[2:, 2:4]) / 2.0)
    _, far = ER.shift_eyes(eb, ang, np.array([[0.0, 0.0, 9.0, 0.0], [0.0, -8.99, 0.0, 0.0]]))
    assert list(far) == [True, False]


def test_exact_contrast_statistics_match_numpy_std():
    rng = np.random.default_rng(5)
    for shape in [(64 * 64,), (16 * 24,), (7,)]:
        for _ in range(20):
            p = rng.integers(0, 256, shape, dtype=np.uint8)
            mean, std = ER.contrast_stats(p)
            x = p.astype(np.float64)
            assert abs(mean - x.mean()) <= 1e-12 * max(1.0, abs(x.mean()))
            assert abs(std - x.std()) <= 1e-12 * x.std()
    out = ER.contrast(np.full((1, 16), 7, dtype=np.uint8), 128.0, 40.0)       # std 0: every pixel becomes the target mean
    assert out.dtype == np.float32 and np.all(out == 128.0)


def test_eye_entry_points_refuse_bad_arguments_on_the_host(native_lib):
    L = native_lib
    h = C.c_void_p()

    def consts(w=8, hh=8, k=9):
        c = _capi.HgEyeConsts()
        c.eye_regression_width = c.eye_regression_height = 64.0
        c.face_sampling, c.eye_sampling, c.tolerance = 0.825, 2.3719, 9.0
        c.target_mean, c.target_std = 128.0, 40.0
        c.eye_w, c.eye_h, c.n_features = w, hh, k
        return c
    f = Flow(helpers.linear_net(0), output_dtype=np.float32)                  # 8 x 8 inputs, 9 outputs
    fh = f._handle(on_device=False).h
    assert L.hg_eyes_create(None, None, None, None, C.byref(consts()), 0, C.byref(h)) == _capi.HG_ERR_ARG          # null flows
    assert b"null eye flow" in L.hg_last_error()
    assert L.hg_eyes_create(fh, None, fh, None, None, 0, C.byref(h)) == _capi.HG_ERR_ARG                           # null constants
    assert L.hg_eyes_create(fh, None, fh, None, C.byref(consts(16, 16)), 0, C.byref(h)) == _capi.HG_ERR_DIM         # input width
    assert b"columns" in L.hg_last_error()
    assert L.hg_eyes_create(fh, None, fh, None, C.byref(consts(k=10)), 0, C.byref(h)) == _capi.HG_ERR_DIM           # kept > outputs
    bad = consts()
    bad.target_std = 0.0
    assert L.hg_eyes_create(fh, None, fh, None, C.byref(bad), 0, C.byref(h)) == _capi.HG_ERR_ARG                    # contrast target
    assert L.hg_eyes_create(fh, None, fh, None, C.byref(consts()), 0, C.byref(h)) == _capi.HG_ERR_ARG               # flow not on the device
    assert not h.value
    n_out, n_before, rows = C.c_int64(), C.c_int64(), C.c_int64()
    lv = (_capi.HgCascadeLevel * 1)()
    assert L.hg_cascade_detect_faces_frame_device(None, None, None, 8, 8, 8, 0, 0, lv, 1, None, 0, C.byref(n_out), C.byref(n_before), None,
                                                  C.byref(rows), None) == _capi.HG_ERR_ARG
    assert L.hg_purge_detections_device(0, None, -1, None, None, None) == _capi.HG_ERR_ARG
    assert L.hg_eyes_locate_device(None, None, 8, 8, 8, None, None, 1, None, None, None, None, None) == _capi.HG_ERR_ARG
    assert L.hg_eyes_boxes_device(None, None, None, 1, None, None, None) == _capi.HG_ERR_ARG
    f.close()


def test_eye_locator_refuses_too_few_kept_columns_and_missing_contrast():
    from pyfaceanalysis_amd.eyes import EyeLocator
    f = Flow(helpers.linear_net(0), output_dtype=np.float32)
    g = GaussianClassifier(np.zeros((2, 9)), np.stack([np.eye(9)] * 2), np.ones(2), np.ones(2) / 2, avg_labels=[-1.0, 1.0])
    with pytest.raises(ValueError, match="kept"):
        EyeLocator(f, g, f, g, contrast=(128.0, 40.0), eye_size=(8, 8), n_features=8)
    with pytest.raises(ValueError, match="columns"):
        EyeLocator(f, g, f, g, contrast=(128.0, 40.0), eye_size=(16, 16))
    with pytest.raises(TypeError):
        EyeLocator(f, g, f, g, eye_size=(8, 8))                               # the contrast targets are required
    loc = EyeLocator(f, g, f, g, contrast=(128.0, 40.0), eye_size=(8, 8))
    assert loc.k == 9 and loc.consts().n_features == 9
