"""CPU: the host restatement of the reference's tracking grid (``track_single_face`` with a face found on the previous frame) against
tests/golden/reference_tracking.npz — the outputs of the reference's own compute_sampling_values / compute_posX_posY_values /
compute_subimage_coordinates_from_posX_posY_values (tests/golden/make_reference_tracking.py), bit for bit on every box: ordinary
boxes, oblong ones, x1 < x0, boxes partly outside the frame, and the edge rows where a fused multiply-add would change the last bit."""
import os

import numpy as np
import pytest

from pyfaceanalysis_amd import grid
from pyfaceanalysis_amd.cascade import tracked_windows

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(HERE, "golden", "reference_tracking.npz"))


def test_fixture_holds_the_cases(fx):
    n = len(fx["box"])
    assert n >= 40 and fx["boxes"].shape == (n, 9, 4)
    subs = {tuple(s) for s in fx["sub"]}
    assert {(64, 64), (128, 128), (16, 16)} <= subs
    b = fx["box"]
    assert (np.abs(b[:, 2] - b[:, 0]) != np.abs(b[:, 3] - b[:, 1])).any()          # not square
    assert (b[:, 2] < b[:, 0]).any()                                              # the abs
    assert (fx["posx"][:, 2] < 0).any()                                           # x0 - sepx outside the frame
    assert fx["fma_side"].sum() >= 8 and fx["fma_corner"].sum() >= 8 and not fx["fma_sep"].any()
    assert np.array_equal(fx["consts"], [grid.FACE_PIPELINE[k] for k in ("net_Dx", "net_Dy", "regression_width", "regression_height")])


def test_tracked_grid_equals_the_reference(fx):
    p = grid.FACE_PIPELINE
    for i, box in enumerate(fx["box"]):
        sw, sh = (int(v) for v in fx["sub"][i])
        assert grid.tracked_sampling_value(box, sw) == fx["sampling"][i], i
        xs, ys, pw, ph, mdx, mdy = grid.tracked_positions(box, sw, sh, p["regression_width"], p["regression_height"], p["net_Dx"], p["net_Dy"])
        assert np.array_equal(xs, fx["posx"][i]) and np.array_equal(ys, fx["posy"][i]), i
        assert np.array_equal([pw, ph], fx["patch"][i]) and np.array_equal([mdx, mdy], fx["maxd"][i]), i
        got = grid.tracked_boxes(box, sw, sh, p["regression_width"], p["regression_height"], p["net_Dx"], p["net_Dy"])
        assert got.shape == (9, 4) and got.dtype == np.float64 and np.array_equal(got, fx["boxes"][i]), i
        boxes, level = tracked_windows(box, p, (sw, sh))
        assert boxes.shape == (9, 4) and level.shape == (9, 3)
        assert np.array_equal(boxes, fx["boxes"][i]), i
        assert np.array_equal(level, np.tile([fx["maxd"][i][0], fx["maxd"][i][1], fx["base_side"][i]], (9, 1))), i
    # the defaults are the pipeline's: 64 x 64
    i = int(np.nonzero((fx["sub"] == 64).all(axis=1))[0][0])
    assert np.array_equal(grid.tracked_boxes(fx["box"][i]), fx["boxes"][i])


def test_nine_windows_are_three_boxes_y_major(fx):
    """posY holds one value three times, so the product is the three distinct boxes — at x0, x0 + sepx, x0 - sepx, in that order —
    repeated three times; window j * 3 + i is (posX[i], posY[j], ...)."""
    for i, box in enumerate(fx["box"]):
        b = grid.tracked_boxes(box, *(int(v) for v in fx["sub"][i]))
        assert np.array_equal(b[0:3], b[3:6]) and np.array_equal(b[0:3], b[6:9]), i
        assert np.array_equal(b[:3, 0], fx["posx"][i]) and (b[:, 1] == box[1]).all(), i
        if fx["sampling"][i] > 0:
            assert b[1, 0] > b[0, 0] > b[2, 0], i
            assert len(np.unique(b, axis=0)) == 3, i
