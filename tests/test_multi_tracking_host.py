"""CPU: the host side of tracking several faces.  ``cascade.tracked_windows`` / ``grid.tracked_boxes`` on a (K, 4) array of boxes
against tests/golden/reference_tracking.npz (the reference's own per-box outputs), the three new C entries in the header and the
library, and the refusals of ``hg_tracker_create_multi`` that are decided before any handle or device is looked at."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from pyfaceanalysis_amd import _capi, grid
from pyfaceanalysis_amd.cascade import tracked_windows

HERE = os.path.dirname(os.path.abspath(__file__))
NEW_ENTRIES = ("hg_cascade_tracked_grid_multi_device", "hg_tracker_create_multi", "hg_tracker_step_frame_multi_device")


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(HERE, "golden", "reference_tracking.npz"))


def fixture_groups(fx):
    """{(sub_w, sub_h): indices of the fixture's boxes with that sub-image size}, in fixture order."""
    groups = {}
    for i, s in enumerate(fx["sub"]):
        groups.setdefault((int(s[0]), int(s[1])), []).append(i)
    return groups


def expected_of(fx, idx):
    boxes = np.concatenate([fx["boxes"][i] for i in idx])
    level = np.concatenate([np.tile([fx["maxd"][i][0], fx["maxd"][i][1], fx["base_side"][i]], (9, 1)) for i in idx])
    return boxes, level


def test_tracked_windows_of_k_boxes_equal_the_reference(fx):
    """Every group of fixture boxes that share a sub-image size, as ONE (K, 4) array: boxes and level rows are the concatenation of the
    fixture's per-box outputs, bit for bit — the rows where a fused multiply-add would change the last bit included."""
    p = grid.FACE_PIPELINE
    groups = fixture_groups(fx)
    assert len(groups) >= 3 and max(len(v) for v in groups.values()) >= 4
    covered = []
    for (sw, sh), idx in groups.items():
        boxes, level = tracked_windows(fx["box"][idx], p, (sw, sh))
        want_boxes, want_level = expected_of(fx, idx)
        assert boxes.shape == (9 * len(idx), 4) and level.shape == (9 * len(idx), 3) and boxes.dtype == level.dtype == np.float64
        assert np.array_equal(boxes, want_boxes), (sw, sh)
        assert np.array_equal(level, want_level), (sw, sh)
        assert np.array_equal(grid.tracked_boxes(fx["box"][idx], sw, sh), want_boxes), (sw, sh)
        covered += idx
    assert sorted(covered) == list(range(len(fx["box"])))
    assert fx["fma_side"][covered].sum() >= 8 and fx["fma_corner"][covered].sum() >= 8


def test_one_box_as_a_row_and_as_a_vector(fx):
    p = grid.FACE_PIPELINE
    for i in (0, len(fx["box"]) // 2, len(fx["box"]) - 1):
        sub = tuple(int(v) for v in fx["sub"][i])
        b1, l1 = tracked_windows(fx["box"][i], p, sub)                  # (4,)
        b2, l2 = tracked_windows(fx["box"][i][None, :], p, sub)         # (1, 4)
        assert b1.shape == b2.shape == (9, 4) and l1.shape == l2.shape == (9, 3)
        assert np.array_equal(b1, b2) and np.array_equal(l1, l2)
        assert np.array_equal(b1, fx["boxes"][i])
    b0, l0 = tracked_windows(np.zeros((0, 4)), p, (64, 64))
    assert b0.shape == (0, 4) and l0.shape == (0, 3)


def test_new_entries_declared_and_exported(native_lib):
    text = open(os.path.join(os.path.dirname(HERE), "include", "higsfa.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(hg_[a-z_0-9]+)\s*\(", text))
    for name in NEW_ENTRIES:
        assert name in declared, name
        assert hasattr(native_lib, name), name
        assert name in _capi.EXPORTED_SYMBOLS, name


def test_create_multi_refusals_need_no_device(native_lib):
    """max_faces outside 1..64 and rescan_every < 0 are refused as bad ARGUMENTS before any handle is looked at (none exists here);
    in range, the null handles are what is refused."""
    tc = _capi.HgTrackedConsts()
    tc.subimage_width = tc.subimage_height = 64.0
    tc.regression_width = tc.regression_height = 128.0
    tc.net_Dx, tc.net_Dy = 40.0, 20.0
    for max_faces, rescan, word in ((0, 0, "max_faces"), (-1, 0, "max_faces"), (65, 0, "max_faces"), (1 << 20, 0, "max_faces"),
                                    (1, -1, "rescan_every"), (64, -5, "rescan_every"), (1, 0, "null"), (64, 3, "null")):
        h = C.c_void_p(1)
        rc = native_lib.hg_tracker_create_multi(None, None, C.byref(tc), max_faces, rescan, C.byref(h))
        assert rc == _capi.HG_ERR_ARG and not h.value, (max_faces, rescan)
        assert word in native_lib.hg_last_error().decode(), (max_faces, rescan, native_lib.hg_last_error())
    assert native_lib.hg_tracker_create_multi(None, None, C.byref(tc), 2, 0, None) == _capi.HG_ERR_ARG
    # the multi grid kernel's argument checks come before the device is touched as well
    assert native_lib.hg_cascade_tracked_grid_multi_device(0, C.byref(tc), None, 3, None, None, None) == _capi.HG_ERR_ARG
    assert native_lib.hg_cascade_tracked_grid_multi_device(0, None, None, 3, None, None, None) == _capi.HG_ERR_ARG


def test_face_tracker_keywords_default_to_one_face():
    """``FaceTracker``'s new keywords exist and default to the single-face tracker; ``tracked_faces`` stands beside ``tracked_face``."""
    import inspect

    from pyfaceanalysis_amd.tracking import MAX_FACES, FaceTracker
    sig = inspect.signature(FaceTracker.__init__)
    assert sig.parameters["max_faces"].default == 1 and sig.parameters["rescan_every"].default == 0 and MAX_FACES == 64
    assert isinstance(FaceTracker.tracked_faces, property) and isinstance(FaceTracker.tracked_face, property)
