"""CPU: tests/filters_restate.py — the BILINEAR / BICUBIC window rule the device kernels implement (include/higsfa.h) — against PIL
itself, bit for bit: EXTENT cuts of 24 boxes (inside, over every edge, entirely outside, magnifying, shrinking about 8 x), rotations
about non-integer centres, the composed rotated window, and BICUBIC's clamp on a 0 / 255 checkerboard."""
import numpy as np
import pytest
from PIL import Image

from tests import filters_cases as FC
from tests import filters_restate as FR


@pytest.mark.parametrize("filt", FC.FILTERS)
def test_extent_equals_pil(filt):
    frame, boxes = FC.frame(), FC.boxes()
    inside = 0
    for size in ((16, 12), (64, 64)):
        for i, b in enumerate(boxes):
            want = FC.pil_window(frame, b, 0.0, size, filt)
            assert np.array_equal(FR.extent(frame, b, size, filt).reshape(-1), want), (size, i)
            inside += int(want.any())
    assert inside >= 40                                     # all but the boxes outside the frame hold pixels
    for i in (14, 15):
        assert not FC.pil_window(frame, boxes[i], 0.0, (16, 12), filt).any(), i


@pytest.mark.parametrize("filt", FC.FILTERS)
def test_rotate_equals_pil(filt):
    frame = FC.frame()
    im = Image.fromarray(frame, "L")
    for ang in FC.ANGLES:
        for c in ((20.3, 15.1), (0.7, 35.9), (52.4, 1.2)):
            want = np.asarray(im.rotate(ang, filt, center=c))
            assert np.array_equal(FR.rotate(frame, ang, c, filt), want), (ang, c)


@pytest.mark.parametrize("filt", FC.FILTERS)
def test_rotated_windows_equal_pil(filt):
    frame = FC.frame()
    boxes = np.concatenate([FC.corner_boxes(), FC.boxes()[[0, 7, 20, 23]]])
    for ang in FC.ANGLES:
        for i, b in enumerate(boxes):
            for size in ((16, 12), (20, 12)):
                assert np.array_equal(FR.window(frame, b, ang, size, filt), FC.pil_window(frame, b, ang, size, filt)), (ang, i, size)


def test_bicubic_clamp_is_reached():
    board = FC.checkerboard()
    seen = set()
    for b, ang in zip(FC.boxes()[:6], (0.0, 17.0, 0.0, -135.0, 0.5, 45.0)):
        want = FC.pil_window(board, b, ang, (64, 64), 3)
        assert np.array_equal(FR.window(board, b, ang, (64, 64), 3), want), (ang, b)
        seen |= set(np.unique(want).tolist())
    assert 0 in seen and 255 in seen
    # the clamp, not only the board's own values: its taps between two equal pixels leave [0, 255] on both sides
    assert list(board[4, 3:7]) == [255, 0, 0, 255] and list(board[4, 5:9]) == [0, 255, 255, 0]
    assert FR._bicubic(0.0, 255.0, 255.0, 0.0, 0.5) > 255 and FR._bicubic(255.0, 0.0, 0.0, 255.0, 0.5) < 0
