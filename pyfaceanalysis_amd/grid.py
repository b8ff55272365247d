"""Sliding-window grid of the detection cascade: which sub-images reach the hot call.

Restates (vectorised; the adaptive branch and the tracking branch) the three grid builders of the reference,
which decide N for every ``flow.execute`` call (SURVEY.md §2.1 "grid builders", Appendix B):

* ``compute_sampling_values``                         face_analysis.py:575-607
* ``compute_posX_posY_values``                        face_analysis.py:610-657
* ``compute_subimage_coordinates_from_posX_posY_values``   face_analysis.py:661-669

and the constants of ``Pipelines/Pipeline_experimental.txt:2`` / FaceDetectUpdated.py:84,110-111,121-122.
These are O(N) host formulas; they are here so that a frame can be turned into the batches of
BASELINE.json config 3 without the reference's script.  The tracking branch (``track_single_face`` with a face
found on the previous frame: ``tracked_sampling_value``, ``tracked_boxes``; face_analysis.py:576-585, :611-623) is
restated too, in plain float64 in the reference's operation order (tests/golden/reference_tracking.npz pins it bit for
bit).  The non-adaptive branches are out of scope.
"""
from __future__ import annotations

import math

import numpy as np

# Pipelines/Pipeline_experimental.txt:2  (net_Dx net_Dy net_Dang net_mins net_maxs subW subH regW regH)
FACE_PIPELINE = dict(net_Dx=40.0, net_Dy=20.0, net_Dang=22.5, net_mins=0.694, net_maxs=0.981,
                     subimage_width=64, subimage_height=64, regression_width=128, regression_height=128)
PATCH_OVERLAP_SAMPLING = 1.1        # FaceDetectUpdated.py:110
PATCH_OVERLAP_POSX_POSY = 1.1       # FaceDetectUpdated.py:111
PRESCALE_SIZE = 1000                # FaceDetectUpdated.py:122


def prescaled_size(width, height, prescale_size=PRESCALE_SIZE):
    """FaceDetectUpdated.py:551-556: shrink so that the larger side is <= prescale_size."""
    f = max(width * 1.0 / prescale_size, height * 1.0 / prescale_size)
    if f > 1.0:
        return int(width / f), int(height / f)
    return width, height


def sampling_values(im_width, im_height, subimage_width, subimage_height, smallest_face, net_mins, net_maxs,
                    patch_overlap_sampling=PATCH_OVERLAP_SAMPLING):
    """Pyramid levels (face_analysis.py:586-598): start at the smallest face box (>= 20 px), grow by
    (net_maxs / net_mins) / overlap while the largest face of the level still fits the image."""
    min_box_side = max(20, min(im_height, im_width) * smallest_face * 0.825 / net_mins)
    s = min_box_side * 1.0 / subimage_width
    step = (net_maxs / net_mins) / patch_overlap_sampling
    out = []
    while subimage_width * s * net_mins / 0.825 < im_width and subimage_height * s * net_mins / 0.825 < im_height:
        out.append(s)
        s *= step
    return out


def level_boxes(im_width, im_height, sampling_value, subimage_width, subimage_height, regression_width, regression_height,
                net_Dx, net_Dy, patch_overlap_posx_posy=PATCH_OVERLAP_POSX_POSY):
    """(N, 4) boxes (x0, y0, x1, y1) of one pyramid level, y-major like the reference
    (face_analysis.py:630-646 grid, :661-669 box = (posX, posY, posX + pw - 1, posY + ph - 1))."""
    pw, ph = subimage_width * sampling_value, subimage_height * sampling_value
    sep_x = net_Dx * 2.0 * pw / regression_width
    sep_y = net_Dy * 2.0 * ph / regression_height
    nx = int(math.ceil((1 + (im_width - pw) / sep_x) * patch_overlap_posx_posy))
    ny = int(math.ceil((1 + (im_height - ph) / sep_y) * patch_overlap_posx_posy))
    xs = np.linspace(0.0, im_width - pw, nx)
    ys = np.linspace(0.0, im_height - ph, ny)
    gx, gy = np.meshgrid(xs, ys)            # row (y) major
    x0, y0 = gx.reshape(-1), gy.reshape(-1)
    return np.stack([x0, y0, x0 + pw - 1, y0 + ph - 1], axis=1)


def frame_boxes(im_width, im_height, smallest_face=0.2, pipeline=None, subimage_size=None):
    """All first-stage windows of one frame: list of (sampling_value, boxes) per pyramid level.
    ``subimage_size`` overrides the pipeline's 64x64 sub-image (BASELINE.json measures 128x128)."""
    p = dict(FACE_PIPELINE if pipeline is None else pipeline)
    if subimage_size is not None:
        p["subimage_width"], p["subimage_height"] = subimage_size
    levels = []
    for s in sampling_values(im_width, im_height, p["subimage_width"], p["subimage_height"], smallest_face,
                             p["net_mins"], p["net_maxs"]):
        levels.append((s, level_boxes(im_width, im_height, s, p["subimage_width"], p["subimage_height"],
                                      p["regression_width"], p["regression_height"], p["net_Dx"], p["net_Dy"])))
    return levels


def tracked_sampling_value(box, subimage_width):
    """The ONE sampling value of a frame that follows a found face (face_analysis.py:576-585): the mean of the tracked box's sides
    over the sub-image width.  ``box``: (x0, y0, x1, y1) of the first purged detection of the previous frame."""
    x0, y0, x1, y1 = (float(v) for v in box[:4])
    face_size = 0.5 * abs(x1 - x0) + 0.5 * abs(y1 - y0)
    return face_size * 1.0 / subimage_width


def tracked_positions(box, subimage_width, subimage_height, regression_width, regression_height, net_Dx, net_Dy):
    """posX (3), posY (3), patch width, patch height, max_Dx_diff, max_Dy_diff of the tracking branch (face_analysis.py:611-623,
    :650-651): the box's corner and one horizontal separation step to either side, all three at the box's own y."""
    x0, y0 = float(box[0]), float(box[1])
    s = tracked_sampling_value(box, subimage_width)
    pw, ph = subimage_width * s, subimage_height * s
    sep_x = net_Dx * 2.0 * pw / regression_width
    return ([x0, x0 + sep_x, x0 - sep_x], [y0, y0, y0], pw, ph, net_Dx * pw / regression_width, net_Dy * ph / regression_height)


def tracked_boxes(box, subimage_width=None, subimage_height=None, regression_width=None, regression_height=None, net_Dx=None, net_Dy=None):
    """(9, 4) windows of a tracked frame: the product of posX and posY (face_analysis.py:661-669), y-major — the three distinct
    boxes (x, y0, x + pw - 1, y0 + ph - 1), three times over, because posY holds the same value three times.  The duplicates reach
    the purge as they do in the reference.  Constants default to ``FACE_PIPELINE``'s.  A (K, 4) array of boxes gives (9 K, 4): the nine
    windows of box 0, then those of box 1, ... (the grid of a tracker that holds several faces)."""
    if np.ndim(box) == 2:
        return np.concatenate([tracked_boxes(b, subimage_width, subimage_height, regression_width, regression_height, net_Dx, net_Dy)
                               for b in np.asarray(box, dtype=np.float64)] or [np.zeros((0, 4))])
    p = FACE_PIPELINE
    sw = p["subimage_width"] if subimage_width is None else subimage_width
    sh = p["subimage_height"] if subimage_height is None else subimage_height
    xs, ys, pw, ph, _, _ = tracked_positions(box, sw, sh, p["regression_width"] if regression_width is None else regression_width,
                                             p["regression_height"] if regression_height is None else regression_height,
                                             p["net_Dx"] if net_Dx is None else net_Dx, p["net_Dy"] if net_Dy is None else net_Dy)
    return np.array([[x, y, x + pw - 1, y + ph - 1] for y in ys for x in xs], dtype=np.float64)
