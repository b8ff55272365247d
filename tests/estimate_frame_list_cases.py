"""Cases of tests/test_estimate_frame_list_host.py and tests/test_estimate_frame_list_gpu.py: pose normalisation and age / race / gender
estimation for faces spread over a LIST of frames of different sizes (``FaceNormalizer.normalize_frame_list``,
``FaceAnalyzer.estimate_frame_list`` / ``estimate_faces_frame_list``, ``DeviceCascade.prescale_frame_list``).  The oracle is always the
per-frame public call on that face's own frame, compared with ``==`` on bytes and bits; nothing here computes an expected value.

The normalise list is the patcher list of tests/frame_list_cases.py: three frames of different sizes and row strides (7 x 5 with ld 9,
97 x 131 with ld 144, 40 x 61 with ld 40) as views out of ONE buffer of 255s with margins, the small one first.  A kernel that took another
frame's width, height, stride or pointer gives other bytes, not a fault: everything it can read is inside the buffer.  The eye sets are
those of tests/normalize_cases.py, made for each face's OWN frame size.  The estimate list is three noise frames of 200 x 150, 97 x 131
and 160 x 120 with the eye pairs of tests/analysis_cases.py::frame_eyes, the analyzers the small ones of that module.
"""
import numpy as np

from tests import analysis_cases as AC
from tests import estimate_frames_cases as EC
from tests import frame_batch_cases as BC
from tests import frame_list_cases as LC
from tests import normalize_cases as NC

SIZES = [(w, h) for w, h, _ld, _seed in LC.PATCH_FRAMES]      # (width, height) of the normalise list's frames
N_FRAMES = len(SIZES)
NORMALIZE_CASES = EC.NORMALIZE_CASES
REFUSED, BAD_FRAMES, STATUS_FRAME_RANGE = EC.REFUSED, EC.BAD_FRAMES, EC.STATUS_FRAME_RANGE
with_bad_rows = EC.with_bad_rows


def host_frames():
    return [BC.noise_frame(w, h, seed) for w, h, _ld, seed in LC.PATCH_FRAMES]


def frame_views(torch, buf, offsets):
    return [torch.as_strided(buf, (h, w), (ld, 1), off) for (w, h, ld, _seed), off in zip(LC.PATCH_FRAMES, offsets)]


def device_list(torch):
    """(buffer, frames, inside): LC.patch_buffer() on the device, the three views of its frames, and the host mask of the bytes that
    belong to a frame (all others are 255 and must stay so)."""
    buf_h, offsets = LC.patch_buffer()
    inside = np.zeros(len(buf_h), dtype=bool)
    for (w, h, ld, _seed), off in zip(LC.PATCH_FRAMES, offsets):
        np.lib.stride_tricks.as_strided(inside[off:], shape=(h, w), strides=(ld, 1))[...] = True
    buf = torch.from_numpy(buf_h).cuda()
    return buf, frame_views(torch, buf, offsets), inside


def border_eyes(w, h):
    """Faces at the four borders of a w x h frame: their crops hang over its left / top, right / bottom, bottom / left and top / right."""
    return [(1.0, 2.5, 14.0, 4.0), (w - 21.0, h - 6.0, w - 2.0, h - 9.5), (-3.0, h - 2.0, 9.0, h + 1.0), (w - 9.0, -1.0, w + 4.0, 1.5)]


def big_eyes(w, h):
    """Two faces seven times the frame's longer side wide, centred near two of its corners: their crops are nearly twice the frame per
    axis and the cut shrinks them more than 4 x per axis — tap by tap at the small output sizes on the two larger frames."""
    d = 7.0 * max(w, h)
    return [(3.0 - d / 2, 4.0, 3.0 + d / 2, 9.0), (w - 3.0 - d / 2, h - 2.0, w - 3.0 + d / 2, h - 6.0)]


N_NAMED = 15                               # faces per frame before the random ones


def spread_faces(sizes=SIZES, n_random=10, seed=0, only=None):
    """(eyes (n, 4), face_frame (n,) int32): the nine eye sets of NC.eye_sets, the four border faces, the two big ones and ``n_random``
    seeded ones for every frame of ``only`` (default: all), each made for ITS frame's size, in an order NOT sorted by frame."""
    rng = np.random.default_rng(4400 + seed)
    eyes, ff = [], []
    for f in (range(len(sizes)) if only is None else only):
        w, h = sizes[f]
        e = [v for _, v in NC.eye_sets(w, h)] + border_eyes(w, h) + big_eyes(w, h) + [tuple(r) for r in NC.random_eyes(n_random + 4, (w, h), seed=seed + 10 * f)[:n_random]]
        eyes += e
        ff += [f] * len(e)
    order = rng.permutation(len(eyes))
    eyes, ff = np.array(eyes, dtype=np.float64)[order], np.array(ff, dtype=np.int32)[order]
    assert len(set(ff)) < 2 or (np.diff(ff) < 0).any(), "the faces are not sorted by frame"
    return eyes, ff


def modes(geoms, out_size):
    """(staged, taps) masks of the faces by the rule of hg::normalize_stage_limit, from the geoms alone."""
    np_ = geoms["rect"][:, 2].astype(np.int64) * geoms["rect"][:, 3]
    limit = 16 * out_size[0] * out_size[1]
    return (np_ > 0) & (np_ <= limit), np_ > limit


def overhang(geoms, ff, sizes=SIZES):
    """Per frame, which edges (left, top, right, bottom) the rectangle some UNROTATED face's cut reads hangs over, in the coordinates of
    that face's own frame (crop origin + rect)."""
    out = {}
    for f, (w, h) in enumerate(sizes):
        g = geoms[(ff == f) & (geoms["status"] == 0) & (geoms["rect"][:, 2] > 0)]
        x0, y0 = g["crop_x0"] + g["rect"][:, 0], g["crop_y0"] + g["rect"][:, 1]
        x1, y1 = x0 + g["rect"][:, 2], y0 + g["rect"][:, 3]
        out[f] = (bool((x0 < 0).any()), bool((y0 < 0).any()), bool((x1 > w).any()), bool((y1 > h).any()))
    return out


# ---- estimation ----------------------------------------------------------------------------------------------------------------------
EST_SIZES = [(200, 150), (97, 131), (160, 120)]
EST_SEEDS = (0, 1, 2)
EST_FACES = (3, 2, 4)                      # faces on frame 0 .. 2
PATCH, PATCH_BOX, PATCH_BOX_OVER = EC.PATCH, EC.PATCH_BOX, EC.PATCH_BOX_OVER


def est_frames():
    return [NC.noise_frame(w, h, seed=s) for (w, h), s in zip(EST_SIZES, EST_SEEDS)]


def est_faces():
    """(eyes (9, 4), face_frame (9,)): 3, 2 and 4 of AC.frame_eyes' pairs for each frame's own size, interleaved (not sorted by frame);
    every frame has one of the two border pairs."""
    fe = [AC.frame_eyes(w, h) for w, h in EST_SIZES]
    rows = [(fe[0][i], 0) for i in (0, 2, 4)] + [(fe[1][i], 1) for i in (1, 5)] + [(fe[2][i], 2) for i in (0, 3, 4, 5)]
    order = [5, 0, 8, 3, 1, 6, 4, 2, 7]
    eyes = np.array([rows[i][0] for i in order], dtype=np.float64)
    ff = np.array([rows[i][1] for i in order], dtype=np.int32)
    assert [int((ff == f).sum()) for f in range(3)] == list(EST_FACES) and (np.diff(ff) < 0).any()
    return eyes, ff
