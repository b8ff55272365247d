"""Cases of tests/test_estimate_frames_host.py and tests/test_estimate_frames_gpu.py: pose normalisation and age / race / gender
estimation for faces spread over a STACK of same-size frames (``FaceNormalizer.normalize_frames``, ``FaceAnalyzer.estimate_frames`` /
``estimate_faces_frames``, ``DeviceCascade.prescale_frames``).  The oracle is always the per-frame public call on that face's own frame,
compared with ``==`` on bytes and bits; nothing here computes an expected value.

The normalise stack is the patcher stack of tests/frame_batch_cases.py: three 97 x 131 frames as views out of ONE buffer of 255s, ``LD`` =
144 bytes between rows, ``FRAME_STRIDE`` = 131 * 144 + 77 bytes between frames (no multiple of LD), margins in front and behind.  The eye
sets are those of tests/normalize_cases.py for that frame size.  The estimate stack is four 200 x 150 noise frames with 0, 1, 3 and 5
faces (tests/analysis_cases.py::frame_eyes), the analyzers the small ones of that module.
"""
import numpy as np

from tests import analysis_cases as AC
from tests import frame_batch_cases as BC
from tests import normalize_cases as NC

FRAME = (BC.W, BC.H)                       # (width, height) of the normalise stack's frames
N_FRAMES = BC.N_FRAMES
# (out_size, method, rotate): the two small outputs rotated and not, and one 256 x 192
NORMALIZE_CASES = [(size, method, rotate) for size, method in NC.SMALL_OUT_SIZES for rotate in (True, False)] + [((256, 192), NC.AREA, True),
                                                                                                                     ((256, 192), NC.AREA, False)]
# refused faces (normalize.STATUS 1 and 2) and frame indices outside a stack of B frames, as offsets from B (BC.BAD_ROWS' -1, B, B + 5)
REFUSED = [((5.0, 5.0, 4.0, 5.0), 1), ((np.nan, 1.0, 2.0, 3.0), 2)]
BAD_FRAMES = (-1, 0, 5)                    # -1, B + 0, B + 5
STATUS_FRAME_RANGE = 5


def host_frames():
    return [BC.noise_frame(BC.W, BC.H, s) for s in BC.FRAME_SEEDS]


def device_stack(torch):
    """(buffer, stack): BC.stack_buffer() on the device and the (3, 131, 97) view of its frames, strides (FRAME_STRIDE, LD, 1)."""
    buf_h, offsets = BC.stack_buffer()
    buf = torch.from_numpy(buf_h).cuda()
    stack = torch.as_strided(buf, (BC.N_FRAMES, BC.H, BC.W), (BC.FRAME_STRIDE, BC.LD, 1), offsets[0])
    return buf, stack


def spread_faces(n_frames=N_FRAMES, frame_size=FRAME, n_random=10, seed=0, only=None):
    """(eyes (n, 4), face_frame (n,) int32): the nine eye sets of NC.eye_sets and ``n_random`` seeded ones on every frame of ``only``
    (default: all), in an order NOT sorted by frame."""
    rng = np.random.default_rng(4300 + seed)
    eyes, ff = [], []
    for f in (range(n_frames) if only is None else only):
        e = [v for _, v in NC.eye_sets(*frame_size)] + [tuple(r) for r in NC.random_eyes(n_random + 4, frame_size, seed=seed + 10 * f)[:n_random]]
        eyes += e
        ff += [f] * len(e)
    order = rng.permutation(len(eyes))
    eyes, ff = np.array(eyes, dtype=np.float64)[order], np.array(ff, dtype=np.int32)[order]
    assert (np.diff(ff) < 0).any(), "the faces are not sorted by frame"
    return eyes, ff


def with_bad_rows(eyes, ff, n_frames):
    """Refused faces and faces with frame indices outside the stack put between good ones.  Returns (eyes, face_frame, status expected
    at the inserted places {row: status}); every inserted row has good rows on both sides."""
    eyes, ff = [tuple(e) for e in eyes], list(ff)
    want = {}
    at = 2
    for e, code in REFUSED:
        eyes.insert(at, e)
        ff.insert(at, 0)
        want[at] = code
        at += 3
    for off in BAD_FRAMES:
        eyes.insert(at, eyes[at - 1])           # a good face's eyes: only its frame index is wrong
        ff.insert(at, off if off < 0 else n_frames + off)
        want[at] = STATUS_FRAME_RANGE
        at += 3
    assert at < len(eyes) and all(r - 1 not in want and r + 1 not in want for r in want)
    return np.array(eyes, dtype=np.float64), np.array(ff, dtype=np.int32), want


# ---- estimation ----------------------------------------------------------------------------------------------------------------------
EST_FRAME = (200, 150)
EST_SEEDS = (0, 1, 2, 3)
EST_FACES = (0, 1, 3, 5)                   # faces on frame 0 .. 3
PATCH = (13, 11)
PATCH_BOX = AC.PATCH_CASES[1][3]           # inside the 40 x 44 crop
PATCH_BOX_OVER = AC.PATCH_CASES[2][3]      # hanging over its left and top edges


def est_frames():
    return [NC.noise_frame(EST_FRAME[0], EST_FRAME[1], seed=s) for s in EST_SEEDS]


def est_faces():
    """(eyes (9, 4), face_frame (9,)): 0, 1, 3 and 5 of AC.frame_eyes' pairs on frames 0 .. 3, interleaved (not sorted by frame)."""
    fe = AC.frame_eyes(*EST_FRAME)
    rows = [(fe[0], 1)] + [(fe[i], 2) for i in (1, 4, 5)] + [(fe[i], 3) for i in (0, 2, 3, 4, 5)]
    order = [4, 0, 8, 1, 5, 2, 6, 3, 7]
    eyes = np.array([rows[i][0] for i in order], dtype=np.float64)
    ff = np.array([rows[i][1] for i in order], dtype=np.int32)
    assert [int((ff == f).sum()) for f in range(4)] == list(EST_FACES)
    return eyes, ff
