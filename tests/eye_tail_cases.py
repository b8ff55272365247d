"""Cases of tests/test_eye_tail_host.py and tests/test_eye_tail_gpu.py: the eye tail of hg_eyes.hip past one 1024-face chunk and at its
contrast and discard edges.  Everything is small: 16 x 16 windows and eye patches on the T5L-16 network (256 inputs, 10 outputs), frames
of a few hundred pixels a side.  Shared tables and frame builders only; nothing here touches the device.

A  ``locate`` on 4097 faces cut from one noise frame, and on its prefixes at the chunk edges (``A_SIZES``).
B  a one-stage cascade that accepts every window, on a frame whose grid has ``B_WINDOWS`` windows: more than one chunk of faces reaches
   the discard, the rows and the purge.
C  the same cascade on a stack of three frames of one size and on a list of three sizes (``C_LIST``), and one stream-set step.
D  eye stages of ONE class, whose regression is their label: 9.0 and its neighbour below, on either axis and with either sign.
E  crafted frames whose eye patches are constant, two-level, all zero, one pixel off, or narrow-band noise (``contrast_frames``).
"""
import numpy as np

from pyfaceanalysis_amd import grid
from pyfaceanalysis_amd.cascade import frame_windows
from tests import eyes_restate as ER

SUB = (16, 16)                     # face windows and eye patches
K = 10                             # T5L-16 has 10 outputs
REG_SIZE = (16.0, 16.0)            # the eye stages' regression size at 16 x 16 patches
CONTRAST = (128.0, 48.0)
CONTRAST_REF = (0.11 * 255, 0.15 * 255)      # the reference's obj_avg / obj_std read as fractions of 255 (a guess)
CHUNK = 1024                       # k_eyes_glue's workgroup, k_purge's rank-sort tile, k_frame_segments' stride

# ---- A ---------------------------------------------------------------------------------------------------------------------------------
A_FRAME, A_SEED = (320, 240), 8801
A_N = 4097
A_SIZES = (1, 1023, 1024, 1025, 2049, 4097)

# ---- B, C ------------------------------------------------------------------------------------------------------------------------------
B_FRAME, B_SEED, B_SF = (320, 240), 8802, 0.08
B_WINDOWS = 2096                                   # grid.py's count for B_FRAME at B_SF (pinned by tests/test_eye_tail_host.py)
C_STACK_SEEDS = (8803, 8804, 8805)                 # three B_FRAME-sized frames; the middle one is ``sparse_frame``
C_LIST = ((320, 240), (32, 32), (200, 150))        # the small frame sits between the others
C_LIST_SEEDS = (8806, 8807, 8808)
C_LIST_WINDOWS = (2096, 18, 1009)
SMALL_ROWS = 64                                    # the small frame gives fewer rows than this
# the stream set: 16 streams x 8 held faces x 9 windows = 1152 tracked windows in one pass, 72 per stream in a tracker of its own
S_STREAMS, S_FACES, S_FRAME, S_SF = 16, 8, (97, 131), 0.2
S_SEEDS = tuple(range(8820, 8820 + S_STREAMS))
MAX_STREAM_WINDOWS = 8192

# ---- D ---------------------------------------------------------------------------------------------------------------------------------
TOLERANCE = 9.0
JUST_INSIDE = float(np.nextafter(9.0, 0.0))
D_FRAME, D_SEED, D_SF, D_WINDOWS = (64, 64), 8809, 0.2, 99
# (label of EyeLX, label of EyeLY, every face too far)
D_CASES = tuple((x, y, far) for v, far in ((TOLERANCE, True), (-TOLERANCE, True), (JUST_INSIDE, False), (-JUST_INSIDE, False))
                for x, y in ((v, 0.0), (0.0, v)))

# ---- E ---------------------------------------------------------------------------------------------------------------------------------
E_FRAME = (96, 80)
E_EYE_SIZES = ((16, 16), (64, 64), (24, 20))       # 24 x 20 = 480 pixels: not a multiple of k_eye_contrast's 256 threads
E_TARGETS = (CONTRAST, CONTRAST_REF)
F_TARGETS = E_TARGETS + ((0.0, 0.16),)             # the fixture's: also the reference's own defaults' neighbourhood (mean 0 clips half)


def noise_frame(w, h, seed):
    """Box-filtered noise, the frames of tests/frame_batch_cases.py."""
    from pyfaceanalysis_amd import synth
    rng = np.random.default_rng(seed)
    return np.rint(synth._box3(rng.integers(0, 256, (h, w), dtype=np.uint8))).astype(np.uint8)


def pipeline():
    return dict(grid.FACE_PIPELINE)


def n_windows(size, smallest_face):
    return len(frame_windows(size[0], size[1], smallest_face, pipeline(), SUB)[0])


def locate_faces(n=A_N, seed=A_SEED):
    """(boxes (n, 4), angles (n)) for A: grid windows of A_FRAME drawn with replacement and moved by a fraction of a pixel; every 9th
    pushed over the left / top border, every 31st over the right one; angles in +-22.5 with 0, +-90 and 180 interleaved — every kind
    occurs in every chunk of 1024."""
    rng = np.random.default_rng(seed)
    grid_boxes, _ = frame_windows(A_FRAME[0], A_FRAME[1], 0.1, pipeline(), SUB)
    boxes = grid_boxes[rng.integers(0, len(grid_boxes), n)].copy()
    boxes += np.tile(rng.uniform(-2.0, 2.0, (n, 2)), 2)
    side = (boxes[:, 2] - boxes[:, 0])[:, None]
    boxes[0::9] -= 0.4 * side[0::9] + np.array([30.0, 20.0, 30.0, 20.0])
    boxes[5::31] += np.array([float(A_FRAME[0]) - 40.0, 0.0, float(A_FRAME[0]) - 40.0, 0.0])
    angles = rng.uniform(-22.5, 22.5, n)
    angles[::7] = 0.0
    angles[1::23], angles[2::23], angles[3::23] = 90.0, -90.0, 180.0
    return boxes, angles


def sparse_frame(w, h, seed):
    """A black frame with one 24 x 24 island of noise: the eye patches of every window that misses the island are all zero, one constant
    patch whose regressions lie beyond the tolerance with these eye stages, so only the few windows on the island give rows (a frame of
    another constant level keeps the windows along its border too: their eye boxes reach outside, where the patch is zero)."""
    f = np.zeros((h, w), dtype=np.uint8)
    f[100:124, 150:174] = noise_frame(24, 24, seed)
    return f


# ---- E: crafted frames and faces ------------------------------------------------------------------------------------------------------
def contrast_frames():
    """name -> (80, 96) uint8 frame."""
    w, h = E_FRAME
    rng = np.random.default_rng(8810)
    out = {}
    for level in (0, 1, 128, 255):
        out["const%d" % level] = np.full((h, w), level, dtype=np.uint8)
    dots = np.zeros((h, w), dtype=np.uint8)
    dots[3::11, 5::13] = 255                                              # single pixels, none next to another
    out["black_dots"] = dots
    out["white_holes"] = (255 - dots).astype(np.uint8)
    split = np.full((h, w), 127, dtype=np.uint8)
    split[:, w // 2:] = 128
    out["split127_128"] = split
    out["noise100_110"] = rng.integers(100, 110, (h, w)).astype(np.uint8)
    out["noise250_256"] = rng.integers(250, 256, (h, w)).astype(np.uint8)
    return out


def contrast_faces():
    """(boxes, angles): faces inside E_FRAME, over each border, and wholly outside it; angle 0 and a few rotations."""
    w, h = E_FRAME
    boxes = np.array([[8.0, 6.0, 56.0, 54.0], [30.0, 20.0, 70.0, 60.0], [40.5, 10.25, 88.0, 57.75], [2.0, 30.0, 34.0, 62.0],
                      [-30.0, 10.0, 30.0, 70.0], [60.0, -25.0, 110.0, 25.0], [70.0, 50.0, 130.0, 110.0], [-20.0, -20.0, 20.0, 20.0],
                      [w + 40.0, 10.0, w + 90.0, 60.0], [10.0, -120.0, 60.0, -70.0], [-200.0, -200.0, -150.0, -150.0], [20.0, h + 60.0, 60.0, h + 100.0],
                      [10.0, 10.0, 80.0, 80.0], [44.0, 4.0, 92.0, 52.0]])
    angles = np.array([0.0, 0.0, 0.0, 11.5, 0.0, -17.0, 0.0, 22.5, 0.0, 0.0, 90.0, 0.0, 180.0, -90.0])
    return boxes, angles


def host_patches(frame, boxes, angles, eye_size, eye_boxes=None):
    """The uint8 eye patches (2n, w h) of the faces on ``frame`` by the host restatements (eye boxes: ER.all_eye_boxes unless given)."""
    from oracle import pil_restate
    eb = ER.all_eye_boxes(boxes, angles) if eye_boxes is None else eye_boxes
    return pil_restate.extract_subimages_rotate(frame, eb, -np.concatenate([angles, angles]), eye_size)


def patch_kinds(u8, target):
    """What a set of uint8 patches contains, by the restated contrast rule: counts of (std 0 patches whose output is target_mean
    everywhere, patches with a pixel clipped to 0, patches with a pixel clipped to 255, all-zero patches).  A clip is counted where the
    UNCLIPPED value lies outside [0, 255]."""
    flat, clip0, clip255, zero = 0, 0, 0, 0
    out = ER.contrast(u8, *target)
    for p, o in zip(np.asarray(u8), out):
        mean, std = ER.contrast_stats(p)
        raw = (p.astype(np.float64) - mean) / (std / target[1] + 0.00000001) + target[0]
        flat += int(std == 0.0 and bool(np.all(o == np.float32(target[0]))))
        clip0 += int((raw < 0.0).any() and (o == 0.0).any())
        clip255 += int((raw > 255.0).any() and (o == 255.0).any())
        zero += int(not p.any())
    return flat, clip0, clip255, zero


def fixture_patches(eye_size):
    """The patches the reference fixture keeps for one eye size (tests/golden/make_reference_glue.py): every fourth distinct host patch
    of the crafted frames at (16, 16) and (24, 20); at (64, 64) two of them, one of noise and one of single bright pixels."""
    frames = contrast_frames()
    boxes, angles = contrast_faces()
    if tuple(eye_size) == (64, 64):
        return np.stack([host_patches(frames["noise100_110"], boxes[:1], angles[:1], eye_size)[0],
                         host_patches(frames["black_dots"], boxes[4:5], angles[4:5], eye_size)[0]])
    every = np.unique(np.concatenate([host_patches(f, boxes, angles, eye_size) for f in frames.values()]), axis=0)
    return every[::4]                                                     # a quarter of them, in sorted order: still every kind (asserted)


# ---- G: a numpy model of k_eyes_glue's chunked compaction -----------------------------------------------------------------------------
def chunked_compaction(keep, chunk=CHUNK, fault=None):
    """row_src of the faces kept, as k_eyes_glue writes it: chunk after chunk, each chunk's kept faces placed from the running ``base``
    on.  fault "base": the base is not carried into the next chunk; fault "tail": the last partial chunk is skipped.  Returns
    (row_src, count); entries never written stay -1."""
    keep = np.asarray(keep, dtype=bool)
    n = len(keep)
    row_src = np.full(n, -1, dtype=np.int64)
    base = 0
    for i0 in range(0, n, chunk):
        if fault == "tail" and n - i0 < chunk:
            break
        idx = i0 + np.nonzero(keep[i0:i0 + chunk])[0]
        start = 0 if fault == "base" else base
        row_src[start:start + len(idx)] = idx
        base = start + len(idx) if fault == "base" else base + len(idx)
    return row_src, base


def keep_pattern(n=B_WINDOWS, seed=8811, share=0.2):
    """A keep mask of B's shape: ``share`` of n faces discarded at random, so on both sides of 1024."""
    rng = np.random.default_rng(seed)
    return rng.random(n) >= share
