"""Cases of tests/test_frame_list_gpu.py and tests/test_frame_list_host.py: lists of frames of DIFFERENT sizes through one pooled pass.

The patcher case: three grey frames of different sizes and row strides cut as views out of ONE buffer of 255s, ordered small -> large ->
small; the windows of a row are scaled to that row's OWN frame (inside it, overhanging each side, wholly outside), so a kernel that took
another frame's width, height or row stride gives other bytes — not a fault: everything it could read is inside the buffer.

The cascade cases reuse tests/frame_batch_cases.py (sizes, seeds and the per-(size, seed) survivors recorded there on an MI355X: the
per-frame results do not depend on the batch, so those premises carry over).
"""
import numpy as np

from tests import frame_batch_cases as BC

# ---- the patcher case ------------------------------------------------------------------------------------------------------------------
# (w, h, ld, seed): 7x5 with ld 9 is narrower than an 8-byte and a 16-byte load
PATCH_FRAMES = ((7, 5, 9, 9111), (97, 131, 144, 9112), (40, 61, 40, 9113))
PATCH_MARGIN = 4 * 144 + 13
PATCH_GAP = 77                              # bytes of 255 between two frames
N_ROWS = 60
BAD_ROWS = {7: -1, 23: len(PATCH_FRAMES), 41: -1, 42: len(PATCH_FRAMES) + 5}


def patch_buffer():
    """(buffer, offsets): the 1-d uint8 buffer of 255s and the byte offset of every frame's first pixel."""
    offsets, at = [], PATCH_MARGIN
    for (w, h, ld, _seed) in PATCH_FRAMES:
        offsets.append(at)
        at += (h - 1) * ld + w + PATCH_GAP
    buf = np.full(at + PATCH_MARGIN, 255, dtype=np.uint8)
    for (w, h, ld, seed), off in zip(PATCH_FRAMES, offsets):
        np.lib.stride_tricks.as_strided(buf[off:], shape=(h, w), strides=(ld, 1))[...] = BC.noise_frame(w, h, seed)
    return buf, offsets


def patch_windows():
    """(boxes (N_ROWS, 4), angles (N_ROWS,), row_frame (N_ROWS,) int32): BC.windows' kinds of window, each scaled to its row's own frame."""
    rng = np.random.default_rng(4343)
    row_frame = (np.arange(N_ROWS) % len(PATCH_FRAMES)).astype(np.int32)      # interleaved: 0 1 2 0 1 2 ...
    rng.shuffle(row_frame[30:])
    boxes = np.zeros((N_ROWS, 4))
    for i in range(N_ROWS):
        w, h = PATCH_FRAMES[row_frame[i]][:2]
        side = rng.uniform(0.25, 0.8) * min(w, h)
        kind = (i // len(PATCH_FRAMES)) % 6          # every frame meets every kind
        if kind in (0, 1):
            x0, y0 = rng.uniform(0.0, w - side), rng.uniform(0.0, h - side)      # inside
        elif kind == 2:
            x0, y0 = -side / 3.0, rng.uniform(0.0, h - side)                     # over the left edge
        elif kind == 3:
            x0, y0 = w - side / 2.0, h - side / 2.0                              # over the right and the bottom edge
        elif kind == 4:
            x0, y0 = rng.uniform(0.0, w - side), -side / 2.0                     # over the top edge
        else:
            x0, y0 = (w + 5.0, 1.0) if i % 2 else (1.0, -side - 3.0)             # wholly outside
        boxes[i] = (x0, y0, x0 + side, y0 + side)
    angles = np.array([BC.ANGLES[i % len(BC.ANGLES)] for i in range(N_ROWS)])
    for i, f in BAD_ROWS.items():
        row_frame[i] = f
    return boxes, angles, row_frame


# ---- the cascade cases -------------------------------------------------------------------------------------------------------------------
S, M, LONG = BC.SMALL, BC.MEDIUM, BC.LONG
# test 2: a frame with survivors, one with none (between two that have some), one with one; the purge drops a row of MEDIUM 9210
MIXED = ((S, 9209), (M, 9210), (S, 9200), (M, 9200), (S, 9202))
# test 4: 5148 + 3 * 1308 + 397 = 9469 candidates, above 2 * kChunk = 8192; the frame boundaries (5148, 6456, 7764, 9072) miss the 8192 edge
CHUNKED = ((LONG, 9200), (M, 9210), (M, 9200), (M, 9211), (S, 9209))
CHUNKED_TOTAL = 9469
# test 5a: 1280x720 and 1920x1080 share the grid of 1000x562 (1738 windows) behind the prescale; 320x240 and 640x480 have 1308 windows each
# and different grids (tests/test_grid_patches.py::test_frame_stream_premises)
SHARED_GRID = ((1280, 720), (1920, 1080))
EQUAL_COUNT = ((320, 240), (640, 480))
TABLES = (((1280, 720), 9300), ((320, 240), 9210), ((1920, 1080), 9301), ((640, 480), 9302))      # survivors on an MI355X: 644, 38, 1271, 208
# test 5b: six small sizes, six distinct grids — more than the four slots of the patcher's keyed ring.  Seeds: for each size the first of the
# 32 seeds from 9400 on whose per-frame call keeps a survivor, with BC.KEEP / BC.LATER_KEEP, on an MI355X;
# None: none of the 32.  size: seed, (cascade survivors, faces before the purge, faces kept)
MANY_GRIDS = {
    (97, 131): (9406, (1, 1, 1)),       # 397 windows
    (131, 97): (9414, (6, 1, 1)),       # 379
    (120, 120): (9400, (2, 1, 1)),      # 462
    (160, 100): (9400, (4, 1, 1)),      # 509
    (100, 160): (9400, (5, 1, 1)),      # 540
    (140, 140): (9400, (5, 1, 1)),      # 640
}
MANY_FALLBACK_SEED = 9400                   # the frame of a size without such a seed (it then has no survivor: the list still holds its grid)


def many_grids_list():
    return tuple((size, seed if seed is not None else MANY_FALLBACK_SEED) for size, (seed, _counts) in MANY_GRIDS.items())
