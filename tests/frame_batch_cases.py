"""Cases of tests/test_frame_batch_gpu.py: the stack of frames the patcher test cuts from, its windows, and the seeds of the cascade tests.

The patcher case: three 97x131 frames as views out of ONE larger buffer filled with 255 — a margin in front, ``LD`` = 144 bytes between
rows, ``FRAME_STRIDE`` bytes between frames (NOT a multiple of LD), a margin behind.  Frame pixels are box-filtered noise, far from
255: a read across a frame's border shows up as a wrong byte, not as a fault.
"""
import numpy as np

W, H = 97, 131
LD = 144
FRAME_STRIDE = H * LD + 77                 # 18941 = 131 * 144 + 77; >= (H - 1) * LD + W = 18817
MARGIN = 4 * LD + 13
N_FRAMES = 3
FRAME_SEEDS = (9101, 9102, 9103)
N_ROWS = 60
BAD_ROWS = {7: -1, 23: N_FRAMES, 41: -1, 42: N_FRAMES + 5}      # row -> a frame index outside the stack; their neighbours are ordinary rows
ANGLES = (0.0, 90.0, -90.0, 180.0, 22.5, -22.5, 0.0, 11.0)
OUT_SIZES = ((64, 64), (24, 24), (6, 5))   # (64, 64): the 16-pixel paths; (24, 24): four pixels per thread; (6, 5): scalar
FILTERS = (0, 2, 3)


def noise_frame(w, h, seed):
    from pyfaceanalysis_amd import synth
    rng = np.random.default_rng(seed)
    return np.rint(synth._box3(rng.integers(0, 256, (h, w), dtype=np.uint8))).astype(np.uint8)


def stack_buffer():
    """(buffer, offsets): the 1-d uint8 buffer and the byte offset of every frame's first pixel."""
    assert FRAME_STRIDE % LD != 0 and FRAME_STRIDE >= (H - 1) * LD + W
    buf = np.full(MARGIN + N_FRAMES * FRAME_STRIDE + MARGIN, 255, dtype=np.uint8)
    offsets = [MARGIN + f * FRAME_STRIDE for f in range(N_FRAMES)]
    for f, off in enumerate(offsets):
        view = np.lib.stride_tricks.as_strided(buf[off:], shape=(H, W), strides=(LD, 1))
        view[...] = noise_frame(W, H, FRAME_SEEDS[f])
    return buf, offsets


def windows():
    """(boxes (N_ROWS, 4), angles (N_ROWS,), row_frame (N_ROWS,) int32): windows inside the frame, overhanging on every side and wholly
    outside it, the angles cycling through ANGLES, the frame indices interleaved at random with BAD_ROWS set."""
    rng = np.random.default_rng(4242)
    boxes = np.zeros((N_ROWS, 4))
    for i in range(N_ROWS):
        side = rng.uniform(20.0, 80.0)
        kind = i % 6
        if kind in (0, 1):
            x0, y0 = rng.uniform(0.0, W - side), rng.uniform(0.0, H - side)      # inside
        elif kind == 2:
            x0, y0 = -side / 3.0, rng.uniform(0.0, H - side)                     # over the left edge
        elif kind == 3:
            x0, y0 = W - side / 2.0, H - side / 2.0                              # over the right and the bottom edge
        elif kind == 4:
            x0, y0 = rng.uniform(0.0, W - side), -side / 2.0                     # over the top edge
        else:
            x0, y0 = (W + 5.0, 10.0) if i % 12 == 5 else (10.0, -side - 3.0)     # wholly outside
        boxes[i] = (x0, y0, x0 + side, y0 + side)
    angles = np.array([ANGLES[i % len(ANGLES)] for i in range(N_ROWS)])
    row_frame = rng.integers(0, N_FRAMES, N_ROWS).astype(np.int32)
    for i, f in BAD_ROWS.items():
        row_frame[i] = f
    return boxes, angles, row_frame


# ---- the cascade tests: seeds of noise frames (tests/test_frame_stream_gpu.py's frames), chosen on an MI355X for what each test asserts
SMALL = (97, 131)          # 397 windows, no prescale
MEDIUM = (320, 240)        # 1308 windows, no prescale
LONG = (2000, 300)         # prescaled to 1000 x 150: 5148 windows; two of them are above 2 * kChunk = 8192 candidates
HD = (1280, 720)           # prescaled to 1000 x 562: 1738 windows

# The synthetic cascade's calibration (tests/test_frame_stream_gpu.py's Rig(keep, later_keep)).  The stream test's 0.3 / 0.7 leaves NO
# survivor on any 97x131 noise frame (180 seeds tried) and no purge drop at 320x240; with 0.8 / 0.9, on an MI355X, as
# seed: cascade survivors / faces before the purge / faces kept:
KEEP, LATER_KEEP = 0.8, 0.9
SMALL_SEEDS = (9209, 9200, 9202)       # 97x131:  4/0/0, 0/0/0, 1/1/1 — a frame without a survivor between two that have some
MEDIUM_SEEDS = (9210, 9200, 9211)      # 320x240: 38/26/25, 34/23/23, 40/32/31 — the purge drops a row of the first and of the third
LONG_SEEDS = (9200, 9201)              # 2000x300: 355/304/271, 319/277/254
HD_SEEDS = (9300, 9302)                # 1280x720 (hd_frame) as RGB (n, n, 255 - n) behind the BILINEAR prescale: 3/1/1, 2/2/2; its "L" behind NEAREST: 14/11/11, 12/12/12


def hd_frame(seed):
    """A 1280x720 frame that keeps survivors behind an antialiased prescale: a 640x360 noise frame with every pixel doubled (plain
    1280x720 noise, smoothed by the BILINEAR resize, leaves the calibrated cascade with none)."""
    n = noise_frame(HD[0] // 2, HD[1] // 2, seed)
    return np.ascontiguousarray(n[(np.arange(HD[1]) // 2)[:, None], (np.arange(HD[0]) // 2)[None, :]])
