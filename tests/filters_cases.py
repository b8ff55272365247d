"""Frames, boxes and angles shared by tests/test_filters_host.py and tests/test_filters_gpu.py, and PIL called the way the reference
calls it (``transform(EXTENT)`` of the frame, or of ``rotate(center = box centre)`` with the same filter)."""
import numpy as np

FILTERS = (2, 3)                                            # Image.BILINEAR, Image.BICUBIC
ANGLES = (0.5, -0.5, 17.0, 45.0, 90.0, 180.0, -135.0, 360.0)
FRAME_W, FRAME_H = 53, 37


def frame():
    return np.random.default_rng(4101).integers(0, 256, (FRAME_H, FRAME_W), dtype=np.uint8)


def checkerboard():
    """0 / 255 squares of two pixels: between two equal pixels BICUBIC's taps are (0, 255, 255, 0) or (255, 0, 0, 255), which overshoot
    255 and undershoot 0, so its clamp is reached on both sides."""
    yy, xx = np.mgrid[0:FRAME_H, 0:FRAME_W]
    return ((((xx >> 1) + (yy >> 1)) & 1) * 255).astype(np.uint8)


def boxes():
    """24 seeded boxes (x0, y0, x1, y1), corners off the pixel grid: 6 inside, 2 over each of the four edges, 2 entirely outside, 4
    magnifying (smaller than any output size used) and 4 shrinking about 8 x a (16, 12) output."""
    rng = np.random.default_rng(4102)
    W, H = FRAME_W, FRAME_H
    out = []
    for _ in range(6):
        x0, y0 = rng.uniform(0, W - 22), rng.uniform(0, H - 16)
        out.append([x0, y0, x0 + rng.uniform(14, 22), y0 + rng.uniform(10, 16)])
    for dx, dy in ((-1, 0), (1, 0), (0, -1), (0, 1)):
        for _ in range(2):
            w, h = rng.uniform(16, 30), rng.uniform(12, 24)
            cx = (W / 2 + rng.uniform(-4, 4)) if dx == 0 else (0.0 if dx < 0 else W) + rng.uniform(-3, 3)
            cy = (H / 2 + rng.uniform(-4, 4)) if dy == 0 else (0.0 if dy < 0 else H) + rng.uniform(-3, 3)
            out.append([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2])
    out.append([-40.3, -30.2, -5.1, -2.7])
    out.append([W + 3.2, H + 1.9, W + 25.5, H + 20.4])
    for _ in range(4):
        x0, y0 = rng.uniform(-1, W - 6), rng.uniform(-1, H - 5)
        out.append([x0, y0, x0 + rng.uniform(3, 7), y0 + rng.uniform(2.5, 6)])
    for _ in range(4):
        cx, cy = rng.uniform(10, W - 10), rng.uniform(8, H - 8)
        w, h = 128 * rng.uniform(0.9, 1.1), 96 * rng.uniform(0.9, 1.1)
        out.append([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2])
    b = np.array(out)
    assert b.shape == (24, 4)
    return b


def corner_boxes():
    """Boxes near the frame's corners with non-integer centres: a rotation about them reads outside the source, so its zero fill
    enters the taps of the cut."""
    W, H = FRAME_W, FRAME_H
    return np.array([[-3.3, -2.1, 14.9, 11.6], [W - 15.2, -4.4, W + 2.7, 9.3], [-2.6, H - 12.7, 13.1, H + 3.2], [W - 17.3, H - 11.2, W + 1.4, H + 2.9],
                     [18.2, 9.7, 37.5, 26.4]])


def pil_window(img, box, delta_ang, size, filt):
    from PIL import Image
    im = Image.fromarray(img, "L")
    b = tuple(float(v) for v in box)
    if float(delta_ang) % 360.0 != 0.0:
        im = im.rotate(float(delta_ang), filt, center=((b[0] + b[2]) / 2.0, (b[1] + b[3]) / 2.0))
    return np.asarray(im.transform(size, Image.EXTENT, b, filt)).reshape(-1)


def pil_windows(img, boxes, delta_angs, size, filt):
    return np.stack([pil_window(img, b, a, size, filt) for b, a in zip(boxes, delta_angs)])
