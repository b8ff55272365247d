"""Shared by tests/test_normalize_host.py and tests/test_normalize_gpu.py: the frames, eye sets and output sizes of the pose
normalisation tests, the reference's geometry transcribed to Python 3 (``geometry_restate``; face_normalization_tools.py:23-47 and
:151-313 for the one configuration both reference callers use, with ``math.atan2`` / ``cos`` / ``sin`` / ``sqrt``), and the oracle for the
pixels: PIL itself, composed as the reference composes it (``pil_normalize``)."""
import math

import numpy as np

AREA, AREAZ = 0, 1
# (out_size, method): the reference's two callers, then two small ones that are no multiple of any tile
OUT_SIZES = [((256, 260), AREAZ), ((256, 192), AREA), ((32, 24), AREA), ((17, 13), AREAZ)]
SMALL_OUT_SIZES = OUT_SIZES[2:]
FRAME_SIZES = [(97, 61), (160, 120), (64, 64)]      # (width, height)
GEOM_FIELDS = ("crop_x0", "crop_y0", "W", "H", "angle", "shift", "m", "box", "rotated", "status", "rect")


def noise_frame(w, h, seed=0):
    return np.random.default_rng(1000 + 7 * w + h + seed).integers(0, 256, (h, w), dtype=np.uint8)


def wide_eyes(w, h, dist):
    """Eyes ``dist`` pixels apart above a w x h frame, so that the face's centre is the frame's: the box of a small output is several
    times the output (tap by tap where the crop is large enough to hold it), that of a large one is clipped by the crop's edge."""
    cx, y = w / 2.0 + 0.3, h / 2.0 - (42.0 / 37.0) * dist / 2
    return (cx - dist / 2, y + 1.5, cx + dist / 2, y - 2.5)


# eyes 300 pixels apart are scale 8: the (17, 13) areaZ box steps 4 pixels per output pixel, its taps tile 68 x 52 = 16 * 17 * 13 pixels of
# rot exactly — the largest rectangle that is still staged
AT_THE_BOUND = ("160x120-at-the-bound-17x13", (160, 120), wide_eyes(160, 120, 300.0), (17, 13), AREAZ)


def eye_sets(w, h):
    """Nine eye sets (lx, ly, rx, ry) for a w x h frame, by name."""
    cx, cy, d = w / 2.0 + 0.3, h / 2.0 - 4.6, w / 5.0

    def tilted(deg):
        c, s = math.cos(math.radians(deg)), math.sin(math.radians(deg))
        return (cx - d / 2 * c, cy - d / 2 * s, cx + d / 2 * c, cy + d / 2 * s)
    return [
        ("level", (cx - d / 2, cy, cx + d / 2, cy)),
        ("tilt+18", tilted(18.0)),
        ("tilt-43", tilted(-43.0)),
        ("one-pixel", (cx, cy + 0.25, cx + 1.0, cy + 0.25)),                 # strong upsampling
        ("corners-down", (0.0, 0.0, w - 1.0, h - 1.0)),                      # eyes at both frame corners
        ("corners-up", (0.0, h - 1.0, w - 1.0, 0.0)),
        ("vertical+90", (cx + 3.2, cy - 6.0, cx + 3.2, cy + 6.0)),
        ("vertical-90", (cx + 3.2, cy + 6.0, cx + 3.2, cy - 6.0)),
        ("wider", wide_eyes(w, h, 330.0)),                                   # a face wider than the frame
    ]


# a 65 x 65 frame whose crop is square (65 x 65, centre pixel (32, 32)) with the eye line at exactly +90 / -90 degrees: Image.rotate's
# transpose shortcut
SQUARE_FRAME = (65, 65)
SQUARE_EYES = [("square+90", (37.7, 27.0, 37.7, 37.0)), ("square-90", (26.3, 37.0, 26.3, 27.0))]
# two faces on a 1000 x 562 frame: the box is 0.4 x and 8 x the output (pose preset: ori_w = 256 * dist / 37.5)
LARGE_FRAME = (1000, 562)
LARGE_EYES = [("large-0.4x", (400.0, 300.5, 415.0, 301.5)), ("large-8x", (360.0, 250.0, 660.0, 262.0))]


def small_cases():
    """(name, frame size, eyes, out size, method) on the three small frames and the square one: every eye set x every output size."""
    out = []
    for fs in FRAME_SIZES:
        for name, e in eye_sets(*fs):
            for size, method in OUT_SIZES:
                out.append(("%dx%d-%s-%dx%d" % (fs[0], fs[1], name, size[0], size[1]), fs, e, size, method))
    for name, e in SQUARE_EYES:
        for size, method in OUT_SIZES[1:3]:
            out.append(("%s-%dx%d" % (name, size[0], size[1]), SQUARE_FRAME, e, size, method))
    return out + [AT_THE_BOUND]


def large_cases():
    return [("%s-%dx%d" % (name, size[0], size[1]), LARGE_FRAME, e, size, method) for name, e in LARGE_EYES for size, method in OUT_SIZES[:2]]


def gpu_cases():
    """The device tests' cases: frames 97 x 61, 160 x 120 and 65 x 65, output sizes (32, 24) and (17, 13), one (256, 260) per eye set on the
    160 x 120 frame."""
    out = []
    for fs in FRAME_SIZES[:2]:
        for name, e in eye_sets(*fs):
            for size, method in SMALL_OUT_SIZES:
                out.append(("%dx%d-%s-%dx%d" % (fs[0], fs[1], name, size[0], size[1]), fs, e, size, method))
    for name, e in eye_sets(160, 120)[1:2]:
        out.append(("160x120-%s-256x260" % name, (160, 120), e, (256, 260), AREAZ))
    for name, e in SQUARE_EYES + eye_sets(*SQUARE_FRAME)[:3] + eye_sets(*SQUARE_FRAME)[8:]:
        for size, method in SMALL_OUT_SIZES:
            out.append(("65x65-%s-%dx%d" % (name, size[0], size[1]), SQUARE_FRAME, e, size, method))
    return out + [AT_THE_BOUND]


def random_eyes(n, frame_size, seed=5):
    """Seeded eye pairs with lx <= rx, inside and around the frame, every eye distance from below a pixel to several frames."""
    rng = np.random.default_rng(seed)
    w, h = frame_size
    c = rng.uniform([-0.5 * w, -0.5 * h], [1.5 * w, 1.5 * h], (n, 2))
    dist = np.exp(rng.uniform(math.log(0.3), math.log(4.0 * w), n))
    ang = rng.uniform(-90.0, 90.0, n)
    ang[::11] = 0.0
    dx, dy = dist / 2 * np.cos(np.radians(ang)), dist / 2 * np.sin(np.radians(ang))
    e = np.stack([c[:, 0] - dx, c[:, 1] - dy, c[:, 0] + dx, c[:, 1] + dy], axis=1)
    e[::5] = np.rint(e[::5])                    # integer eye coordinates: centres on exact halves
    swap = e[:, 0] > e[:, 2]
    e[swap] = e[swap][:, [2, 3, 0, 1]]
    return e[~((e[:, 0] == e[:, 2]) & (e[:, 1] == e[:, 3]))]


def _axis_range(lo, hi, n, lim):
    """The columns of a lim-wide image the BICUBIC EXTENT cut (lo, hi) -> n pixels reads: x - 1 .. x + 2 of every output pixel that is inside."""
    a = (hi - lo) / n
    first, last = None, None
    for i in range(n):
        xs = a * (i + 0.5) + lo
        if not (0 <= xs < lim):
            continue
        x = math.floor(xs - 0.5)
        t0, t1 = min(max(x - 1, 0), lim - 1), min(max(x + 2, 0), lim - 1)
        first = t0 if first is None else min(first, t0)
        last = t1 if last is None else max(last, t1)
    return (0, 0) if first is None else (first, last - first + 1)


def geometry_restate(eye, frame_size, out_size, method, rotate=True):
    """normalize_image's geometry for one face, the reference's lines in its order (face_normalization_tools.py line numbers on the
    right), Python floats.  A dict with GEOM_FIELDS; a refused face has only its status set (everything else 0)."""
    LeftEyeCenter_x, LeftEyeCenter_y, RightEyeCenter_x, RightEyeCenter_y = (float(v) for v in eye)
    im_size = (int(frame_size[0]), int(frame_size[1]))
    zero = dict(crop_x0=0, crop_y0=0, W=0, H=0, angle=0.0, shift=[0.0, 0.0], m=[0.0] * 6, box=[0.0] * 4, rotated=0, rect=[0, 0, 0, 0])
    if not all(math.isfinite(v) for v in (LeftEyeCenter_x, LeftEyeCenter_y, RightEyeCenter_x, RightEyeCenter_y)):
        return dict(zero, status=2)
    if LeftEyeCenter_x > RightEyeCenter_x:                                                                                   # :166-168
        return dict(zero, status=1)
    eyes_x_m = (RightEyeCenter_x + LeftEyeCenter_x) / 2.0                                                                    # :151
    eyes_y_m = (RightEyeCenter_y + LeftEyeCenter_y) / 2.0                                                                    # :152
    ddx, ddy = LeftEyeCenter_x - RightEyeCenter_x, LeftEyeCenter_y - RightEyeCenter_y
    dist_eyes = math.sqrt(ddx * ddx + ddy * ddy)                                                                             # :157
    if not math.isfinite(dist_eyes):
        return dict(zero, status=2)
    if dist_eyes == 0:
        return dict(zero, status=3)
    eye_line_angle = math.atan2(RightEyeCenter_y - LeftEyeCenter_y, RightEyeCenter_x - LeftEyeCenter_x) * 180 / math.pi    # :164
    desired_area = 37.0 * 42.0 / 2.0 * (37.5 / 37.0) ** 2                                                                    # :173
    eye_dx = RightEyeCenter_x - LeftEyeCenter_x                                                                              # :37
    eye_dy = RightEyeCenter_y - LeftEyeCenter_y                                                                              # :38
    inferred_mouth_x = eyes_x_m - (42.0 / 37.0) * eye_dy                                                                     # :44
    inferred_mouth_y = eyes_y_m + (42.0 / 37.0) * eye_dx                                                                     # :45
    hx, hy = eyes_x_m - inferred_mouth_x, eyes_y_m - inferred_mouth_y
    height_triangle_with_inferred_mouth = math.sqrt(hx * hx + hy * hy)                                                       # :179-180
    current_area_with_inferred_mouth = dist_eyes * height_triangle_with_inferred_mouth / 2.0                                 # :181
    midpoint_eyes_inferred_mouth_x = (eyes_x_m + inferred_mouth_x) / 2.0                                                     # :182
    midpoint_eyes_inferred_mouth_y = (eyes_y_m + inferred_mouth_y) / 2.0                                                     # :183
    scale_factor = math.sqrt(current_area_with_inferred_mouth / desired_area)                                                # :193 / :197
    if method == AREA:
        ori_width = out_size[0] * scale_factor                                                                               # :194-195
        ori_height = out_size[1] * scale_factor
    else:
        ori_width = out_size[0] * scale_factor / 2                                                                           # :198-199
        ori_height = out_size[1] * scale_factor / 2
    rotation_center_x = midpoint_eyes_inferred_mouth_x                                                                       # :215-216
    rotation_center_y = midpoint_eyes_inferred_mouth_y
    if abs(rotation_center_x) > 2.0 ** 20 or abs(rotation_center_y) > 2.0 ** 20:
        return dict(zero, status=4)
    rotation_angle = eye_line_angle if rotate else 0.0                                                                       # :233-236
    rotation_center_x_int = int(rotation_center_x + 0.5)                                                                     # :243-244
    rotation_center_y_int = int(rotation_center_y + 0.5)
    rotation_window_width = 2 * max(im_size[0] - 1 - rotation_center_x_int + 0.5, rotation_center_x_int + 0.5)              # :249-251
    rotation_window_height = 2 * max(im_size[1] - 1 - rotation_center_y_int + 0.5, rotation_center_y_int + 0.5)
    Delta_x = rotation_center_x - rotation_center_x_int                                                                      # :253-254
    Delta_y = rotation_center_y - rotation_center_y_int
    rotation_angle_rad = -rotation_angle * math.pi / 180.0                                                                   # :257
    Delta_x_rotated = Delta_x * math.cos(rotation_angle_rad) - Delta_y * math.sin(rotation_angle_rad)                        # :258
    Delta_y_rotated = Delta_y * math.cos(rotation_angle_rad) + Delta_x * math.sin(rotation_angle_rad)                        # :259
    rotation_crop_x0 = rotation_center_x_int - (rotation_window_width - 1) / 2.0                                             # :261-262
    rotation_crop_y0 = rotation_center_y_int - (rotation_window_height - 1) / 2.0
    crop_size = (int(rotation_window_width + 0.5), int(rotation_window_height + 0.5))                                        # :266
    assert rotation_crop_x0 == int(rotation_crop_x0) and rotation_crop_y0 == int(rotation_crop_y0) and crop_size[0] & 1 and crop_size[1] & 1
    center_x_geometric = (crop_size[0] - 1) / 2.0                                                                            # :296-297
    center_y_geometric = (crop_size[1] - 1) / 2.0
    new_center_x = center_x_geometric + Delta_x_rotated                                                                      # :300-301
    new_center_y = center_y_geometric + Delta_y_rotated
    x0 = (new_center_x - (ori_width - 1) / 2.0)                                                                              # :307-310
    x1 = (new_center_x + (ori_width - 1) / 2.0) + 1
    y0 = (new_center_y - (ori_height - 1) / 2.0)
    y1 = (new_center_y + (ori_height - 1) / 2.0) + 1
    # Image.rotate(rotation_angle) on the crop, default centre (tests/filters_restate.py::rotate_matrix)
    a = rotation_angle % 360.0
    if a == 0:
        m, rotated = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0], 0
    else:
        r = -math.radians(a)
        m = [round(math.cos(r), 15), round(math.sin(r), 15), 0.0, round(-math.sin(r), 15), round(math.cos(r), 15), 0.0]
        center = (crop_size[0] / 2.0, crop_size[1] / 2.0)
        x, y = -center[0], -center[1]
        m[2], m[5] = m[0] * x + m[1] * y + m[2], m[3] * x + m[4] * y + m[5]
        m[2] += center[0]
        m[5] += center[1]
        rotated = 1
    rx, rw = _axis_range(x0, x1, out_size[0], crop_size[0])
    ry, rh = _axis_range(y0, y1, out_size[1], crop_size[1])
    rect = [rx, ry, rw, rh] if rw and rh else [0, 0, 0, 0]
    return dict(crop_x0=int(rotation_crop_x0), crop_y0=int(rotation_crop_y0), W=crop_size[0], H=crop_size[1], angle=rotation_angle,
                shift=[Delta_x_rotated, Delta_y_rotated], m=m, box=[x0, y0, x1, y1], rotated=rotated, status=0, rect=rect)


def pil_normalize(frame, geom, out_size):
    """The oracle: the three PIL calls of normalize_image on ``frame`` (H, W) uint8 with the geometry ``geom`` (a record of
    ``normalize.geometry`` or a dict of ``geometry_restate``); a refused face is all zero.  (out_h, out_w) uint8."""
    from PIL import Image
    if int(geom["status"]) != 0:
        return np.zeros((out_size[1], out_size[0]), np.uint8)
    W, H, cx0, cy0 = (int(geom[k]) for k in ("W", "H", "crop_x0", "crop_y0"))
    im = Image.fromarray(np.ascontiguousarray(frame))
    crop = im.transform((W, H), Image.EXTENT, (cx0, cy0, cx0 + W, cy0 + H))      # NEAREST, an integer box: a shift
    rot = crop.rotate(float(geom["angle"]), Image.BICUBIC)
    out = rot.transform(tuple(out_size), Image.EXTENT, tuple(float(v) for v in geom["box"]), Image.BICUBIC)
    return np.asarray(out)


def pitched(frame, pad=5, fill=0xA5):
    """A view of ``frame`` inside a buffer whose rows are ``pad`` bytes longer, the gap filled with ``fill``."""
    h, w = frame.shape
    buf = np.full((h, w + pad), fill, np.uint8)
    buf[:, :w] = frame
    return buf[:, :w]


def crop_view(frame, left=3, top=2, right=4, bottom=5, seed=3):
    """A view of ``frame`` as the inside of a larger noise frame."""
    h, w = frame.shape
    big = np.random.default_rng(seed).integers(0, 256, (h + top + bottom, w + left + right), dtype=np.uint8)
    big[top:top + h, left:left + w] = frame
    return big[top:top + h, left:left + w]
