"""Regenerate tests/golden/reference_glue.npz from the reference's own glue functions.

    python tests/golden/make_reference_glue.py <reference checkout>

The reference (PyFaceAnalysis, Python 2) keeps its float64 glue in pure numpy functions of face_analysis.py; the module itself
imports packages that are not installed (scipy, cuicuilco).  This script reads that file at run time, converts its print
statements with lib2to3, picks the functions it needs out of the syntax tree BY NAME and executes only them, with numpy in their
namespace.  None of their text is stored here or in the fixture: the fixture holds our chosen inputs and the functions' outputs.
Two shims, both ours: print goes through lib2to3's fix_print (the purge prints its sorted confidences; the output is discarded),
and numpy.linspace receives int(num) (the reference passes the float that numpy.ceil returns, which numpy 2 refuses).

Besides random inputs the fixture holds EDGE ROWS: inputs built with exact rational arithmetic so that the reference's comparison
lands exactly on its threshold, and where a fused multiply-add (a * b + c rounded once) would decide the other way.  The
generator asserts that every hazard kind has such a row.  The eye step's contrast rule (image_array_contrast_normalize_avg_std) is
extracted too, on the crafted patches of tests/eye_tail_cases.py; its eye shift is not — the reference computes it inside
find_Left_Right_eyes, which calls the networks (see contrast_fixture).  No test imports this script; the tests read the .npz only."""
from __future__ import annotations

import ast
import contextlib
import io
import math
import os
import sys
import types
from fractions import Fraction

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "reference_glue.npz")

FUNCTIONS = ("compute_sampling_values", "compute_posX_posY_values", "compute_subimage_coordinates_from_posX_posY_values",
             "update_current_subimage_coordinates", "identify_patches_to_discard", "compute_approximate_eye_boxes_coordinates",
             "relative_error_detection", "purgue_detected_faces_angles_eyes_confidence", "image_array_contrast_normalize_avg_std")

# the constants the product passes (grid.FACE_PIPELINE, cascade.DeviceCascade._consts, FaceDetectUpdated.py:113-115)
NET_DX, NET_DY, NET_DANG, NET_MINS, NET_MAXS = 40.0, 20.0, 22.5, 0.694, 0.981
REG_W = REG_H = 128.0
DESIRED_SAMPLING = 0.825
TOL = 1.1
MAX_SCALE_RADIO, MIN_SCALE_RADIO = NET_MAXS / 0.825, NET_MINS / 0.825
CUT_OFF = 0.5

# grid cases: (frame width, frame height, smallest_face, sub-image width, sub-image height)
GRID_CASES = [(1000, 562, 0.1, 128, 128), (1000, 562, 0.2, 64, 64), (1920, 1080, 0.05, 64, 64), (160, 90, 0.3, 16, 16),
              (133, 131, 0.9, 128, 128), (40, 400, 0.5, 32, 32), (3648, 2736, 0.02, 64, 64), (400, 30, 0.9, 32, 32)]
STAGES = ("Disc", "PosX", "PosY", "PAng", "Scale")


def load_reference(ref_dir):
    from lib2to3 import refactor
    path = os.path.join(ref_dir, "face_analysis.py")
    src = open(path).read()
    tool = refactor.RefactoringTool(["lib2to3.fixes.fix_print"])
    tree = ast.parse(str(tool.refactor_string(src + ("\n" if not src.endswith("\n") else ""), path)))
    defs = {n.name: n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in FUNCTIONS}
    missing = set(FUNCTIONS) - set(defs)
    if missing:
        raise SystemExit("not found in %s: %s" % (path, sorted(missing)))
    shim = types.ModuleType("numpy_shim")
    shim.__dict__.update({k: getattr(np, k) for k in dir(np) if not k.startswith("__")})
    shim.linspace = lambda start, stop, num=50, *a, **k: np.linspace(start, stop, int(num), *a, **k)
    ns = {"numpy": shim}
    exec(compile(ast.Module(body=[defs[f] for f in FUNCTIONS], type_ignores=[]), path, "exec"), ns)
    return types.SimpleNamespace(**{f: ns[f] for f in FUNCTIONS})


# ---- exact arithmetic: one rounding per operation (numpy) against a fused a * b + c --------------------------------------------
def fma(a, b, c):
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def csqrt(x):
    """Correctly rounded sqrt (math.sqrt is, IEEE 754)."""
    return math.sqrt(x)


def grid_fixture(R, out):
    for ci, (fw, fh, sf, sw, sh) in enumerate(GRID_CASES):
        svals = R.compute_sampling_values(fw, fh, sw, sh, sf, NET_MINS, NET_MAXS, 1.1, True, False, False, None)
        boxes, lv, counts = [], [], []
        for s in svals:
            px, py, pw, ph, mdx, mdy = R.compute_posX_posY_values(fw, fh, sw, sh, REG_W, REG_H, s, NET_DX, NET_DY, 1.1, False, False, True)
            n, b = R.compute_subimage_coordinates_from_posX_posY_values(px, py, pw, ph)
            nx, ny = len(px), len(py)
            # the boxes are a y-major mesh: box j * nx + i = (X0[i], Y0[j], X1[i], Y1[j]); stored as its four axes, losslessly
            ax = [b[:nx, 0], b[::nx, 1], b[:nx, 2], b[::nx, 3]]
            assert n == len(b) == nx * ny and np.array_equal(b, np.stack([ax[0][None, :].repeat(ny, 0).ravel(), ax[1][:, None].repeat(nx, 1).ravel(),
                                                                          ax[2][None, :].repeat(ny, 0).ravel(), ax[3][:, None].repeat(nx, 1).ravel()], 1))
            boxes.append(np.concatenate(ax))
            lv.append([mdx, mdy])
            counts.append([nx, ny])
        out["grid%d_case" % ci] = np.array([fw, fh, sf, sw, sh], dtype=np.float64)
        out["grid%d_axes" % ci] = np.concatenate(boxes)
        out["grid%d_level" % ci] = np.array(lv, dtype=np.float64)
        out["grid%d_counts" % ci] = np.array(counts, dtype=np.int64)
    assert any((out["grid%d_counts" % ci] == 1).any() for ci in range(len(GRID_CASES))), "no single-point axis"


def reference_step(R, kind, coords, angles, reg, oidx, ocoords, oangles, olevel):
    """update_current_subimage_coordinates + identify_patches_to_discard, one call per distinct level row (the reference takes the
    level constants as scalars)."""
    c, a = R.update_current_subimage_coordinates(kind, coords.copy(), angles.copy(), reg.copy(), REG_W, REG_H, DESIRED_SAMPLING)
    wrong = np.zeros(len(c), dtype=bool)
    lv = olevel[oidx]
    keys = np.unique(lv, axis=0)
    for key in keys:
        sel = np.nonzero((lv == key).all(axis=1))[0]
        w = R.identify_patches_to_discard(kind, c[sel], np.asarray(a)[sel], reg[sel], key[2], 1e9, 1e9, oidx[sel], ocoords, oangles, key[0], key[1],
                                          TOL, MAX_SCALE_RADIO, MIN_SCALE_RADIO, TOL, NET_DANG, TOL, CUT_OFF)
        wrong[sel] = w
    return c, np.asarray(a, dtype=np.float64), wrong


def random_candidates(rng, kind, n, n_levels=6):
    """n candidates of n_levels pyramid levels, each a moved copy of one of n / 4 original windows (as in the cascade, several
    candidates descend from one window)."""
    m = n // 4
    side = rng.choice(20.0 * 1.25 ** np.arange(n_levels), m)
    lvl_id = np.searchsorted(np.unique(side), side)
    x0, y0 = rng.uniform(-10, 900, m), rng.uniform(-10, 500, m)
    ocoords = np.stack([x0, y0, x0 + side - 1, y0 + side - 1], axis=1)
    pw = side
    olevel = np.stack([NET_DX * pw / REG_W, NET_DY * pw / REG_H, np.sqrt(pw ** 2 + pw ** 2)], axis=1)
    oangles = np.where(rng.random(m) < 0.5, 0.0, rng.uniform(-30, 30, m))
    oidx = rng.integers(0, m, n).astype(np.int32)
    coords = ocoords[oidx] + rng.normal(0, 1, (n, 4)) * olevel[oidx, :1] * 0.6
    angles = oangles[oidx] + rng.uniform(-10, 10, n) * (rng.random(n) < 0.7)
    if kind == "Disc":
        reg = rng.uniform(0, 1, n)
    elif kind in ("PosX", "PosY"):
        reg = rng.normal(0, 25, n)
    elif kind == "PAng":
        reg = rng.normal(0, 18, n)
    else:
        reg = rng.uniform(0.45, 1.6, n)
    assert len(np.unique(lvl_id)) >= 3
    return coords, angles, reg, oidx, ocoords, oangles, olevel


# ---- edge rows ---------------------------------------------------------------------------------------------------------------
def pang_edges(rng, want):
    """ang == oa +- net_Dang * tol under numpy (on the limit: not discarded), while the fused oa +- fma lands on the other side."""
    lim = NET_DANG * TOL
    rows = []
    while len(rows) < want:
        oa = float(rng.uniform(-60, 60))
        for sign in (1.0, -1.0):
            t = oa + sign * lim                               # numpy: the limit, rounded twice
            fused = fma(sign * NET_DANG, TOL, oa)             # one rounding
            if fused == t:
                continue
            r = float(rng.uniform(-3, 3))
            prev = t - r
            if prev + r != t:
                continue
            # numpy keeps it (ang == limit); the fused limit moved inward would discard it
            disagree = (t > fused) if sign > 0 else (t < fused)
            rows.append((oa, prev, r, disagree))
    return rows


def scale_update(x0, y0, x1, y1, r):
    ow, oh = x1 - x0, y1 - y0
    xc, yc = (x1 + x0) / 2.0, (y1 + y0) / 2.0
    w, h = ow / r * DESIRED_SAMPLING, oh / r * DESIRED_SAMPLING
    return xc - w / 2.0, yc - h / 2.0, xc + w / 2.0, yc + h / 2.0


def scale_edges(rng, want):
    """sqrt(dx^2 + dy^2) / base_side == max_scale_radio * tol (or min_scale_radio / tol) under numpy, base_side chosen for it; the
    fused dx * dx + dy * dy crosses the limit."""
    hi, lo = MAX_SCALE_RADIO * TOL, MIN_SCALE_RADIO / TOL
    rows = []
    tries = 0
    while len(rows) < want and tries < 200000:
        tries += 1
        x0, y0 = float(rng.uniform(0, 900)), float(rng.uniform(0, 500))
        s = float(rng.uniform(20, 300))
        box = (x0, y0, x0 + s * float(rng.uniform(0.8, 1.2)), y0 + s * float(rng.uniform(0.8, 1.2)))
        r = float(rng.uniform(0.5, 1.5))
        a0, b0, a1, b1 = scale_update(*box, r)
        dx, dy = a0 - a1, b0 - b1
        side = csqrt(dx * dx + dy * dy)
        fused = [csqrt(fma(dx, dx, dy * dy)), csqrt(fma(dy, dy, dx * dx))]
        if all(f == side for f in fused):
            continue
        for limit, is_hi in ((hi, True), (lo, False)):
            base = side / limit
            for _ in range(64):
                q = side / base
                if q == limit:
                    break
                base = float(np.nextafter(base, np.inf if q > limit else -np.inf))
            if side / base != limit:
                continue
            disagree = any(((f / base > limit) if is_hi else (f / base < limit)) for f in fused)
            rows.append((box, r, base, disagree))
    return rows


def posxy_edges(rng, kind, want):
    """|centre shift| == max_D * tol exactly (not discarded: the test is >)."""
    rows = []
    while len(rows) < want:
        x0, y0 = float(rng.uniform(0, 900)), float(rng.uniform(0, 500))
        s = float(rng.uniform(20, 300))
        box = [x0, y0, x0 + s - 1, y0 + s - 1]
        r = float(rng.normal(0, 20))
        ax = 0 if kind == "PosX" else 1
        ro = r * (box[2 + ax] - box[ax]) / REG_W
        n0, n1 = box[ax] - ro, box[2 + ax] - ro
        d = abs((n1 + n0) / 2 - (box[2 + ax] + box[ax]) / 2)
        md = d / TOL
        for _ in range(64):
            if md * TOL == d:
                break
            md = float(np.nextafter(md, np.inf if md * TOL < d else -np.inf))
        if md * TOL == d and d > 0:
            rows.append((box, r, md))
    return rows


def update_fixture(R, rng, out):
    n_disagree = {}
    for kind in STAGES:
        coords, angles, reg, oidx, ocoords, oangles, olevel = random_candidates(rng, kind, 200)
        edge = []
        if kind == "PAng":
            for oa, prev, r, dis in pang_edges(rng, 24):
                edge.append(([100.0, 100.0, 163.0, 163.0], prev, r, [100.0, 100.0, 163.0, 163.0], oa, [5.0, 2.5, 89.0], dis))
        elif kind == "Scale":
            for box, r, base, dis in scale_edges(rng, 24):
                edge.append((list(box), 0.0, r, list(box), 0.0, [5.0, 2.5, base], dis))
        elif kind in ("PosX", "PosY"):
            for box, r, md in posxy_edges(rng, kind, 16):
                lv = [md, 7.0, 100.0] if kind == "PosX" else [7.0, md, 100.0]
                edge.append((box, 0.0, r, box, 0.0, lv, False))
        else:
            for r in (CUT_OFF, float(np.nextafter(CUT_OFF, 0.0)), float(np.nextafter(CUT_OFF, 1.0))):
                edge.append(([1.0, 2.0, 33.0, 34.0], 0.0, r, [1.0, 2.0, 33.0, 34.0], 0.0, [5.0, 2.5, 45.0], False))
        m0, n0 = len(ocoords), len(coords)
        e_coords = np.array([e[0] for e in edge], dtype=np.float64)
        coords = np.vstack([coords, e_coords])
        angles = np.concatenate([angles, [e[1] for e in edge]])
        reg = np.concatenate([reg, [e[2] for e in edge]])
        ocoords = np.vstack([ocoords, np.array([e[3] for e in edge], dtype=np.float64)])
        oangles = np.concatenate([oangles, [e[4] for e in edge]])
        olevel = np.vstack([olevel, np.array([e[5] for e in edge], dtype=np.float64)])
        oidx = np.concatenate([oidx, m0 + np.arange(len(edge))]).astype(np.int32)
        c, a, wrong = reference_step(R, kind, coords, angles, reg, oidx, ocoords, oangles, olevel)
        edge_mask = np.zeros(len(coords), dtype=bool)
        edge_mask[n0:] = True
        dis = np.zeros(len(coords), dtype=bool)
        dis[n0:] = [e[6] for e in edge]
        if kind in ("PAng", "Scale", "PosX", "PosY"):
            assert not wrong[n0:].any(), kind                # on the limit: kept by the reference
        else:
            assert list(wrong[n0:]) == [True, False, True]
        n_disagree[kind] = int(dis.sum())
        p = "upd_%s_" % kind
        out.update({p + "coords": coords, p + "angles": angles, p + "reg": reg, p + "oidx": oidx, p + "ocoords": ocoords, p + "oangles": oangles,
                    p + "olevel": olevel, p + "out_wrong": wrong, p + "edge": edge_mask, p + "fma_flips": dis})
        # (what a stage leaves unchanged is not stored: Disc and PAng keep the coordinates, only PAng moves the angles)
        if kind in ("Disc", "PAng"):
            assert np.array_equal(c, coords)
        else:
            out[p + "out_coords"] = c
        if kind == "PAng":
            out[p + "out_angles"] = a
        else:
            assert np.array_equal(a, angles)
    assert n_disagree["PAng"] > 0 and n_disagree["Scale"] > 0, n_disagree
    out["consts"] = np.array([REG_W, REG_H, DESIRED_SAMPLING, TOL, TOL, TOL, MAX_SCALE_RADIO, MIN_SCALE_RADIO, NET_DANG, CUT_OFF])


def eye_fixture(R, rng, out):
    n = 120
    x0, y0 = rng.uniform(-50, 900, n), rng.uniform(-50, 500, n)
    s = rng.uniform(10, 300, n)
    boxes = np.stack([x0, y0, x0 + s * rng.uniform(0.9, 1.1, n), y0 + s * rng.uniform(0.9, 1.1, n)], axis=1)
    angles = rng.uniform(-70, 70, n)
    special = [0.0, 90.0, -90.0, 180.0, -180.0, 24.75, -24.75, 1e-12, -1e-12, 1e-300, -0.0, 0.0, 0.0, 0.0]
    angles[:len(special)] = special
    boxes[0] = [-20.5, -10.25, 40.0, 50.0]                  # partly outside the frame
    eyes, left, right = [], [], []
    for b, a in zip(boxes, angles):
        e, l, r = R.compute_approximate_eye_boxes_coordinates(b, face_sampling=0.825, eye_sampling=2.3719, rot_angle=a)
        eyes.append(e)
        left.append(l)
        right.append(r)
    out.update(eye_boxes=boxes, eye_angles=angles, eye_coords=np.array(eyes), eye_left=np.array(left), eye_right=np.array(right))


def purge_cases(rng):
    def rows(n):
        r = np.zeros((n, 10))
        r[:, 0:4] = rng.uniform(0, 1000, (n, 4))
        r[:, 4] = rng.uniform(-20, 20, n)
        r[:, 5:7] = rng.uniform(0, 1000, (n, 2))
        r[:, 7:9] = r[:, 5:7] + rng.uniform(10, 80, (n, 2))
        r[:, 9] = rng.uniform(0, 1, n)
        return r
    cases = {"n0": np.zeros((0, 10)), "n1": rows(1), "n2": rows(2), "n40": rows(40)}
    d = rows(60)                                            # duplicates within and beyond a quarter of the eye distance
    base = d[:12]
    for j, f in enumerate((0.05, 0.2, 0.26, 0.6)):
        c = base.copy()
        dist = np.hypot(c[:, 7] - c[:, 5], c[:, 8] - c[:, 6])
        c[:, 5:9] += (f * dist / np.sqrt(2))[:, None] * np.array([1.0, 0.0, 1.0, 0.0])
        c[:, 9] = rng.uniform(0, 1, len(c))                 # no ties here: beyond 16 rows numpy's default argsort is not stable
        d[12 * (j + 1):12 * (j + 2)] = c
    cases["dups"] = d
    t = rows(12)                                            # exact ties of the weighted confidence (n <= 16: numpy sorts by insertion)
    t[6:, 9] = t[:6, 9]
    t[6:, 7:9] = t[6:, 5:7] + (t[:6, 7:9] - t[:6, 5:7])
    cases["ties"] = t
    z = rows(3)
    z[:, 7:9] = z[:, 5:7]                                   # every eye distance zero: NaN weights, n + 1 rows kept
    cases["zero"] = z
    zm = rows(6)
    zm[2, 7:9] = zm[2, 5:7]                                 # one zero-area row among others
    cases["zero_one"] = zm
    return cases


def purge_fixture(R, rng, out):
    names = []
    for name, rows in purge_cases(rng).items():
        with contextlib.redirect_stdout(io.StringIO()), np.errstate(divide="ignore", invalid="ignore"):
            got = R.purgue_detected_faces_angles_eyes_confidence(rows.copy())
        got = np.array(got, dtype=np.float64).reshape(-1, 10)
        out["purge_%s_in" % name] = rows
        out["purge_%s_out" % name] = got
        names.append(name)
    assert len(out["purge_zero_out"]) == 4
    out["purge_names"] = np.array(names)


def contrast_fixture(R, out):
    """image_array_contrast_normalize_avg_std on the crafted eye patches of tests/eye_tail_cases.py (constant, two-level, all zero, single
    pixels off, narrow-band noise) at 16 x 16 and 24 x 20, two patches at 64 x 64, for every target pair of ``F_TARGETS``: the uint8
    inputs and the function's float64 outputs (it works in place on a float64 copy).  The eye shift that follows it in the eye step is
    NOT extracted: the reference computes it inside find_Left_Right_eyes, between the calls of its networks, not in a function of its
    own; tests/eyes_restate.shift_eyes restates those lines."""
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    from tests import eye_tail_cases as TC
    kinds = np.zeros(4, dtype=np.int64)
    for w, h in ((16, 16), (24, 20), (64, 64)):
        u8 = TC.fixture_patches((w, h))
        out["contrast_%dx%d_in" % (w, h)] = u8
        for ti, (mean, std) in enumerate(TC.F_TARGETS):
            x = u8.astype(np.float64)
            R.image_array_contrast_normalize_avg_std(x, mean, std)
            out["contrast_%dx%d_out%d" % (w, h, ti)] = x
            kinds += np.array(TC.patch_kinds(u8, (mean, std)))
    assert (kinds > 0).all(), kinds                         # std 0, clipped at 0, clipped at 255, all zero
    out["contrast_targets"] = np.array(TC.F_TARGETS, dtype=np.float64)


# ---- rotated windows: box centres where a fused m2 / m5 moves a 16.16 coefficient -------------------------------------------
def pil_matrix(angle):
    """What Image.rotate builds (PIL's Image.py, Python floats): cos / sin of -radians(angle % 360) rounded to 15 decimals."""
    a = -math.radians(angle % 360.0)
    return round(math.cos(a), 15), round(math.sin(a), 15)


def fix16(v):
    return math.floor(v * 65536.0 + 0.5)


def coef_variants(c, s, cx, cy):
    """PIL's (m2, m5) and the four a fused m0 (-cx) + m1 (-cy) (m3 (-cx) + m4 (-cy)) could give, either product fused."""
    m0, m1, m3, m4 = c, s, -s, c
    plain = (m0 * -cx + m1 * -cy + 0.0 + cx, m3 * -cx + m4 * -cy + 0.0 + cy)
    fm2 = [fma(m0, -cx, m1 * -cy) + 0.0 + cx, fma(m1, -cy, m0 * -cx) + 0.0 + cx]
    fm5 = [fma(m3, -cx, m4 * -cy) + 0.0 + cy, fma(m4, -cy, m3 * -cx) + 0.0 + cy]
    return plain, [(f2, f5) for f2 in fm2 for f5 in fm5]


def fixed_coefs(c, s, m2, m5):
    """affine_fixed's (A0 .. A5) for the matrix (c, s, m2, -s, c, m5): FIX(v) = floor(v * 65536 + 0.5), offsets by half a pixel."""
    m0, m1, m3, m4 = c, s, -s, c
    return (fix16(m0), fix16(m1), fix16(m2 + m0 * 0.5 + m1 * 0.5), fix16(m3), fix16(m4), fix16(m5 + m3 * 0.5 + m4 * 0.5))


def extent_axis(lo, hi, m, lim):
    """Image.transform(EXTENT, NEAREST) along one axis: PIL's running sum of the source coordinate; -1 outside [0, lim)."""
    a = (hi - lo) / m
    o, out = lo + a * 0.5, []
    for _ in range(m):
        v = -1 if o < 0.0 else int(o)
        out.append(v if v < lim else -1)
        o += a
    return np.array(out, dtype=np.int64)


def sampled_sources(box, size, fw, fh, A):
    """(xs, ys) of the frame pixel behind every output pixel of the rotated window; -1 where PIL leaves it 0."""
    xr, yr = extent_axis(box[0], box[2], size[0], fw), extent_axis(box[1], box[3], size[1], fh)
    X, Y = np.meshgrid(xr, yr)
    xs = (A[2] + Y * A[1] + X * A[0]) >> 16
    ys = (A[5] + Y * A[4] + X * A[3]) >> 16
    ok = (X >= 0) & (Y >= 0) & (xs >= 0) & (xs < fw) & (ys >= 0) & (ys < fh)
    return np.where(ok, xs, -1), np.where(ok, ys, -1)


def _bits(x):
    return int(np.float64(x).view(np.int64))


def _from_bits(i):
    return float(np.int64(i).view(np.float64))


ROT_FRAME_HW, ROT_HALF, ROT_SIZES = (120, 160), 32.0, ((64, 64), (37, 21))


def rotation_fixture(rng, out, want=8):
    """Boxes (64-pixel squares about their centre) on a 160 x 120 frame whose windows change if m2 / m5 are fused.  For a few angles
    the centre cx (or cy) is bisected over the floats to where PIL's A2 (A5) steps from one 16.16 value to the next; its nextafter
    neighbours are scanned for a centre where EVERY fused variant moves the source of at least one sampled pixel of the 64 x 64
    window (a one-unit change of A2 moves (A2 + yr A1 + xr A0) >> 16 only where that sum sits on a multiple of 65536).  Stored with
    each box: PIL's (m2, m5) and two fused ones, so that the test can check against PIL that the case is sensitive."""
    fh, fw = ROT_FRAME_HW
    boxes, angs, plains, fuseds = [], [], [], []
    angles = [7.5, -13.0, 22.5, 24.75, -24.75, 3.0, 45.0, -37.25]
    tries = 0
    while len(boxes) < want and tries < 20000:
        tries += 1
        ang = angles[tries % len(angles)]
        c, s = pil_matrix(ang)
        which = tries % 2                                   # 0: A2 through cx, 1: A5 through cy
        other = float(rng.uniform(40, 80))
        v0 = float(rng.uniform(40, 110))

        def coefs(v):
            cx, cy = (v, other) if which == 0 else (other, v)
            plain, fused = coef_variants(c, s, cx, cy)
            return (cx, cy), plain, fused, fixed_coefs(c, s, *plain), [fixed_coefs(c, s, *f) for f in fused]

        # A2 grows by (1 - cos) per unit of cx (A5 likewise with cy): within 2 / (65536 (1 - cos)) it steps at least once
        k = 2 + 3 * which
        lo, hi = _bits(v0), _bits(v0 + 2.0 / (65536.0 * (1.0 - c)))
        p_lo = coefs(_from_bits(lo))[3][k]
        if p_lo == coefs(_from_bits(hi))[3][k]:
            continue
        while hi - lo > 1:
            mid = (lo + hi) // 2
            if coefs(_from_bits(mid))[3][k] == p_lo:
                lo = mid
            else:
                hi = mid
        for i in range(lo - 300, hi + 300):
            (cx, cy), plain, fused, A, AF = coefs(_from_bits(i))
            if all(f == A for f in AF):
                continue
            b = [cx - ROT_HALF, cy - ROT_HALF, cx + ROT_HALF, cy + ROT_HALF]
            if (b[0] + b[2]) / 2.0 != cx or (b[1] + b[3]) / 2.0 != cy:
                continue
            src = sampled_sources(b, ROT_SIZES[0], fw, fh, A)
            moved = [any((g != h).any() for g, h in zip(src, sampled_sources(b, ROT_SIZES[0], fw, fh, F))) for F in AF]
            if all(moved):
                boxes.append(b)
                angs.append(ang)
                plains.append(plain)
                fuseds.append([fused[0], fused[3]])          # m0 (-cx) fused, and m1 (-cy) fused
            break
    assert len(boxes) == want, (len(boxes), tries)
    out["rot_boxes"] = np.array(boxes, dtype=np.float64)
    out["rot_angles"] = np.array(angs, dtype=np.float64)
    out["rot_m25"] = np.array(plains, dtype=np.float64)               # (n, 2): PIL's m2, m5
    out["rot_m25_fused"] = np.array(fuseds, dtype=np.float64)         # (n, 2 variants, 2)
    out["rot_frame_hw"] = np.array(ROT_FRAME_HW, dtype=np.int64)


def main(argv):
    if len(argv) != 2:
        raise SystemExit(__doc__)
    R = load_reference(argv[1])
    rng = np.random.default_rng(20261016)
    out = {}
    grid_fixture(R, out)
    update_fixture(R, rng, out)
    eye_fixture(R, rng, out)
    purge_fixture(R, rng, out)
    rotation_fixture(rng, out)
    contrast_fixture(R, out)
    np.savez_compressed(OUT, **out)
    print("%s: %d arrays, %d bytes; fma flips: %s" % (OUT, len(out), os.path.getsize(OUT),
                                                      {k: int(out["upd_%s_fma_flips" % k].sum()) for k in STAGES}))


if __name__ == "__main__":
    main(sys.argv)
