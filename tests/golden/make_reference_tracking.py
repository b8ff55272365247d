"""Regenerate tests/golden/reference_tracking.npz from the reference's own grid functions, tracking branch.

    python tests/golden/make_reference_tracking.py <reference checkout>

The method is make_reference_glue.py's: face_analysis.py is read at run time, its print statements are converted with lib2to3, the
three grid builders are picked out of the syntax tree BY NAME and only they are executed, with numpy in their namespace.  None of
their text is stored here or in the fixture: the fixture holds our chosen tracked boxes and the functions' outputs.  Three shims,
all ours: print goes through lib2to3's fix_print; numpy.linspace receives int(num) (unused by the tracking branch, kept so that the
namespace is the one make_reference_glue.py builds); and ``tracked_face`` is SET IN THE NAMESPACE the functions execute in before
every call of compute_posX_posY_values — in the reference it is a free name of that function, not a parameter, so as shipped the
tracking branch raises NameError (face_analysis.py:622).

Per tracked box, with ``track_single_face`` and ``face_has_been_found`` true (face_analysis.py:576-585, :611-623, :650-651, :661-669;
FaceDetectUpdated.py:603-604): the one sampling value, posX (3), posY (3), patch width / height, max_Dx_diff, max_Dy_diff, the nine
windows (y-major: the three distinct boxes, three times) and base_side = numpy.sqrt(patch_width ** 2 + patch_height ** 2), computed
here on the functions' own numpy.float64 outputs as the reference's script does.

Besides random boxes (square and not, x1 < x0, partly outside the frame, of the magnitude the eye purge hands over, sub-images 64x64,
128x128 and 16x16) the fixture holds EDGE ROWS, found by search with exact rational arithmetic: boxes where a fused multiply-add
(a * b + c rounded once) would change the last bit of
  * base_side, through patch_width * patch_width + patch_height ** 2 (either product fused), or
  * a window's x1 / y1, through posX + subimage_width * sampling_value (the patch size is a product that feeds the addition).
posX +- patch_sepx itself cannot flip with the pipeline's constants: patch_sepx = (net_Dx * 2.0 * patch_width) / regression_width ends
in a division by 128, which is exact, so the sum rounds the same fused or not (counted below and asserted to be 0); the product that
can be fused into that corner is the patch size.  With the pipeline's own sub-images (64x64, 128x128, 16x16: square, powers of two) NO
fused form can flip anything — subimage_width * sampling_value is then exact, and patch_width == patch_height makes the sum of squares
an exact doubling; the search below confirms it (asserted: 0 flips in 20000 boxes per size).  The edge rows therefore use two further
sub-image sizes, 48x40 and 100x60 (neither square nor a power of two), where both hazards exist; the functions under test take the
sub-image size as a parameter.  The generator asserts that it found rows of both kinds.  It also asserts that
``patch_width ** 2`` (C pow) equals ``patch_width * patch_width`` on every stored box: the device squares by multiplying.
No test imports this script; the tests read the .npz only."""
from __future__ import annotations

import ast
import math
import os
import sys
import types
from fractions import Fraction

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "reference_tracking.npz")

FUNCTIONS = ("compute_sampling_values", "compute_posX_posY_values", "compute_subimage_coordinates_from_posX_posY_values")

# grid.FACE_PIPELINE
NET_DX, NET_DY, NET_MINS, NET_MAXS = 40.0, 20.0, 0.694, 0.981
REG_W = REG_H = 128
FRAME = (1000, 562)                # the tracking branch ignores the frame size; the functions still take it
SUBS = ((64, 64), (128, 128), (16, 16))
EDGE_SUBS = ((48, 40), (100, 60))  # where a fused form can change a bit (see the docstring)
N_EDGE = 8                         # edge rows per kind and sub-image size


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
    return ns


def reference_tracked(ns, box, sw, sh):
    """The reference's outputs for one tracked box (a tuple of numpy.float64, as FaceDetectUpdated.py:1191-1192 builds it)."""
    face = tuple(np.float64(v) for v in box)
    svals = ns["compute_sampling_values"](FRAME[0], FRAME[1], sw, sh, 0.2, NET_MINS, NET_MAXS, 1.1, True, True, True, face)
    assert len(svals) == 1
    ns["tracked_face"] = face                                # the third shim: a free name of compute_posX_posY_values
    px, py, pw, ph, mdx, mdy = ns["compute_posX_posY_values"](FRAME[0], FRAME[1], sw, sh, REG_W, REG_H, svals[0], NET_DX, NET_DY, 1.1, True, True, True)
    del ns["tracked_face"]
    n, boxes = ns["compute_subimage_coordinates_from_posX_posY_values"](px, py, pw, ph)
    assert n == 9 and boxes.shape == (9, 4)
    base_side = np.sqrt(pw ** 2 + ph ** 2)                   # FaceDetectUpdated.py:603-604
    assert float(pw ** 2) == float(pw) * float(pw) and float(ph ** 2) == float(ph) * float(ph), box
    return dict(sampling=float(svals[0]), posx=np.array(px, dtype=np.float64), posy=np.array(py, dtype=np.float64),
                patch=np.array([pw, ph], dtype=np.float64), maxd=np.array([mdx, mdy], dtype=np.float64), boxes=np.asarray(boxes, dtype=np.float64),
                base_side=float(base_side))


# ---- exact arithmetic: what a fused a * b + c (one rounding) would give --------------------------------------------------------
def fma(a, b, c):
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def fused_flips(box, sw, sh):
    """(base_side flips, a window corner flips, posX +- sepx flips) for one box, in plain float64 against the fused forms."""
    x0, y0, x1, y1 = (float(v) for v in box)
    s = (0.5 * abs(x1 - x0) + 0.5 * abs(y1 - y0)) * 1.0 / sw
    pw, ph = sw * s, sh * s
    side = math.sqrt(pw * pw + ph * ph)
    side_f = {math.sqrt(fma(pw, pw, ph * ph)), math.sqrt(fma(ph, ph, pw * pw))}
    a = NET_DX * 2.0 * pw
    sepx = a / REG_W
    xs = [x0, x0 + sepx, x0 - sepx]
    corner = any(fma(sw, s, x) - 1 != x + pw - 1 for x in xs) or fma(sh, s, y0) - 1 != y0 + ph - 1
    sep = fma(a, 1.0 / REG_W, x0) != x0 + sepx or fma(-a, 1.0 / REG_W, x0) != x0 - sepx
    return side_f != {side}, corner, sep


def random_box(rng, kind):
    if kind == "purge":          # the magnitude of an eye-purge output row on a 1000 x 562 frame: a face of 60 .. 400 pixels, fractional corners
        s = float(rng.uniform(60, 400))
        x0, y0 = float(rng.uniform(0, 1000 - s)), float(rng.uniform(0, 562 - s * 0.5))
        return [x0, y0, x0 + s * float(rng.uniform(0.97, 1.03)), y0 + s * float(rng.uniform(0.97, 1.03))]
    if kind == "oblong":
        x0, y0 = float(rng.uniform(0, 800)), float(rng.uniform(0, 400))
        return [x0, y0, x0 + float(rng.uniform(20, 300)), y0 + float(rng.uniform(20, 300))]
    if kind == "flipped":        # x1 < x0 (and once y1 < y0): the abs of the sampling value
        x0, y0 = float(rng.uniform(200, 800)), float(rng.uniform(100, 400))
        b = [x0, y0, x0 - float(rng.uniform(20, 150)), y0 + float(rng.uniform(20, 150))]
        if rng.random() < 0.3:
            b[3] = y0 - float(rng.uniform(20, 150))
        return b
    if kind == "outside":        # x0 - sepx < 0 (sepx = 0.625 of the face size), some with x0 < 0 itself or beyond the right / lower edge
        s = float(rng.uniform(80, 300))
        x0 = float(rng.uniform(-0.3 * s, 0.6 * s))
        y0 = float(rng.uniform(-0.3 * s, 562 - 0.5 * s))
        if rng.random() < 0.3:
            x0 = float(rng.uniform(1000 - 1.2 * s, 1000 - 0.4 * s))
        return [x0, y0, x0 + s, y0 + s]
    raise ValueError(kind)


def main(argv):
    if len(argv) != 2:
        raise SystemExit(__doc__)
    ns = load_reference(argv[1])
    try:                                                     # as shipped the branch cannot run: the reason for the third shim
        ns["compute_posX_posY_values"](FRAME[0], FRAME[1], 64, 64, REG_W, REG_H, 1.0, NET_DX, NET_DY, 1.1, True, True, True)
        raise SystemExit("compute_posX_posY_values ran without tracked_face: the reference changed")
    except NameError:
        pass
    rng = np.random.default_rng(20261017)
    cases = []                                               # (box, sw, sh, kind)
    cases.append(([100.0, 50.0, 164.0, 114.0], 64, 64, "plain"))               # sampling value exactly 1
    cases.append(([10.0, 20.0, 10.0, 20.0], 64, 64, "plain"))                  # a box of no size: sampling value 0, nine equal windows
    cases.append(([-20.5, -10.25, 40.0, 50.0], 64, 64, "outside"))
    for sw, sh in SUBS:
        for kind, n in (("purge", 4), ("oblong", 4), ("flipped", 3), ("outside", 4)):
            for _ in range(n):
                cases.append((random_box(rng, kind), sw, sh, kind))
    for sw, sh in SUBS:                                      # the pipeline's sizes: nothing to flip
        for t in range(20000):
            assert fused_flips(random_box(rng, "purge" if t % 2 else "oblong"), sw, sh) == (False, False, False), (sw, sh)
    for sw, sh in EDGE_SUBS:                                 # ordinary boxes on the two further sizes
        for kind in ("purge", "oblong", "flipped", "outside"):
            cases.append((random_box(rng, kind), sw, sh, kind))
    n_random = len(cases)
    found = {"side": 0, "corner": 0}
    for sw, sh in EDGE_SUBS:
        for want in ("side", "corner"):
            got = tries = 0
            while got < N_EDGE and tries < 100000:
                tries += 1
                b = random_box(rng, "purge" if tries % 2 else "oblong")
                side, corner, sep = fused_flips(b, sw, sh)
                assert not sep, b                            # division by 128 is exact: see the docstring
                if (side if want == "side" else corner):
                    cases.append((b, sw, sh, "edge_" + want))
                    got += 1
            found[want] += got
    assert found["side"] == 2 * N_EDGE and found["corner"] == 2 * N_EDGE, found
    out = {k: [] for k in ("box", "sub", "sampling", "posx", "posy", "patch", "maxd", "boxes", "base_side", "fma_side", "fma_corner", "fma_sep")}
    kinds = []
    for b, sw, sh, kind in cases:
        r = reference_tracked(ns, b, sw, sh)
        side, corner, sep = fused_flips(b, sw, sh)
        out["box"].append(b)
        out["sub"].append([sw, sh])
        for k in ("sampling", "posx", "posy", "patch", "maxd", "boxes", "base_side"):
            out[k].append(r[k])
        out["fma_side"].append(side)
        out["fma_corner"].append(corner)
        out["fma_sep"].append(sep)
        kinds.append(kind)
    arrays = {k: np.array(v, dtype=np.int64 if k == "sub" else (bool if k.startswith("fma_") else np.float64)) for k, v in out.items()}
    arrays["kind"] = np.array(kinds)
    arrays["consts"] = np.array([NET_DX, NET_DY, REG_W, REG_H], dtype=np.float64)
    assert len(cases) >= 40 and not arrays["fma_sep"].any()
    assert arrays["fma_side"].sum() >= 2 * N_EDGE and arrays["fma_corner"].sum() >= 2 * N_EDGE
    assert (arrays["box"][:, 2] < arrays["box"][:, 0]).any() and (arrays["posx"][:, 2] < 0).any()
    assert all((arrays["sub"] == s).all(axis=1).any() for s in SUBS)
    np.savez_compressed(OUT, **arrays)
    print("%s: %d boxes (%d chosen or random, %d edge rows), %d bytes; fma flips: base_side %d, corner %d, sepx %d" %
          (OUT, len(cases), n_random, len(cases) - n_random, os.path.getsize(OUT), arrays["fma_side"].sum(), arrays["fma_corner"].sum(),
           arrays["fma_sep"].sum()))


if __name__ == "__main__":
    main(sys.argv)
