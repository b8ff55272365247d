"""What pose normalisation costs on the device (normalize.FaceNormalizer, hg_patcher_normalize_device) on a 1000 x 562 frame — the
prescaled frame of BASELINE.json configs[2], the one the rows of detect_faces refer to — for both presets ("age": 256 x 260 areaZ, "pose":
256 x 192 area) and 1 / 4 / 16 / 64 faces whose eye distances span strong upsampling to the tap-by-tap bound, some of them at the frame's
border: device time between two events and the time around the call (the host returns before the device has finished), beside the PIL
composition of the reference (transform, rotate, transform; tests/normalize_cases.py::pil_normalize) timed in the same process, per face.
Then the staged path against the tap-by-tap path (flags 1 / 2) on both sides of the work-equality bound — 16 faces of one shrink factor
each from 2 x to 8 x, a 64 x 48 output so that the frame can hold a box of 8 x the output.  One process, the variants alternated call by call; minimum,
median and maximum over --reps calls each, appended to --out with the library that was loaded.  Every timed configuration is checked
against PIL on its first face before it is timed.

    python tools/normalize_times.py [--reps 30] [--label this] [--out profiles/r15_normalize_times.txt]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pyfaceanalysis_amd import _capi, normalize as N, synth  # noqa: E402
from tests import normalize_cases as NC  # noqa: E402

FW, FH = 1000, 562


def stats(ms):
    return "min %.4f  median %.4f  max %.4f ms" % (np.min(ms), np.median(ms), np.max(ms))


def faces(n, rng, lo=8.0, hi=150.0):
    """n eye rows: eye distances geometric in [lo, hi] pixels, tilts in +-25 degrees, every fourth face centred within 20 pixels of a
    frame edge."""
    dist = np.exp(np.linspace(np.log(lo), np.log(hi), n)) if n > 1 else np.array([60.0])
    rng.shuffle(dist)
    ang = np.radians(rng.uniform(-25.0, 25.0, n))
    cx, cy = rng.uniform(0.15 * FW, 0.85 * FW, n), rng.uniform(0.15 * FH, 0.7 * FH, n)
    cx[3::4] = rng.choice([rng.uniform(0, 20), rng.uniform(FW - 20, FW)], len(cx[3::4]))
    dx, dy = dist / 2 * np.cos(ang), dist / 2 * np.sin(ang)
    return np.stack([cx - dx, cy - dy, cx + dx, cy + dy], axis=1)


def shrunk_faces(n, factor, out_w, rng):
    """n faces whose box is `factor` x a pose output of out_w pixels (ori_w = out_w * dist / 37.5), centred well inside the frame."""
    dist = factor * 37.5
    ang = np.radians(rng.uniform(-20.0, 20.0, n))
    cx, cy = rng.uniform(0.35 * FW, 0.65 * FW, n), rng.uniform(0.3 * FH, 0.5 * FH, n) - (42.0 / 37.0) * dist / 2
    dx, dy = dist / 2 * np.cos(ang), dist / 2 * np.sin(ang)
    return np.stack([cx - dx, cy - dy, cx + dx, cy + dy], axis=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--label", default="this build")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r15_normalize_times.txt"))
    a = ap.parse_args()
    if a.reps < 30:
        ap.error("--reps must be at least 30")
    rng = np.random.default_rng(synth.INPUT_SEED)
    frame = np.rint(synth._box3(rng.integers(0, 256, (FH, FW), dtype=np.uint8))).astype(np.uint8)
    fdev = torch.from_numpy(frame).cuda()

    def wall_and_device_ms(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        t0 = time.perf_counter()
        fn()
        call = (time.perf_counter() - t0) * 1e3
        e1.record()
        e1.synchronize()
        return call, e0.elapsed_time(e1)

    variants, pil_sets, notes = {}, {}, {}
    norms = []
    for preset in ("age", "pose"):
        size = N.PRESETS[preset][0]
        for n in (1, 4, 16, 64):
            fn = N.FaceNormalizer(0, preset=preset)
            norms.append(fn)
            eyes = faces(n, rng)
            g = fn.geometry(eyes, (FW, FH))
            out = torch.empty((n, size[1], size[0]), dtype=torch.uint8, device="cuda")
            n_taps = int(np.sum(g["rect"][:, 2].astype(np.int64) * g["rect"][:, 3] > 16 * size[0] * size[1]))
            notes[preset, n, "default"] = "%d staged, %d tap by tap" % (n - n_taps, n_taps)
            variants[preset, n, "default"] = (fn, eyes, g, out, 0)
            if n == 4:
                pil_sets[preset] = (g, size)
    # staged against tap by tap around the bound: pose method, 64 x 48 output, 16 faces of one shrink factor
    for factor in (2.0, 3.0, 3.5, 4.0, 4.5, 6.0, 8.0):
        fn = N.FaceNormalizer(0, preset="pose", out_size=(64, 48))
        norms.append(fn)
        eyes = shrunk_faces(16, factor, 64, rng)
        g = fn.geometry(eyes, (FW, FH))
        out = torch.empty((16, 48, 64), dtype=torch.uint8, device="cuda")
        rect = np.median(g["rect"][:, 2].astype(np.int64) * g["rect"][:, 3])
        for flags, path in ((1, "staged"), (2, "tap by tap")):
            variants["64x48 shrink %.1fx" % factor, 16, path] = (fn, eyes, g, out, flags)
            notes["64x48 shrink %.1fx" % factor, 16, path] = "median rect %d pixels, the cut's taps %d" % (rect, 16 * 64 * 48)

    def run(v):
        fn, eyes, g, out, flags = v
        fn.normalize(fdev, geoms=g, out=out, flags=flags)
    for key, v in variants.items():           # warm-up (code objects, records, scratch), and what is timed is PIL's image
        for _ in range(3):
            run(v)
        torch.cuda.synchronize()
        assert np.array_equal(v[3][0].cpu().numpy(), NC.pil_normalize(frame, v[2][0], v[0].out_size)), key
    t = {k: ([], []) for k in variants}
    tp = {k: [] for k in pil_sets}
    for _ in range(a.reps):                   # alternated: every variant once per round
        for k, v in variants.items():
            c, d = wall_and_device_ms(lambda: run(v))
            t[k][0].append(c)
            t[k][1].append(d)
        for k, (g, size) in pil_sets.items():
            t0 = time.perf_counter()
            for gi in g:
                NC.pil_normalize(frame, gi, size)
            tp[k].append((time.perf_counter() - t0) * 1e3 / len(g))
    import PIL
    lines = ["== %s: %s, %s, %d calls each, alternated ==" % (a.label, os.path.relpath(_capi._LIB_PATH, ROOT), torch.cuda.get_device_name(0), a.reps),
             "frame %dx%d; every configuration checked against PIL (Pillow %s) on its first face before it was timed" % (FW, FH, PIL.__version__)]
    for k in variants:
        lines.append("%-20s %2d faces %-10s device %s | around the call %s   (%s)" % (k[0], k[1], k[2], stats(t[k][1]), stats(t[k][0]), notes[k]))
    for k in pil_sets:
        lines.append("%-20s PIL composition on this host, per face (4 faces)  %s" % (k, stats(tp[k])))
    text = "\n".join(lines)
    print(text, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as fh:
        fh.write(text + "\n")
    torch.cuda.synchronize()
    for fn in norms:
        fn.close()


if __name__ == "__main__":
    main()
