"""What an antialiased prescale costs: PIL's Image.resize filters on the device (frames.resize, hg_patcher_resize_device) for the
1920x1080 -> 1000x562 prescale of BASELINE.json configs[2] — every filter; grey input, RGB input with grey output and RGB input with RGB output; the one-launch (fused)
kernel forced (flags 2) against the two launches forced (flags 1), each filter through a patcher of its own so that every timed call finds
its tables; beside the NEAREST prescale through the same entry and through DeviceCascade.prescale (device time between two events) — and detect_frame /
detect_faces (one host call each, wall time) through cascades with each prescale filter, with the survivor and face counts beside them:
the synthetic cascade is calibrated on NEAREST pixels, so part of any difference is the networks' load, as with the window filters
(tools/filter_times.py).  One process, the variants alternated call by call; minimum, median and maximum over --reps calls each,
appended to --out with the library that was loaded.  The default path against the parent commit's library is measured with
tools/color_frames_times.py --formats L (HIGSFA_LIB, tools/build_ref_lib.sh), which does exactly what that library does.

    python tools/resize_times.py [--reps 30] [--label this] [--out profiles/r12_prescale_filters.txt]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pyfaceanalysis_amd import _capi, frames, grid, synth, synth_cascade  # noqa: E402
from pyfaceanalysis_amd.cascade import DeviceCascade, frame_windows  # noqa: E402
from pyfaceanalysis_amd.eyes import EyeLocator  # noqa: E402
from pyfaceanalysis_amd.flow import Flow  # noqa: E402
from pyfaceanalysis_amd.patches import Patcher  # noqa: E402
from tests import color_cases as CC  # noqa: E402
from tests import eyes_restate as ER  # noqa: E402

CONTRAST = (128.0, 48.0)
SF = 0.1
FILTERS = ("NEAREST", "BOX", "BILINEAR", "HAMMING", "BICUBIC", "LANCZOS")


def stats(ms):
    return "min %.4f  median %.4f  max %.4f ms" % (np.min(ms), np.median(ms), np.max(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--label", default="this build")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r12_prescale_filters.txt"))
    a = ap.parse_args()
    if a.reps < 30:
        ap.error("--reps must be at least 30")
    from PIL import Image
    rng = np.random.default_rng(synth.INPUT_SEED)
    frame = np.rint(synth._box3(rng.integers(0, 256, (1080, 1920), dtype=np.uint8))).astype(np.uint8)
    rgb, _ = CC.color_twin(frame, 2801)
    assert np.array_equal(CC.pil_gray(rgb, "RGB"), frame)
    dev = {"L": torch.from_numpy(frame).cuda(), "RGB": torch.from_numpy(rgb).cuda()}
    pipe = dict(grid.FACE_PIPELINE)
    # bench.py's configs[2] cascade and tools/eyes_times.py's eye stages, calibrated on the NEAREST prescale of the grey frame
    small = np.asarray(Image.fromarray(frame, "L").resize((1000, 562), Image.NEAREST))
    boxes, _ = frame_windows(1000, 562, SF, pipe, (128, 128))
    pt = Patcher()
    subs = pt.extract(small, boxes, (128, 128), dtype=np.uint8)
    _, nodes128 = synth.cached_preset_blob("U11L-128")
    _, nodes64 = synth.cached_preset_blob("U11L-64")
    flows4 = [Flow(nodes128, output_dtype=np.float32)] + [Flow(synth.build_preset("U11L-128", seed=synth.WEIGHT_SEED + 1009 * i, device=0), output_dtype=np.float32)
                                                          for i in (1, 2, 3)]
    feats4 = [f.execute(subs, n_cols=20) for f in flows4]
    stages = synth_cascade.build_face_cascade(flows4, feats4, pipe, keep_fraction=0.2, later_keep_fraction=0.6)
    eye_flow = Flow(nodes64, output_dtype=np.float32)
    pick = rng.choice(len(boxes), 300, replace=False)
    ang = rng.uniform(-22.5, 22.5, 300)
    eu8 = pt.extract(small, ER.all_eye_boxes(boxes[pick], ang), (64, 64), dtype=np.uint8, delta_angs=-np.concatenate([ang, ang]))
    eye_stages = synth_cascade.build_eye_stages(eye_flow, eye_flow.execute(ER.contrast(eu8, *CONTRAST), n_cols=12))
    loc = EyeLocator(*eye_stages, contrast=CONTRAST)
    dcs = {f: DeviceCascade(stages, (128, 128), 20, pipe, prescale_filter=f) for f in FILTERS}

    def wall_ms(fn):
        t0 = time.perf_counter()
        r = fn()
        return (time.perf_counter() - t0) * 1e3, r

    def device_ms(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)
    out = torch.empty((562, 1000), dtype=torch.uint8, device="cuda")
    pts = {f: Patcher() for f in FILTERS[1:]}      # one per filter: a patcher keeps four axes' tables, and a miss rebuilds and uploads them
    out3 = torch.empty((562, 1000, 3), dtype=torch.uint8, device="cuda")
    singles = {("NEAREST", "L->L", "prescale()"): lambda: dcs["NEAREST"].prescale(dev["L"]),
               ("NEAREST", "L->L", "frames.resize"): lambda: frames.resize(dev["L"], (1000, 562), "NEAREST", out=out, patcher=pt)}
    for f in FILTERS[1:]:
        for fmt, ofmt in (("L", "L"), ("RGB", "L"), ("RGB", "RGB")):
            for flags, path in ((2, "one launch"), (1, "two launches")):
                singles[f, fmt + "->" + ofmt, path] = (lambda f=f, fmt=fmt, ofmt=ofmt, flags=flags: frames.resize(
                    dev[fmt], (1000, 562), f, fmt, ofmt, out=out if ofmt == "L" else out3, patcher=pts[f], flags=flags))
    ref = {}
    for _ in range(5):                            # warm-up: tables, plans, workspaces, code objects
        for f in FILTERS:
            ref[f] = (dcs[f].detect_frame(dev["L"], smallest_face=SF), dcs[f].detect_faces(dev["L"], loc, smallest_face=SF))
        for fn in singles.values():
            fn()
    torch.cuda.synchronize()
    for f in FILTERS:                             # what is timed is PIL's resize
        want = np.asarray(Image.fromarray(frame, "L").resize((1000, 562), frames.RESAMPLE[f]))
        assert np.array_equal(dcs[f].prescale(dev["L"]).cpu().numpy(), want), f
        if f != "NEAREST":
            for fmt in ("L", "RGB"):
                for flags in (0, 1, 2):
                    assert np.array_equal(frames.resize(dev[fmt], (1000, 562), f, fmt, patcher=pt, flags=flags).cpu().numpy(), want), (f, fmt, flags)
    t = {(f, what): [] for f in FILTERS for what in ("detect_frame", "detect_faces")}
    ts = {name: [] for name in singles}
    for _ in range(a.reps):                       # alternated: every variant once per round
        for f in FILTERS:
            t[f, "detect_frame"].append(wall_ms(lambda: dcs[f].detect_frame(dev["L"], smallest_face=SF))[0])
            t[f, "detect_faces"].append(wall_ms(lambda: dcs[f].detect_faces(dev["L"], loc, smallest_face=SF))[0])
        for name, fn in singles.items():
            ts[name].append(device_ms(fn))
    lines = ["== %s: %s, %s, %d calls each, alternated ==" % (a.label, os.path.relpath(_capi._LIB_PATH, ROOT), torch.cuda.get_device_name(0), a.reps),
             "frame 1920x1080 -> 1000x562, smallest_face %.1f; every prescale checked against PIL before it was timed" % SF]
    for name in singles:
        lines.append("resize %-8s %-8s %-13s (device)  %s" % (name + (stats(ts[name]),)))
    for what in ("detect_frame", "detect_faces"):
        for f in FILTERS:
            r = ref[f][0] if what == "detect_frame" else ref[f][1]
            n = "survivors %d, rows executed %d" % (len(r["coords"]), r["rows_executed"]) if what == "detect_frame" else "faces %d, rows executed %d" % (len(r["faces"]), r["rows_executed"])
            d = "" if f == "NEAREST" else "   median - NEAREST median %+.4f ms" % (np.median(t[f, what]) - np.median(t["NEAREST", what]))
            lines.append("%-8s %-13s %s   %s%s" % (f, what, stats(t[f, what]), n, d))
    text = "\n".join(lines)
    print(text, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as fh:
        fh.write(text + "\n")
    for dc in dcs.values():
        dc.close()
    loc.close()
    for q in pts.values():
        q.close()
    pt.close()
    eye_flow.close()
    for fl in flows4:
        fl.close()


if __name__ == "__main__":
    main()
