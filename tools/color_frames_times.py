"""What a colour frame costs: detect_frame, detect_faces and a tracked FaceTracker.step (one host call each) on the synthetic 1920x1080
frame of BASELINE.json configs[2] as a grey frame and as RGB and BGRA frames whose PIL grey is that frame (tests/color_cases.py
``color_twin``), through cascades of those frame formats; frames.to_gray of the colour frames alone; and the prescale of the RGB frame
to 1000 x 562 as the cascade does it — one launch through the format gather, which converts the sampled pixels only — against its
composition, to_gray of the whole frame followed by the grey prescale (device time between two events).  One process, the variants
alternated call by call; minimum, median and maximum over --reps calls each, appended to --out with the library that was loaded.  A
library of an older commit (HIGSFA_LIB, tools/build_ref_lib.sh) has no colour entries: its run gives the grey figures to compare with;
--formats L makes this build's process do exactly what that one does (the grey path of the two builds, like for like).

    python tools/color_frames_times.py [--reps 30] [--formats L,RGB,BGRA] [--label this] [--out profiles/r10_color_frames.txt]
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
from pyfaceanalysis_amd.tracking import FaceTracker  # noqa: E402
from tests import color_cases as CC  # noqa: E402
from tests import eyes_restate as ER  # noqa: E402

CONTRAST = (128.0, 48.0)
SF = 0.1


def stats(ms):
    return "min %.4f  median %.4f  max %.4f ms" % (np.min(ms), np.median(ms), np.max(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--formats", default="L,RGB,BGRA", help="L alone: the grey path only, as a library without colour frames runs it")
    ap.add_argument("--label", default="this build")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r10_color_frames.txt"))
    a = ap.parse_args()
    if a.reps < 30:
        ap.error("--reps must be at least 30")
    L = _capi.lib()
    has_color = hasattr(L, "hg_cascade_set_frame_format") and a.formats != "L"
    if a.formats not in ("L", "L,RGB,BGRA"):
        ap.error("--formats is L or L,RGB,BGRA")
    rng = np.random.default_rng(synth.INPUT_SEED)
    frame = np.rint(synth._box3(rng.integers(0, 256, (1080, 1920), dtype=np.uint8))).astype(np.uint8)
    rgb, fell_back = CC.color_twin(frame, 2801)
    assert np.array_equal(CC.pil_gray(rgb, "RGB"), frame)
    dev = {"L": torch.from_numpy(frame).cuda()}
    if has_color:
        dev["RGB"] = torch.from_numpy(rgb).cuda()
        dev["BGRA"] = torch.from_numpy(CC.as_format(rgb, "BGRA")).cuda()
    pipe = dict(grid.FACE_PIPELINE)
    # bench.py's configs[2] cascade and tools/eyes_times.py's eye stages, calibrated on the grey frame
    from PIL import Image
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
    dcs = {f: DeviceCascade(stages, (128, 128), 20, pipe, **(dict(frame_format=f) if f != "L" else {})) for f in dev}
    trs = {f: FaceTracker(dcs[f], loc, smallest_face=SF) for f in dev}

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

    def tracked_step(f):      # untimed: forget the face and find it again on the full grid; timed: the tracked frame
        trs[f].reset()
        trs[f].step(dev[f])
        ms, r = wall_ms(lambda: trs[f].step(dev[f]))
        if not r["tracked"]:
            raise SystemExit("the full grid keeps no face on this frame: nothing to track")
        return ms, r
    gray_buf = torch.empty((1080, 1920), dtype=torch.uint8, device="cuda")
    singles = {"prescale grey frame           (device)": lambda: dcs["L"].prescale(dev["L"])}
    if has_color:
        singles = {"to_gray RGB  (device)": lambda: frames.to_gray(dev["RGB"], "RGB", out=gray_buf),
                   "to_gray BGRA (device)": lambda: frames.to_gray(dev["BGRA"], "BGRA", out=gray_buf),
                   "prescale RGB, one launch      (device)": lambda: dcs["RGB"].prescale(dev["RGB"]),
                   "prescale RGB, to_gray + grey  (device)": lambda: dcs["L"].prescale(frames.to_gray(dev["RGB"], "RGB", out=gray_buf)),
                   "prescale grey frame           (device)": lambda: dcs["L"].prescale(dev["L"])}
    ref = {}
    for _ in range(5):                            # warm-up: plans, workspaces, code objects
        for f in dev:
            ref[f] = (dcs[f].detect_frame(dev[f], smallest_face=SF), dcs[f].detect_faces(dev[f], loc, smallest_face=SF), tracked_step(f)[1])
        for fn in singles.values():
            fn()
    torch.cuda.synchronize()
    for f in dev:                                 # the colour cascades must give the grey cascade's answer
        assert np.array_equal(ref[f][0]["coords"], ref["L"][0]["coords"]) and np.array_equal(ref[f][1]["faces"], ref["L"][1]["faces"]), f
        assert np.array_equal(ref[f][2]["faces"], ref["L"][2]["faces"]), f
    if has_color:
        assert torch.equal(dcs["RGB"].prescale(dev["RGB"]), dcs["L"].prescale(dev["L"]))
    t = {(f, what): [] for f in dev for what in ("detect_frame", "detect_faces", "tracked step")}
    ts = {name: [] for name in singles}
    for _ in range(a.reps):                       # alternated: every variant once per round
        for f in dev:
            t[f, "detect_frame"].append(wall_ms(lambda: dcs[f].detect_frame(dev[f], smallest_face=SF))[0])
            t[f, "detect_faces"].append(wall_ms(lambda: dcs[f].detect_faces(dev[f], loc, smallest_face=SF))[0])
            t[f, "tracked step"].append(tracked_step(f)[0])
        for name, fn in singles.items():
            ts[name].append(device_ms(fn))
    lines = ["== %s: %s (colour frames %s), %s, %d calls each, alternated ==" % (a.label, os.path.relpath(_capi._LIB_PATH, ROOT), "available" if hasattr(L, "hg_cascade_set_frame_format") else "not in this build",
                                                                                 torch.cuda.get_device_name(0), a.reps),
             "frame 1920x1080 -> 1000x562, smallest_face %.1f: survivors %d, faces %d; colour twin: %.1f %% of the pixels are (g, g, g)" %
             (SF, len(ref["L"][0]["coords"]), len(ref["L"][1]["faces"]), 100 * fell_back.mean())]
    for what in ("detect_frame", "detect_faces", "tracked step"):
        for f in dev:
            d = "" if f == "L" else "   median - grey median %+.4f ms" % (np.median(t[f, what]) - np.median(t["L", what]))
            lines.append("%-4s %-13s %s%s" % (f, what, stats(t[f, what]), d))
    for name in singles:
        lines.append("%-40s %s" % (name, stats(ts[name])))
    text = "\n".join(lines)
    print(text, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as fh:
        fh.write(text + "\n")
    for tr in trs.values():
        tr.close()
    for dc in dcs.values():
        dc.close()
    loc.close()
    pt.close()
    eye_flow.close()
    for fl in flows4:
        fl.close()


if __name__ == "__main__":
    main()
