"""Time a tracked frame against the full grid and against the composed nine-window path, on the frame leg's setup of bench.py.

    python tools/tracking_times.py [--frames 40] [--out profiles/r07_tracking_times.txt]
    python tools/tracking_times.py --max-faces 1,2,4,8 --frames 30 [--ab-lib tools/ab/libhigsfa_parent.so] [--out profiles/r11_multi_tracking.txt]

One synthetic 1920x1080 frame prescaled to 1000x562, smallest_face 0.1, the configs[2] cascade of bench.py's frame leg (U11L-128 in
the roles of the pipeline's four face flows, 128x128 sub-images, the synthetic 17-stage cascade with keep 0.2 / 0.6) and U11L-64 eye
stages calibrated as tests/test_frame_stream_gpu.py calibrates them.  Three cases, each frame timed on its own (every call is
synchronous), median and min - max over --frames frames after 10 warm-up frames:

  (a) full      DeviceCascade.detect_faces: prescale, the whole pyramid (1738 windows), cascade, eyes, purge
  (b) composed  the nine windows around frame 0's first face through the calls that existed before the tracker:
                prescale -> detect(windows=tracked_windows(box)) -> EyeLocator.locate -> assemble_rows -> purge_detections;
                the cascade polls a survivor count after every Disc stage.  The yardstick.
  (c) tracked   FaceTracker.step on a tracked frame: the same nine windows, built on the device, everything enqueued back to back,
                one host wait.  Every timed step follows an untimed reset + full-grid step on the same frame, so that each one
                tracks the same box as (b).

--max-faces K[,K...] measures the tracker that holds several faces instead (profiles/r11_multi_tracking.txt): for every K a
``FaceTracker(max_faces=K)`` whose timed tracked step follows an untimed reset + full-grid step (so it holds the frame's first K faces:
9 K windows), ALTERNATED call by call with ``detect_faces`` on the full grid of the same frame; per-frame medians.  K = 1 is the
default tracker (``hg_tracker_create``), which an older library has too: --ab-lib PATH (tools/build_ref_lib.sh) repeats the K = 1
measurement --ab-rounds times with that library and with the in-tree one in turn, one child process each, and reports whether this
commit's medians lie inside the other library's min - max spread of the same run.

Without --measure this is a driver: the measuring step runs as a child process under ``timeout -k 10``, and nothing runs after a step
that fails."""
from __future__ import annotations

import argparse
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SIDE, N_COLS, SF = 128, 20, 0.1
CONTRAST = (128.0, 48.0)


def stats(ts):
    ts = np.array(ts) * 1e3
    return "median %.3f ms  (min %.3f - max %.3f, %d frames)" % (float(np.median(ts)), ts.min(), ts.max(), len(ts))


def setup():
    """bench.py's frame-leg objects: (device, frame, pipeline, cascade, eye locator, full-grid result, close())."""
    import torch
    from pyfaceanalysis_amd import grid, synth, synth_cascade
    from pyfaceanalysis_amd.blob import flow_to_blob
    from pyfaceanalysis_amd.cascade import DeviceCascade, frame_windows
    from pyfaceanalysis_amd.eyes import EyeLocator
    from pyfaceanalysis_amd.flow import Flow
    from pyfaceanalysis_amd.patches import Patcher
    from tests import eyes_restate as ER
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(synth.INPUT_SEED)
    frame_np = np.rint(synth._box3(rng.integers(0, 256, (1080, 1920), dtype=np.uint8))).astype(np.uint8)
    frame = torch.from_numpy(frame_np).to(dev)
    pipe = dict(grid.FACE_PIPELINE)
    pt = Patcher()
    # the four face flows and their calibration features (bench.py's frame leg)
    blob, _ = synth.cached_preset_blob("U11L-128")
    blobs = [blob] + [flow_to_blob(synth.build_preset("U11L-128", seed=synth.WEIGHT_SEED + 1009 * i, device=0)) for i in (1, 2, 3)]
    flows4 = [Flow.from_blob(b, device=0, output_dtype=np.float32) for b in blobs]
    pw, ph = grid.prescaled_size(1920, 1080)
    from PIL import Image
    small_np = np.array(Image.fromarray(frame_np, "L").resize((pw, ph), Image.NEAREST))
    boxes, _ = frame_windows(pw, ph, SF, pipe, (SIDE, SIDE))
    subs = pt.extract(small_np, boxes, (SIDE, SIDE), dtype=np.uint8)
    feats4 = [f.execute(subs, n_cols=N_COLS) for f in flows4]
    stages = synth_cascade.build_face_cascade(flows4, feats4, pipe, keep_fraction=0.2, later_keep_fraction=0.6)
    dc = DeviceCascade(stages, (SIDE, SIDE), N_COLS, pipe)
    # the eye stages: U11L-64, calibrated on ~300 faces cut from the grid (tests/test_frame_stream_gpu.py's Rig)
    eblob, _ = synth.cached_preset_blob("U11L-64")
    eye_flow = Flow.from_blob(eblob, device=0, output_dtype=np.float32)
    r17 = np.random.default_rng(17)
    fb = boxes[r17.choice(len(boxes), 300, replace=False)].copy()
    fa = r17.uniform(-22.5, 22.5, 300)
    eb = ER.all_eye_boxes(fb, fa)
    u8 = pt.extract(small_np, eb, (64, 64), dtype=np.uint8, delta_angs=-np.concatenate([fa] * 2))
    efeats = eye_flow.execute(ER.contrast(u8, *CONTRAST), n_cols=12)
    _, clf_x, _, clf_y = synth_cascade.build_eye_stages(eye_flow, efeats)
    loc = EyeLocator(eye_flow, clf_x, eye_flow, clf_y, contrast=CONTRAST)
    full = dc.detect_faces(frame, loc, smallest_face=SF)
    if not len(full["faces"]):
        raise SystemExit("the full grid keeps no face on this frame: nothing to track")

    def close():
        loc.close()
        dc.close()
        pt.close()
        eye_flow.close()
        for f in flows4:
            f.close()
    return dev, frame, pipe, (pw, ph), dc, loc, full, close


def measure(n_frames, out_path):
    import torch
    from pyfaceanalysis_amd import eyes as E
    from pyfaceanalysis_amd.cascade import tracked_windows
    from pyfaceanalysis_amd.tracking import FaceTracker
    dev, frame, pipe, (pw, ph), dc, loc, full, close = setup()
    tr = FaceTracker(dc, loc, smallest_face=SF)
    box = full["faces"][0, :4].copy()
    win = tracked_windows(box, pipe, (SIDE, SIDE))

    def case_full():
        return dc.detect_faces(frame, loc, smallest_face=SF)["faces"]

    def case_composed():
        pre = dc.prescale(frame)
        det = dc.detect(pre, windows=win)
        out = loc.locate(pre, det["coords"], det["angles"])
        rows = E.assemble_rows(det["coords"], det["angles"], det["confidence"], out["eye_coords"], out["too_far"])
        return E.purge_detections(rows), det["counts"]

    def timed(fn, before=None):
        ts, last = [], None
        for i in range(10 + n_frames):
            if before is not None:
                before()
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            last = fn()
            torch.cuda.synchronize(dev)
            if i >= 10:
                ts.append(time.perf_counter() - t0)
        return ts, last

    def arm():      # untimed: forget, find the face again on the full grid
        tr.reset()
        r = tr.step(frame)
        assert not r["tracked"] and np.array_equal(r["faces"], full["faces"])

    def case_tracked():
        r = tr.step(frame)
        assert r["tracked"]
        return r["faces"]

    ta, fa_ = timed(case_full)
    tb, (fb_, counts_b) = timed(case_composed)
    tc, fc_ = timed(case_tracked, before=arm)
    same = fb_.shape == fc_.shape and np.array_equal(fb_, fc_)
    lines = ["tracking_times: 1920x1080 frame prescaled to %dx%d, smallest_face %.1f, configs[2] cascade (U11L-128 x 4, 17 stages), U11L-64 eyes" % (pw, ph, SF),
             "device: %s" % torch.cuda.get_device_name(dev),
             "full grid: %d windows, counts %s, %d faces" % (full["n_windows"], full["counts"], len(full["faces"])),
             "tracked box %s; composed nine-window counts %s, %d faces; tracked step equals composed path: %s" %
             (np.array2string(box, precision=3), counts_b, len(fb_), same),
             "(a) full      detect_faces                     %s" % stats(ta),
             "(b) composed  nine windows, existing calls     %s" % stats(tb),
             "(c) tracked   FaceTracker.step, tracked frame  %s" % stats(tc)]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write(text)
    if not same:
        raise SystemExit("the tracked step and the composed path disagree")
    tr.close()
    close()


def measure_multi(ks, n_frames, out_path):
    """Tracked steps of FaceTracker(max_faces=K), K in ``ks``, alternated with detect_faces on the same frame; appends to out_path."""
    import torch
    from pyfaceanalysis_amd.tracking import FaceTracker
    dev, frame, pipe, (pw, ph), dc, loc, full, close = setup()
    lines = ["multi tracking_times [%s]: 1920x1080 frame prescaled to %dx%d, full grid %d windows, %d faces; device %s; %d alternated calls per case" %
             (os.path.relpath(os.environ["HIGSFA_LIB"], ROOT) if os.environ.get("HIGSFA_LIB") else "in-tree library", pw, ph, full["n_windows"], len(full["faces"]), torch.cuda.get_device_name(dev), n_frames)]
    for k in ks:
        tr = FaceTracker(dc, loc, smallest_face=SF, max_faces=k)
        t_tracked, t_full, held, kept = [], [], 0, 0
        for i in range(10 + n_frames):
            tr.reset()                                  # untimed: forget, find the faces again on the full grid
            r = tr.step(frame)
            assert not r["tracked"] and np.array_equal(r["faces"], full["faces"])
            held = len(r["faces"][:k])
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            r = tr.step(frame)
            torch.cuda.synchronize(dev)
            t1 = time.perf_counter()
            f = dc.detect_faces(frame, loc, smallest_face=SF)
            torch.cuda.synchronize(dev)
            t2 = time.perf_counter()
            assert r["tracked"] and r["n_windows"] == 9 * held and np.array_equal(f["faces"], full["faces"])
            kept = len(r["faces"])
            if i >= 10:
                t_tracked.append(t1 - t0)
                t_full.append(t2 - t1)
        tr.close()
        lines.append("max_faces %d: %d held, %3d windows, %2d rows kept   tracked step %s" % (k, held, 9 * held, kept, stats(t_tracked)))
        lines.append("                                            full grid    %s" % stats(t_full))
        print("RESULT max_faces=%d tracked_median_ms=%.4f min_ms=%.4f max_ms=%.4f" %
              (k, float(np.median(t_tracked)) * 1e3, min(t_tracked) * 1e3, max(t_tracked) * 1e3), flush=True)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "a") as f:
            f.write(text)
    close()


def multi_driver(args, ks):
    """Each measuring process a fresh child under its own time limit; the first failure ends the run."""
    import re
    me = [sys.executable, os.path.abspath(__file__), "--measure", "--frames", str(args.frames)]
    if args.out and os.path.exists(args.out):
        os.remove(args.out)
    out = ["--out", args.out] if args.out else []

    def child(k_list, lib):
        env = dict(os.environ)
        env.pop("HIGSFA_LIB", None)
        if lib:
            env["HIGSFA_LIB"] = os.path.abspath(lib)
        cmd = ["timeout", "-k", "10", str(args.step_timeout)] + me + ["--max-faces", ",".join(str(k) for k in k_list)] + out
        r = subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, text=True)
        sys.stdout.write(r.stdout)
        if r.returncode != 0:
            raise SystemExit("step failed with status %d: %s" % (r.returncode, " ".join(cmd)))
        return [tuple(float(v) for v in m) for m in re.findall(r"RESULT max_faces=\d+ tracked_median_ms=(\S+) min_ms=(\S+) max_ms=(\S+)", r.stdout)]

    child(ks, None)
    if args.ab_lib:
        other, mine = [], []
        for _ in range(args.ab_rounds):
            other += child([1], args.ab_lib)
            mine += child([1], None)
        lo, hi = min(m[1] for m in other), max(m[2] for m in other)
        inside = all(lo <= m[0] <= hi for m in mine)
        text = ("single-face tracked step, %d rounds in turn, one process each (median ms per process):\n  %s: %s  (per-frame min %.3f - max %.3f)\n"
                "  in-tree: %s\n  every in-tree median inside the other library's min - max spread: %s\n" %
                (args.ab_rounds, args.ab_lib, " ".join("%.3f" % m[0] for m in other), lo, hi, " ".join("%.3f" % m[0] for m in mine), inside))
        print(text, end="")
        if args.out:
            with open(args.out, "a") as f:
                f.write(text)
        if not inside:
            raise SystemExit("the single-face tracked step left the other library's spread")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--frames", type=int, default=40, help="timed frames per case (>= 30)")
    ap.add_argument("--out", default=None, help="also write the report to this file")
    ap.add_argument("--measure", action="store_true", help="run the measurement in this process (what the driver starts)")
    ap.add_argument("--step-timeout", type=int, default=300, help="seconds the measuring step may take")
    ap.add_argument("--max-faces", default=None, help="K or K,K,...: time FaceTracker(max_faces=K) tracked steps alternated with the full grid")
    ap.add_argument("--ab-lib", default=None, help="with --max-faces: also K = 1 with this library against the in-tree one, in turn")
    ap.add_argument("--ab-rounds", type=int, default=3, help="rounds of the --ab-lib comparison")
    args = ap.parse_args()
    if args.frames < 30:
        ap.error("--frames must be at least 30")
    ks = [int(k) for k in args.max_faces.split(",")] if args.max_faces else []
    if any(k < 1 or k > 64 for k in ks):
        ap.error("--max-faces values must lie in 1..64")
    if args.measure:
        if ks:
            measure_multi(ks, args.frames, args.out)
        else:
            measure(args.frames, args.out)
        return
    if ks:
        multi_driver(args, ks)
        return
    # the driver: each GPU step a fresh child under its own time limit; the first failure ends the run
    steps = [["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--measure", "--frames", str(args.frames)] +
             (["--out", args.out] if args.out else [])]
    for cmd in steps:
        rc = subprocess.call(cmd, cwd=ROOT)
        if rc != 0:
            raise SystemExit("step failed with status %d: %s" % (rc, " ".join(cmd)))


if __name__ == "__main__":
    main()
