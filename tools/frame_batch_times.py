"""Time a stack of same-size frames through one pooled pass against the same frames one call each, on the frame leg's setup of bench.py.

    python tools/frame_batch_times.py [--calls 30] [--batches 1,2,4,8,16] [--runs 2] [--out profiles/r17_frame_batch.txt]

Synthetic 1920x1080 frames (one seed per frame) prescaled to 1000x562, smallest_face 0.1, the configs[2] cascade of bench.py's frame
leg and the U11L-64 eye stages, all as tools/tracking_times.py sets them up (its ``setup``).  For every B, alternated call by call,

  (a) B sequential ``detect_faces`` calls          (b) one ``detect_faces_frames`` call on the stack of the same B frames
  (c) B sequential ``detect_frame`` calls          (d) one ``detect_frames`` call

each timed on its own (every call is synchronous); the report gives the median per FRAME over --calls alternated calls after three
warm-up rounds, and checks once per B that the pooled answers are the per-frame answers.  --runs repeats the whole measurement in a fresh
process; the runs are reported one after the other.

Without --measure this is a driver: every measuring run is a child process under ``timeout -k 10``, and nothing runs after one fails."""
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

SF = 0.1
WARMUP = 3


def measure(batches, n_calls, out_path, run):
    import torch
    from pyfaceanalysis_amd import synth
    from tools.tracking_times import setup
    dev, frame0, pipe, (pw, ph), dc, loc, full, close = setup()
    frames = [frame0]
    for i in range(1, max(batches)):
        rng = np.random.default_rng(synth.INPUT_SEED + 7919 * i)
        frames.append(torch.from_numpy(np.rint(synth._box3(rng.integers(0, 256, (1080, 1920), dtype=np.uint8))).astype(np.uint8)).to(dev))
    lines = ["frame_batch_times run %d: 1920x1080 frames prescaled to %dx%d, %d windows a frame, smallest_face %.1f; device %s; medians per frame over "
             "%d alternated calls" % (run, pw, ph, full["n_windows"], SF, torch.cuda.get_device_name(dev), n_calls),
             "  B   faces: B x detect_faces   detect_faces_frames   ratio | detections: B x detect_frame   detect_frames   ratio   (ms per frame; faces kept)"]

    def timed(fn):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize(dev)
        return time.perf_counter() - t0, r

    for b in batches:
        stack = torch.stack(frames[:b])
        cases = [lambda: [dc.detect_faces(f, loc, smallest_face=SF) for f in frames[:b]], lambda: dc.detect_faces_frames(stack, loc, smallest_face=SF),
                 lambda: [dc.detect_frame(f, smallest_face=SF) for f in frames[:b]], lambda: dc.detect_frames(stack, smallest_face=SF)]
        ts = [[] for _ in cases]
        last = [None] * len(cases)
        for i in range(WARMUP + n_calls):
            for c, fn in enumerate(cases):
                t, last[c] = timed(fn)
                if i >= WARMUP:
                    ts[c].append(t)
        same = all(np.array_equal(x["faces"], y) for x, y in zip(last[0], last[1]["faces"])) and \
            all(np.array_equal(x[k], y[k]) for x, y in zip(last[2], last[3]["frames"]) for k in ("coords", "angles", "orig_index", "confidence"))
        if not same:
            raise SystemExit("B = %d: the pooled answers are not the per-frame answers" % b)
        med = [float(np.median(t)) * 1e3 / b for t in ts]
        lines.append(" %2d          %8.3f            %8.3f         %5.2f |                 %8.3f        %8.3f     %5.2f   (%d faces)" %
                     (b, med[0], med[1], med[0] / med[1], med[2], med[3], med[2] / med[3], sum(len(x) for x in last[1]["faces"])))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "a") as f:
            f.write(text)
    close()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--calls", type=int, default=30, help="timed alternated calls per case")
    ap.add_argument("--batches", default="1,2,4,8,16", help="stack sizes B, comma separated")
    ap.add_argument("--runs", type=int, default=2, help="repeat the measurement in this many fresh processes")
    ap.add_argument("--out", default=None, help="also append the report to this file")
    ap.add_argument("--measure", type=int, default=0, help="run the measurement in this process as run N (what the driver starts)")
    ap.add_argument("--step-timeout", type=int, default=400, help="seconds one measuring run may take")
    args = ap.parse_args()
    batches = [int(b) for b in args.batches.split(",")]
    if any(b < 1 or b > 64 for b in batches):
        ap.error("--batches values must lie in 1..64")
    if args.measure:
        measure(batches, args.calls, args.out, args.measure)
        return
    for run in range(1, args.runs + 1):      # each GPU step a fresh child under its own time limit; the first failure ends the run
        cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--measure", str(run), "--calls", str(args.calls),
               "--batches", args.batches] + (["--out", args.out] if args.out else [])
        rc = subprocess.call(cmd, cwd=ROOT)
        if rc != 0:
            raise SystemExit("step failed with status %d: %s" % (rc, " ".join(cmd)))


if __name__ == "__main__":
    main()
