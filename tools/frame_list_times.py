"""Time a LIST of frames of different sizes through one pooled pass against the same frames one call each, on the frame leg's setup of bench.py.

    python tools/frame_list_times.py [--calls 30] [--batches 2,4,8,16] [--runs 2] [--out profiles/r23_frame_list.txt] [--parent-lib PATH]

Synthetic frames (one seed per frame) of four sizes in turn — 1920x1080, 1280x720, 640x480, 3648x2736 — smallest_face 0.1, the configs[2]
cascade of bench.py's frame leg and the U11L-64 eye stages, all as tools/tracking_times.py sets them up (its ``setup``).  Alternated call
by call, each timed on its own (every call is synchronous), medians over --calls alternated calls after three warm-up rounds:

  (a) for every B: B sequential ``detect_faces`` calls against one ``detect_faces_frame_list`` call on the same B frames (ms per frame)
  (b) 16 frames of 1920x1080: ``detect_faces_frame_list`` against ``detect_faces_frames`` on the stack
  (c) with --parent-lib (the library of the parent commit, tools/build_ref_lib.sh): the default path on this library and on that one as
      alternated pairs of processes — bench.py's value, ``detect_faces``, ``detect_faces_frames`` at B = 16 and one ``FaceTracker``
      tracked step (the step after a full-grid step that found a face); both spreads and medians per item at the end

and checks once per case that the pooled answers are the per-frame answers.  --runs repeats (a) and (b) in a fresh process.

Without --measure this is a driver: every measuring run is a child process under ``timeout -k 10``, and nothing runs after one fails."""
from __future__ import annotations

import argparse
import json
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
SIZES = ((1920, 1080), (1280, 720), (640, 480), (3648, 2736))


def noise(dev, w, h, seed):
    import torch
    from pyfaceanalysis_amd import synth
    rng = np.random.default_rng(seed)
    return torch.from_numpy(np.rint(synth._box3(rng.integers(0, 256, (h, w), dtype=np.uint8))).astype(np.uint8)).to(dev)


def alternate(dev, cases, n_calls):
    """Medians (seconds) of the cases called in turn, and each case's last result."""
    import torch
    ts, last = [[] for _ in cases], [None] * len(cases)
    for i in range(WARMUP + n_calls):
        for c, fn in enumerate(cases):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            last[c] = fn()
            torch.cuda.synchronize(dev)
            if i >= WARMUP:
                ts[c].append(time.perf_counter() - t0)
    return [float(np.median(t)) for t in ts], last


def measure(batches, n_calls, out_path, run, default_path):
    import torch
    from pyfaceanalysis_amd import synth
    from tools.tracking_times import setup
    dev, frame0, pipe, (pw, ph), dc, loc, full, close = setup()
    lines = []
    if default_path:      # (c): one process of a pair — detect_faces, detect_faces_frames at B = 16 and one tracked step on whichever library is loaded
        from pyfaceanalysis_amd.tracking import FaceTracker
        hd = [frame0] + [noise(dev, 1920, 1080, synth.INPUT_SEED + 7919 * i) for i in range(1, 16)]
        stack = torch.stack(hd)
        tr = FaceTracker(dc, loc, smallest_face=SF)
        tracked = []

        def tracked_step():      # untimed: forget and find the face again on the full grid; timed inside: the tracked step that follows
            tr.reset()
            assert not tr.step(frame0)["tracked"]
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            r = tr.step(frame0)
            torch.cuda.synchronize(dev)
            tracked.append(time.perf_counter() - t0)
            assert r["tracked"]
        med, _ = alternate(dev, [lambda: dc.detect_faces(frame0, loc, smallest_face=SF), lambda: dc.detect_faces_frames(stack, loc, smallest_face=SF), tracked_step],
                           n_calls)
        print(json.dumps(dict(detect_faces_ms=med[0] * 1e3, detect_faces_frames_16_ms_per_frame=med[1] * 1e3 / 16,
                              tracked_step_ms=float(np.median(tracked[WARMUP:])) * 1e3)))
        tr.close()
        close()
        return
    lines.append("frame_list_times run %d: smallest_face %.1f; device %s; medians over %d alternated calls" % (run, SF, torch.cuda.get_device_name(dev), n_calls))
    lines.append("(a) frames of %s in turn;  B   B x detect_faces   detect_faces_frame_list   ratio   (ms per frame; windows; faces kept)" %
                 ", ".join("%dx%d" % s for s in SIZES))
    frames = [noise(dev, *SIZES[i % len(SIZES)], synth.INPUT_SEED + 7919 * (i + 1)) for i in range(max(batches + [1]))]
    for b in batches:
        fl = frames[:b]
        med, last = alternate(dev, [lambda: [dc.detect_faces(f, loc, smallest_face=SF) for f in fl], lambda: dc.detect_faces_frame_list(fl, loc, smallest_face=SF)],
                              n_calls)
        if not all(np.array_equal(x["faces"], y) for x, y in zip(last[0], last[1]["faces"])):
            raise SystemExit("B = %d: the list's answers are not the per-frame answers" % b)
        lines.append("    %2d        %8.3f              %8.3f           %5.2f   (%d windows, %d faces)" %
                     (b, med[0] * 1e3 / b, med[1] * 1e3 / b, med[0] / med[1], last[1]["n_windows"], sum(len(x) for x in last[1]["faces"])))
    hd = [frame0] + [noise(dev, 1920, 1080, synth.INPUT_SEED + 7919 * i) for i in range(1, 16)]
    stack = torch.stack(hd)
    med, last = alternate(dev, [lambda: dc.detect_faces_frames(stack, loc, smallest_face=SF), lambda: dc.detect_faces_frame_list(hd, loc, smallest_face=SF)], n_calls)
    if not all(np.array_equal(x, y) for x, y in zip(last[0]["faces"], last[1]["faces"])):
        raise SystemExit("16 same-size frames: the list's answers are not the stack's")
    lines.append("(b) 16 frames of 1920x1080:  detect_faces_frames (stack) %.3f   detect_faces_frame_list %.3f   ms per frame; list / stack = %.3f" %
                 (med[0] * 1e3 / 16, med[1] * 1e3 / 16, med[1] / med[0]))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "a") as f:
            f.write(text)
    close()


def child(cmd, env=None, timeout=400):
    """One GPU step: a fresh child process under its own time limit; its last JSON line, or the end of the run."""
    full = ["timeout", "-k", "10", str(timeout)] + cmd
    p = subprocess.run(full, cwd=ROOT, env=env, stdout=subprocess.PIPE, universal_newlines=True)
    if p.returncode != 0:
        raise SystemExit("step failed with status %d: %s" % (p.returncode, " ".join(full)))
    rows = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    return json.loads(rows[-1]) if rows else None


def pairs(parent_lib, n_pairs, n_calls, out_path):
    """(c): the default path on this library and on the parent commit's, as alternated pairs of processes."""
    me = [sys.executable, os.path.abspath(__file__), "--measure", "1", "--default-path", "--calls", str(n_calls)]
    bench = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "30", "--warmup", "5"]
    env_parent = dict(os.environ, HIGSFA_LIB=os.path.abspath(parent_lib))
    rows = {}
    for _ in range(n_pairs):
        for name, env in (("parent", env_parent), ("this", None)):
            b = child(bench, env)
            d = child(me, env)
            rows.setdefault(name, []).append((b.get("value"), d["detect_faces_ms"], d["detect_faces_frames_16_ms_per_frame"], d["tracked_step_ms"]))
    lines = ["(c) the default path, %d alternated pairs of processes (parent commit's library, this one): bench.py value (%s), detect_faces ms, "
             "detect_faces_frames at B = 16 ms per frame, one FaceTracker tracked step ms" % (n_pairs, "higher is better")]
    for name in ("parent", "this"):
        for r in rows[name]:
            lines.append("    %-6s  bench %.4e   detect_faces %.3f   detect_faces_frames %.3f   tracked step %.3f" % ((name, r[0]) + r[1:]))
    names = ("bench.py", "detect_faces", "detect_faces_frames", "tracked step")
    for i, what in enumerate(names):
        p, t = [r[i] for r in rows["parent"]], [r[i] for r in rows["this"]]
        lines.append("    %-20s parent %.5g .. %.5g (median %.5g)   this %.5g .. %.5g (median %.5g)" %
                     (what, min(p), max(p), float(np.median(p)), min(t), max(t), float(np.median(t))))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if out_path:
        with open(out_path, "a") as f:
            f.write(text)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--calls", type=int, default=30, help="timed alternated calls per case")
    ap.add_argument("--batches", default="2,4,8,16", help="list lengths B, comma separated")
    ap.add_argument("--runs", type=int, default=2, help="repeat (a) and (b) in this many fresh processes")
    ap.add_argument("--out", default=None, help="also append the report to this file")
    ap.add_argument("--parent-lib", default=None, help="(c): the parent commit's libhigsfa.so")
    ap.add_argument("--pairs", type=int, default=3, help="(c): alternated pairs of processes")
    ap.add_argument("--measure", type=int, default=0, help="run the measurement in this process as run N (what the driver starts)")
    ap.add_argument("--default-path", action="store_true", help="with --measure: time the default path only and print one JSON line")
    ap.add_argument("--step-timeout", type=int, default=400, help="seconds one measuring run may take")
    args = ap.parse_args()
    batches = [int(b) for b in args.batches.split(",")]
    if any(b < 1 or b > 64 for b in batches):
        ap.error("--batches values must lie in 1..64")
    if args.measure:
        measure(batches, args.calls, args.out, args.measure, args.default_path)
        return
    for run in range(1, args.runs + 1):      # each GPU step a fresh child under its own time limit; the first failure ends the run
        cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--measure", str(run), "--calls", str(args.calls),
               "--batches", args.batches] + (["--out", args.out] if args.out else [])
        rc = subprocess.call(cmd, cwd=ROOT)
        if rc != 0:
            raise SystemExit("step failed with status %d: %s" % (rc, " ".join(cmd)))
    if args.parent_lib:
        pairs(args.parent_lib, args.pairs, args.calls, args.out)


if __name__ == "__main__":
    main()
