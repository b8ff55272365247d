"""Time a pooled tracked step over B frame streams against B sequential FaceTracker steps, on the frame leg's setup of bench.py.

    python tools/stream_set_times.py [--calls 30] [--runs 2] [--out profiles/r22_stream_set.txt]
    python tools/stream_set_times.py --default-paths --ab-lib tools/ab/libhigsfa_parent.so [--pairs 3] [--out ...]

tools/tracking_times.py's rig: one synthetic 1920x1080 frame prescaled to 1000x562, smallest_face 0.1, the configs[2] cascade of
bench.py's frame leg (U11L-128 x 4, 128x128 sub-images, 17 stages) and U11L-64 eye stages.  Every stream is fed that frame.

For B = 1 / 2 / 4 / 8 / 16 streams holding K = 1 and 4 faces each: ``StreamSetTracker(n_streams=B, max_faces=K).step`` on a step where
every stream is tracked (9 B K windows in one pass, one host wait) ALTERNATED call by call with B ``FaceTracker(max_faces=K).step`` calls
one after the other on the same cascade and eye handles (9 K windows and one wait each).  Every timed call follows an untimed reset +
full-grid step, so each one tracks the frame's first K faces.  Milliseconds per FRAME (the call's time / B), medians over --calls
alternated calls after 10 warm-up calls, --runs fresh processes.  The results of the two are compared (array_equal) on the last call.
Then a MIXED step at every B > 1: stream 0 reset before the timed call, so the call runs the full-grid pass on one frame and the tracked
pass on B - 1; against one full-grid and B - 1 tracked FaceTracker steps.

--default-paths: what this feature leaves alone — ``detect_faces`` and a single ``FaceTracker`` tracked step (medians over --calls
alternated calls) and ``bench.py --gpus 1 --steps 300 --warmup 50`` — with the library HIGSFA_LIB selects; with --ab-lib PATH
(tools/build_ref_lib.sh) in --pairs alternated pairs of processes, the other library and the in-tree one, and a verdict: every in-tree
figure inside the other library's min - max over its own processes.

Without --measure this is a driver: every measuring step is a child process under ``timeout -k 10``, and nothing runs after a step that
fails."""
from __future__ import annotations

import argparse
import json
import os
import re
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SF, WARMUP = 0.1, 10
KEYS = ("faces", "tracked", "n_windows", "n_before_purge", "slots", "n_held")


def report(lines, out_path):
    text = "\n".join(lines) + "\n"
    print(text, end="", flush=True)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "a") as f:
            f.write(text)


def timed(torch, dev, fn):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t0) * 1e3, r


def measure(batches, faces, n_calls, out_path, run):
    import torch
    from pyfaceanalysis_amd.tracking import FaceTracker, StreamSetTracker
    from tools.tracking_times import setup
    dev, frame, pipe, (pw, ph), dc, loc, full, close = setup()
    lines = ["stream_set_times run %d: 1920x1080 frames prescaled to %dx%d, full grid %d windows, %d faces; device %s; medians over %d alternated calls, ms per FRAME"
             % (run, pw, ph, full["n_windows"], len(full["faces"]), torch.cuda.get_device_name(dev), n_calls),
             "  B  K  windows | B x FaceTracker.step   StreamSetTracker.step   ratio |  mixed (stream 0 on the grid): sequential   pooled   ratio"]
    for k in faces:
        for b in batches:
            stack = frame[None].expand(b, -1, -1).contiguous()
            single = [FaceTracker(dc, loc, smallest_face=SF, max_faces=k) for _ in range(b)]
            pooled = StreamSetTracker(dc, loc, b, smallest_face=SF, max_faces=k)

            def arm(mixed):      # untimed: forget, find the faces again on the full grid; mixed: stream 0 forgets once more
                pooled.reset()
                r = pooled.step(stack)
                assert r["n_grid"] == b
                for tr in single:
                    tr.reset()
                    assert not tr.step(frame)["tracked"]
                if mixed:
                    pooled.reset(0)
                    single[0].reset()

            ts = {False: ([], []), True: ([], [])}
            windows = 0
            for mixed in ((False, True) if b > 1 else (False,)):
                for i in range(WARMUP + n_calls):
                    arm(mixed)
                    t_seq, seq = timed(torch, dev, lambda: [tr.step(frame) for tr in single])
                    arm(mixed)
                    t_pool, got = timed(torch, dev, lambda: pooled.step(stack))
                    if i >= WARMUP:
                        ts[mixed][0].append(t_seq / b)
                        ts[mixed][1].append(t_pool / b)
                assert got["n_grid"] == (1 if mixed else 0) and got["n_tracked"] == b - got["n_grid"]
                for s in range(b):
                    for key in KEYS:
                        if key in seq[s] and not np.array_equal(got["streams"][s][key], seq[s][key]):      # (max_faces = 1: no slots, no n_held)
                            raise SystemExit("B = %d, K = %d, stream %d: the pooled %s is not the tracker's" % (b, k, s, key))
                if not mixed:
                    windows = sum(st["n_windows"] for st in got["streams"])
            med = {m: [float(np.median(t)) if t else float("nan") for t in ts[m]] for m in ts}
            line = " %2d %2d   %5d  |       %8.3f               %8.3f         %5.2f  |" % (b, k, windows, med[False][0], med[False][1], med[False][0] / med[False][1])
            if b > 1:
                line += "                               %8.3f %8.3f   %5.2f" % (med[True][0], med[True][1], med[True][0] / med[True][1])
            lines.append(line)
            print("RESULT b=%d k=%d seq_ms=%.4f pooled_ms=%.4f" % (b, k, med[False][0], med[False][1]), flush=True)
            pooled.close()
            for tr in single:
                tr.close()
    report(lines, out_path)
    close()


def measure_default_paths(n_calls, out_path, label):
    """The paths this feature leaves alone, with whatever library HIGSFA_LIB selects."""
    import torch
    from pyfaceanalysis_amd import _capi
    from pyfaceanalysis_amd.tracking import FaceTracker
    from tools.tracking_times import setup
    dev, frame, pipe, (pw, ph), dc, loc, full, close = setup()
    tr = FaceTracker(dc, loc, smallest_face=SF)
    t_full, t_tracked = [], []
    for i in range(WARMUP + n_calls):
        t, f = timed(torch, dev, lambda: dc.detect_faces(frame, loc, smallest_face=SF))
        tr.reset()
        assert not tr.step(frame)["tracked"]
        t2, r = timed(torch, dev, lambda: tr.step(frame))
        assert r["tracked"] and np.array_equal(f["faces"], full["faces"])
        if i >= WARMUP:
            t_full.append(t)
            t_tracked.append(t2)
    tr.close()
    close()
    lib = os.path.relpath(_capi._LIB_PATH, ROOT)
    report(["default paths, %s (%s): medians over %d alternated calls, ms" % (label, lib, n_calls),
            "  detect_faces            %8.4f" % np.median(t_full), "  FaceTracker tracked step %7.4f" % np.median(t_tracked)], out_path)
    print("RESULT detect_faces_ms=%.5f tracked_ms=%.5f" % (np.median(t_full), np.median(t_tracked)), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--calls", type=int, default=30, help="timed alternated calls per case")
    ap.add_argument("--batches", default="1,2,4,8,16", help="stream counts B, comma separated")
    ap.add_argument("--faces", default="1,4", help="faces held per stream, comma separated")
    ap.add_argument("--runs", type=int, default=2, help="repeat the measurement in this many fresh processes")
    ap.add_argument("--out", default=None, help="also append the report to this file")
    ap.add_argument("--default-paths", action="store_true", help="time detect_faces, a FaceTracker step and bench.py instead (see above)")
    ap.add_argument("--ab-lib", default=None, help="with --default-paths: another build of the library to alternate with the in-tree one")
    ap.add_argument("--pairs", type=int, default=3, help="alternated pairs of processes with --ab-lib")
    ap.add_argument("--measure", type=int, default=0, help="run the measurement in this process as run N (what the driver starts)")
    ap.add_argument("--label", default="in-tree", help="names the library in a --default-paths report")
    ap.add_argument("--step-timeout", type=int, default=300, help="seconds one measuring run may take")
    args = ap.parse_args()
    batches = [int(b) for b in args.batches.split(",")]
    faces = [int(m) for m in args.faces.split(",")]
    if any(b < 1 or b > 64 for b in batches) or any(m < 1 or m > 64 for m in faces):
        ap.error("--batches and --faces values must lie in 1..64")
    if args.measure:
        if args.default_paths:
            measure_default_paths(args.calls, args.out, args.label)
        else:
            measure(batches, faces, args.calls, args.out, args.measure)
        return
    out = ["--out", args.out] if args.out else []
    base = [sys.executable, os.path.abspath(__file__), "--calls", str(args.calls)] + out

    def child(cmd, lib):      # a fresh child under its own time limit; the first failure ends the run
        env = dict(os.environ)
        env.pop("HIGSFA_LIB", None)
        if lib:
            env["HIGSFA_LIB"] = os.path.abspath(lib)
        r = subprocess.run(["timeout", "-k", "10", str(args.step_timeout)] + cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, text=True)
        sys.stdout.write(r.stdout)
        sys.stdout.flush()
        if r.returncode != 0:
            raise SystemExit("step failed with status %d: %s" % (r.returncode, " ".join(cmd)))
        return r.stdout

    if not args.default_paths:
        for run in range(1, args.runs + 1):
            child(base + ["--measure", str(run), "--batches", args.batches, "--faces", args.faces], None)
        return
    figures = {"other": [], "in-tree": []}
    for pair in range(1, args.pairs + 1 if args.ab_lib else 2):
        for label, lib in ((("other", args.ab_lib),) if args.ab_lib else ()) + (("in-tree", None),):
            text = child(base + ["--default-paths", "--measure", str(pair), "--label", "the other library" if lib else "in-tree"], lib)
            m = re.search(r"RESULT detect_faces_ms=(\S+) tracked_ms=(\S+)", text)
            bench = child([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "300", "--warmup", "50"], lib)
            value = [json.loads(ln)["value"] for ln in bench.splitlines() if ln.startswith('{"metric"')][-1]
            figures[label].append((float(m.group(1)), float(m.group(2)), float(value)))
            report(["  bench.py, %s, pair %d: %.0f sub-images/s" % (label, pair, value)], args.out)
    if args.ab_lib:
        names = ("detect_faces ms", "FaceTracker tracked step ms", "bench.py sub-images/s")
        lines, inside = ["default paths, %d alternated pairs of processes (%s / in-tree):" % (args.pairs, args.ab_lib)], True
        for j, name in enumerate(names):
            other, mine = [f[j] for f in figures["other"]], [f[j] for f in figures["in-tree"]]
            # the other library's own spread, widened by nothing: a figure that is BETTER than all of the other's is inside as well
            better = (lambda v: v <= max(other)) if j < 2 else (lambda v: v >= min(other))
            ok = all(better(v) for v in mine)
            inside = inside and ok
            lines.append("  %-28s other %s | in-tree %s | no in-tree figure worse than the other's worst: %s" %
                         (name, " ".join("%.4g" % v for v in other), " ".join("%.4g" % v for v in mine), ok))
        report(lines, args.out)
        if not inside:
            raise SystemExit("a default path left the other library's spread")


if __name__ == "__main__":
    main()
