"""Time age, race and gender estimation over a LIST of frames of different sizes in one pooled call against the same faces one frame per
call, on the setup of tools/estimate_frames_times.py.

    python tools/estimate_frame_list_times.py [--calls 30] [--batches 1,2,4,8,16] [--faces 1,4] [--runs 2] [--out profiles/r24_estimate_frame_list.txt]
    python tools/estimate_frame_list_times.py --default-paths [--ab-lib tools/ab/libhigsfa_base.so] [--pairs 3] [--out ...]

Synthetic frames of 1920 x 1080, 1280 x 720, 640 x 480 and 3648 x 2736 in turn (a folder of photographs), prescaled as the cascade
prescales them (``DeviceCascade.prescale_frame_list``, NEAREST, 1000 pixels: 1000 x 562, 1000 x 562, 640 x 480, 1000 x 750), the
reference's shape — 256 x 260 crops, a 96 x 96 patch under the default box, the linearPCANetworkU11L shape, three synthetic classifiers —
and the faces of tools/analysis_times.py scaled to each frame's own size.  For every B and every number of faces per frame, alternated
call by call,

  (a) B sequential ``estimate`` calls, one per frame          (b) one ``estimate_frame_list`` call on the list of the same B frames

each timed around the call (every call waits for its one read-back) and on the device between two events; the report gives the medians
over --calls alternated calls after three warm-up rounds and checks once per case that the pooled values are the per-frame values, bit
for bit.  Then B = 16 frames of ONE size (1000 x 562) through ``estimate_frame_list`` against ``estimate_frames`` on their stack: what the
list records cost.  --runs repeats the measurement in a fresh process.

--default-paths times what this feature must leave alone — the single-frame ``estimate`` at 1 and 64 faces, ``estimate_frames`` at B = 16
and ``detect_faces`` on bench.py's frame leg — in one process with the library ``HIGSFA_LIB`` selects (none of the list entries is
called); with --ab-lib the driver runs --pairs alternated pairs of processes, that library and the in-tree one (tools/build_ref_lib.sh).

Without --measure this is a driver: every measuring run is a child process under ``timeout -k 10``, and nothing runs after one fails."""
from __future__ import annotations

import argparse
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools.estimate_frames_times import FH, FW, VALUE_KEYS, WARMUP, report, rig, timed      # noqa: E402

SIZES = ((1920, 1080), (1280, 720), (640, 480), (3648, 2736))      # (width, height), in turn


def photo_list(torch, n_frames):
    """n_frames prescaled grey frames on the device, each a tensor of its own: one noise frame per size, rolled by the frame's number so
    that no two frames hold the same pixels, through a bare cascade's ``prescale_frame_list``."""
    from pyfaceanalysis_amd.cascade import DeviceCascade
    dc = DeviceCascade([], (64, 64), 20)
    base = [np.random.default_rng(4242 + i).integers(0, 256, (h, w), dtype=np.uint8) for i, (w, h) in enumerate(SIZES)]
    out = []
    for lo in range(0, n_frames, len(SIZES)):      # four frames at a time: a 3648 x 2736 frame is 10 MB
        full = [torch.from_numpy(np.roll(base[(lo + i) % len(SIZES)], 37 * (lo + i), axis=1)).cuda() for i in range(min(len(SIZES), n_frames - lo))]
        out += [s.clone() for s in dc.prescale_frame_list(full)]
    torch.cuda.synchronize()
    dc.close()
    return out


def scaled_faces(faces, m, rng, size):
    """m of tools/analysis_times.py's faces (made for 1000 x 562), scaled to a frame of ``size``."""
    e = faces(m, rng)
    return e * np.array([size[0] / FW, size[1] / FH, size[0] / FW, size[1] / FH])


def measure(batches, per_frame, n_calls, out_path, run):
    torch, frames, norm, fa, faces, close = rig(16)
    photos = photo_list(torch, max(batches))
    sizes = [(int(p.shape[1]), int(p.shape[0])) for p in photos]
    lines = ["estimate_frame_list_times run %d: frames of %s prescaled to %s in turn, crops 256x260, patches 96x96, U11L-96; device %s; medians over %d alternated calls"
             % (run, " / ".join("%dx%d" % s for s in SIZES), " / ".join("%dx%d" % s for s in sizes[:len(SIZES)]), torch.cuda.get_device_name(0), n_calls),
             "  B  faces/frame | B x estimate: around the calls   device | estimate_frame_list: around the call   device | ratio around   ratio device   (ms per LIST)"]

    def alternate(cases):
        ts = [([], []) for _ in cases]
        last = [None] * len(cases)
        for i in range(WARMUP + n_calls):
            for c, fn in enumerate(cases):
                call, device, last[c] = timed(torch, fn)
                if i >= WARMUP:
                    ts[c][0].append(call)
                    ts[c][1].append(device)
        return [[float(np.median(t)) for t in pair] for pair in ts], last
    for m in per_frame:
        for b in batches:
            rng = np.random.default_rng(1000 * m + b)
            geoms = [norm.geometry(scaled_faces(faces, m, rng, sizes[f]), sizes[f]) for f in range(b)]
            pooled = np.concatenate(geoms)
            ff = np.repeat(np.arange(b, dtype=np.int32), m)
            fl = photos[:b]
            med, last = alternate([lambda: [fa.estimate(fl[f], geoms=geoms[f]) for f in range(b)], lambda: fa.estimate_frame_list(fl, geoms=pooled, face_frame=ff)])
            for k in VALUE_KEYS:
                if not np.array_equal(np.concatenate([r[k] for r in last[0]]), last[1][k], equal_nan=True):
                    raise SystemExit("B = %d, %d faces a frame: the pooled %s is not the per-frame one" % (b, m, k))
            lines.append(" %2d      %2d       |            %8.3f        %8.3f |                      %8.3f        %8.3f |    %5.2f          %5.2f" %
                         (b, m, med[0][0], med[0][1], med[1][0], med[1][1], med[0][0] / med[1][0], med[0][1] / med[1][1]))
    lines.append("  16 frames of ONE size (%dx%d): estimate_frames on the stack | estimate_frame_list on the list of its frames | list / stack   (ms per call, around / device)" % (FW, FH))
    stack = torch.stack(frames[:16])
    for m in per_frame:
        rng = np.random.default_rng(5000 + m)
        pooled = np.concatenate([norm.geometry(faces(m, rng), (FW, FH)) for _ in range(16)])
        ff = np.repeat(np.arange(16, dtype=np.int32), m)
        med, last = alternate([lambda: fa.estimate_frames(stack, geoms=pooled, face_frame=ff), lambda: fa.estimate_frame_list(frames[:16], geoms=pooled, face_frame=ff)])
        for k in VALUE_KEYS:
            if not np.array_equal(last[0][k], last[1][k], equal_nan=True):
                raise SystemExit("one size, %d faces a frame: the list's %s is not the stack's" % (m, k))
        lines.append("     %2d faces/frame |            %8.3f / %8.3f |                  %8.3f / %8.3f |   %5.2f / %5.2f" %
                     (m, med[0][0], med[0][1], med[1][0], med[1][1], med[1][0] / med[0][0], med[1][1] / med[0][1]))
    report(lines, out_path)
    close()


def measure_default_paths(n_calls, out_path, label):
    """The paths this feature leaves alone, with whatever library HIGSFA_LIB selects."""
    from pyfaceanalysis_amd import _capi
    from tools.tracking_times import setup
    torch, frames, norm, fa, faces, close = rig(16)
    dev, frame0, pipe, (pw, ph), dc, loc, full, close_frame = setup()
    rng = np.random.default_rng(77)
    geoms = {n: norm.geometry(faces(n, rng), (FW, FH)) for n in (1, 64)}
    stack = torch.stack(frames)
    pooled = np.concatenate([norm.geometry(faces(4, rng), (FW, FH)) for _ in range(16)])
    ff = np.repeat(np.arange(16, dtype=np.int32), 4)
    cases = {"estimate, 1 face": lambda: fa.estimate(frames[0], geoms=geoms[1]), "estimate, 64 faces": lambda: fa.estimate(frames[0], geoms=geoms[64]),
             "estimate_frames, B = 16": lambda: fa.estimate_frames(stack, geoms=pooled, face_frame=ff),
             "detect_faces": lambda: dc.detect_faces(frame0, loc, smallest_face=0.1)}
    ts = {k: ([], []) for k in cases}
    for i in range(WARMUP + n_calls):
        for k, fn in cases.items():
            call, device, _ = timed(torch, fn)
            if i >= WARMUP:
                ts[k][0].append(call)
                ts[k][1].append(device)
    lines = ["default paths, %s (%s): medians over %d alternated calls, ms around the call / device" % (label, os.path.relpath(_capi._LIB_PATH, ROOT), n_calls)]
    lines += ["  %-24s %8.4f / %8.4f" % (k, np.median(ts[k][0]), np.median(ts[k][1])) for k in cases]
    report(lines, out_path)
    close_frame()
    close()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--calls", type=int, default=30, help="timed alternated calls per case")
    ap.add_argument("--batches", default="1,2,4,8,16", help="list lengths B, comma separated")
    ap.add_argument("--faces", default="1,4", help="faces per frame, comma separated")
    ap.add_argument("--runs", type=int, default=2, help="repeat the measurement in this many fresh processes")
    ap.add_argument("--out", default=None, help="also append the report to this file")
    ap.add_argument("--default-paths", action="store_true", help="time the paths the feature leaves alone instead (see above)")
    ap.add_argument("--ab-lib", default=None, help="with --default-paths: another build of the library to alternate with the in-tree one")
    ap.add_argument("--pairs", type=int, default=3, help="alternated pairs of processes with --ab-lib")
    ap.add_argument("--measure", type=int, default=0, help="run the measurement in this process as run N (what the driver starts)")
    ap.add_argument("--label", default="in-tree", help="names the library in a --default-paths report")
    ap.add_argument("--step-timeout", type=int, default=300, help="seconds one measuring run may take")
    args = ap.parse_args()
    batches = [int(b) for b in args.batches.split(",")]
    per_frame = [int(m) for m in args.faces.split(",")]
    if any(b < 1 or b > 64 for b in batches) or any(m < 1 or m > 64 for m in per_frame):
        ap.error("--batches and --faces values must lie in 1..64")
    if args.measure:
        if args.default_paths:
            measure_default_paths(args.calls, args.out, args.label)
        else:
            measure(batches, per_frame, args.calls, args.out, args.measure)
        return
    base = [sys.executable, os.path.abspath(__file__), "--calls", str(args.calls)] + (["--out", args.out] if args.out else [])
    steps = []
    if args.default_paths:
        for pair in range(1, args.pairs + 1 if args.ab_lib else 2):
            if args.ab_lib:
                steps.append((base + ["--default-paths", "--measure", str(pair), "--label", "the other library"], os.path.abspath(args.ab_lib)))
            steps.append((base + ["--default-paths", "--measure", str(pair), "--label", "in-tree"], None))
    else:
        steps = [(base + ["--measure", str(run), "--batches", args.batches, "--faces", args.faces], None) for run in range(1, args.runs + 1)]
    for cmd, lib in steps:      # each GPU step a fresh child under its own time limit; the first failure ends the run
        env = dict(os.environ)
        env.pop("HIGSFA_LIB", None)
        if lib:
            env["HIGSFA_LIB"] = lib
        rc = subprocess.call(["timeout", "-k", "10", str(args.step_timeout)] + cmd, cwd=ROOT, env=env)
        if rc != 0:
            raise SystemExit("step failed with status %d: %s" % (rc, " ".join(cmd)))


if __name__ == "__main__":
    main()
