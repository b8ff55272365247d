"""Time age, race and gender estimation over a stack of frames in one pooled call against the same faces one frame per call, on the setup
of tools/analysis_times.py.

    python tools/estimate_frames_times.py [--calls 30] [--batches 1,2,4,8,16] [--faces 1,4] [--runs 2] [--out profiles/r21_estimate_frames.txt]
    python tools/estimate_frames_times.py --default-paths [--ab-lib tools/ab/libhigsfa_base.so] [--pairs 3] [--out ...]

Synthetic 1000 x 562 frames (one seed per frame; the prescaled frame of BASELINE.json configs[2]), the reference's shape — 256 x 260 crops, a
96 x 96 patch under the default box, the linearPCANetworkU11L shape (tests/helpers.linear_u11l_96, random weights), three synthetic
classifiers — and the faces of tools/analysis_times.py (eye distances 8 .. 150 pixels, every fourth face at the border).  For every B and
every number of faces per frame, alternated call by call,

  (a) B sequential ``estimate`` calls, one per frame          (b) one ``estimate_frames`` call on the stack of the same B frames

each timed around the call (every call waits for its one read-back) and on the device between two events; the report gives the medians
over --calls alternated calls after three warm-up rounds and checks once per case that the pooled values are the per-frame values, bit
for bit.  --runs repeats the measurement in a fresh process.

--default-paths times what this feature must leave alone — the single-frame ``estimate`` at 1 and 64 faces, ``normalize`` at 16 faces
and ``detect_faces`` on bench.py's frame leg — in one process with the library ``HIGSFA_LIB`` selects (none of the stack entries is
called); with --ab-lib the driver runs --pairs alternated pairs of processes, that library and the in-tree one (tools/build_ref_lib.sh).

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

FW, FH = 1000, 562
WARMUP = 3
VALUE_KEYS = ("age", "age_std", "race", "gender")


def rig(n_frames):
    """The frames on the device, the flow, the classifiers and an analyzer of tools/analysis_times.py's shape."""
    import torch
    from pyfaceanalysis_amd import analysis as A, normalize as N, synth
    from pyfaceanalysis_amd.flow import Flow
    from tests import analysis_cases as AC, helpers
    from tools.analysis_times import faces
    frames = []
    for i in range(n_frames):
        rng = np.random.default_rng(synth.INPUT_SEED + 7919 * i)
        frames.append(torch.from_numpy(np.rint(synth._box3(rng.integers(0, 256, (FH, FW), dtype=np.uint8))).astype(np.uint8)).cuda())
    flow = Flow(helpers.linear_u11l_96(0), output_dtype=np.float32)
    norm = N.FaceNormalizer(0, preset="age")
    rng = np.random.default_rng(synth.INPUT_SEED)
    crops = norm.normalize(frames[0], faces(16, rng))[0]
    feats = flow.execute(AC.patch_oracle(crops.cpu().numpy(), (96, 96), A.age_patch_box(), 0, AC.CONTRAST))
    clfs = AC.classifiers(feats, (30, 12, 8), seed=21)
    fa = A.FaceAnalyzer(flow, *clfs, contrast=AC.CONTRAST)

    def close():
        torch.cuda.synchronize()
        fa.close()
        for c in clfs:
            c.close()
        norm.close()
        flow.close()
    return torch, frames, norm, fa, faces, close


def timed(torch, fn):
    """(seconds around the call, device milliseconds between two events, result)."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    t0 = time.perf_counter()
    r = fn()
    call = time.perf_counter() - t0
    e1.record()
    e1.synchronize()
    return call * 1e3, e0.elapsed_time(e1), r


def report(lines, out_path):
    text = "\n".join(lines) + "\n"
    print(text, end="", flush=True)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "a") as f:
            f.write(text)


def measure(batches, per_frame, n_calls, out_path, run):
    torch, frames, norm, fa, faces, close = rig(max(batches))
    lines = ["estimate_frames_times run %d: %dx%d frames, crops 256x260, patches 96x96, U11L-96; device %s; medians over %d alternated calls"
             % (run, FW, FH, torch.cuda.get_device_name(0), n_calls),
             "  B  faces/frame | B x estimate: around the calls   device | estimate_frames: around the call   device | ratio around   ratio device   (ms per STACK)"]
    for m in per_frame:
        for b in batches:
            rng = np.random.default_rng(1000 * m + b)
            geoms = [norm.geometry(faces(m, rng), (FW, FH)) for _ in range(b)]
            pooled = np.concatenate(geoms)
            ff = np.repeat(np.arange(b, dtype=np.int32), m)
            stack = torch.stack(frames[:b])
            cases = [lambda: [fa.estimate(frames[f], geoms=geoms[f]) for f in range(b)], lambda: fa.estimate_frames(stack, geoms=pooled, face_frame=ff)]
            ts = [([], []) for _ in cases]
            last = [None, None]
            for i in range(WARMUP + n_calls):
                for c, fn in enumerate(cases):
                    call, device, last[c] = timed(torch, fn)
                    if i >= WARMUP:
                        ts[c][0].append(call)
                        ts[c][1].append(device)
            for k in VALUE_KEYS:
                if not np.array_equal(np.concatenate([r[k] for r in last[0]]), last[1][k], equal_nan=True):
                    raise SystemExit("B = %d, %d faces a frame: the pooled %s is not the per-frame one" % (b, m, k))
            med = [[float(np.median(t)) for t in pair] for pair in ts]
            lines.append(" %2d      %2d       |            %8.3f        %8.3f |                  %8.3f        %8.3f |    %5.2f          %5.2f" %
                         (b, m, med[0][0], med[0][1], med[1][0], med[1][1], med[0][0] / med[1][0], med[0][1] / med[1][1]))
    report(lines, out_path)
    close()


def measure_default_paths(n_calls, out_path, label):
    """The paths this feature leaves alone, with whatever library HIGSFA_LIB selects."""
    from pyfaceanalysis_amd import _capi
    from tools.tracking_times import setup
    torch, frames, norm, fa, faces, close = rig(1)
    dev, frame0, pipe, (pw, ph), dc, loc, full, close_frame = setup()
    rng = np.random.default_rng(77)
    geoms = {n: norm.geometry(faces(n, rng), (FW, FH)) for n in (1, 16, 64)}
    out16 = torch.empty((16, 260, 256), dtype=torch.uint8, device="cuda")
    cases = {"estimate, 1 face": lambda: fa.estimate(frames[0], geoms=geoms[1]), "estimate, 64 faces": lambda: fa.estimate(frames[0], geoms=geoms[64]),
             "normalize, 16 faces": lambda: norm.normalize(frames[0], geoms=geoms[16], out=out16), "detect_faces": lambda: dc.detect_faces(frame0, loc, smallest_face=0.1)}
    ts = {k: ([], []) for k in cases}
    for i in range(WARMUP + n_calls):
        for k, fn in cases.items():
            call, device, _ = timed(torch, fn)
            if i >= WARMUP:
                ts[k][0].append(call)
                ts[k][1].append(device)
    lines = ["default paths, %s (%s): medians over %d alternated calls, ms around the call / device" % (label, os.path.relpath(_capi._LIB_PATH, ROOT), n_calls)]
    lines += ["  %-20s %8.4f / %8.4f" % (k, np.median(ts[k][0]), np.median(ts[k][1])) for k in cases]
    report(lines, out_path)
    close_frame()
    close()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--calls", type=int, default=30, help="timed alternated calls per case")
    ap.add_argument("--batches", default="1,2,4,8,16", help="stack sizes B, comma separated")
    ap.add_argument("--faces", default="1,4", help="faces per frame, comma separated")
    ap.add_argument("--runs", type=int, default=2, help="repeat the measurement in this many fresh processes")
    ap.add_argument("--out", default=None, help="also append the report to this file")
    ap.add_argument("--default-paths", action="store_true", help="time the single-frame paths instead (see above)")
    ap.add_argument("--ab-lib", default=None, help="with --default-paths: another build of the library to alternate with the in-tree one")
    ap.add_argument("--pairs", type=int, default=3, help="alternated pairs of processes with --ab-lib")
    ap.add_argument("--in-tree-first", action="store_true", help="with --ab-lib: the in-tree library runs first in every pair")
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
            both = [(base + ["--default-paths", "--measure", str(pair), "--label", "in-tree"], None)]
            if args.ab_lib:
                both.insert(0, (base + ["--default-paths", "--measure", str(pair), "--label", "the other library"], os.path.abspath(args.ab_lib)))
            steps += both[::-1] if args.in_tree_first else both
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
