"""What age, race and gender estimation costs on the device (analysis.FaceAnalyzer, hg_estimator_estimate_device) on a 1000 x 562 frame —
the prescaled frame of BASELINE.json configs[2], the one the rows of detect_faces refer to — for 1 / 4 / 16 / 64 faces, the reference's
shape: 256 x 260 crops, a 96 x 96 patch under the default box, the linearPCANetworkU11L shape (tests/helpers.linear_u11l_96, random
weights) and three synthetic classifiers.  Three questions:

  the whole call     ``estimate`` from the call to the returned dict (it waits for its one read-back), and the device time between two events
  the patch step     the fused kernel (flag bit 1) against the composed path (flag bit 0: hg_patcher_extract_filter_device per face, then the
                     contrast kernel) for NEAREST, BILINEAR and BICUBIC, device time of ``patches`` on the crops of those faces
  normalise's share  the device time of ``FaceNormalizer.normalize`` on the same faces over the device time of the chain

One process, the variants alternated call by call; minimum, median and maximum over --reps calls each, appended to --out with the library
that was loaded.  Every timed configuration is checked first: the patches of its first face against PIL and the restated contrast.

    python tools/analysis_times.py [--reps 30] [--label this] [--out profiles/r16_analysis_times.txt] [--patches-only]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pyfaceanalysis_amd import _capi, analysis as A, normalize as N, synth  # noqa: E402
from pyfaceanalysis_amd.flow import Flow  # noqa: E402
from tests import analysis_cases as AC, helpers  # noqa: E402

FW, FH = 1000, 562
COUNTS = (1, 4, 16, 64)


def stats(ms):
    return "min %.4f  median %.4f  max %.4f ms" % (np.min(ms), np.median(ms), np.max(ms))


def faces(n, rng, lo=8.0, hi=150.0):
    """n eye rows: eye distances geometric in [lo, hi] pixels, tilts in +-25 degrees, every fourth face centred within 20 pixels of a
    frame edge (tools/normalize_times.py)."""
    dist = np.exp(np.linspace(np.log(lo), np.log(hi), n)) if n > 1 else np.array([60.0])
    rng.shuffle(dist)
    ang = np.radians(rng.uniform(-25.0, 25.0, n))
    cx, cy = rng.uniform(0.15 * FW, 0.85 * FW, n), rng.uniform(0.15 * FH, 0.7 * FH, n)
    cx[3::4] = rng.choice([rng.uniform(0, 20), rng.uniform(FW - 20, FW)], len(cx[3::4]))
    dx, dy = dist / 2 * np.cos(ang), dist / 2 * np.sin(ang)
    return np.stack([cx - dx, cy - dy, cx + dx, cy + dy], axis=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--label", default="this build")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r16_analysis_times.txt"))
    ap.add_argument("--patches-only", action="store_true", help="the patch step alone (a build with another workgroup size)")
    a = ap.parse_args()
    if a.reps < 30:
        ap.error("--reps must be at least 30")
    rng = np.random.default_rng(synth.INPUT_SEED)
    frame = np.rint(synth._box3(rng.integers(0, 256, (FH, FW), dtype=np.uint8))).astype(np.uint8)
    fdev = torch.from_numpy(frame).cuda()
    flow = Flow(helpers.linear_u11l_96(0), output_dtype=np.float32)
    norm = N.FaceNormalizer(0, preset="age")
    box = A.age_patch_box()
    eyes = {n: faces(n, rng) for n in COUNTS}
    geoms = {n: norm.geometry(eyes[n], (FW, FH)) for n in COUNTS}
    crops = {n: norm.normalize(fdev, geoms=geoms[n])[0] for n in COUNTS}
    feats = flow.execute(AC.patch_oracle(crops[16].cpu().numpy(), (96, 96), box, 0, AC.CONTRAST))
    clfs = AC.classifiers(feats, (30, 12, 8), seed=21)
    fa = {f: A.FaceAnalyzer(flow, *clfs, contrast=AC.CONTRAST, interpolation=f) for f in AC.FILTERS}

    def device_ms(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        t0 = time.perf_counter()
        fn()
        call = (time.perf_counter() - t0) * 1e3
        e1.record()
        e1.synchronize()
        return call, e0.elapsed_time(e1)

    variants = {}
    for n in COUNTS:
        if not a.patches_only:
            variants["estimate NEAREST", n, "default"] = lambda n=n: fa["NEAREST"].estimate(fdev, geoms=geoms[n])
            out_n = torch.empty((n, 260, 256), dtype=torch.uint8, device="cuda")
            variants["normalize alone", n, "default"] = lambda n=n, o=out_n: norm.normalize(fdev, geoms=geoms[n], out=o)
        for f in AC.FILTERS:
            out_p = torch.empty((n, 96 * 96), dtype=torch.float32, device="cuda")
            for flags, path in ((A.FLAG_FUSED, "fused"), (A.FLAG_COMPOSED, "composed")):
                variants["patches " + f, n, path] = lambda n=n, f=f, o=out_p, fl=flags: fa[f].patches(crops[n], out=o, flags=fl)
    for f in AC.FILTERS:                      # what is timed is PIL's patch
        want = AC.patch_oracle(crops[4].cpu().numpy()[:1], (96, 96), box, AC.FILTERS[f], AC.CONTRAST)
        for flags in (A.FLAG_FUSED, A.FLAG_COMPOSED, 0):
            assert np.array_equal(fa[f].patches(crops[4], flags=flags)[:1].cpu().numpy(), want), (f, flags)
    for fn in variants.values():              # warm-up (code objects, scratch, workspaces)
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    t = {k: ([], []) for k in variants}
    for _ in range(a.reps):                   # alternated: every variant once per round
        for k, fn in variants.items():
            c, d = device_ms(fn)
            t[k][0].append(c)
            t[k][1].append(d)
    import PIL
    lines = ["== %s: %s, %s, %d calls each, alternated ==" % (a.label, os.path.relpath(_capi._LIB_PATH, ROOT), torch.cuda.get_device_name(0), a.reps),
             "frame %dx%d, crops 256x260, patches 96x96, box %s; every filter's patches checked against PIL (Pillow %s) on both paths before timing" %
             (FW, FH, tuple(round(v, 2) for v in box), PIL.__version__)]
    for k in variants:
        lines.append("%-18s %2d faces %-9s device %s | around the call %s" % (k[0], k[1], k[2], stats(t[k][1]), stats(t[k][0])))
    if not a.patches_only:
        for n in COUNTS:
            est, nrm = np.median(t["estimate NEAREST", n, "default"][1]), np.median(t["normalize alone", n, "default"][1])
            lines.append("normalise's share  %2d faces: %.4f of %.4f ms device time = %.0f %%" % (n, nrm, est, 100.0 * nrm / est))
    for f in AC.FILTERS:
        for n in COUNTS:
            fu, co = np.median(t["patches " + f, n, "fused"][1]), np.median(t["patches " + f, n, "composed"][1])
            lines.append("fused / composed   %-8s %2d faces: %.4f / %.4f ms (median device time) = %.2f" % (f, n, fu, co, fu / co))
    text = "\n".join(lines)
    print(text, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as fh:
        fh.write(text + "\n")
    torch.cuda.synchronize()
    for x in fa.values():
        x.close()
    for c in clfs:
        c.close()
    norm.close()
    flow.close()


if __name__ == "__main__":
    main()
