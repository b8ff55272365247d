"""What the eye step and the purge add to a frame: detect_frame (prescale + grid + cascade) against detect_faces (the same, then eyes,
discard, rows, purge — one host call each), alternated in one process after a warm-up, on the synthetic 1920x1080 frame of
BASELINE.json configs[2]; then the same pair on a cascade calibrated to leave about 100 survivors.  Prints one line per cascade.

    python tools/eyes_times.py [--reps 200]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
from pyfaceanalysis_amd import grid, synth, synth_cascade  # noqa: E402
from pyfaceanalysis_amd.cascade import DeviceCascade, frame_windows  # noqa: E402
from pyfaceanalysis_amd.eyes import EyeLocator  # noqa: E402
from pyfaceanalysis_amd.flow import Flow  # noqa: E402
from pyfaceanalysis_amd.patches import Patcher  # noqa: E402
import eyes_restate as ER  # noqa: E402

CONTRAST = (128.0, 48.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    a = ap.parse_args()
    rng = np.random.default_rng(synth.INPUT_SEED)
    frame = np.rint(synth._box3(rng.integers(0, 256, (1080, 1920), dtype=np.uint8))).astype(np.uint8)
    pipe = dict(grid.FACE_PIPELINE)
    _, nodes128 = synth.cached_preset_blob("U11L-128")
    _, nodes64 = synth.cached_preset_blob("U11L-64")
    flow = Flow(nodes128, output_dtype=np.float32)
    fdev = torch.from_numpy(frame).cuda()
    pt = Patcher()
    from PIL import Image
    small = np.asarray(Image.fromarray(frame, "L").resize((1000, 562), Image.NEAREST))
    boxes, _ = frame_windows(1000, 562, 0.1, pipe, (128, 128))
    subs = pt.extract(small, boxes, (128, 128), dtype=np.uint8)
    # bench.py's configs[2] cascade: four networks of the same architecture in the roles of the pipeline's four face flows
    flows4 = [flow] + [Flow(synth.build_preset("U11L-128", seed=synth.WEIGHT_SEED + 1009 * i, device=0), output_dtype=np.float32) for i in (1, 2, 3)]
    feats4 = [f.execute(subs, n_cols=20) for f in flows4]
    eye_flow = Flow(nodes64, output_dtype=np.float32)
    pick = rng.choice(len(boxes), 300, replace=False)
    ang = rng.uniform(-22.5, 22.5, 300)
    eb = ER.all_eye_boxes(boxes[pick], ang)
    efeats = eye_flow.execute(ER.contrast(pt.extract(small, eb, (64, 64), dtype=np.uint8, delta_angs=-np.concatenate([ang, ang])), *CONTRAST),
                              n_cols=12)
    loc = EyeLocator(*synth_cascade.build_eye_stages(eye_flow, efeats), contrast=CONTRAST)
    for label, kw in (("configs[2] cascade (bench.py)", dict(keep_fraction=0.2, later_keep_fraction=0.6)),
                      ("~100-survivor cascade", dict(keep_fraction=0.35, later_keep_fraction=0.9))):
        dc = DeviceCascade(synth_cascade.build_face_cascade(flows4, feats4, pipe, **kw), (128, 128), 20, pipe)
        for _ in range(10):                       # warm-up: plans, workspaces, code objects
            d = dc.detect_frame(fdev, smallest_face=0.1)
            f = dc.detect_faces(fdev, loc, smallest_face=0.1)
        torch.cuda.synchronize()
        tf, tx = [], []
        for _ in range(a.reps):                   # alternated, one call each, wall time of the synchronous call
            t0 = time.perf_counter()
            dc.detect_frame(fdev, smallest_face=0.1)
            t1 = time.perf_counter()
            dc.detect_faces(fdev, loc, smallest_face=0.1)
            t2 = time.perf_counter()
            tf.append(t1 - t0)
            tx.append(t2 - t1)
        mf, mx = np.median(tf) * 1e3, np.median(tx) * 1e3
        print("%s: survivors %d, after discard %d, after purge %d | detect_frame median %.3f ms (p10 %.3f p90 %.3f) | detect_faces median "
              "%.3f ms (p10 %.3f p90 %.3f) | added %.3f ms per frame" % (
                  label, len(d["coords"]), f["n_before_purge"], len(f["faces"]), mf, np.percentile(tf, 10) * 1e3, np.percentile(tf, 90) * 1e3,
                  mx, np.percentile(tx, 10) * 1e3, np.percentile(tx, 90) * 1e3, mx - mf), flush=True)
        dc.close()
    loc.close()
    pt.close()
    eye_flow.close()
    for f in flows4:
        f.close()


if __name__ == "__main__":
    main()
