"""What the interpolation filters cost a frame: detect_frame and detect_faces (one host call each) on the synthetic 1920x1080 frame of
BASELINE.json configs[2] with every stage NEAREST, every stage BILINEAR and every stage BICUBIC (cascade and eye patches alike), and the
first stage's extraction alone (1738 windows of 128 x 128 from the prescaled frame; coordinate tables + gather through the unkeyed device
entry, device time between two events).  One process, one machine; minimum, median and maximum over --reps calls each, appended to
--out with the library that was loaded.  A library of an older commit (HIGSFA_LIB, tools/build_ref_lib.sh) has no filters: its run
gives the NEAREST figures to compare with.  Also 300 ROTATED windows (17 degrees, 128 x 128) cut from 320 and from 576 pixels of the
prescaled frame (shrunk 2.5 x and 4.5 x): the sizes on either side of the limits below which k_filter_gather_rot stages a tile's
rectangle of the rotated frame in LDS (hg_extract.hip; runs A and B of profiles/r08_filter_times.txt are the figures those limits were chosen from).

    python tools/filter_times.py [--reps 30] [--label this] [--out profiles/r08_filter_times.txt]
    rocprofv3 --kernel-trace --stats ... -- python tools/filter_times.py --filters BICUBIC --frame-only --out <scratch file>
(--frame-only: detect_frame alone, so that the kernel statistics are those of the frame's stages).
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from pyfaceanalysis_amd import _capi, grid, synth, synth_cascade  # noqa: E402
from pyfaceanalysis_amd.cascade import DeviceCascade, frame_windows  # noqa: E402
from pyfaceanalysis_amd.eyes import EyeLocator  # noqa: E402
from pyfaceanalysis_amd.flow import Flow  # noqa: E402
import eyes_restate as ER  # noqa: E402

CONTRAST = (128.0, 48.0)
FILTERS = (("NEAREST", 0), ("BILINEAR", 2), ("BICUBIC", 3))


def stats(ms):
    return "min %.3f  median %.3f  max %.3f ms" % (np.min(ms), np.median(ms), np.max(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--label", default="this build")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r08_filter_times.txt"))
    ap.add_argument("--filters", default="NEAREST,BILINEAR,BICUBIC")
    ap.add_argument("--frame-only", action="store_true")
    a = ap.parse_args()
    if a.reps < 15:
        ap.error("--reps must be at least 15")
    L = _capi.lib()
    has_filters = hasattr(L, "hg_cascade_set_interpolation")
    rng = np.random.default_rng(synth.INPUT_SEED)
    frame = np.rint(synth._box3(rng.integers(0, 256, (1080, 1920), dtype=np.uint8))).astype(np.uint8)
    pipe = dict(grid.FACE_PIPELINE)
    _, nodes128 = synth.cached_preset_blob("U11L-128")
    _, nodes64 = synth.cached_preset_blob("U11L-64")
    flow = Flow(nodes128, output_dtype=np.float32)
    fdev = torch.from_numpy(frame).cuda()
    from PIL import Image
    small = np.asarray(Image.fromarray(frame, "L").resize((1000, 562), Image.NEAREST))
    boxes, _ = frame_windows(1000, 562, 0.1, pipe, (128, 128))
    ph = C.c_void_p()
    _capi.check(L.hg_patcher_create(0, C.byref(ph)))
    sdev, bdev = torch.from_numpy(small).cuda(), torch.from_numpy(boxes).cuda()
    odev = torch.empty((len(boxes), 128 * 128), dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream

    def first_stage(filt):
        if filt == 0:
            rc = L.hg_patcher_extract_device(ph, sdev.data_ptr(), _capi.HG_U8, 562, 1000, 1000, bdev.data_ptr(), len(boxes), 128, 128, odev.data_ptr(),
                                             _capi.HG_U8, 128 * 128, stream)
        else:
            rc = L.hg_patcher_extract_filter_device(ph, filt, sdev.data_ptr(), _capi.HG_U8, 562, 1000, 1000, bdev.data_ptr(), None, len(boxes), 128, 128,
                                                    odev.data_ptr(), _capi.HG_U8, 128 * 128, stream)
        _capi.check(rc)
    first_stage(0)
    torch.cuda.synchronize()
    subs = odev.cpu().numpy()
    # rotated windows of two sizes, centres spread over the frame (the larger ones hang over its edges, as a cascade's do)
    NR = 300
    cx, cy = rng.uniform(100, 900, NR), rng.uniform(100, 462, NR)
    rdev = {side: torch.from_numpy(np.stack([cx - side / 2, cy - side / 2, cx + side / 2, cy + side / 2], axis=1)).cuda() for side in (320.0, 576.0)}
    adev = torch.full((NR,), 17.0, dtype=torch.float64, device="cuda")

    def rotated(filt, side):
        if filt == 0:
            rc = L.hg_patcher_extract_rotate_device(ph, sdev.data_ptr(), _capi.HG_U8, 562, 1000, 1000, rdev[side].data_ptr(), adev.data_ptr(), NR, 128, 128,
                                                    odev.data_ptr(), _capi.HG_U8, 128 * 128, stream)
        else:
            rc = L.hg_patcher_extract_filter_device(ph, filt, sdev.data_ptr(), _capi.HG_U8, 562, 1000, 1000, rdev[side].data_ptr(), adev.data_ptr(), NR, 128,
                                                    128, odev.data_ptr(), _capi.HG_U8, 128 * 128, stream)
        _capi.check(rc)

    def device_ms(fn, *args):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn(*args)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)
    # bench.py's configs[2] cascade and tools/eyes_times.py's eye stages, calibrated on NEAREST windows whatever the filter timed
    flows4 = [flow] + [Flow(synth.build_preset("U11L-128", seed=synth.WEIGHT_SEED + 1009 * i, device=0), output_dtype=np.float32) for i in (1, 2, 3)]
    feats4 = [f.execute(subs, n_cols=20) for f in flows4]
    eye_flow = Flow(nodes64, output_dtype=np.float32)
    pick = rng.choice(len(boxes), 300, replace=False)
    ang = rng.uniform(-22.5, 22.5, 300)
    eb = ER.all_eye_boxes(boxes[pick], ang)
    eu8 = np.empty((600, 4096), dtype=np.uint8)
    dang = -np.concatenate([ang, ang])
    _capi.check(L.hg_patcher_extract_rotate(ph, small.ctypes.data, _capi.HG_U8, 562, 1000, 1000, eb.ctypes.data, dang.ctypes.data, 600, 64, 64,
                                            eu8.ctypes.data, _capi.HG_U8, 4096))
    efeats = eye_flow.execute(ER.contrast(eu8, *CONTRAST), n_cols=12)
    eye_stages = synth_cascade.build_eye_stages(eye_flow, efeats)
    stages = synth_cascade.build_face_cascade(flows4, feats4, pipe, keep_fraction=0.2, later_keep_fraction=0.6)
    lines = ["== %s: %s (filters %s), %d calls each ==" % (a.label, os.path.relpath(_capi._LIB_PATH, ROOT), "available" if has_filters else "not in this build", a.reps)]
    for name, filt in FILTERS:
        if name not in a.filters.split(",") or (filt and not has_filters):
            continue
        kw = dict(interpolation_formats=[filt] * 10) if filt else {}
        ekw = dict(interpolation=filt) if filt else {}
        dc = DeviceCascade(stages, (128, 128), 20, pipe, **kw)
        loc = EyeLocator(*eye_stages, contrast=CONTRAST, **ekw)
        for _ in range(5):                        # warm-up: plans, workspaces, code objects
            d = dc.detect_frame(fdev, smallest_face=0.1)
            if a.frame_only:
                continue
            f = dc.detect_faces(fdev, loc, smallest_face=0.1)
            first_stage(filt)
            rotated(filt, 320.0)
            rotated(filt, 576.0)
        torch.cuda.synchronize()
        tf, tx, te, tr = [], [], [], {320.0: [], 576.0: []}
        for _ in range(a.reps):                   # alternated, wall time of the synchronous calls; device time of the extraction
            t0 = time.perf_counter()
            dc.detect_frame(fdev, smallest_face=0.1)
            t1 = time.perf_counter()
            tf.append((t1 - t0) * 1e3)
            if a.frame_only:
                continue
            dc.detect_faces(fdev, loc, smallest_face=0.1)
            t2 = time.perf_counter()
            tx.append((t2 - t1) * 1e3)
            te.append(device_ms(first_stage, filt))
            for side in tr:
                tr[side].append(device_ms(rotated, filt, side))
        lines.append("%-8s survivors %d, counts %s" % (name, len(d["coords"]), d["counts"]))
        lines.append("%-8s detect_frame            %s" % (name, stats(tf)))
        if a.frame_only:
            loc.close()
            dc.close()
            continue
        lines.append("%-8s faces %d" % (name, len(f["faces"])))
        lines.append("%-8s detect_faces            %s" % (name, stats(tx)))
        lines.append("%-8s first-stage extraction  %s" % (name, stats(te)))
        for side in tr:
            lines.append("%-8s 300 rotated from %d px   %s" % (name, side, stats(tr[side])))
        loc.close()
        dc.close()
    text = "\n".join(lines)
    print(text, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as fh:
        fh.write(text + "\n")
    L.hg_patcher_free(ph)
    eye_flow.close()
    for fl in flows4:
        fl.close()


if __name__ == "__main__":
    main()
