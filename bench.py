#!/usr/bin/env python
"""Headline benchmark: 128x128 sub-images/s through the 11-layer HiGSFA net (BASELINE.json).

    python bench.py --gpus N --steps K --warmup W
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...

One "step" = one pass of the hot path (flow.execute on a device-resident batch) over
ROWS_PER_GPU synthetic 128x128 sub-images per GPU (BASELINE.json configs[1]: 4096 on one GPU;
configs[3]: 32768 sharded over 8 GPUs = 4096 per GPU, i.e. weak scaling), fp32, network
"U11L-128"  with trained random-init weights.  Inputs are resident in HBM before
the timed region; for N > 1 every step ends with the RCCL all-gather of the first 20 slow
features (north_star).  Rank 0 prints ONE JSON line.

A plain run sets up, warms up, times the K steps and prints the line (headline fields: metric, value, unit,
higher_is_better, dtype, ms_per_step, config).  Everything beside the headline — per-kernel event times and the
roofline, batches in flight, parity against the oracle, the frame leg, the extra legs, the CPU baselines — runs
only with --full (the --no-* switches then leave out single parts of it, as before).

--dump-outputs DIR writes what the last timed step returned (the float32 features a caller of the step receives,
(world * rows, 20)) to DIR/features.npy; inputs and weights are seeded, so runs with the same arguments are
comparable output for output.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

ROWS_PER_GPU = 4096
N_COLS = 20                      # first 20 slow features are what callers consume
SETTLE_MS = 150.0                # untimed load before short runs (see main)
SETTLE_STEPS_DISTRIBUTED = 300   # the same as a fixed step count when every step ends in a collective
SIDE = 128
PRESET = "U11L-128"
PEAK_MFMA_F32_TFLOPS = 157.3     # /opt/skills/guides/MI355X_MICROARCH.md "Peak FP32 (matrix)"
PEAK_HBM_GBS = 8000.0
PEAK_MFMA_F64_TFLOPS = 78.6      # MI355X data sheet: FP64 matrix = FP64 vector = half the FP32 rate above (the guide lists no fp64 row)
TRAFFIC_PROFILE = "r05_traffic.json"   # committed PMC summary the roofline's `traffic` is read from


def cpu_baseline(nodes, n=256, reps=6):
    """MDP-structured numpy float64 restatement (oracle/) timed on this box's host cores.
    Bounded sample: `reps` passes over n sub-images after one warm-up; best pass reported."""
    from oracle import mdp_restate
    from pyfaceanalysis_amd import synth
    x = synth.make_subimages(n, SIDE, dtype=np.float64)

    def best_of(k):
        mdp_restate.execute_flow(nodes, x)
        b = 1e30
        for _ in range(k):
            t0 = time.perf_counter()
            mdp_restate.execute_flow(nodes, x)
            b = min(b, time.perf_counter() - t0)
        return b
    best = best_of(reps)
    threads = os.cpu_count() or 1
    at12 = None
    try:
        from threadpoolctl import threadpool_info, threadpool_limits
        blas = [p["num_threads"] for p in threadpool_info() if p.get("user_api") == "blas"]
        if blas:
            threads = max(blas)
        # BASELINE.md §4 run C2: the author's setting, mkl.set_num_threads(12) (FaceDetectUpdated.py:72-77)
        with threadpool_limits(limits=12, user_api="blas"):
            t12 = min(12, threads)
            at12 = {"value": n / best_of(3), "unit": "sub-images/s", "cores": t12,
                    "sample": "same restatement and sample with the BLAS pool limited to %d threads (FaceDetectUpdated.py:74), "
                              "best of 3 after 1 warm-up" % t12}
    except Exception:
        pass
    quota = None
    try:      # cgroup v2 CPU quota of this container ("max" = none)
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()
        quota = None if q == "max" else float(q) / float(per)
    except Exception:
        pass
    avail = len(os.sched_getaffinity(0))
    cpus_available = int(min(avail, quota)) if quota else avail
    out = {"value": n / best, "unit": "sub-images/s", "cores": min(threads, cpus_available), "kind": "port",
           "cpus_available": cpus_available, "cpu_affinity": avail, "cpu_quota": quota, "blas_threads": threads,
           "sample": "%d sub-images of 128x128 float64 through oracle/mdp_restate.py (MDP-structured numpy "
                     "restatement: per-node Python loop + numpy.dot), best of %d passes after 1 warm-up; "
                     "numpy BLAS pool %d threads on %d CPUs available to this process (affinity %d, cgroup quota %s)"
                     % (n, reps, threads, cpus_available, avail, "none" if quota is None else "%.0f" % quota)}
    if at12 is not None:
        out["blas_12_threads"] = at12
    # the "good CPU" point: the same flow from one flat op list in C, float64, row chunks
    # that stay in cache, OpenMP over rows, vector pow (oracle/fast_cpu.c)
    try:
        from oracle import fast_cpu
        cores = min(16, len(os.sched_getaffinity(0)))
        plan = fast_cpu.Plan(nodes)
        xo = synth.make_subimages(4 * n, SIDE, dtype=np.float64)
        plan.run(xo, cores)
        bo = 1e30
        for _ in range(3):
            t0 = time.perf_counter()
            plan.run(xo, cores)
            bo = min(bo, time.perf_counter() - t0)
        out["optimised_port"] = {"value": 4 * n / bo, "unit": "sub-images/s", "cores": cores,
                                 "sample": "%d sub-images through oracle/fast_cpu.c (flat op list, float64, AVX2, "
                                           "OpenMP over 16-row chunks), best of 3 after 1 warm-up" % (4 * n)}
    except TypeError as e:          # node kinds the C leg does not cover (iGSFA variant)
        out["optimised_port"] = {"value": None, "note": str(e)}
    return out


def frame_leg(flow, dev, reps=100, flow_factory=None):
    return _frame_leg(flow, dev, reps, flow_factory)


def _frame_leg(flow, dev, reps, flow_factory):
    """BASELINE.json configs[2] as an extra figure beside the headline: one synthetic 1920x1080 frame, smallest_face 0.1,
    prescaled to 1000x562 (FaceDetectUpdated.py:551-556) -> 10 pyramid levels / 1738 first-stage windows of 128x128, all
    levels as ONE batch, through the synthetic 17-stage face cascade (pyfaceanalysis_amd/synth_cascade.py: the pipeline's
    stage structure; FOUR distinct synthetic networks in the roles of the pipeline's four face flows,
    Pipelines/Pipeline_experimental.txt, each with its own handle, weights and workspace; Gaussian classifiers with the
    class counts of the reference's files, 10 for Disc and 50 for the pose regressors), everything on the device: prescale, rotated window extraction,
    flow.execute, Gaussian regression, coordinate update, discard, compaction; the host reads one survivor count per stage.
    `first_stage_ms` is the chain extract -> execute -> regression over all 1738 windows with no host hop at all."""
    import torch
    from pyfaceanalysis_amd import grid, synth, synth_cascade
    from pyfaceanalysis_amd.cascade import DeviceCascade, frame_windows
    rng = np.random.default_rng(synth.INPUT_SEED)
    frame = torch.from_numpy(np.rint(synth._box3(rng.integers(0, 256, (1080, 1920), dtype=np.uint8))).astype(np.uint8)).to(dev)
    pipe = dict(grid.FACE_PIPELINE)
    boot = DeviceCascade([synth_cascade.Stage("Disc1", flow, synth_cascade.quantile_classifier(rng.normal(size=(50, 20)), 9, [0.0, 1.0]))],
                         (SIDE, SIDE), N_COLS, pipe)
    small = boot.prescale(frame)
    boxes, level = frame_windows(int(small.shape[1]), int(small.shape[0]), 0.1, pipe, (SIDE, SIDE))
    n0 = len(boxes)
    # calibration sample for the synthetic classifiers: first-stage features of this frame
    b_dev = torch.from_numpy(boxes).to(dev)
    subs = torch.empty((n0, SIDE * SIDE), dtype=torch.uint8, device=dev)
    feats = torch.empty((n0, N_COLS), dtype=torch.float32, device=dev)
    reg = torch.empty(n0, dtype=torch.float64, device=dev)
    st = torch.cuda.current_stream(dev)
    flow.reserve(n0)

    def first_stage(clf):
        boot.patcher.extract_device(small.data_ptr(), np.uint8, small.shape[0], small.shape[1], small.stride(0), b_dev.data_ptr(), n0,
                                    (SIDE, SIDE), subs.data_ptr(), np.uint8, SIDE * SIDE, stream=st.cuda_stream)
        flow.execute_device(subs.data_ptr(), np.uint8, n0, SIDE * SIDE, feats.data_ptr(), np.float32, N_COLS, N_COLS, stream=st.cuda_stream)
        clf.regression_device(feats.data_ptr(), np.float32, n0, N_COLS, reg.data_ptr(), stream=st.cuda_stream)
    first_stage(boot.stages[0].classifier)
    torch.cuda.synchronize(dev)
    # three more networks of the same architecture (other seeds), trained on the GPU (< 1 s each): with `flow` they play the
    # pipeline's four face flows (synth_cascade.FLOW_ROLE)
    from pyfaceanalysis_amd.blob import flow_to_blob
    from pyfaceanalysis_amd.flow import Flow
    more_blobs = [flow_to_blob(synth.build_preset(PRESET, seed=synth.WEIGHT_SEED + 1009 * i, device=dev.index)) for i in (1, 2, 3)]

    def four_flows(first):
        fl = [first] + [Flow.from_blob(b, device=dev.index, output_dtype=np.float32) for b in more_blobs]
        for f_ in fl:
            f_.reserve(n0)
        return fl

    def calib(fl):       # first-stage features of this frame through every flow: the classifiers' calibration samples
        out_ = []
        for f_ in fl:
            f_.execute_device(subs.data_ptr(), np.uint8, n0, SIDE * SIDE, feats.data_ptr(), np.float32, N_COLS, N_COLS, stream=st.cuda_stream)
            torch.cuda.synchronize(dev)
            out_.append(feats.cpu().numpy().copy())
        return out_
    flows4 = four_flows(flow)
    feats4 = calib(flows4)
    stages = synth_cascade.build_face_cascade(flows4, feats4, pipe, keep_fraction=0.2, later_keep_fraction=0.6)
    dc = DeviceCascade(stages, (SIDE, SIDE), N_COLS, pipe)
    win = (boxes, level)
    for _ in range(40):      # ~60 ms of frames before the timed ones: the chip has idled through the calibration above
        out = dc.detect_frame(frame, smallest_face=0.1)
    torch.cuda.synchronize(dev)
    # five batches of `reps` frames, the median batch reported (one host hiccup of a few ms in a single 0.13 s batch moved the
    # figure by 2-3 %: round 5 saw 1.25 ... 1.30 ms from one build on one box); all five are in the line
    batches = []
    first_out = dc.detect_frame(frame, smallest_face=0.1)
    frames_identical = True      # every timed frame's survivors (boxes, angles, confidences, counts per stage) against the first frame's, bit for bit
    for _ in range(5):
        outs = []
        t0 = time.perf_counter()
        for _ in range(reps):
            outs.append(dc.detect_frame(frame, smallest_face=0.1))
        torch.cuda.synchronize(dev)
        batches.append((time.perf_counter() - t0) / reps)
        out = outs[-1]
        for o in outs:      # (compared outside the timed region)
            frames_identical = frames_identical and list(o["counts"]) == list(first_out["counts"]) and all(
                np.array_equal(o[k], first_out[k]) for k in ("coords", "angles", "orig_index", "confidence"))
    batches.sort()
    per_frame = batches[2]
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(3):
        first_stage(stages[0].classifier)
    e0.record(st)
    for _ in range(reps):
        first_stage(stages[0].classifier)
    e1.record(st)
    torch.cuda.synchronize(dev)
    # Several frames in flight: further cascades (their own flow handles and workspaces), one stream and one host thread each.
    # Frames are independent; most launches of a frame are far too small to fill the chip (survivor batches of 340 ... 2
    # rows), and the host waits for one survivor count per Disc stage, so other frames fill those gaps.
    two = None
    if flow_factory is not None:
        import threading
        extra = []
        for _ in range(3):
            f2 = four_flows(flow_factory())
            extra.append((f2, DeviceCascade(synth_cascade.build_face_cascade(f2, feats4, pipe, keep_fraction=0.2, later_keep_fraction=0.6), (SIDE, SIDE), N_COLS, pipe)))
        cascades = [dc] + [c for _, c in extra]
        streams = [torch.cuda.Stream(dev) for _ in cascades]
        outs = [None] * len(cascades)

        def worker(i, k):
            torch.cuda.set_device(dev)
            with torch.cuda.stream(streams[i]):
                for _ in range(k):
                    outs[i] = cascades[i].detect_frame(frame, smallest_face=0.1)
            streams[i].synchronize()

        def run_group(n_par, k):
            th = [threading.Thread(target=worker, args=(i, k)) for i in range(n_par)]
            for t_ in th:
                t_.start()
            for t_ in th:
                t_.join()
        two = {}
        for n_par in (2, 3, 4):
            torch.cuda.synchronize(dev)
            run_group(n_par, 3)
            t0 = time.perf_counter()
            run_group(n_par, reps)
            dtp = time.perf_counter() - t0
            same = all(all(int(a) == int(b) for a, b in zip(outs[i]["counts"], out["counts"])) for i in range(n_par))
            two[str(n_par)] = {"frames_per_s": n_par * reps / dtp, "same_survivor_counts_as_sequential": bool(same)}
        for f2, c2 in extra:
            c2.close()
            for f_ in f2:
                f_.close()
    res = {"frames_per_s": 1.0 / per_frame, "ms_per_frame": per_frame * 1e3, "ms_per_frame_batches": [round(b * 1e3, 4) for b in batches], "frames_identical": bool(frames_identical), "frame": "1920x1080 synthetic, prescaled 1000x562, smallest_face 0.1",
           "levels": int(len(np.unique(level[:, 2]))), "windows": n0, "stages": len(stages), "rows_executed": int(out["rows_executed"]),
           "survivors_per_stage": [int(c) for c in out["counts"]], "detections": int(out["counts"][-1]),
           "detections_per_s": float(out["counts"][-1]) / per_frame,
           "first_stage_ms": e0.elapsed_time(e1) / reps,
           "distinct_flow_handles": len({id(s_.flow) for s_ in stages if s_.flow is not None}),
           "classifier_classes": sorted({int(s_.classifier.means.shape[0]) for s_ in stages}),
           "note": "synthetic networks and classifiers (trained flows are not shipped): timing only; host work per frame = "
                   "grid constants + 17 launches' worth of ctypes calls + one 4-byte count readback per stage"}
    if two is not None:
        res["frames_in_flight"] = two
    dc.close()
    boot.close()
    for f_ in flows4[1:]:
        f_.close()
    return res


def host_path_leg(blob):
    """The reference's actual call hands over HOST ndarrays (face_analysis.py:786 -> FaceDetectUpdated.py:699): time
    hg_flow_execute — packers narrowing / copying rows straight into device memory, passes sized by the planner, features
    back, synchronous — on float64 (what images_asarray yields), float32 and uint8 batches of 4096 and 728 rows (728 = the
    largest single execute of a real 1080p frame).  Best and median of 9 after two warm-up calls.
    Beside every figure the ceiling that bounds it, MEASURED in this process on this box (round 5; rounds 3-4 used constants
    from a micro-benchmark on another box, and one call beat its "ceiling"): `pack_ms` — the library's packer threads alone over
    the very array of the call (hg_host_pack_probe: same pool, placement and routines, destinations in cache), i.e. how fast
    this host reads and narrows these rows; `wire_ms` — the call's wire bytes (16 KiB per row: float rows holding integer
    pixel values cross PCIe as uint8 after the exact narrowing) at the FASTER of host stores into device memory
    (hg_host_store_probe, six writers as in the call) and a pinned copy-engine transfer (hg_host_dma_probe), 64 MiB each.
    `ceiling_ms` = max(pack_ms, wire_ms); `frac_of_ceiling` = ceiling_ms / ms_per_call.  `caller_GBps` = bytes of the
    caller's array per second (NOT the PCIe rate)."""
    import ctypes as C
    from pyfaceanalysis_amd import _capi, synth
    from pyfaceanalysis_amd.flow import Flow
    L = _capi.lib()
    out = {}
    f = Flow.from_blob(blob, output_dtype=np.float64)
    probe_bytes = 64 << 20
    t_store, t_dma, direct = C.c_double(), C.c_double(), C.c_int()
    _capi.check(L.hg_host_store_probe(0, probe_bytes, 5, C.byref(t_store), C.byref(direct)))
    _capi.check(L.hg_host_dma_probe(0, probe_bytes, 5, C.byref(t_dma)))
    store_GBps = probe_bytes / t_store.value / 1e9 if direct.value and t_store.value > 0 else None
    dma_GBps = probe_bytes / t_dma.value / 1e9
    link = max(store_GBps or 0.0, dma_GBps)
    for dt in (np.float64, np.float32, np.uint8):
        for n in (4096, 728):
            x = synth.make_subimages(n, SIDE, dtype=dt)
            f.execute(x[:64], n_cols=N_COLS)
            f.execute(x, n_cols=N_COLS)
            ts = []
            for _ in range(9):
                t0 = time.perf_counter()
                f.execute(x, n_cols=N_COLS)
                ts.append(time.perf_counter() - t0)
            best, med = min(ts), sorted(ts)[len(ts) // 2]
            t_pack = C.c_double()
            _capi.check(L.hg_host_pack_probe(x.ctypes.data_as(C.c_void_p), _capi.np_dtype_code(x.dtype), n, x.shape[1], x.shape[1], 9, C.byref(t_pack)))
            t_link = n * SIDE * SIDE / (link * 1e9)
            floor = max(t_pack.value, t_link)
            out["%s_n%d" % (np.dtype(dt).name, n)] = {
                "sub_images_per_s": n / best, "ms_per_call": best * 1e3, "ms_per_call_median": med * 1e3, "caller_GBps": x.nbytes / best / 1e9,
                "wire_GBps": n * SIDE * SIDE / best / 1e9, "pack_ms": t_pack.value * 1e3, "pack_GBps": x.nbytes / t_pack.value / 1e9,
                "wire_ms": t_link * 1e3, "ceiling": "host packers (read + narrow)" if t_pack.value >= t_link else "PCIe (faster of BAR stores and pinned DMA)",
                "ceiling_ms": floor * 1e3, "frac_of_ceiling": floor / best, "transport": {1: "direct stores", 0: "pinned ring"}.get(f.host_transport(), "?")}
    f.close()
    out["ceilings"] = {"bar_store_GBps": store_GBps, "pinned_dma_GBps": dma_GBps, "link_GBps_used": link, "probe_bytes": probe_bytes,
                       "source": "measured in this process: hg_host_store_probe / hg_host_dma_probe (64 MiB, best of 5), hg_host_pack_probe per case (best of 9)"}
    out["note"] = "Flow.execute(host ndarray) -> host float64 (N, 20): includes packing, PCIe, kernels, features back; never `value`"
    return out


def u11l_64_leg(dev, rows, steps):
    """The shipped pipelines feed the face flows 64x64 sub-images (Pipelines/Pipeline_experimental.txt:2): the
    same step on the U11L-64 preset, device resident, plus its error against the oracle on 64 rows."""
    import torch
    from oracle import mdp_restate
    from pyfaceanalysis_amd import synth
    from pyfaceanalysis_amd.flow import Flow
    blob, nodes = synth.cached_preset_blob("U11L-64")
    flow = Flow.from_blob(blob, device=dev.index, output_dtype=np.float32)
    flow.reserve(rows)
    xh = synth.make_subimages(rows, 64, dtype=np.float32)
    x = torch.from_numpy(xh).to(dev)
    y = torch.empty((rows, N_COLS), dtype=torch.float32, device=dev)
    st = torch.cuda.current_stream(dev)

    def run(k):
        for _ in range(k):
            flow.execute_device(x.data_ptr(), np.float32, rows, x.shape[1], y.data_ptr(), np.float32, N_COLS, N_COLS, stream=st.cuda_stream)
        torch.cuda.synchronize(dev)
    run(max(100, steps // 4))
    t0 = time.perf_counter()
    run(steps)
    dt = (time.perf_counter() - t0) / steps
    ref = mdp_restate.execute_flow(nodes, xh[:64].astype(np.float64))[:, :N_COLS]
    err = float(np.abs(y[:64].cpu().numpy() - ref).max() / np.abs(ref).max())
    fl = synth.flops_per_row(nodes)
    flow.close()
    return {"workload": "U11L-64 (11 layers, 64x64 sub-images, first 20 features), %d rows resident in HBM" % rows, "sub_images_per_s": rows / dt,
            "ms_per_step": dt * 1e3, "flops_per_subimage": int(fl), "tflops": fl * rows / dt / 1e12, "max_rel_err_vs_oracle": err}


def train_leg(dev, n=100_000):
    """BASELINE.json configs[4]: one SFA training step — per-node mean / covariance / covariance of the time differences in
    fp64, then the generalised symmetric eigen-solve — over 100 000 synthetic 128x128 patches (uint8, 1.64 GB resident),
    layer-0 geometry (1024 nodes x 16 pixels); eigenvalues and B-normalised eigenvectors of three nodes against
    scipy.linalg.eigh (budget 1e-5).  The sequence is a window gliding over a texture, as in tests/test_train_gpu.py."""
    import scipy.linalg
    import torch
    from pyfaceanalysis_amd import nodes as N, synth
    from pyfaceanalysis_amd.train import sfa_train_layer
    rng = np.random.default_rng(3)
    tex = torch.from_numpy(np.rint(synth._box3(rng.integers(0, 256, (SIDE + 600, SIDE + 600), dtype=np.uint8))).astype(np.uint8)).to(dev)
    t = torch.arange(n, device=dev, dtype=torch.float64)
    px = torch.round((0.5 + 0.5 * torch.sin(0.0021 * t)) * 599).long()
    py = torch.round((0.5 + 0.5 * torch.sin(0.00153 * t + 1.0)) * 599).long()
    x = torch.empty((n, SIDE * SIDE), dtype=torch.uint8, device=dev)
    idx = torch.arange(SIDE, device=dev)
    for i0 in range(0, n, 5000):
        sl = slice(i0, min(n, i0 + 5000))
        x[sl] = tex[(py[sl, None] + idx[None, :])[:, :, None], (px[sl, None] + idx[None, :])[:, None, :]].reshape(-1, SIDE * SIDE)
    torch.cuda.synchronize(dev)
    conn = N.Rectangular2dSwitchboard((SIDE, SIDE), (4, 4), (4, 4), 1).connections.reshape(-1, 16)
    sfa_train_layer(x.data_ptr(), conn, device=dev.index, x_dtype=np.uint8, n=2000, ldx=SIDE * SIDE)        # warm-up (library handles)
    best = None
    for _ in range(3):
        t0 = time.perf_counter()
        ev, W, mu, tms = sfa_train_layer(x.data_ptr(), conn, device=dev.index, x_dtype=np.uint8, n=n, ldx=SIDE * SIDE)
        wall = (time.perf_counter() - t0) * 1e3
        if best is None or tms[0] + tms[1] < best[0] + best[1]:
            best = (tms[0], tms[1], wall)
    worst_val = worst_vec = 0.0
    for k in (0, 517, 1023):
        xk = x[:, torch.from_numpy(conn[k].astype(np.int64)).to(dev)].double().cpu().numpy()
        B = np.cov(xk.T)
        dx = xk[1:] - xk[:-1]
        A = dx.T @ dx / (n - 1)
        w, v = scipy.linalg.eigh(A, B)
        worst_val = max(worst_val, float(np.abs(ev[k] / w - 1).max()))
        worst_vec = max(worst_vec, float(np.abs(np.abs(np.diag(v.T @ B @ W[k])) - 1).max()))
    del x
    torch.cuda.empty_cache()
    return {"workload": "configs[4]: %d patches of 128x128 uint8 resident in HBM, 1024 nodes x 16 inputs" % n, "statistics_ms": best[0],
            "eigensolve_ms": best[1], "wall_ms": best[2], "input_GBps": n * SIDE * SIDE / best[0] / 1e6,
            "statistics_gflops_f64": n * 1024.0 * (16 * 16 * 2) * 2 / best[0] / 1e6,
            # the two roofs of the statistics kernel: HBM for the patch read (MI355X_MICROARCH.md: 8 TB/s), the fp64 matrix rate for the
            # products as ISSUED — both 16 x 16 products (covariance, covariance of the differences) in full, although each is symmetric
            "roofline": {"hbm": {"achieved_GBps": n * SIDE * SIDE / best[0] / 1e6, "peak_GBps": PEAK_HBM_GBS, "frac": n * SIDE * SIDE / best[0] / 1e6 / PEAK_HBM_GBS},
                         "mfma_f64": {"achieved_TFLOPs": n * 1024.0 * (16 * 16 * 2) * 2 / best[0] / 1e9, "peak_TFLOPs": PEAK_MFMA_F64_TFLOPS,
                                      "frac": n * 1024.0 * (16 * 16 * 2) * 2 / best[0] / 1e9 / PEAK_MFMA_F64_TFLOPS,
                                      "peak_source": "MI355X data sheet FP64 matrix = FP64 vector rate, half the FP32 rate of MI355X_MICROARCH.md (157.3)",
                                      "symmetric_half_TFLOPs": n * 1024.0 * (16 * 17) * 2 / best[0] / 1e9},
                         "bound": "neither: 1.64 GB of uint8 patches widened to fp64 in registers, 16 patch columns per node"},
            "max_rel_err_eigenvalues_vs_scipy": worst_val, "max_err_eigenvectors_vs_scipy": worst_vec, "nodes_checked": 3, "budget": 1e-5}


def uniform_leg(flow, nodes, dev, rows, steps):
    """SURVEY.md §8d's stress variant of the input: pure uniform random pixels (no 3x3 low-pass), same step, same checks."""
    import torch
    from oracle import mdp_restate
    rng = np.random.default_rng(12345600)
    xh = rng.integers(0, 256, (rows, SIDE * SIDE), dtype=np.uint8).astype(np.float32)
    x = torch.from_numpy(xh).to(dev)
    y = torch.empty((rows, N_COLS), dtype=torch.float32, device=dev)
    st = torch.cuda.current_stream(dev)

    def run(k):
        for _ in range(k):
            flow.execute_device(x.data_ptr(), np.float32, rows, x.shape[1], y.data_ptr(), np.float32, N_COLS, N_COLS, stream=st.cuda_stream)
        torch.cuda.synchronize(dev)
    run(50)
    t0 = time.perf_counter()
    run(steps)
    dt = (time.perf_counter() - t0) / steps
    ref = mdp_restate.execute_flow(nodes, xh[:64].astype(np.float64))[:, :N_COLS]
    err = float(np.abs(y[:64].cpu().numpy() - ref).max() / np.abs(ref).max())
    return {"input": "uniform random 0..255 per pixel", "sub_images_per_s": rows / dt, "ms_per_step": dt * 1e3, "max_rel_err_vs_oracle": err}


def spawn_ranks(n_gpus, argv):
    """`python bench.py --gpus N` (N > 1) without a launcher: this process has not imported torch.cuda work or touched HIP
    and never will — it builds the native pieces if stale, starts `torch.distributed.run` with one rank per GPU as a fresh
    CHILD process (never an exec of a process that holds the GPU), relays rank 0's single JSON line and returns the
    child's exit code."""
    import subprocess
    from pyfaceanalysis_amd import build as native_build
    if native_build.is_stale():
        native_build.build()
    oracle_dir = os.path.join(ROOT, "oracle")
    if native_build.oracle_is_stale(oracle_dir):
        subprocess.check_call(["make", "-s", "-C", oracle_dir])
    import torch                                   # device_count() alone does not initialise the GPU
    have = torch.cuda.device_count()
    if have < n_gpus:
        print("bench.py: --gpus %d asked for, %d GPU(s) visible on this node" % (n_gpus, have), file=sys.stderr)
        return 2
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")      # dmabuf IPC only on this pool (RCCL needs it)
    env.setdefault("OMP_NUM_THREADS", str(max(1, (os.cpu_count() or n_gpus) // n_gpus)))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--standalone", "--local-addr", "127.0.0.1", "--nnodes=1",
           "--nproc-per-node", str(n_gpus), os.path.abspath(__file__)] + list(argv)
    child = subprocess.Popen(cmd, env=env, stdout=subprocess.PIPE, text=True)
    line = None
    for ln in child.stdout:                        # stderr goes straight through; stdout is scanned for the result line
        if ln.startswith('{"metric"'):
            line = ln.rstrip("\n")
        else:
            sys.stderr.write(ln)
    rc = child.wait()
    if line is not None:
        print(line, flush=True)
    elif rc == 0:
        print("bench.py: the ranks exited with 0 but rank 0 printed no result line", file=sys.stderr)
        rc = 1
    return rc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    # defaults: 0.55 s timed after 55 ms of warm-up.  A run of 20 steps after 3 (12 ms in all) ends before the chip has left its
    # idle power state and reads 10 % low (0.611 against 0.552 / 0.547 ms per step at 200 / 1000 steps on one box)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--rows", type=int, default=ROWS_PER_GPU, help="sub-images per GPU per step")
    ap.add_argument("--input-dtype", default="float32", choices=["float32", "uint8", "float64"])
    ap.add_argument("--generic", action="store_true", help="force the generic plan (diagnostic)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baselines")
    ap.add_argument("--no-frame", action="store_true", help="with --full: skip the configs[2] frame leg (frames_per_s)")
    ap.add_argument("--no-inflight", action="store_true", help="with --full: skip the batches-in-flight figure")
    ap.add_argument("--no-extra-legs", action="store_true",
                    help="with --full: skip host_path / u11l_64 / train_leg / uniform_input (figures beside the headline, outside the timed region)")
    ap.add_argument("--gather-stream", default="side", choices=["side", "same"],
                    help="distributed path: the all-gather on a side stream under the next step's kernels (default) or on the kernels' own stream")
    ap.add_argument("--compare-collective", action="store_true",
                    help="distributed path: after the headline, time the same step collective-free, with the side-stream gather and with the "
                         "same-stream gather in THIS process (collective_compare in the line; VERDICT r4 item 3)")
    ap.add_argument("--node-kind", default="pca_exp_sfa", choices=["pca_exp_sfa", "igsfa"],
                    help="node type of the synthetic 11-layer net (default: the BASELINE.md workload)")
    ap.add_argument("--full", action="store_true",
                    help="after the headline, also the figures beside it: per-kernel times + roofline, batches in flight, oracle parity, "
                         "frame leg, extra legs, CPU baselines (a plain run does only the headline)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the features the last timed step returned to DIR/features.npy (float32)")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    if args.gpus > 1 and "RANK" not in os.environ:
        raise SystemExit(spawn_ranks(args.gpus, sys.argv[1:]))

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    # Native pieces first, before torch or HIP are touched in this process: compiler children are never started from a
    # process that holds the GPU (or that a profiler has attached to).  An up-to-date tree starts no child at all.
    if rank == 0:
        from pyfaceanalysis_amd import build as native_build
        if native_build.is_stale():
            native_build.build()
        oracle_dir = os.path.join(ROOT, "oracle")
        if native_build.oracle_is_stale(oracle_dir):
            import subprocess
            subprocess.check_call(["make", "-s", "-C", oracle_dir])

    import torch
    import torch.distributed as dist
    if world != args.gpus:
        raise SystemExit("bench.py: --gpus %d but the launcher started %d rank(s)" % (args.gpus, world))
    dev = torch.device("cuda", local_rank)
    torch.cuda.set_device(dev)
    # launched by torch.distributed.run (RANK set): the process-group path runs even with one rank, so that
    # the N > 1 code can be rehearsed on a one-GPU box; plain `python bench.py` stays collective-free
    distributed = world > 1 or "RANK" in os.environ
    if distributed:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("nccl", device_id=dev)

    from pyfaceanalysis_amd import synth
    from pyfaceanalysis_amd.flow import Flow
    from pyfaceanalysis_amd.sharded import ShardedFlow

    # --- model: rank 0 trains (and caches) the net, the others load the cached blob
    if rank == 0:
        blob, nodes = synth.cached_preset_blob(PRESET, node_kind=args.node_kind)
    if distributed:
        dist.barrier()
    if rank != 0:
        blob, nodes = synth.cached_preset_blob(PRESET, node_kind=args.node_kind)
    flow = Flow.from_blob(blob, device=local_rank, output_dtype=np.float32, force_generic=args.generic)
    info = flow.info()
    rows = args.rows
    flow.reserve(rows)

    # --- data: this rank's shard of the global batch, resident in HBM
    in_dt = np.dtype(args.input_dtype)
    x_host = synth.make_subimages(rows, SIDE, seed=synth.INPUT_SEED + rank, dtype=in_dt)
    x = torch.from_numpy(x_host).to(dev)
    # the step is pyfaceanalysis_amd.sharded.ShardedFlow.step — the class tests/test_sharded_gloo.py runs over gloo:
    # flow.execute_device on this rank's block, then (N > 1) the RCCL all-gather of the first 20 features on a side
    # stream, double-buffered so that the gather of step i runs under the kernels of step i + 1
    gather_events = None
    if distributed:
        # Before anything is timed: the overlapped gather against a blocking one, on inputs that change from step to step and differ
        # between ranks (x is rank-seeded), every rank comparing every rank's block.  First with the device-scope hand-off event
        # (3-4 us per step cheaper); if any rank sees a mismatch, all ranks fall back to the ordinary event and check again.
        x_alts = [x, torch.roll(x, shifts=1 + rank, dims=0), torch.flip(x, dims=(0,))]
        light_ok = False
        if args.gather_stream == "same":
            sf = ShardedFlow.for_flow(flow, N_COLS, rows, dev, collective=True, gather_stream="same")
            if not sf.verify_against_blocking_gather(x_alts, steps=6):
                raise SystemExit("bench.py: the same-stream all-gather does not reproduce a blocking one (rank %d)" % rank)
            gather_events = "all-gather on the kernels' own stream; 6 steps on changing inputs equal to a blocking all-gather on every rank"
        else:
            sf = ShardedFlow.for_flow(flow, N_COLS, rows, dev, collective=True, light_events=True)
            if sf.verify_against_blocking_gather(x_alts, steps=6):
                light_ok = True
                gather_events = "device-scope hand-off event; 6 steps on changing inputs equal to a blocking all-gather on every rank"
            else:
                sf.close()
                sf = ShardedFlow.for_flow(flow, N_COLS, rows, dev, collective=True, light_events=False)
                if not sf.verify_against_blocking_gather(x_alts, steps=6):
                    raise SystemExit("bench.py: the overlapped all-gather does not reproduce a blocking one (rank %d)" % rank)
                gather_events = "system-scope hand-off event (the device-scope form FAILED verification on this node)"
    else:
        sf = ShardedFlow.for_flow(flow, N_COLS, rows, dev, collective=False)
    stream = sf.stream

    def step():
        return sf.step(x)

    # Power-state settle, before the warm-up proper and outside every count: the chip needs tens of milliseconds of load to
    # leave its idle clocks (a 20-step run after 3 warm-up steps reads 10 % low), so short --steps / --warmup settings are
    # preceded by untimed steps until SETTLE_MS of wall time have passed.  Reported as config.settle_ms.
    settle_ms = 0.0
    if args.warmup < 100:
        t_s = time.perf_counter()
        if distributed:
            # every step ends in a collective: all ranks must run the SAME number of settle steps (a wall-clock loop would not)
            for _ in range(SETTLE_STEPS_DISTRIBUTED):
                step()
            torch.cuda.synchronize(dev)
        else:
            while (time.perf_counter() - t_s) * 1e3 < SETTLE_MS:
                for _ in range(10):
                    step()
                torch.cuda.synchronize(dev)
        settle_ms = (time.perf_counter() - t_s) * 1e3
    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize(dev)
    if distributed:
        dist.barrier()
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for _ in range(args.steps):
        y_last = step()
    torch.cuda.synchronize(dev)      # every stream of the device: kernels and the last gathers
    if distributed:
        dist.barrier()
    torch.cuda.synchronize(dev)
    elapsed = time.perf_counter() - t0
    if distributed:
        t = torch.tensor([elapsed], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
        # the gathered matrix holds this rank's block where the sharding says (checked outside the timed region)
        for b_ in ((0, 1) if sf._n >= 2 else ((sf._n - 1) & 1,)):       # both buffers: the last two steps' gathers
            if not torch.equal(sf.y_alls[b_][rank * rows:(rank + 1) * rows], sf.ys[b_]):
                raise SystemExit("bench.py: all-gather result (buffer %d) does not contain this rank's features" % b_)
        # every rank's block arrived: the blocks differ (rank-seeded inputs) and none is left at its initial zeros
        blocks = sf.y_alls[(sf._n - 1) & 1].view(world, rows, N_COLS)
        if not bool((blocks.abs().amax(dim=(1, 2)) > 0).all()) or (world > 1 and torch.equal(blocks[0], blocks[1])):
            raise SystemExit("bench.py: all-gather result misses a rank's block")
    if args.dump_outputs and rank == 0:
        # what the last timed step handed its caller, copied out before anything else runs on the device
        os.makedirs(args.dump_outputs, exist_ok=True)
        np.save(os.path.join(args.dump_outputs, "features.npy"), y_last.cpu().numpy().astype(np.float32))
    # --- the same step with and without the collective, in THIS process (--compare-collective; every rank runs every variant)
    collective_compare = None
    if distributed and args.compare_collective:
        def timed_variant(sfv):
            for _ in range(max(args.warmup, 100)):
                sfv.step(x)
            torch.cuda.synchronize(dev)
            dist.barrier()
            torch.cuda.synchronize(dev)
            t1 = time.perf_counter()
            for _ in range(args.steps):
                sfv.step(x)
            torch.cuda.synchronize(dev)
            dist.barrier()
            torch.cuda.synchronize(dev)
            tt = torch.tensor([time.perf_counter() - t1], dtype=torch.float64, device=dev)
            dist.all_reduce(tt, op=dist.ReduceOp.MAX)
            return float(tt.item()) / args.steps * 1e3
        collective_compare = {"order": [], "ms_per_step": []}
        for name in ("collective_free", "side_stream", "same_stream", "collective_free", "side_stream", "same_stream"):
            if name == "collective_free":
                sfv = ShardedFlow.for_flow(flow, N_COLS, rows, dev, collective=False)
            elif name == "side_stream":
                sfv = ShardedFlow.for_flow(flow, N_COLS, rows, dev, collective=True, light_events=light_ok or args.gather_stream == "same")
            else:
                sfv = ShardedFlow.for_flow(flow, N_COLS, rows, dev, collective=True, gather_stream="same")
            if sfv.collective and not sfv.verify_against_blocking_gather(x_alts, steps=4):
                raise SystemExit("bench.py: %s does not reproduce a blocking all-gather (rank %d)" % (name, rank))
            collective_compare["order"].append(name)
            collective_compare["ms_per_step"].append(round(timed_variant(sfv), 5))
            sfv.close()
    y = sf.ys[(sf._n - 1) & 1]
    y_prof = torch.empty((rows, N_COLS), dtype=torch.float32, device=dev)

    # --- per-kernel durations: HIP events recorded by the library around every stage launch, on
    # the stream the kernels run on (separate passes, outside the timed region)
    stage_rows = []
    if rank == 0 and args.full:
        L = None
        from pyfaceanalysis_amd import _capi
        L = _capi.lib()
        h = flow._handle()
        prof_steps = max(5, min(11, args.steps))
        samples, names = [], []
        for _ in range(prof_steps):      # one sample per pass; the median drops a pass hit by a host hiccup
            # every profiled pass ends in a synchronisation and a read-back: without load in between the chip's clock sags and the event
            # times read 10-12 % long (seen in round 4's torchrun world-1 line and again in round 5) — 20 plain steps keep it up
            for _ in range(20):
                flow.execute_device(x.data_ptr(), in_dt, rows, x.shape[1], y_prof.data_ptr(), np.float32, N_COLS, N_COLS, stream=stream.cuda_stream)
            _capi.check(L.hg_flow_reset_profile(h.h))
            flow.execute_device(x.data_ptr(), in_dt, rows, x.shape[1], y_prof.data_ptr(), np.float32, N_COLS, N_COLS,
                                stream=stream.cuda_stream, profile=True)
            torch.cuda.synchronize(dev)
            st = flow.stage_times()
            names = [nm for nm, _, _ in st]
            samples.append([ms / max(cnt, 1) for _, ms, cnt in st])
        stage_rows = list(zip(names, np.median(np.asarray(samples), axis=0).tolist()))

    # --- extra figure, NOT the headline: independent batches in flight.  `value` above is one batch after the other on one
    # stream (the contract's step, and what rocprofv3 sees).  A job that has many batches (frames, videos) can keep two or
    # three of them in flight on their own streams, each with its own flow handle and workspace: the ramp and the tail of
    # one batch's kernels (SIMD arbiter skew) are filled by the other's.  Same K full steps, same results.
    in_flight = None
    if args.full and not distributed and not args.no_inflight and not args.generic:
        in_flight = {}
        extra_flows = [Flow.from_blob(blob, device=local_rank, output_dtype=np.float32) for _ in range(2)]
        for f in extra_flows:
            f.reserve(rows)
        pool = [flow] + extra_flows
        streams = [torch.cuda.Stream(dev) for _ in pool]
        ys_f = [torch.empty((rows, N_COLS), dtype=torch.float32, device=dev) for _ in pool]
        for n_par in (2, 3):
            def run(k):
                for s_ in range(k):
                    i = s_ % n_par
                    pool[i].execute_device(x.data_ptr(), in_dt, rows, x.shape[1], ys_f[i].data_ptr(), np.float32, N_COLS, N_COLS,
                                           stream=streams[i].cuda_stream)
                torch.cuda.synchronize(dev)
            run(max(args.warmup, 100))
            t1 = time.perf_counter()
            run(args.steps)
            dt1 = time.perf_counter() - t1
            in_flight[str(n_par)] = {"value": rows * args.steps / dt1, "ms_per_step": dt1 / args.steps * 1e3,
                                     "same_features_as_serial": bool(all(torch.equal(ys_f[i], y) for i in range(min(n_par, args.steps))))}
        for f in extra_flows:
            f.close()

    if rank == 0:
        if args.full:
            # parity of the timed configuration on a slice of the batch (oracle = checker only)
            from oracle import mdp_restate
            m = 64
            check_rows = np.arange(m) * (rows // m) if rows >= m else np.arange(rows)      # rows 0, rows/64, 2 rows/64, ...: every part of the batch
            m = len(check_rows)
            ref = mdp_restate.execute_flow(nodes, x_host[check_rows].astype(np.float64))[:, :N_COLS]
            got = y.cpu().numpy()[check_rows].astype(np.float64)
            max_rel = float(np.abs(got - ref).max() / np.abs(ref).max())
            # worst case per column over the first 20: each column against ITS OWN largest reference magnitude
            per_col = np.abs(got - ref).max(axis=0) / np.abs(ref).max(axis=0)

        total_rows = rows * world
        value = total_rows * args.steps / elapsed
        flops_row = int(info.flops_per_row)
        # dominant kernel = the stage with the largest average duration
        per_layer = []           # (algorithmic FLOPs, algorithmic bytes) per sub-image for every layer kernel
        nodes_out_bytes = []     # fp32 bytes of each layer's output per sub-image
        in_bytes = SIDE * SIDE * in_dt.itemsize
        for nd in nodes:
            if type(nd).__name__ in ("Layer", "CloneLayer"):
                out_bytes = nd.output_dim * 4
                per_layer.append((synth.flops_per_row([nd]), in_bytes + out_bytes))
                nodes_out_bytes.append(out_bytes)
                in_bytes = out_bytes
        roof = None
        if stage_rows:
            # kernels actually launched: a stage that reports ~0 ms was fused into the previous kernel
            # (layers 0+1 share one persistent kernel): merge its FLOPs, keep first input / last output bytes
            kernels = []     # [name, ms, flops/row, bytes/row]
            for i, (nm, ms) in enumerate(stage_rows):
                fl, by = per_layer[i] if (info.plan_kind == 1 and i < len(per_layer)) else (0, 0)
                in_prev = kernels and ms < 0.02 and ("fused in the same persistent kernel" in kernels[-1][0] or "[in the top-of-hierarchy launch]" in nm)
                if in_prev and info.plan_kind == 1 and i < len(per_layer):
                    kernels[-1][2] += fl
                    kernels[-1][3] += nodes_out_bytes[i] - nodes_out_bytes[i - 1]     # swap the intermediate output for the final one
                    kernels[-1][0] += " + " + nm.split(":")[0]
                else:
                    kernels.append([nm, ms, fl, by])
            k_pos = max(range(len(kernels)), key=lambda i: kernels[i][1])
            k_name, k_ms, k_fl, k_by = kernels[k_pos]
            # HBM bytes of this launch: NOT measured in this run (PMC counters need their own rocprofv3 passes) but read
            # from the committed counter profile of the same configuration: entry of the same launch position whose
            # rocprofv3 duration agrees with the live one within 15 % — otherwise the profile is stale and traffic is null
            traffic, traffic_source = None, None
            try:
                if rows == ROWS_PER_GPU and in_dt == np.float32 and world == 1 and args.node_kind == "pca_exp_sfa" and not args.generic:
                    tj = json.load(open(os.path.join(ROOT, "profiles", TRAFFIC_PROFILE)))
                    for key, val in tj.items():
                        if key.startswith("%d|" % k_pos) and abs(val["avg_us"] - k_ms * 1e3) <= 0.15 * k_ms * 1e3:
                            traffic = val["hbm_read_bytes"] + val["hbm_write_bytes"]
                            traffic_source = ("profiles/%s: rocprofv3 --pmc FETCH_SIZE (x2, gfx950 correction) + WRITE_SIZE of "
                                              "kernel %r, committed profile of this configuration, not measured in this run"
                                              % (TRAFFIC_PROFILE, key.split("|", 1)[1]))
            except Exception:
                traffic = None
            if info.plan_kind == 1 and k_fl > 0:
                # the roofline that binds this kernel: arithmetic intensity against the ridge point
                k_flops, k_bytes = k_fl * rows, k_by * rows
                ridge = PEAK_MFMA_F32_TFLOPS * 1e12 / (PEAK_HBM_GBS * 1e9)
                if k_flops / k_bytes >= ridge:
                    ach = k_flops / (k_ms * 1e-3) / 1e12
                    roof = {"bound": "mfma", "achieved": ach, "peak": PEAK_MFMA_F32_TFLOPS, "unit": "TFLOP/s",
                            "frac": ach / PEAK_MFMA_F32_TFLOPS, "traffic": traffic}
                else:
                    ach = k_bytes / (k_ms * 1e-3) / 1e9
                    roof = {"bound": "hbm", "achieved": ach, "peak": PEAK_HBM_GBS, "unit": "GB/s",
                            "frac": ach / PEAK_HBM_GBS, "traffic": traffic}
                roof.update({"traffic_source": traffic_source, "kernel": k_name, "kernel_ms": k_ms, "flops_per_launch": k_flops,
                             "algorithmic_bytes_per_launch": k_bytes,
                             "arithmetic_intensity": k_flops / k_bytes, "ridge": ridge,
                             "tflops": k_flops / (k_ms * 1e-3) / 1e12})
            else:
                gb = rows * SIDE * SIDE * in_dt.itemsize / 1e9
                ach = gb / (k_ms * 1e-3)
                roof = {"bound": "hbm", "achieved": ach, "peak": PEAK_HBM_GBS, "unit": "GB/s",
                        "frac": ach / PEAK_HBM_GBS, "traffic": None, "kernel": k_name, "kernel_ms": k_ms}
            # whole-pipeline view: all kernels of one step against the fp32 MFMA peak
            sum_ms = sum(k_[1] for k_ in kernels)      # launches only: a stage fused into the previous launch reports just the gap between two event records
            roof["pipeline_tflops"] = flops_row * rows / (sum_ms * 1e-3) / 1e12
            roof["pipeline_frac"] = roof["pipeline_tflops"] / PEAK_MFMA_F32_TFLOPS
            roof["stages_ms"] = [round(ms, 4) for _, ms in stage_rows]
            # the same against the untimed loop (the stage durations above carry ~3 us of event overhead each)
            roof["pipeline_frac_timed_loop"] = flops_row * rows / (elapsed / args.steps) / 1e12 / PEAK_MFMA_F32_TFLOPS
        out = {
            "metric": "128x128 sub-images/sec through 11L HiGSFA net",
            "value": value, "unit": "sub-images/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": elapsed / args.steps * 1e3, "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": "f32", "data": "synthetic",
            "config": {"workload": "configs[1]: U11L-128 (11-layer net, " + ("iGSFA nodes, " if args.node_kind == "igsfa" else "") + "trained random-init weights), "
                                   "%d synthetic 128x128 sub-images per GPU per step, %s input resident in HBM, "
                                   "first %d slow features out%s" % (rows, in_dt.name, N_COLS,
                                                                     (", RCCL all-gather of the features " + ("on the kernels' stream" if args.gather_stream == "same" else "overlapped with the next step")) if distributed else ""),
                       "settle_ms": round(settle_ms, 1), "rows_per_gpu": rows, "global_rows": total_rows, "plan": "fused" if info.plan_kind == 1 else "generic",
                       "parallelism": "row-shard x%d" % world, **({"gather_events": gather_events} if gather_events else {})},
            **({"max_rel_err_vs_oracle": max_rel,
                "max_rel_err_first20_percol": {"worst": float(per_col.max()), "worst_column": int(per_col.argmax()),
                                               "per_column": [float("%.3e" % v) for v in per_col], "rows_checked": m,
                                               "row_set": "rows k * %d, k = 0 .. %d (strided over the whole batch)" % (max(1, rows // 64), m - 1),
                                               "definition": "max_i |y[i,c] - ref[i,c]| / max_i |ref[i,c]| per column c"}} if args.full else {}),
            "flops_per_subimage": flops_row, "padded_flops_per_subimage": int(info.padded_flops_per_row),
            **({"roofline": roof} if args.full else {}),
        }
        if in_flight is not None:
            out["batches_in_flight"] = in_flight
        if collective_compare is not None:
            out["collective_compare"] = collective_compare
        if args.full and not args.no_frame and world == 1 and info.plan_kind == 1 and args.node_kind == "pca_exp_sfa":
            try:
                fr = frame_leg(flow, dev, flow_factory=lambda: Flow.from_blob(blob, device=local_rank, output_dtype=np.float32))
                out["frames_per_s"] = fr["frames_per_s"]                 # one frame at a time (latency figure)
                if "frames_in_flight" in fr:
                    out["frames_per_s_4_in_flight"] = fr["frames_in_flight"]["4"]["frames_per_s"]
                out["frame_leg"] = fr
            except Exception as exc:      # noqa: BLE001
                out["frame_leg"] = {"error": "%s: %s" % (type(exc).__name__, exc)}
        if args.full and not args.no_extra_legs and world == 1 and info.plan_kind == 1 and args.node_kind == "pca_exp_sfa" and rows == ROWS_PER_GPU:
            leg_steps = max(50, min(args.steps, 400))
            # figures beside the headline: a leg that fails reports its error and leaves the headline line intact
            for key, leg in (("uniform_input", lambda: uniform_leg(flow, nodes, dev, rows, leg_steps)), ("u11l_64", lambda: u11l_64_leg(dev, rows, leg_steps)),
                             ("host_path", lambda: host_path_leg(blob)), ("train_leg", lambda: train_leg(dev))):
                try:
                    out[key] = leg()
                except Exception as exc:      # noqa: BLE001
                    out[key] = {"error": "%s: %s" % (type(exc).__name__, exc)}
        if args.full and not args.no_cpu_baseline and world == 1:
            out["cpu_baseline"] = cpu_baseline(nodes)
            out["speedup_vs_cpu_baseline"] = value / out["cpu_baseline"]["value"]
            op = out["cpu_baseline"].get("optimised_port")
            if op and op.get("value"):      # the honest CPU point: flat float64 C port, AVX2 + OpenMP, on `cores` of the box's cores
                out["speedup_vs_optimised_c_port"] = {"ratio": value / op["value"], "cores": op.get("cores")}
        # a leg that failed left {"error": ...} under its key: named at the top level too (tools/run_gpu_suite.sh fails on it; the exit
        # code stays 0 so that the headline of a run whose side leg broke is not lost — ADVICE r4)
        out["legs_failed"] = [k for k, v in out.items() if isinstance(v, dict) and "error" in v]
        print(json.dumps(out), flush=True)
    flow.close()
    if distributed:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
