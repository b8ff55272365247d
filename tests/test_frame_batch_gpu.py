"""GPU: a stack of same-size frames through one pooled pass — ``hg_patcher_extract_frames_device``, ``DeviceCascade.detect_frames`` and
``DeviceCascade.detect_faces_frames`` — against the per-frame calls, which are their exact oracle: every row of the cascade is
independent of its batch and every compaction keeps row order, so every comparison is ``array_equal``.

The pieces are those of tests/test_frame_stream_gpu.py (its ``Rig``: U11L-64 as the face flow and the eye flow, SUB = (64, 64), K = 20,
SF = 0.1, box-filtered seeded noise frames, ``Rig.fresh()`` objects per frame as the oracle; the cascade calibrated with
BC.KEEP / BC.LATER_KEEP so that the small frames have survivors); the cases are in tests/frame_batch_cases.py.
The per-frame answers of a (size, seed) are computed once on fresh objects and shared among the tests.
"""
import numpy as np
import pytest

from tests import frame_batch_cases as BC
from tests import test_frame_stream_gpu as FS

pytestmark = pytest.mark.gpu

SF = FS.SF
DET_KEYS = FS.DET_KEYS


@pytest.fixture(scope="module")
def rig(native_lib, nets):
    r = FS.Rig(nets, keep=BC.KEEP, later_keep=BC.LATER_KEEP)
    yield r
    r.close()


_ANSWERS = {}


def frame_of(size, seed):
    """A frame of the cascade tests: seeded noise, or a constant grey frame for seed = None."""
    w, h = size
    return np.full((h, w), 128, dtype=np.uint8) if seed is None else BC.noise_frame(w, h, seed)


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def per_frame(rig, size, seed):
    """(detect_frame, detect_faces) of objects created for this frame alone; computed once per (size, seed) and never modified."""
    key = (size, seed)
    if key not in _ANSWERS:
        _ANSWERS[key] = rig.fresh_answers(dev(frame_of(size, seed)), smallest_face=SF)
    return _ANSWERS[key]


def pooled_counts(dets):
    """What the pooled call reports for these per-frame results: the sum where the counts are read, -1 where they are not.  A frame
    that has lost all its candidates reports 0 for every later stage without reading anything; pooled, such a stage is read or not as
    it is for the frames that still have candidates — -1 as soon as one frame says -1, else the sum (all 0 when every frame is out)."""
    counts = np.array([d["counts"] for d in dets])
    assert all((col[col >= 0] == 0).all() for col in counts.T if (col == -1).any()), "beside a count that was not read only a frame that is out"
    return [(-1 if (col == -1).any() else int(col.sum())) for col in counts.T]


def assert_pooled_detection(got, dets, what):
    assert len(got["frames"]) == len(dets), what
    for f, (g, d) in enumerate(zip(got["frames"], dets)):
        for key in DET_KEYS:
            assert g[key].shape == d[key].shape and g[key].dtype == d[key].dtype and np.array_equal(g[key], d[key]), (what, f, key)
    assert got["counts"] == pooled_counts(dets), what
    assert got["rows_executed"] == sum(d["rows_executed"] for d in dets), what
    assert got["n_windows"] == sum(d["n_windows"] for d in dets), what


def assert_pooled_faces(got, faces, what):
    assert len(got["faces"]) == len(faces) and len(got["n_before_purge"]) == len(faces), what
    for f, (g, d) in enumerate(zip(got["faces"], faces)):
        assert g.shape == d["faces"].shape and np.array_equal(g, d["faces"]), (what, f)
        assert got["n_before_purge"][f] == d["n_before_purge"], (what, f)
    assert got["counts"] == pooled_counts(faces), what
    assert got["rows_executed"] == sum(d["rows_executed"] for d in faces), what
    assert got["n_windows"] == sum(d["n_windows"] for d in faces), what


def stack_of(size, seeds):
    import torch
    return torch.stack([dev(frame_of(size, s)) for s in seeds])


def survivors(det):
    return len(det["coords"])


# ---- 1. the patcher entry -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("filt", BC.FILTERS)
def test_patcher_frames_against_per_frame_entry(native_lib, filt):
    """Three 97x131 frames cut as views out of one buffer of 255s (ld 144, frame stride 18941, not a multiple of ld), 60 rows with
    interleaved frame indices: windows inside, overhanging on each side and wholly outside, unrotated (no angles) and rotated by
    0, 90, -90, 180, +-22.5 and 11 degrees, outputs 64x64, 24x24 and 6x5 as uint8 and float32.  Every row equals the per-frame entry's
    row on that frame alone; the rows whose frame index is -1 or >= n_frames are all zero while their neighbours are right."""
    import torch
    from pyfaceanalysis_amd.patches import Patcher
    buf_h, offsets = BC.stack_buffer()
    boxes_h, angles_h, row_frame_h = BC.windows()
    buf, boxes, angles, row_frame = dev(buf_h), dev(boxes_h), dev(-angles_h), dev(row_frame_h)
    good = np.array([0 <= f < BC.N_FRAMES for f in row_frame_h])
    assert (~good).sum() == len(BC.BAD_ROWS) and all(good[i - 1] and good[i + 1] for i in (7, 23)) and good[40] and good[43]
    assert len(set(row_frame_h[good])) == BC.N_FRAMES
    pt, ref = Patcher(), Patcher()
    stream = torch.cuda.current_stream().cuda_stream
    try:
        for (w, h) in BC.OUT_SIZES:
            for dt, tdt in ((np.uint8, torch.uint8), (np.float32, torch.float32)):
                for ang in (None, angles):
                    what = (filt, w, h, dt.__name__, ang is not None)
                    out = torch.full((BC.N_ROWS, w * h), 7, dtype=tdt, device="cuda")
                    pt.extract_frames_device(buf.data_ptr() + offsets[0], BC.N_FRAMES, BC.FRAME_STRIDE, BC.H, BC.W, BC.LD, boxes.data_ptr(),
                                             row_frame.data_ptr(), BC.N_ROWS, (w, h), out.data_ptr(), dt, w * h, stream=stream,
                                             delta_angs_ptr=None if ang is None else ang.data_ptr(), interpolation=filt)
                    want = torch.zeros((BC.N_ROWS, w * h), dtype=tdt, device="cuda")
                    for f in range(BC.N_FRAMES):
                        idx = np.flatnonzero(row_frame_h == f)
                        b_f = boxes[torch.from_numpy(idx).cuda()].contiguous()
                        a_f = None if ang is None else ang[torch.from_numpy(idx).cuda()].contiguous()
                        o_f = torch.empty((len(idx), w * h), dtype=tdt, device="cuda")
                        ref.extract_device(buf.data_ptr() + offsets[f], np.uint8, BC.H, BC.W, BC.LD, b_f.data_ptr(), len(idx), (w, h), o_f.data_ptr(), dt,
                                           w * h, stream=stream, delta_angs_ptr=None if a_f is None else a_f.data_ptr(), interpolation=filt)
                        want[torch.from_numpy(idx).cuda()] = o_f
                    torch.cuda.synchronize()
                    got_h, want_h = out.cpu().numpy(), want.cpu().numpy()
                    assert np.array_equal(got_h, want_h), (what, np.flatnonzero((got_h != want_h).any(axis=1)))
                    assert not got_h[~good].any(), what
                    assert (want_h[good] != 0).any(axis=1).sum() >= 30, "the oracle's rows are not empty windows"
    finally:
        pt.close()
        ref.close()


def test_patcher_frames_n_zero_and_refusals_on_a_live_handle(native_lib):
    """n == 0 is HG_OK; a frame stride one byte below the bound and ld < frame_w are refused by a live handle as by a dummy one."""
    import torch
    from pyfaceanalysis_amd.patches import Patcher
    pt = Patcher()
    try:
        buf = torch.zeros(4096, dtype=torch.uint8, device="cuda")
        boxes = torch.zeros((1, 4), dtype=torch.float64, device="cuda")
        rf = torch.zeros(1, dtype=torch.int32, device="cuda")
        out = torch.zeros(64, dtype=torch.uint8, device="cuda")
        args = lambda stride, ld, n: (buf.data_ptr(), 2, stride, 10, 20, ld, boxes.data_ptr(), rf.data_ptr(), n, (8, 8), out.data_ptr(), np.uint8, 64)
        pt.extract_frames_device(*args(9 * 24 + 20, 24, 0))
        pt.extract_frames_device(*args(9 * 24 + 20, 24, 1))
        with pytest.raises(ValueError):
            pt.extract_frames_device(*args(9 * 24 + 19, 24, 1))
        with pytest.raises(ValueError):
            pt.extract_frames_device(*args(4000, 19, 1))
        torch.cuda.synchronize()
    finally:
        pt.close()


# ---- 2. detect_frames against detect_frame ----------------------------------------------------------------------------------------------
def test_detect_frames_three_small_frames(rig):
    """B = 3 of 97x131 (3 x 397 windows), seeds BC.SMALL_SEEDS, against ``detect_frame`` on fresh objects per frame: every per-frame
    array, the pooled counts (sums, and -1 where the per-frame counts are -1), rows_executed, n_windows.  Survivors per frame, observed
    on an MI355X and asserted below: see BC.SMALL_SEEDS."""
    dets = [per_frame(rig, BC.SMALL, s)[0] for s in BC.SMALL_SEEDS]
    n = [survivors(d) for d in dets]
    assert sum(1 for x in n if x > 0) >= 2 and 0 in n and len(set(x for x in n if x > 0)) >= 2, n
    assert all(d["n_windows"] == 397 for d in dets)
    dc, loc, close = rig.fresh()
    try:
        assert_pooled_detection(dc.detect_frames(stack_of(BC.SMALL, BC.SMALL_SEEDS), smallest_face=SF), dets, "B = 3 of 97x131")
    finally:
        close()


# ---- 3. B = 1 --------------------------------------------------------------------------------------------------------------------------
def test_single_frame_stack_equals_per_frame_calls(rig):
    """B = 1 equals ``detect_frame`` / ``detect_faces`` in every field (a frame with survivors and faces)."""
    seed = BC.MEDIUM_SEEDS[0]
    det, faces = per_frame(rig, BC.MEDIUM, seed)
    assert survivors(det) > 0 and len(faces["faces"]) > 0
    dc, loc, close = rig.fresh()
    try:
        st = stack_of(BC.MEDIUM, [seed])
        got = dc.detect_frames(st, smallest_face=SF)
        assert_pooled_detection(got, [det], "B = 1")
        assert got["counts"] == det["counts"] and got["rows_executed"] == det["rows_executed"] and got["n_windows"] == det["n_windows"]
        gf = dc.detect_faces_frames(st, loc, smallest_face=SF)
        assert_pooled_faces(gf, [faces], "B = 1, faces")
        assert gf["counts"] == faces["counts"] and gf["n_before_purge"] == [faces["n_before_purge"]]
    finally:
        close()


# ---- 4. the same frame four times, and a permutation -----------------------------------------------------------------------------------
def test_repeated_and_permuted_stacks(rig):
    """The same frame four times gives four identical answers (the one frame's); a permuted stack gives the permuted answers."""
    seeds = BC.SMALL_SEEDS
    dets = [per_frame(rig, BC.SMALL, s)[0] for s in seeds]
    live = [s for s, d in zip(seeds, dets) if survivors(d) > 0][0]
    dc, loc, close = rig.fresh()
    try:
        got = dc.detect_frames(stack_of(BC.SMALL, [live] * 4), smallest_face=SF)
        assert_pooled_detection(got, [per_frame(rig, BC.SMALL, live)[0]] * 4, "one frame four times")
        perm = (2, 0, 1)
        got = dc.detect_frames(stack_of(BC.SMALL, [seeds[p] for p in perm]), smallest_face=SF)
        assert_pooled_detection(got, [dets[p] for p in perm], "permuted stack")
        gf = dc.detect_faces_frames(stack_of(BC.SMALL, [seeds[p] for p in perm]), loc, smallest_face=SF)
        assert_pooled_faces(gf, [per_frame(rig, BC.SMALL, seeds[p])[1] for p in perm], "permuted stack, faces")
    finally:
        close()


# ---- 5. the chunked glue path ------------------------------------------------------------------------------------------------------------
def test_two_long_frames_take_the_chunked_glue(rig):
    """B = 2 of 2000x300 (prescaled to 1000x150: 2 x 5148 = 10296 candidates, above 2 * kChunk = 8192): the two-launch glue of the
    first group, against the per-frame calls (which take the single-workgroup glue)."""
    pairs = [per_frame(rig, BC.LONG, s) for s in BC.LONG_SEEDS]
    assert all(p[0]["n_windows"] == 5148 for p in pairs) and 2 * 5148 > 2 * 4096
    assert any(survivors(p[0]) > 0 for p in pairs)
    dc, loc, close = rig.fresh()
    try:
        st = stack_of(BC.LONG, BC.LONG_SEEDS)
        assert_pooled_detection(dc.detect_frames(st, smallest_face=SF), [p[0] for p in pairs], "B = 2 of 2000x300")
        assert_pooled_faces(dc.detect_faces_frames(st, loc, smallest_face=SF), [p[1] for p in pairs], "B = 2 of 2000x300, faces")
    finally:
        close()


# ---- 6. detect_faces_frames against detect_faces ---------------------------------------------------------------------------------------
def test_detect_faces_frames_against_detect_faces(rig):
    """B = 3 of 320x240 (seeds BC.MEDIUM_SEEDS) and B = 3 of 97x131 (BC.SMALL_SEEDS: a frame without a survivor between two that have
    some), as separate calls on the same objects — sizes do not mix — against ``detect_faces`` per frame: faces, n_before_purge, counts.  At least one
    frame's purge drops a row.  Observed on an MI355X: see BC.MEDIUM_SEEDS / BC.SMALL_SEEDS."""
    dc, loc, close = rig.fresh()
    try:
        dropped = 0
        for size, seeds in ((BC.MEDIUM, BC.MEDIUM_SEEDS), (BC.SMALL, BC.SMALL_SEEDS)):
            faces = [per_frame(rig, size, s)[1] for s in seeds]
            if size == BC.SMALL:
                n = [survivors(per_frame(rig, size, s)[0]) for s in seeds]
                assert n[0] > 0 and n[1] == 0 and n[2] > 0, n
            dropped += sum(1 for d in faces if d["n_before_purge"] > len(d["faces"]))
            assert_pooled_faces(dc.detect_faces_frames(stack_of(size, seeds), loc, smallest_face=SF), faces, ("faces", size))
        assert dropped >= 1, "no frame's purge drops a row: the per-frame purge is not exercised"
    finally:
        close()


# ---- 7. prescale and colour ------------------------------------------------------------------------------------------------------------
def test_prescale_and_colour_stacks(rig):
    """Two 1280x720 RGB frames with prescale_filter = "BILINEAR" (prescaled to 1000x562, 1738 windows each), pooled against per-frame;
    then the same frames grey (PIL's "L" of them) with the NEAREST prescale."""
    import torch
    from pyfaceanalysis_amd.cascade import DeviceCascade
    w, h = BC.HD
    from pyfaceanalysis_amd import frames as F
    noise = [BC.hd_frame(s) for s in BC.HD_SEEDS]
    rgb = [np.ascontiguousarray(np.stack([n, n, 255 - n], axis=2)) for n in noise]
    grey = [F.to_gray_host(frame, "RGB") for frame in rgb]
    for fmt, filt, frames in (("RGB", "BILINEAR", rgb), ("L", "NEAREST", grey)):
        dc = DeviceCascade(rig.stages, FS.SUB, FS.K, rig.pipe, frame_format=fmt, prescale_filter=filt)
        try:
            fdev = [dev(f) for f in frames]
            dets = [dc.detect_frame(f, smallest_face=SF) for f in fdev]
            faces = [dc.detect_faces(f, rig.loc, smallest_face=SF) for f in fdev]
            assert all(d["n_windows"] == 1738 for d in dets) and any(survivors(d) > 0 for d in dets)
            assert_pooled_detection(dc.detect_frames(torch.stack(fdev), smallest_face=SF), dets, (fmt, filt))
            assert_pooled_faces(dc.detect_faces_frames(torch.stack(fdev), rig.loc, smallest_face=SF), faces, (fmt, filt, "faces"))
        finally:
            dc.close()


# ---- 8. stage filters ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("filt", (2, 3))
def test_stage_filters(rig, filt):
    """interpolation_formats all BILINEAR / all BICUBIC, B = 2 of 97x131, pooled against per-frame; with BICUBIC also
    ``EyeLocator(interpolation="BICUBIC")`` through ``detect_faces_frames``."""
    import torch
    from pyfaceanalysis_amd.cascade import DeviceCascade
    from pyfaceanalysis_amd.eyes import EyeLocator
    dc = DeviceCascade(rig.stages, FS.SUB, FS.K, rig.pipe, interpolation_formats=[filt] * 10)
    loc = EyeLocator(rig.eye_flow, rig.clf_x, rig.eye_flow, rig.clf_y, contrast=FS.CONTRAST, interpolation=filt)
    try:
        fdev = [dev(frame_of(BC.SMALL, s)) for s in BC.SMALL_SEEDS[:2]]
        dets = [dc.detect_frame(f, smallest_face=SF) for f in fdev]
        faces = [dc.detect_faces(f, loc, smallest_face=SF) for f in fdev]
        assert_pooled_detection(dc.detect_frames(torch.stack(fdev), smallest_face=SF), dets, ("stage filter", filt))
        assert_pooled_faces(dc.detect_faces_frames(torch.stack(fdev), loc, smallest_face=SF), faces, ("stage filter", filt, "faces"))
    finally:
        loc.close()
        dc.close()


# ---- 9. layouts ------------------------------------------------------------------------------------------------------------------------
def test_stack_layouts(rig):
    """The stack as every second frame of a larger stack, with stride(1) > W (crops of wider frames), as a contiguous tensor and as a
    list of tensors: the same results, the per-frame calls'.  The frames between and the columns beside hold 255."""
    import torch
    w, h = BC.MEDIUM
    seeds = BC.MEDIUM_SEEDS
    faces = [per_frame(rig, BC.MEDIUM, s)[1] for s in seeds]
    dets = [per_frame(rig, BC.MEDIUM, s)[0] for s in seeds]
    frames = [frame_of(BC.MEDIUM, s) for s in seeds]
    big = torch.full((2 * len(seeds), h, w), 255, dtype=torch.uint8, device="cuda")
    wide = torch.full((len(seeds), h + 3, w + 37), 255, dtype=torch.uint8, device="cuda")
    for f, fr in enumerate(frames):
        big[2 * f] = dev(fr)
        wide[f, 2:2 + h, 5:5 + w] = dev(fr)
    layouts = {"every second frame": big[::2], "stride(1) > W": wide[:, 2:2 + h, 5:5 + w], "contiguous": torch.stack([dev(f) for f in frames]),
               "list": [dev(f) for f in frames]}
    assert layouts["every second frame"].stride(0) == 2 * h * w and layouts["stride(1) > W"].stride(1) == w + 37
    dc, loc, close = rig.fresh()
    try:
        for name, st in layouts.items():
            assert_pooled_detection(dc.detect_frames(st, smallest_face=SF), dets, name)
            assert_pooled_faces(dc.detect_faces_frames(st, loc, smallest_face=SF), faces, name)
        with pytest.raises(ValueError):
            dc.detect_frames(dev(frames[0])[None].expand(3, h, w), smallest_face=SF)      # a broadcast view: frames 0 bytes apart
        with pytest.raises(ValueError):
            dc.detect_frames(dev(frames[0])[:, :1].expand(h, w)[None], smallest_face=SF)  # stride(2) == 0
    finally:
        close()


# ---- 10. state -------------------------------------------------------------------------------------------------------------------------
def test_state_across_pooled_and_per_frame_calls(rig):
    """ONE long-lived cascade and locator: pooled B = 3 (320x240), a per-frame ``detect_faces``, pooled B = 2 of another size (97x131),
    pooled B = 5 of the first size (the buffers grow), a per-frame call again — each against fresh objects.  Crosses the keyed table
    ring, ``reserve``, the prescale state and the eye workspace."""
    dc, loc, close = rig.fresh()
    try:
        m, s = BC.MEDIUM_SEEDS, BC.SMALL_SEEDS
        assert_pooled_faces(dc.detect_faces_frames(stack_of(BC.MEDIUM, m), loc, smallest_face=SF), [per_frame(rig, BC.MEDIUM, x)[1] for x in m], "pooled B = 3")
        FS.assert_same_faces(dc.detect_faces(dev(frame_of(BC.MEDIUM, m[2])), loc, smallest_face=SF), per_frame(rig, BC.MEDIUM, m[2])[1], "per frame after pooled")
        assert_pooled_faces(dc.detect_faces_frames(stack_of(BC.SMALL, s[:2]), loc, smallest_face=SF), [per_frame(rig, BC.SMALL, x)[1] for x in s[:2]], "pooled B = 2, other size")
        five = [m[0], m[2], m[1], m[0], m[2]]
        assert_pooled_faces(dc.detect_faces_frames(stack_of(BC.MEDIUM, five), loc, smallest_face=SF), [per_frame(rig, BC.MEDIUM, x)[1] for x in five], "pooled B = 5")
        assert_pooled_detection(dc.detect_frames(stack_of(BC.MEDIUM, five), smallest_face=SF), [per_frame(rig, BC.MEDIUM, x)[0] for x in five], "pooled B = 5, detections")
        FS.assert_same_faces(dc.detect_faces(dev(frame_of(BC.SMALL, s[0])), loc, smallest_face=SF), per_frame(rig, BC.SMALL, s[0])[1], "per frame at the end")
        FS.assert_same_detection(dc.detect_frame(dev(frame_of(BC.MEDIUM, m[0])), smallest_face=SF), per_frame(rig, BC.MEDIUM, m[0])[0], "detect_frame at the end")
    finally:
        close()


# ---- 11. HIGSFA_CASCADE_NO_GROUPS ------------------------------------------------------------------------------------------------------
def test_no_groups_gives_the_same_rows(rig, monkeypatch):
    """HIGSFA_CASCADE_NO_GROUPS=1 (every stage a group of its own) gives the pooled call's same rows."""
    dc, loc, close = rig.fresh()
    try:
        st = stack_of(BC.MEDIUM, BC.MEDIUM_SEEDS)
        a = dc.detect_frames(st, smallest_face=SF)
        fa = dc.detect_faces_frames(st, loc, smallest_face=SF)
        monkeypatch.setenv("HIGSFA_CASCADE_NO_GROUPS", "1")
        b = dc.detect_frames(st, smallest_face=SF)
        fb = dc.detect_faces_frames(st, loc, smallest_face=SF)
        monkeypatch.delenv("HIGSFA_CASCADE_NO_GROUPS")
        assert sum(len(f["coords"]) for f in a["frames"]) > 0
        for f, (x, y) in enumerate(zip(a["frames"], b["frames"])):
            for key in DET_KEYS:
                assert np.array_equal(x[key], y[key]), (f, key)
        for f, (x, y) in enumerate(zip(fa["faces"], fb["faces"])):
            assert x.shape == y.shape and np.array_equal(x, y), f
        assert fa["n_before_purge"] == fb["n_before_purge"]
        # ungrouped, a count is read after every stage: where both report one it is the same number
        assert all(p == q for p, q in zip(a["counts"], b["counts"]) if p >= 0 and q >= 0) and b["counts"][-1] == a["counts"][-1]
    finally:
        close()
