"""GPU: a LIST of frames of different sizes through one pooled pass — ``hg_patcher_extract_frame_list_device``,
``DeviceCascade.detect_frame_list`` and ``DeviceCascade.detect_faces_frame_list`` — against the per-frame calls, which are their exact
oracle (rows are independent of their batch, every compaction keeps row order): every comparison is ``array_equal``.

The rig, the per-frame answers (computed once per (size, seed) on fresh objects and shared) and the pooled-count rule are those of
tests/test_frame_batch_gpu.py; the cases are in tests/frame_list_cases.py.  Every test asserts its premises from the per-frame answers
before it compares, so none can pass on empty results.
"""
import numpy as np
import pytest

from tests import frame_batch_cases as BC
from tests import frame_list_cases as LC
from tests import test_frame_batch_gpu as FB
from tests import test_frame_stream_gpu as FS

pytestmark = pytest.mark.gpu

SF = FS.SF
dev, frame_of, per_frame, survivors = FB.dev, FB.frame_of, FB.per_frame, FB.survivors
assert_pooled_detection, assert_pooled_faces = FB.assert_pooled_detection, FB.assert_pooled_faces


@pytest.fixture(scope="module")
def rig(native_lib, nets):
    r = FS.Rig(nets, keep=BC.KEEP, later_keep=BC.LATER_KEEP)
    yield r
    r.close()


def list_of(case):
    return [dev(frame_of(size, seed)) for size, seed in case]


def answers(rig, case):
    pairs = [per_frame(rig, size, seed) for size, seed in case]
    return [p[0] for p in pairs], [p[1] for p in pairs]


def check_list(rig, dc, loc, case, what, frames=None):
    dets, faces = answers(rig, case)
    fl = list_of(case) if frames is None else frames
    assert_pooled_detection(dc.detect_frame_list(fl, smallest_face=SF), dets, what)
    assert_pooled_faces(dc.detect_faces_frame_list(fl, loc, smallest_face=SF), faces, (what, "faces"))


# ---- 1. the patcher entry -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("filt", BC.FILTERS)
def test_patcher_frame_list_against_per_frame_entry(native_lib, filt):
    """Three frames of different sizes and row strides (7x5 / ld 9, 97x131 / ld 144, 40x61 / ld 40: small, large, small) as views out of
    one buffer of 255s, 60 rows with interleaved frame indices, the windows scaled to each row's own frame; unrotated and rotated by
    BC.ANGLES, BC.OUT_SIZES, uint8 and float32.  Every row equals hg_patcher_extract_filter_device's on that frame alone; the rows
    whose frame index is -1 or >= n_frames are all zero between correct neighbours."""
    import torch
    from pyfaceanalysis_amd.patches import Patcher
    buf_h, offsets = LC.patch_buffer()
    boxes_h, angles_h, row_frame_h = LC.patch_windows()
    nf = len(LC.PATCH_FRAMES)
    buf, boxes, angles, row_frame = dev(buf_h), dev(boxes_h), dev(-angles_h), dev(row_frame_h)
    good = np.array([0 <= f < nf for f in row_frame_h])
    assert (~good).sum() == len(LC.BAD_ROWS) and all(good[i - 1] and good[i + 1] for i in (7, 23)) and good[40] and good[43]
    assert len(set(row_frame_h[good])) == nf
    sizes = [f[0] * f[1] for f in LC.PATCH_FRAMES]
    assert sizes[0] < sizes[1] > sizes[2], "small -> large -> small"
    refs = [(buf.data_ptr() + off, h, w, ld) for (w, h, ld, _s), off in zip(LC.PATCH_FRAMES, offsets)]
    pt, ref = Patcher(), Patcher()
    stream = torch.cuda.current_stream().cuda_stream
    try:
        for (w, h) in BC.OUT_SIZES:
            for dt, tdt in ((np.uint8, torch.uint8), (np.float32, torch.float32)):
                for ang in (None, angles):
                    what = (filt, w, h, dt.__name__, ang is not None)
                    out = torch.full((LC.N_ROWS, w * h), 7, dtype=tdt, device="cuda")
                    pt.extract_frame_list_device(refs, boxes.data_ptr(), row_frame.data_ptr(), LC.N_ROWS, (w, h), out.data_ptr(), dt, w * h, stream=stream,
                                                 delta_angs_ptr=None if ang is None else ang.data_ptr(), interpolation=filt)
                    want = torch.zeros((LC.N_ROWS, w * h), dtype=tdt, device="cuda")
                    for f, (ptr, fh, fw, ld) in enumerate(refs):
                        idx = torch.from_numpy(np.flatnonzero(row_frame_h == f)).cuda()
                        b_f = boxes[idx].contiguous()
                        a_f = None if ang is None else ang[idx].contiguous()
                        o_f = torch.empty((len(idx), w * h), dtype=tdt, device="cuda")
                        ref.extract_device(ptr, np.uint8, fh, fw, ld, b_f.data_ptr(), len(idx), (w, h), o_f.data_ptr(), dt, w * h, stream=stream,
                                           delta_angs_ptr=None if a_f is None else a_f.data_ptr(), interpolation=filt)
                        want[idx] = o_f
                    torch.cuda.synchronize()
                    got_h, want_h = out.cpu().numpy(), want.cpu().numpy()
                    assert np.array_equal(got_h, want_h), (what, np.flatnonzero((got_h != want_h).any(axis=1)))
                    assert not got_h[~good].any(), what
                    for f in range(nf):      # the oracle's rows of EVERY frame are not empty windows
                        assert (want_h[row_frame_h == f] != 0).any(axis=1).sum() >= 8, (what, f)
    finally:
        pt.close()
        ref.close()


# ---- 2. the list pass against the per-frame calls -----------------------------------------------------------------------------------
def test_mixed_list_against_per_frame_calls(rig):
    """[SMALL 9209, MEDIUM 9210, SMALL 9200, MEDIUM 9200, SMALL 9202]: a frame with survivors, one with none between two that have some,
    one with one; the purge drops a row of MEDIUM 9210.  Counts, rows_executed, n_windows and n_before_purge by the pooled rule."""
    dets, faces = answers(rig, LC.MIXED)
    n = [survivors(d) for d in dets]
    assert n[0] > 1 and n[2] == 0 and n[4] == 1 and n[1] > 0 and n[3] > 0, n
    assert faces[1]["n_before_purge"] > len(faces[1]["faces"]), "the purge drops a row of MEDIUM 9210"
    assert [d["n_windows"] for d in dets] == [397, 1308, 397, 1308, 397]
    dc, loc, close = rig.fresh()
    try:
        check_list(rig, dc, loc, LC.MIXED, "mixed list")
    finally:
        close()


# ---- 3. equivalences ----------------------------------------------------------------------------------------------------------------
def test_list_equivalences(rig):
    """A list of one frame; a same-size list equals ``detect_frames`` on the stack; a permuted list gives the permuted results; one frame
    three times between others."""
    import torch
    dc, loc, close = rig.fresh()
    try:
        one = (LC.MIXED[1],)
        det, faces = per_frame(rig, *one[0])
        assert survivors(det) > 0 and len(faces["faces"]) > 0
        got = dc.detect_frame_list(list_of(one), smallest_face=SF)
        assert_pooled_detection(got, [det], "a list of one")
        assert got["counts"] == det["counts"] and got["rows_executed"] == det["rows_executed"] and got["n_windows"] == det["n_windows"]
        gf = dc.detect_faces_frame_list(list_of(one), loc, smallest_face=SF)
        assert_pooled_faces(gf, [faces], "a list of one, faces")
        assert gf["counts"] == faces["counts"] and gf["n_before_purge"] == [faces["n_before_purge"]]

        same = tuple((BC.MEDIUM, s) for s in BC.MEDIUM_SEEDS)
        fl = list_of(same)
        a, b = dc.detect_frame_list(fl, smallest_face=SF), dc.detect_frames(torch.stack(fl), smallest_face=SF)
        assert sum(survivors(f) for f in b["frames"]) > 0
        assert_pooled_detection(a, answers(rig, same)[0], "same-size list")
        for x, y in zip(a["frames"], b["frames"]):
            for key in FS.DET_KEYS:
                assert np.array_equal(x[key], y[key]), key
        assert (a["counts"], a["rows_executed"], a["n_windows"]) == (b["counts"], b["rows_executed"], b["n_windows"])
        fa, fb = dc.detect_faces_frame_list(fl, loc, smallest_face=SF), dc.detect_faces_frames(torch.stack(fl), loc, smallest_face=SF)
        assert all(np.array_equal(x, y) for x, y in zip(fa["faces"], fb["faces"])) and fa["n_before_purge"] == fb["n_before_purge"]
        assert fa["counts"] == fb["counts"]

        perm = (3, 0, 4, 2, 1)
        check_list(rig, dc, loc, tuple(LC.MIXED[p] for p in perm), "permuted list")
        thrice = (LC.MIXED[0], LC.MIXED[1], LC.MIXED[3], LC.MIXED[1], LC.MIXED[4], LC.MIXED[1])
        check_list(rig, dc, loc, thrice, "one frame three times between others")
    finally:
        close()


# ---- 4. the chunked glue ------------------------------------------------------------------------------------------------------------
def test_list_takes_the_chunked_glue(rig):
    """[LONG 9200, MEDIUM 9210, MEDIUM 9200, MEDIUM 9211, SMALL 9209]: 9469 candidates, above 2 * kChunk = 8192, the frame boundaries off
    the 8192 edge: the two-launch glue of the first group against the per-frame calls (which take the single-workgroup glue)."""
    dets, faces = answers(rig, LC.CHUNKED)
    total = sum(d["n_windows"] for d in dets)
    first = np.cumsum([0] + [d["n_windows"] for d in dets])
    assert total == LC.CHUNKED_TOTAL == 9469 and total > 8192 and 8192 not in first and first[1] < 8192 < first[-1]
    assert survivors(dets[0]) > 0 and survivors(dets[-1]) > 0 and all(survivors(d) > 0 for d in dets[1:4])
    dc, loc, close = rig.fresh()
    try:
        check_list(rig, dc, loc, LC.CHUNKED, "chunked list")
    finally:
        close()


# ---- 5. tables ----------------------------------------------------------------------------------------------------------------------
def test_shared_and_equal_count_grids(rig):
    """1280x720 and 1920x1080 share one grid (and one set of first-stage tables) behind the prescale; 320x240 and 640x480 have equal
    window counts and different grids (their own tables)."""
    dets, faces = answers(rig, LC.TABLES)
    assert [d["n_windows"] for d in dets] == [1738, 1308, 1738, 1308]
    assert sum(1 for d in dets if survivors(d) > 0) >= 3, [survivors(d) for d in dets]
    dc, loc, close = rig.fresh()
    try:
        check_list(rig, dc, loc, LC.TABLES, "shared and equal-count grids")
    finally:
        close()


def test_more_grids_than_ring_slots(rig):
    """Six small sizes with six distinct grids — more than the keyed ring's four slots — called twice and then in reverse order: the
    tables of a call live in one buffer for the whole call."""
    case = LC.many_grids_list()
    dets, faces = answers(rig, case)
    assert sum(1 for d in dets if survivors(d) > 0) >= 3, [survivors(d) for d in dets]
    for (size, (seed, counts)), d, f in zip(LC.MANY_GRIDS.items(), dets, faces):
        if seed is not None:
            assert (survivors(d), f["n_before_purge"], len(f["faces"])) == counts, (size, seed)
    dc, loc, close = rig.fresh()
    try:
        check_list(rig, dc, loc, case, "six grids")
        check_list(rig, dc, loc, case, "six grids, again")
        check_list(rig, dc, loc, case[::-1], "six grids, reversed")
    finally:
        close()


# ---- 6. layouts and formats ---------------------------------------------------------------------------------------------------------
def test_crops_with_their_own_row_strides(rig):
    """Every frame a crop of a larger tensor of 255s with its own row stride."""
    import torch
    frames = []
    for i, (size, seed) in enumerate(LC.MIXED):
        w, h = size
        big = torch.full((h + 3 + i, w + 11 + 7 * i), 255, dtype=torch.uint8, device="cuda")
        big[2:2 + h, 5 + i:5 + i + w] = dev(frame_of(size, seed))
        frames.append(big[2:2 + h, 5 + i:5 + i + w])
    assert len({f.stride(0) for f in frames}) == len(frames) and all(f.stride(0) > f.shape[1] for f in frames)
    assert any(survivors(d) > 0 for d in answers(rig, LC.MIXED)[0])
    dc, loc, close = rig.fresh()
    try:
        check_list(rig, dc, loc, LC.MIXED, "crops", frames=frames)
    finally:
        close()


def test_colour_list_behind_a_bilinear_prescale(rig):
    """An RGB list of [hd_frame 9300 as (n, n, 255 - n), a 320x240 frame] with prescale_filter = "BILINEAR": the first is prescaled, the
    second converted whole; against the per-frame calls of the same cascade configuration."""
    from pyfaceanalysis_amd.cascade import DeviceCascade
    n = BC.hd_frame(BC.HD_SEEDS[0])
    m = frame_of(BC.MEDIUM, BC.MEDIUM_SEEDS[0])
    rgb = [np.ascontiguousarray(np.stack([x, x, 255 - x], axis=2)) for x in (n, m)]
    dc = DeviceCascade(rig.stages, FS.SUB, FS.K, rig.pipe, frame_format="RGB", prescale_filter="BILINEAR")
    ref = DeviceCascade(rig.stages, FS.SUB, FS.K, rig.pipe, frame_format="RGB", prescale_filter="BILINEAR")
    try:
        fdev = [dev(f) for f in rgb]
        dets = [ref.detect_frame(f, smallest_face=SF) for f in fdev]
        faces = [ref.detect_faces(f, rig.loc, smallest_face=SF) for f in fdev]
        assert [d["n_windows"] for d in dets] == [1738, 1308] and all(survivors(d) > 0 for d in dets)
        assert_pooled_detection(dc.detect_frame_list(fdev, smallest_face=SF), dets, "RGB list")
        assert_pooled_faces(dc.detect_faces_frame_list(fdev, rig.loc, smallest_face=SF), faces, "RGB list, faces")
    finally:
        ref.close()
        dc.close()


@pytest.mark.parametrize("filt", (2, 3))
def test_stage_and_eye_filters_on_a_list(rig, filt):
    """interpolation_formats all BILINEAR / all BICUBIC and the eye locator's filter likewise, on the list of test 2."""
    from pyfaceanalysis_amd.cascade import DeviceCascade
    from pyfaceanalysis_amd.eyes import EyeLocator
    dc = DeviceCascade(rig.stages, FS.SUB, FS.K, rig.pipe, interpolation_formats=[filt] * 10)
    loc = EyeLocator(rig.eye_flow, rig.clf_x, rig.eye_flow, rig.clf_y, contrast=FS.CONTRAST, interpolation=filt)
    try:
        fdev = list_of(LC.MIXED)
        dets = [dc.detect_frame(f, smallest_face=SF) for f in fdev]
        faces = [dc.detect_faces(f, loc, smallest_face=SF) for f in fdev]
        assert sum(1 for d in dets if survivors(d) > 0) >= 2 and sum(len(f["faces"]) for f in faces) > 0
        assert_pooled_detection(dc.detect_frame_list(fdev, smallest_face=SF), dets, ("stage filter", filt))
        assert_pooled_faces(dc.detect_faces_frame_list(fdev, loc, smallest_face=SF), faces, ("stage filter", filt, "faces"))
    finally:
        loc.close()
        dc.close()


def test_no_groups_on_a_list(rig, monkeypatch):
    """HIGSFA_CASCADE_NO_GROUPS=1 (every stage a group of its own) gives the list call's same rows."""
    dets, faces = answers(rig, LC.MIXED)
    assert sum(survivors(d) for d in dets) > 0
    dc, loc, close = rig.fresh()
    try:
        monkeypatch.setenv("HIGSFA_CASCADE_NO_GROUPS", "1")
        got = dc.detect_frame_list(list_of(LC.MIXED), smallest_face=SF)
        gf = dc.detect_faces_frame_list(list_of(LC.MIXED), loc, smallest_face=SF)
        monkeypatch.delenv("HIGSFA_CASCADE_NO_GROUPS")
        for f, (g, d) in enumerate(zip(got["frames"], dets)):
            for key in FS.DET_KEYS:
                assert np.array_equal(g[key], d[key]), (f, key)
        for f, (g, d) in enumerate(zip(gf["faces"], faces)):
            assert g.shape == d["faces"].shape and np.array_equal(g, d["faces"]), f
        assert gf["n_before_purge"] == [d["n_before_purge"] for d in faces]
    finally:
        close()


def test_equal_grids_behind_different_frame_sizes_on_one_cascade(rig):
    """ONE long-lived cascade: a list with 1280x720, then a list of the same length with 1920x1080 in its place — the same prescaled size,
    the same level table, another whole-frame box of the prescale: what is kept per list must not serve the second list — each against
    fresh objects; then the per-frame calls of the 1080p frame on the same cascade (the prescale's keyed tables are the per-frame path's
    too)."""
    (s720, seed720), other, (s1080, seed1080) = LC.TABLES[0], LC.TABLES[1], LC.TABLES[2]
    assert (s720, s1080) == LC.SHARED_GRID
    a, b = ((s720, seed720), other), ((s1080, seed1080), other)
    da, db = answers(rig, a)[0], answers(rig, b)[0]
    assert da[0]["n_windows"] == db[0]["n_windows"] == 1738 and survivors(da[0]) > 0 and survivors(db[0]) > 0
    assert not np.array_equal(da[0]["coords"], db[0]["coords"]), "the two frames have different answers"
    dc, loc, close = rig.fresh()
    try:
        check_list(rig, dc, loc, a, "a list with 1280x720")
        check_list(rig, dc, loc, b, "the same list with 1920x1080 in its place")
        det, faces = per_frame(rig, s1080, seed1080)
        fdev = dev(frame_of(s1080, seed1080))
        FS.assert_same_detection(dc.detect_frame(fdev, smallest_face=SF), det, "detect_frame of the 1080p frame after the lists")
        FS.assert_same_faces(dc.detect_faces(fdev, loc, smallest_face=SF), faces, "detect_faces of the 1080p frame after the lists")
        check_list(rig, dc, loc, a, "the first list again")
    finally:
        close()


# ---- 7. state -----------------------------------------------------------------------------------------------------------------------
def test_state_across_list_stack_and_per_frame_calls(rig):
    """ONE long-lived cascade and locator: the list call, a per-frame call, a stack call, a list call with other sizes and another B, the
    first list again — each against fresh objects."""
    dc, loc, close = rig.fresh()
    try:
        assert sum(survivors(d) for d in answers(rig, LC.MIXED)[0]) > 0
        check_list(rig, dc, loc, LC.MIXED, "first list")
        FS.assert_same_faces(dc.detect_faces(dev(frame_of(BC.MEDIUM, 9211)), loc, smallest_face=SF), per_frame(rig, BC.MEDIUM, 9211)[1], "per frame after a list")
        stack = FB.stack_of(BC.SMALL, BC.SMALL_SEEDS)
        assert_pooled_faces(dc.detect_faces_frames(stack, loc, smallest_face=SF), [per_frame(rig, BC.SMALL, s)[1] for s in BC.SMALL_SEEDS], "stack after a list")
        check_list(rig, dc, loc, LC.CHUNKED[1:4] + LC.MIXED[:1] + LC.CHUNKED[:1] + LC.MIXED[4:], "another list, B = 6")
        check_list(rig, dc, loc, LC.MIXED, "first list again")
    finally:
        close()
