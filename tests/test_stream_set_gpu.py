"""GPU: faces tracked on SEVERAL frame streams in one pooled step (``tracking.StreamSetTracker``, include/higsfa.h ``hg_stream_tracker``).
The oracle of stream s is a ``tracking.FaceTracker`` of its own, on a cascade and an eye handle of a SECOND rig, fed the same frames
(tests/stream_set_cases.py ``Pair``): every cascade and eye row depends on its own window and frame only, the HIP path is bit-identical
across batch sizes, every compaction keeps row order and the purge and the hand-over are per stream — so every comparison is exact.  The
rig, the sub-image size and the frames are tests/test_tracking_gpu.py's and tests/test_multi_tracking_gpu.py's: 64x64 sub-images, 640x480
frames, 2000x300 frames prescaled to 1000x150.

Premises, asserted before they are relied on (the ``pics`` fixture): ``detect_faces`` keeps at least 3 faces on the 640x480 frame of seed
7104 (8 observed on an MI355X) and on the 2000x300 frame of seed 7101 (7 observed); a constant frame keeps none; the 7104 frame with one
held face's search region zeroed and one 640x480 frame of another seed keep a stream tracked step after step.
Observed on an MI355X (the prints of a run with -s): the 7104 frame keeps 11 faces and holds 8 / 5 / 5 / 4 / 3 / 3 over six steps of one
tracker, the 7101 frame keeps 6 and holds 6 / 6 / 7; zeroing the region of held face 0 or 1 lets a stream lose everything within six steps,
held face 2's does not (held 8 / 5 / 5 / 7 / 5 / 5); of OTHER_SEEDS 9901 is the first that keeps a stream tracked (8 / 6 / 6 / 5 / 5 / 6).
Step 0 of the four mixed streams keeps 11 / 0 / 13 / 19 faces.  Further figures in the tests' docstrings."""
import ctypes as C
import os

import numpy as np
import pytest

from pyfaceanalysis_amd import _capi, grid
from pyfaceanalysis_amd.cascade import frame_levels
from tests import stream_set_cases as SC
from tests.test_frame_stream_gpu import CONTRAST, K as N_FEATURES, SF, SUB, Rig
from tests.test_multi_tracking_gpu import carried_of, region_of
from tests.test_tracking_gpu import HERE, SIZE_A, SIZE_B, device_frame

pytestmark = pytest.mark.gpu

MIN_FACES = 3
MAX_FACES = 8
OTHER_SEEDS = (9900, 9901, 9902, 9903, 7102, 7103, 7105, 7106)


@pytest.fixture(scope="module")
def rig(native_lib, nets):
    r = Rig(nets)
    yield r
    r.close()


@pytest.fixture(scope="module")
def orig(native_lib, nets):
    """The oracle trackers' own cascade and eye handle."""
    r = Rig(nets)
    yield r
    r.close()


def sustained(orig, frame, steps=6):
    """Held counts of one ``FaceTracker`` (max_faces = 8) fed ``frame`` ``steps`` times: the frame keeps a stream tracked if none is 0."""
    from pyfaceanalysis_amd.tracking import FaceTracker
    tr = FaceTracker(orig.dc, orig.loc, smallest_face=SF, max_faces=MAX_FACES)
    try:
        return [tr.step(frame)["n_held"] for _ in range(steps)]
    finally:
        tr.close()


@pytest.fixture(scope="module")
def pics(orig):
    """The frames of the tests, computed once and left unchanged: a (640x480, seed 7104), const (zeros), zeroed (a with the search
    region of one held face zeroed: face 0's, else the next face's for which the frame still keeps a stream tracked), other (the first
    frame of OTHER_SEEDS that keeps a stream tracked) and b (2000x300, seed 7101).  "Keeps a stream tracked": a ``FaceTracker`` fed the
    frame six times holds a face after every step."""
    import torch
    a, b = device_frame(SIZE_A), device_frame(SIZE_B)
    faces_a = orig.dc.detect_faces(a, orig.loc, smallest_face=SF)["faces"]
    faces_b = orig.dc.detect_faces(b, orig.loc, smallest_face=SF)["faces"]
    assert len(faces_a) >= MIN_FACES and len(faces_b) >= MIN_FACES, (len(faces_a), len(faces_b))
    held_a, held_b = sustained(orig, a), sustained(orig, b, 3)
    assert min(held_a) >= 1 and min(held_b) >= 1, (held_a, held_b)
    const = torch.zeros((SIZE_A[1], SIZE_A[0]), dtype=torch.uint8, device="cuda")
    assert len(orig.dc.detect_faces(const, orig.loc, smallest_face=SF)["faces"]) == 0
    held = carried_of(faces_a, MAX_FACES)
    zeroed, victim, held_z = None, None, None
    for victim in range(len(held)):
        x_lo, y_lo, x_hi, y_hi = region_of(orig, held[victim], SIZE_A[0], SIZE_A[1])
        cand = a.clone()
        cand[y_lo:y_hi, x_lo:x_hi] = 0
        held_z = sustained(orig, cand)
        if min(held_z) >= 1:
            zeroed = cand
            break
    other, seed_other, held_o = None, None, None
    for seed in OTHER_SEEDS:
        f = device_frame(SIZE_A, seed)
        held_o = sustained(orig, f)
        if min(held_o) >= 1:
            other, seed_other = f, seed
            break
    print("frames: a keeps %d (held %s), b keeps %d (held %s), zeroed (victim %s) held %s, other (seed %s) held %s" %
          (len(faces_a), held_a, len(faces_b), held_b, victim, held_z, seed_other, held_o))
    assert zeroed is not None and other is not None
    return dict(a=a, b=b, const=const, zeroed=zeroed, other=other, faces_a=faces_a, faces_b=faces_b)


def stack_of(*frames):
    import torch
    return torch.stack(list(frames))


def make_pair(rig, orig, n, **kw):
    return SC.Pair(rig.dc, rig.loc, orig.dc, orig.loc, n, SF, **kw)


def tracked_consts_of(sub):
    p, tc = grid.FACE_PIPELINE, _capi.HgTrackedConsts()
    tc.subimage_width, tc.subimage_height = float(sub[0]), float(sub[1])
    tc.regression_width, tc.regression_height, tc.net_Dx, tc.net_Dy = p["regression_width"], p["regression_height"], p["net_Dx"], p["net_Dy"]
    return tc


def test_grid_kernel_alone(native_lib):
    """1. hg_cascade_tracked_grid_streams_device on five streams that hold 0, 1, 3, max_faces = 8 and 0 faces, for every group of fixture
    boxes (one sub-image size each; the groups with rows where a fused multiply-add would change the last bit included, those boxes
    first): stream s's windows and level rows, at its period of 72 rows, equal hg_cascade_tracked_grid_multi_device on its boxes and the
    reference's outputs bit for bit; the holes of faces not held and the guard row behind each output stay NaN; a count outside
    0..max_faces is read as the nearer end."""
    import torch
    fx = np.load(os.path.join(HERE, "golden", "reference_tracking.npz"))
    L = _capi.lib()
    stream = torch.cuda.current_stream().cuda_stream
    groups = {}
    for i, s in enumerate(fx["sub"]):
        groups.setdefault((int(s[0]), int(s[1])), []).append(i)
    held, k = [0, 1, 3, MAX_FACES, 0], MAX_FACES
    b, per = len(held), 9 * MAX_FACES
    fma_seen = 0
    for sub, idx in groups.items():
        idx = sorted(idx, key=lambda i: -(int(fx["fma_side"][i]) + int(fx["fma_corner"][i])))
        assert len(idx) >= sum(held), sub
        fma_seen += int(fx["fma_side"][idx[:sum(held)]].sum() + fx["fma_corner"][idx[:sum(held)]].sum())
        tc = tracked_consts_of(sub)
        faces = np.full((b, k, 4), np.nan)
        owner, at = {}, 0
        for s, h in enumerate(held):
            for j in range(h):
                faces[s, j], owner[(s, j)] = fx["box"][idx[at]], idx[at]
                at += 1
        for given in (held, [-3, 1, 3, MAX_FACES + 5, 0]):          # the second: clamped to the same counts
            fdev, hdev = torch.from_numpy(faces).cuda(), torch.tensor(given, dtype=torch.int32, device="cuda")
            boxes = torch.full((b * per + 1, 4), float("nan"), dtype=torch.float64, device="cuda")
            level = torch.full((b * per + 1, 3), float("nan"), dtype=torch.float64, device="cuda")
            _capi.check(L.hg_cascade_tracked_grid_streams_device(0, C.byref(tc), fdev.data_ptr(), hdev.data_ptr(), b, k, boxes.data_ptr(), level.data_ptr(), stream))
            got_b, got_l = boxes.cpu().numpy(), level.cpu().numpy()
            assert np.isnan(got_b[-1]).all() and np.isnan(got_l[-1]).all(), sub
            for s, h in enumerate(held):
                lo = s * per
                assert np.isnan(got_b[lo + 9 * h:lo + per]).all() and np.isnan(got_l[lo + 9 * h:lo + per]).all(), (sub, s)
                if not h:
                    continue
                one_b = torch.full((9 * h + 1, 4), float("nan"), dtype=torch.float64, device="cuda")
                one_l = torch.full((9 * h + 1, 3), float("nan"), dtype=torch.float64, device="cuda")
                _capi.check(L.hg_cascade_tracked_grid_multi_device(0, C.byref(tc), fdev[s].data_ptr(), h, one_b.data_ptr(), one_l.data_ptr(), stream))
                assert got_b[lo:lo + 9 * h].tobytes() == one_b.cpu().numpy()[:-1].tobytes() and got_l[lo:lo + 9 * h].tobytes() == one_l.cpu().numpy()[:-1].tobytes(), (sub, s)
                want_b = np.concatenate([fx["boxes"][owner[(s, j)]] for j in range(h)])
                want_l = np.concatenate([np.tile([fx["maxd"][owner[(s, j)]][0], fx["maxd"][owner[(s, j)]][1], fx["base_side"][owner[(s, j)]]], (9, 1)) for j in range(h)])
                assert np.array_equal(got_b[lo:lo + 9 * h], want_b) and np.array_equal(got_l[lo:lo + 9 * h], want_l), (sub, s)
    assert fma_seen >= 8, fma_seen
    # a refusal launches nothing
    out_b = torch.full((b * per, 4), 7.0, dtype=torch.float64, device="cuda")
    out_l = torch.full((b * per, 3), 7.0, dtype=torch.float64, device="cuda")
    for bad_b, bad_k in ((0, k), (_capi.HG_MAX_STACK_FRAMES + 1, k), (b, 0), (b, 65)):
        assert L.hg_cascade_tracked_grid_streams_device(0, C.byref(tc), fdev.data_ptr(), hdev.data_ptr(), bad_b, bad_k, out_b.data_ptr(), out_l.data_ptr(),
                                                        stream) == _capi.HG_ERR_ARG
    assert L.hg_cascade_tracked_grid_streams_device(0, C.byref(tc), fdev.data_ptr(), None, b, k, out_b.data_ptr(), out_l.data_ptr(), stream) == _capi.HG_ERR_ARG
    torch.cuda.synchronize()
    assert (out_b.cpu().numpy() == 7.0).all() and (out_l.cpu().numpy() == 7.0).all()


def test_step_zero_is_detect_faces_per_stream(rig, orig, pics):
    """2. B = 4, nothing held: every stream goes through the full grid in ONE pooled pass and equals ``detect_faces`` on its frame; the
    state is the hand-over rule's, the slots are -1.  Observed: 8 / 0 / (zeroed) / (other) faces."""
    frames = [pics["a"], pics["const"], pics["zeroed"], pics["other"]]
    p = make_pair(rig, orig, 4, max_faces=MAX_FACES)
    try:
        got = p.step(stack_of(*frames), "step 0")
        assert got["n_grid"] == 4 and got["n_tracked"] == 0
        for s, f in enumerate(frames):
            want = orig.dc.detect_faces(f, orig.loc, smallest_face=SF)
            st = got["streams"][s]
            assert np.array_equal(st["faces"], want["faces"]) and st["n_before_purge"] == want["n_before_purge"] and st["n_windows"] == want["n_windows"], s
            assert (st["slots"] == -1).all() and st["tracked"] is False, s
            assert np.array_equal(p.set.tracked_faces(s), carried_of(want["faces"], MAX_FACES)) and st["n_held"] == len(carried_of(want["faces"], MAX_FACES)), s
        print("step 0 keeps", [len(st["faces"]) for st in got["streams"]])
        assert len(got["streams"][0]["faces"]) >= MIN_FACES and len(got["streams"][1]["faces"]) == 0
    finally:
        p.close()


def test_mixed_streams(rig, orig, pics):
    """3. Six steps, B = 4, max_faces = 8: the seed-7104 frame, a constant frame, the 7104 frame with held face 0's region zeroed,
    another seed.  Step 1: three streams tracked and the constant stream on the full grid again — both passes in one call.  Step 3:
    stream 0's frame turns constant: it is tracked, loses everything, holds nothing, and is back on the grid at step 4 while streams 2
    and 3 stay tracked.  Every step, every stream: the dict of its ``FaceTracker``.
    Observed (windows / before the purge / kept / held per stream): step 1 72 1308 72 72 / 15 0 15 18 / 5 0 5 6 / 5 0 5 6; step 2
    45 1308 45 54 / 15 0 15 24 / 5 0 5 6; step 3 45 1308 45 54 / 0 0 27 18 / 0 0 7 5; step 4 1308 1308 63 45 / 11 0 27 21 / 11 0 5 5 /
    8 0 5 5; step 5 72 1308 45 45 / 15 0 21 24 / 5 0 5 6."""
    p = make_pair(rig, orig, 4, max_faces=MAX_FACES)
    try:
        for i in range(6):
            first = pics["const"] if i == 3 else pics["a"]
            got = p.step(stack_of(first, pics["const"], pics["zeroed"], pics["other"]), "step %d" % i)
            print("step %d: tracked %s, windows %s, before purge %s, kept %s, held %s" % (
                i, [st["tracked"] for st in got["streams"]], [st["n_windows"] for st in got["streams"]], [st["n_before_purge"] for st in got["streams"]],
                [len(st["faces"]) for st in got["streams"]], [st["n_held"] for st in got["streams"]]))
        flags = p.flags()
        assert flags[0] == [False] * 4
        assert flags[1] == [True, False, True, True] and p.log[1]["n_tracked"] == 3 and p.log[1]["n_grid"] == 1
        assert len({int(x) for st in p.log[1]["streams"] for x in st["slots"] if x >= 0}) >= 2          # several held faces behind the kept rows
        s0 = p.log[3]["streams"][0]
        assert s0["tracked"] is True and s0["n_windows"] >= 9 and s0["faces"].shape == (0, 10) and s0["n_held"] == 0 and s0["n_before_purge"] == 0
        assert flags[3][2] is True and flags[3][3] is True
        assert flags[4] == [False, False, True, True]
        assert flags[5][0] is True
        assert all(f[1] is False for f in flags)
    finally:
        p.close()


def test_all_streams_lose_everything_in_one_step(rig, orig, pics):
    """4. Three streams hold faces; every frame of step 1 is constant: the live count is 0 under the bound through every group, the eye
    step and every purge; the step returns normally with no row, and step 2 is all grid and equals step 0."""
    p = make_pair(rig, orig, 3, max_faces=MAX_FACES)
    try:
        r0 = p.step(stack_of(pics["a"], pics["zeroed"], pics["other"]), "step 0")
        assert all(st["n_held"] >= 1 for st in r0["streams"])
        r1 = p.step(stack_of(pics["const"], pics["const"], pics["const"]), "step 1")
        assert r1["n_tracked"] == 3 and r1["n_grid"] == 0
        for st in r1["streams"]:
            assert st["faces"].shape == (0, 10) and st["slots"].shape == (0,) and st["n_held"] == 0 and st["n_before_purge"] == 0
        r2 = p.step(stack_of(pics["a"], pics["zeroed"], pics["other"]), "step 2")
        assert r2["n_tracked"] == 0 and r2["n_grid"] == 3
        for x, y in zip(r0["streams"], r2["streams"]):
            assert np.array_equal(x["faces"], y["faces"]) and x["n_held"] == y["n_held"]
    finally:
        p.close()


def test_caps(rig, orig, pics):
    """5. max_faces = 1, rescan_every = 0 (the single-face tracker per stream), compared on the keys ``FaceTracker`` returns then; and
    max_faces = 2 on a frame that keeps more faces: two are carried, the next step runs 18 windows."""
    p = make_pair(rig, orig, 3)
    try:
        for i in range(3):
            got = p.step(stack_of(pics["a"], pics["other"], pics["zeroed"]), "cap 1, step %d" % i)
        assert p.flags()[0] == [False] * 3 and p.flags()[1] == [True] * 3 and all(st["n_windows"] == 9 for st in p.log[1]["streams"])
        assert all(st["n_held"] <= 1 for g in p.log for st in g["streams"])
    finally:
        p.close()
    p = make_pair(rig, orig, 2, max_faces=2)
    try:
        r0 = p.step(stack_of(pics["a"], pics["a"]), "cap 2, step 0")
        assert len(r0["streams"][0]["faces"]) > 2 and r0["streams"][0]["n_held"] == 2
        assert np.array_equal(p.set.tracked_faces(0), r0["streams"][0]["faces"][:2, :4])
        r1 = p.step(stack_of(pics["a"], pics["a"]), "cap 2, step 1")
        assert all(st["tracked"] and st["n_windows"] == 18 and st["n_held"] <= 2 for st in r1["streams"])
    finally:
        p.close()


def test_rescan_out_of_phase(rig, orig, pics):
    """6. rescan_every = 2, max_faces = 4, seven steps, three streams on the 7104 frame; stream 1's frame is constant at step 1, so it
    loses everything there, rescans at step 2 and is out of phase with the others from then on: steps with both passes in one call.
    Observed: streams 0 and 2 F T T F T T F, stream 1 F T F T T F T; four of the seven steps run both passes."""
    p = make_pair(rig, orig, 3, max_faces=4, rescan_every=2)
    try:
        for i in range(7):
            p.step(stack_of(pics["a"], pics["const"] if i == 1 else pics["a"], pics["a"]), "step %d" % i)
        flags = p.flags()
        print("rescan flags:", flags)
        assert [f[0] for f in flags] == [False, True, True, False, True, True, False]
        assert [f[2] for f in flags] == [f[0] for f in flags]
        assert [f[1] for f in flags] == [False, True, False, True, True, False, True]
        assert p.log[1]["streams"][1]["n_held"] == 0
        assert sum(0 < g["n_tracked"] < 3 for g in p.log) >= 4
    finally:
        p.close()


def test_position_independence(rig, orig, pics):
    """7. B = 1 equals ``FaceTracker``; a permuted set of streams gives the permuted results with the same bytes; one frame in all four
    streams gives four equal results."""
    from pyfaceanalysis_amd.tracking import StreamSetTracker
    p1 = make_pair(rig, orig, 1, max_faces=MAX_FACES)
    try:
        for i in range(3):
            p1.step(stack_of(pics["a"]), "B = 1, step %d" % i)
        assert p1.flags() == [[False], [True], [True]]
    finally:
        p1.close()
    frames = [pics["a"], pics["const"], pics["zeroed"], pics["other"]]
    perm = [2, 0, 3, 1]
    p = make_pair(rig, orig, 4, max_faces=MAX_FACES)
    q = StreamSetTracker(rig.dc, rig.loc, 4, smallest_face=SF, max_faces=MAX_FACES)
    same = StreamSetTracker(rig.dc, rig.loc, 4, smallest_face=SF, max_faces=MAX_FACES)
    try:
        for i in range(3):
            a = p.step(stack_of(*frames), "step %d" % i)
            b = q.step(stack_of(*[frames[j] for j in perm]))
            for s, j in enumerate(perm):
                for key in SC.STEP_KEYS:
                    x, y = a["streams"][j][key], b["streams"][s][key]
                    assert np.array_equal(x, y) and np.asarray(x).tobytes() == np.asarray(y).tobytes(), (i, s, key)
                assert np.array_equal(p.set.tracked_faces(j), q.tracked_faces(s)), (i, s)
            assert a["rows_executed"] == b["rows_executed"] and a["n_tracked"] == b["n_tracked"]
            c = same.step(stack_of(*[pics["a"]] * 4))
            for s in range(4):
                for key in SC.STEP_KEYS:
                    assert np.array_equal(c["streams"][s][key], a["streams"][0][key]), (i, s, key)
    finally:
        p.close()
        q.close()
        same.close()


def test_more_than_64_held_faces_in_one_pass(rig, orig, pics):
    """8. B = 16 copies of the 8-face frame, max_faces = 8: 1152 tracked windows in one pass, beyond anything one ``FaceTracker`` could
    send down the bounded path (576); each stream equals the single tracker.  Then the 8192-row bound: 14 streams of up to 64 faces
    (room for 8064 windows, a period of 576 per stream) with the live count far below, stream for stream the single tracker's; 910
    streams of one face (8190) are accepted, 911 (8199) refused, as are 114 x 8 and 15 x 61.
    Observed: B = 16 runs 1152 tracked windows and keeps 5 rows a stream; B = 14 has 387 live windows of 8064."""
    from pyfaceanalysis_amd.tracking import StreamSetTracker
    p = make_pair(rig, orig, 16, max_faces=MAX_FACES)
    try:
        stack = stack_of(*[pics["a"]] * 16)
        r0 = p.step(stack, "B = 16, step 0")
        r1 = p.step(stack, "B = 16, step 1")
        n = sum(st["n_windows"] for st in r1["streams"])
        print("B = 16: %d tracked windows, kept %s" % (n, [len(st["faces"]) for st in r1["streams"]]))
        assert r1["n_tracked"] == 16 and n == 9 * sum(st["n_held"] for st in r0["streams"]) and n > 9 * 64
    finally:
        p.close()
    p = make_pair(rig, orig, 14, max_faces=64)
    try:
        assert 9 * 14 * 64 <= _capi.HG_MAX_STREAM_WINDOWS < 9 * 15 * 61
        frames = [pics["const"]] * 11 + [pics["other"], pics["zeroed"], pics["a"]]
        for i in range(3):
            got = p.step(stack_of(*frames), "B = 14, step %d" % i)
        assert p.flags()[1] == [False] * 11 + [True] * 3
        live = sum(st["n_windows"] for st in p.log[1]["streams"] if st["tracked"])
        print("B = 14, max_faces = 64: %d live windows of %d" % (live, 9 * 14 * 64))
        assert 0 < live < 9 * 14 * 64 // 4
    finally:
        p.close()
    ok = StreamSetTracker(rig.dc, rig.loc, 910, smallest_face=SF, max_faces=1)
    try:
        assert ok._handle() is not None
    finally:
        ok.close()
    h, tc = C.c_void_p(1), tracked_consts_of(SUB)
    for b, k in ((911, 1), (114, 8), (15, 61)):
        assert _capi.lib().hg_stream_tracker_create(rig.dc._handle(), rig.loc._handle(), C.byref(tc), b, k, 0, C.byref(h)) == _capi.HG_ERR_ARG and not h.value
        with pytest.raises(ValueError, match="windows"):
            StreamSetTracker(rig.dc, rig.loc, b, smallest_face=SF, max_faces=k)


def test_size_change_and_back(rig, orig, pics):
    """9. 640x480 -> 2000x300 -> 640x480: every stream drops its boxes at each change and the prescaled size is tracked in between;
    ``reset(s)`` of one stream mid-run sends that stream alone to the grid, ``reset()`` all of them."""
    p = make_pair(rig, orig, 2, max_faces=MAX_FACES)
    try:
        sa, sb = stack_of(pics["a"], pics["other"]), stack_of(pics["b"], pics["b"])
        for i, st in enumerate((sa, sa, sb, sb, sa, sa)):
            p.step(st, "step %d" % i)
        assert p.flags() == [[False, False], [True, True], [False, False], [True, True], [False, False], [True, True]]
        assert all(s["n_windows"] == 5148 for s in p.log[2]["streams"])          # the grid of the prescaled size, 1000 x 150
        p.reset(1)
        assert p.set.tracked_faces(1).shape == (0, 4) and len(p.set.tracked_faces(0)) == p.log[-1]["streams"][0]["n_held"]
        p.step(sa, "after reset(1)")
        assert p.flags()[-1] == [True, False]
        p.reset()
        p.step(sa, "after reset()")
        assert p.flags()[-1] == [False, False]
        p.step(sa, "the step after")
        assert p.flags()[-1] == [True, True]
    finally:
        p.close()


def fresh_pair(rig, n_streams, dc_kw, eye_kw, **kw):
    """A stream set and its oracle on four fresh handles configured alike (own flow handles, the rig's trained pieces)."""
    from pyfaceanalysis_amd.cascade import DeviceCascade, Stage
    from pyfaceanalysis_amd.eyes import EyeLocator
    from pyfaceanalysis_amd.flow import Flow
    made = []
    for _ in range(2):
        ff = Flow.from_blob(rig.blob, output_dtype=np.float32)
        ef = Flow.from_blob(rig.blob, output_dtype=np.float32)
        dc = DeviceCascade([Stage(s.name, ff if s.flow is not None else None, s.classifier) for s in rig.stages], SUB, N_FEATURES, rig.pipe, **dc_kw)
        loc = EyeLocator(ef, rig.clf_x, ef, rig.clf_y, contrast=CONTRAST, **eye_kw)
        made.append((dc, loc, ef, ff))
    p = SC.Pair(made[0][0], made[0][1], made[1][0], made[1][1], n_streams, SF, **kw)

    def close():
        p.close()
        for dc, loc, ef, ff in made:
            loc.close()
            dc.close()
            ef.close()
            ff.close()
    return p, made[1][0], made[1][1], close


def test_layouts_of_grey_stacks(rig, orig, pics):
    """10a. A stack with pitched rows, and frames cut from a larger buffer of 255s with a frame stride that is no multiple of ld, give
    the bytes of the contiguous frames (which the oracle trackers are fed).  Two of the four streams are constant, so step 1 runs the
    tracked pass in place and the full-grid pass on two frames copied together."""
    import torch
    frames = [pics["a"], pics["const"], pics["const"], pics["other"]]
    h, w = SIZE_A[1], SIZE_A[0]
    pitched = torch.full((4, h, w + 24), 255, dtype=torch.uint8, device="cuda")
    ld, gap = w + 8, 13
    stride = h * ld + gap
    assert stride % ld != 0
    buf = torch.full((64 + 4 * stride,), 255, dtype=torch.uint8, device="cuda")
    cut = torch.as_strided(buf, (4, h, w), (stride, ld, 1), 64)
    for s, f in enumerate(frames):
        pitched[s, :, :w] = f
        cut[s] = f
    for name, view in (("pitched rows", pitched[:, :, :w]), ("cut from a buffer", cut)):
        assert not view.is_contiguous()
        p = make_pair(rig, orig, 4, max_faces=MAX_FACES)
        try:
            for i in range(3):
                p.step(view, "%s, step %d" % (name, i), oracle_frames=frames)
            assert p.flags()[1] == [True, False, False, True] and p.flags()[2] == [True, False, False, True]
        finally:
            p.close()
    assert (pitched[:, :, w:] == 255).all() and int((buf != 255).sum()) <= 4 * h * w


def first_with_faces(dc, loc, candidates, what):
    for name, f in candidates:
        n = len(dc.detect_faces(f, loc, smallest_face=SF)["faces"])
        print("%s: candidate %s keeps %d faces" % (what, name, n))
        if n >= 1:
            return f
    raise AssertionError("%s: no candidate frame keeps a face" % what)


def test_rgb_frames_behind_a_bilinear_prescale(native_lib, nets):
    """10b. RGB frames behind PIL's BILINEAR prescale: every frame is converted and resized once into its slot of the grey stack,
    whichever pass reads it.  Noise smoothed by an antialiased resize keeps no face under the cascade above (calibrated on NEAREST
    prescales: 0 faces on eight candidates, observed), so this case runs on tests/test_resample_gpu.py's rig: 320x180 frames prescaled
    to 160x90, 16x16 windows, the T5L-16 network, a cascade calibrated on the BILINEAR prescale; the frames are RGB twins of its grey
    stream (tests/color_cases.py).  Premise: at step 1 a stream is tracked while the constant stream is on the grid.
    Observed (tracked / kept per stream): step 0 F F F / 3 0 3, step 1 T F T / 0 0 2, step 2 F F T / 4 0 0, step 3 T F F / 0 0 3."""
    import torch
    from pyfaceanalysis_amd.patches import Patcher
    from tests import color_cases as CC
    from tests import test_resample_gpu as RG
    pt = Patcher()
    r2 = RG.Rig(nets, pt)
    p = None
    try:
        made = [(r2.cascade(prescale_filter="BILINEAR", frame_format="RGB"), r2.locator()) for _ in range(2)]
        p = SC.Pair(made[0][0], made[0][1], made[1][0], made[1][1], 3, RG.SF, prescale_size=160, max_faces=4)
        twins = [torch.from_numpy(CC.color_twin(f, 5100 + i)[0]).cuda() for i, f in enumerate(r2.stream)]
        const = torch.zeros_like(twins[0])
        for i in range(4):
            got = p.step(torch.stack([twins[i], const, twins[(i + 1) % 4]]), "step %d" % i)
            print("RGB behind BILINEAR, step %d: tracked %s, kept %s" % (i, [st["tracked"] for st in got["streams"]], [len(st["faces"]) for st in got["streams"]]))
        assert p.flags()[0] == [False] * 3 and all(f[1] is False for f in p.flags())
        assert p.log[0]["streams"][0]["n_windows"] > 9 and (p.flags()[1][0] or p.flags()[1][2]), p.flags()
    finally:
        if p is not None:
            p.close()
        r2.close()
        pt.close()


def test_bilinear_stage_and_eye_filters(rig, pics):
    """10c. BILINEAR windows in every stage and in the eye step (hg_cascade_set_interpolation, hg_eyes_set_interpolation): the filtered
    gathers of the tracked pass read every row from its own stream's frame.  The frame is the first of the module's frames and of
    OTHER_SEEDS on which this cascade keeps a face (observed: a and other keep none, zeroed keeps 2)."""
    p, odc, oloc, close = fresh_pair(rig, 3, dict(interpolation_formats=[2] * 10), dict(interpolation=2), max_faces=MAX_FACES)
    try:
        cands = [("a", pics["a"]), ("other", pics["other"]), ("zeroed", pics["zeroed"])] + [("seed %d" % s, device_frame(SIZE_A, s)) for s in OTHER_SEEDS]
        f = first_with_faces(odc, oloc, cands, "BILINEAR filters")
        for i in range(3):
            p.step(stack_of(f, pics["const"], f), "step %d" % i)
        assert p.flags()[0] == [False] * 3 and p.flags()[1] == [True, False, True]
    finally:
        close()


def test_shared_handles(rig, pics):
    """11. ``detect_faces``, ``detect_faces_frames`` and a ``FaceTracker`` stream on the same cascade and eye handles give the same bytes
    before and after stream-set steps; the workspaces grow when a B = 16 step follows a B = 2 set."""
    from pyfaceanalysis_amd.tracking import FaceTracker, StreamSetTracker

    def snapshot():
        one = rig.dc.detect_faces(pics["a"], rig.loc, smallest_face=SF)
        many = rig.dc.detect_faces_frames(stack_of(pics["a"], pics["other"], pics["const"]), rig.loc, smallest_face=SF)
        tr = FaceTracker(rig.dc, rig.loc, smallest_face=SF, max_faces=MAX_FACES)
        try:
            steps = [tr.step(pics["a"]) for _ in range(3)]
        finally:
            tr.close()
        assert [x["tracked"] for x in steps] == [False, True, True]
        return one, many, steps

    def same(x, y, what):
        assert sorted(x) == sorted(y), what
        for key in sorted(x):
            if key == "faces" and isinstance(x[key], list):
                assert all(np.array_equal(u, v) for u, v in zip(x[key], y[key])), (what, key)
            else:
                assert np.array_equal(x[key], y[key]), (what, key)

    before = snapshot()
    logs = []
    for b in (2, 16):
        tr = StreamSetTracker(rig.dc, rig.loc, b, smallest_face=SF, max_faces=MAX_FACES)
        try:
            stack = stack_of(*([pics["a"], pics["other"]] * (b // 2)))
            logs.append([tr.step(stack) for _ in range(3)])
            assert [g["n_tracked"] for g in logs[-1]] == [0, b, b]
        finally:
            tr.close()
    for i in range(3):          # the streams of the B = 16 set repeat those of the B = 2 set
        for s in range(16):
            for key in SC.STEP_KEYS:
                assert np.array_equal(logs[1][i]["streams"][s][key], logs[0][i]["streams"][s % 2][key]), (i, s, key)
    after = snapshot()
    same(before[0], after[0], "detect_faces")
    same(before[1], after[1], "detect_faces_frames")
    for i in range(3):
        same(before[2][i], after[2][i], "FaceTracker step %d" % i)


def test_refusals_through_the_c_abi(rig, pics):
    """12. On a live handle: a stack of another length is HG_ERR_ARG before anything is launched or written; out_cap below the kept
    total is HG_ERR_ARG with no row and no slot written and stream_first all 0, after the hand-overs (n_held is valid and the next
    step tracks); a bad stream index of ``hg_stream_tracker_reset`` is refused."""
    import torch
    from pyfaceanalysis_amd.tracking import StreamSetTracker
    L = _capi.lib()
    tr = StreamSetTracker(rig.dc, rig.loc, 3, smallest_face=SF, max_faces=MAX_FACES)
    try:
        h = tr._handle()
        stack = stack_of(pics["a"], pics["other"], pics["const"])
        fh, fw = SIZE_A[1], SIZE_A[0]
        assert grid.prescaled_size(fw, fh) == (fw, fh)
        levels, n_levels, n0 = frame_levels(fw, fh, SF, rig.dc.pipeline, (rig.dc.w, rig.dc.h))
        stream = torch.cuda.current_stream().cuda_stream

        def call(n_frames, rows, slots, first, held, used):
            vp = lambda a: a.ctypes.data_as(C.c_void_p)
            n_rows = C.c_int64(-5)
            rc = L.hg_stream_tracker_step_frames_device(h, stack.data_ptr(), n_frames, stack.stride(0), fh, fw, stack.stride(1), 0, 0, levels, n_levels, vp(rows),
                                                        len(rows), vp(first), None, vp(used), vp(held), vp(slots), C.byref(n_rows), stream)
            return rc, n_rows.value

        rows, slots = np.full((3 * (n0 + 1), 10), -77.0), np.full(3 * (n0 + 1), -77, dtype=np.int32)
        first, held, used = np.full(4, 77, dtype=np.int32), np.full(3, -5, dtype=np.int32), np.full(3, -5, dtype=np.int32)
        for bad_n in (2, 4, 1):
            rc, n_rows = call(bad_n, rows, slots, first, held, used)
            assert rc == _capi.HG_ERR_ARG and "streams" in L.hg_last_error().decode() and n_rows == -5, bad_n
            assert (rows == -77.0).all() and (slots == -77).all() and (first == 77).all() and (held == -5).all() and (used == -5).all(), bad_n
        want = [rig.dc.detect_faces(f, rig.loc, smallest_face=SF)["faces"] for f in (pics["a"], pics["other"], pics["const"])]
        total = sum(len(x) for x in want)
        small_rows, small_slots = np.full((total - 1, 10), -77.0), np.full(total - 1, -77, dtype=np.int32)
        rc, _ = call(3, small_rows, small_slots, first, held, used)
        assert rc == _capi.HG_ERR_ARG and (small_rows == -77.0).all() and (small_slots == -77).all() and (first == 0).all()
        assert held.tolist() == [len(carried_of(x, MAX_FACES)) for x in want] and used.tolist() == [0, 0, 0]
        rc, _ = call(3, rows, slots, first, held, used)          # the hand-overs have happened: streams 0 and 1 are tracked now
        assert rc == _capi.HG_OK and used.tolist() == [1, 1, 0] and first[0] == 0 and first[3] == first[2]
        assert (slots[:first[2]] >= 0).all() and (slots[first[3]:] == -77).all() and (rows[first[3]:] == -77.0).all()
        for bad in (-2, 3, 99):
            assert L.hg_stream_tracker_reset(h, bad) == _capi.HG_ERR_ARG
        assert L.hg_stream_tracker_reset(h, 2) == _capi.HG_OK and L.hg_stream_tracker_reset(h, -1) == _capi.HG_OK
        rc, _ = call(3, rows, slots, first, held, used)
        assert rc == _capi.HG_OK and used.tolist() == [0, 0, 0]
    finally:
        tr.close()
