"""GPU: the frame path (prescale -> grid -> cascade -> eyes -> purge) on a stream of frames of MIXED sizes through long-lived objects,
as the reference walks a directory of images through one set of networks.  The library keeps state between calls in six places — the
patcher's keyed index-table ring, ``DeviceCascade.prescale``'s cached tensors, ``detect_frame``'s per-size plans, the cascade's
candidate buffers (``reserve``), the prescale state inside the cascade handle, and the eye / fused-executor workspaces that grow on
demand — and every test below crosses at least one of them.  The failure looked for is stale data in an output, so every comparison is
exact (``array_equal``): against the same call on freshly created objects that have seen no other frame, against PIL, and against the
restated stage loop (oracle/cascade_restate.py) fed the device's own features.

Frame sizes: ``helpers.FRAME_STREAM`` (pinned on the CPU by test_grid_patches.py::test_frame_stream_premises).  U11L-64 plays the
face flow and the eye flow, so the sub-image is 64x64; frames are box-filtered seeded noise (synth._box3), one seed per stream element.
"""
import ctypes as C

import numpy as np
import pytest

from oracle import cascade_restate as CR
from pyfaceanalysis_amd import _capi, grid
from tests import eyes_restate as ER
from tests.helpers import FRAME_STREAM, FRAME_STREAM_600

pytestmark = pytest.mark.gpu

CONTRAST = (128.0, 48.0)          # as tests/test_eyes_gpu.py
SUB = (64, 64)
K = 20                            # feature columns the cascade keeps
SF = 0.1
# Calibration of the synthetic cascade (synth_cascade.build_face_cascade), on the union of two frames' first-stage features: chosen so
# that the stream has frames with survivors and frames without (the counts are asserted and recorded in test_stream_*'s docstring)
KEEP, LATER_KEEP = 0.3, 0.7
CALIBRATION_FRAMES = ((1920, 1080), (640, 480))

# The stream: starts at the smallest frame, jumps to the one with the most windows and drops back, walks nine sizes twice (the ring of
# four slots evicts on every call), keeps the three n = 1308 frames together, puts 1280x720 right after 1920x1080 (one grid key, two
# prescale keys) and ends on the very first frame.
CYCLE = [(97, 131), (320, 240), (640, 480), (3648, 2736), (1920, 1080), (1280, 720), (1080, 1920), (1001, 1000)]
STREAM = [(64, 64), (2000, 300)] + CYCLE + [(2000, 300)] + CYCLE + [(64, 64)]
ORACLE_ELEMENTS = (0, 1, 5)       # the first, 2000x300 and an n = 1308 frame (3648x2736): also against PIL and the restated loop
DET_KEYS = ("coords", "angles", "orig_index", "confidence")


def noise_frame(w, h, seed):
    from pyfaceanalysis_amd import synth
    rng = np.random.default_rng(seed)
    return np.rint(synth._box3(rng.integers(0, 256, (h, w), dtype=np.uint8))).astype(np.uint8)


def stream_frame(i):
    """Element i's frame: a seed of its own, except that the last element IS the first frame again."""
    j = 0 if i == len(STREAM) - 1 else i
    w, h = STREAM[j]
    return noise_frame(w, h, 7100 + j)


def pil_prescale(frame, prescale_size=grid.PRESCALE_SIZE):
    from PIL import Image
    pw, ph = grid.prescaled_size(frame.shape[1], frame.shape[0], prescale_size)
    if (pw, ph) == (frame.shape[1], frame.shape[0]):
        return frame
    return np.array(Image.fromarray(frame, "L").resize((pw, ph), Image.NEAREST))


class Rig(object):
    """The trained pieces (nodes, classifiers) and the long-lived device objects built on them."""

    def __init__(self, nets, keep=KEEP, later_keep=LATER_KEEP):
        from pyfaceanalysis_amd import synth_cascade
        from pyfaceanalysis_amd.cascade import DeviceCascade, frame_windows
        from pyfaceanalysis_amd.eyes import EyeLocator
        from pyfaceanalysis_amd.flow import Flow
        from pyfaceanalysis_amd.patches import Patcher
        self.pipe = dict(grid.FACE_PIPELINE)
        self.nodes = nets("U11L-64")
        self.flow = Flow(self.nodes, output_dtype=np.float32)
        self.blob = self.flow.to_blob()
        self.eye_flow = Flow.from_blob(self.blob, output_dtype=np.float32)
        self.pt = Patcher()
        feats = []
        for w, h in CALIBRATION_FRAMES:
            small = pil_prescale(noise_frame(w, h, 7100 + STREAM.index((w, h))))
            boxes, _ = frame_windows(small.shape[1], small.shape[0], SF, self.pipe, SUB)
            feats.append(self.flow.execute(self.pt.extract(small, boxes, SUB, dtype=np.uint8), n_cols=K))
        self.stages = synth_cascade.build_face_cascade(self.flow, np.concatenate(feats), self.pipe, keep_fraction=keep, later_keep_fraction=later_keep)
        self.dc = DeviceCascade(self.stages, SUB, K, self.pipe)
        # the eye stages, calibrated as in tests/test_eyes_gpu.py: ~300 faces cut from a grid, angles in +-22.5 plus 0, +-90, 180
        rng = np.random.default_rng(17)
        self.eye_small = pil_prescale(noise_frame(1920, 1080, 7100 + STREAM.index((1920, 1080))))
        boxes, _ = frame_windows(1000, 562, SF, self.pipe, SUB)
        self.face_boxes = boxes[rng.choice(len(boxes), 300, replace=False)].copy()
        self.face_boxes[:40] -= np.array([60.0, 50.0, 60.0, 50.0])
        self.face_angles = rng.uniform(-22.5, 22.5, 300)
        self.face_angles[::7] = 0.0
        self.face_angles[1::23], self.face_angles[2::23], self.face_angles[3::23] = 90.0, -90.0, 180.0
        eb = ER.all_eye_boxes(self.face_boxes, self.face_angles)
        u8 = self.pt.extract(self.eye_small, eb, (64, 64), dtype=np.uint8, delta_angs=-np.concatenate([self.face_angles] * 2))
        efeats = self.eye_flow.execute(ER.contrast(u8, *CONTRAST), n_cols=12)
        _, self.clf_x, _, self.clf_y = synth_cascade.build_eye_stages(self.eye_flow, efeats)
        self.loc = EyeLocator(self.eye_flow, self.clf_x, self.eye_flow, self.clf_y, contrast=CONTRAST)

    def fresh(self):
        """A cascade and an eye locator that have seen no frame: own flow handles, the trained nodes and classifiers shared."""
        from pyfaceanalysis_amd.cascade import DeviceCascade, Stage
        from pyfaceanalysis_amd.eyes import EyeLocator
        from pyfaceanalysis_amd.flow import Flow
        ff = Flow.from_blob(self.blob, output_dtype=np.float32)
        ef = Flow.from_blob(self.blob, output_dtype=np.float32)
        dc = DeviceCascade([Stage(s.name, ff if s.flow is not None else None, s.classifier) for s in self.stages], SUB, K, self.pipe)
        loc = EyeLocator(ef, self.clf_x, ef, self.clf_y, contrast=CONTRAST)

        def close():
            loc.close()
            dc.close()
            ef.close()
            ff.close()
        return dc, loc, close

    def fresh_answers(self, fdev, faces=True, **kw):
        """``detect_frame`` and ``detect_faces`` of objects created for this frame.  ``detect_faces`` is the locator's FIRST call (its
        workspace does not exist yet), and is then checked against the composed steps on the same objects, as
        test_eyes_gpu.py::test_whole_call_equals_composed_steps does: the fresh objects do not vouch for themselves."""
        from pyfaceanalysis_amd import eyes as E
        dc, loc, close = self.fresh()
        try:
            det = dc.detect_frame(fdev, **kw)
            if not faces:
                return det, None
            got = dc.detect_faces(fdev, loc, **kw)
            small = dc.prescale(fdev, kw.get("prescale_size", grid.PRESCALE_SIZE))
            out = loc.locate(small, det["coords"], det["angles"])
            rows = E.assemble_rows(det["coords"], det["angles"], det["confidence"], out["eye_coords"], out["too_far"])
            want = E.purge_detections(rows)
            assert got["faces"].shape == want.shape and np.array_equal(got["faces"], want), "the whole call against the composed steps"
            assert got["n_before_purge"] == len(rows) and got["counts"] == det["counts"] and got["rows_executed"] == det["rows_executed"]
            return det, got
        finally:
            close()

    def close(self):
        self.loc.close()
        self.dc.close()
        self.pt.close()
        self.eye_flow.close()
        self.flow.close()


@pytest.fixture(scope="module")
def rig(native_lib, nets):
    r = Rig(nets)
    yield r
    r.close()


def assert_same_detection(got, want, what):
    for key in DET_KEYS:
        assert got[key].shape == want[key].shape and np.array_equal(got[key], want[key]), (what, key)
    assert got["counts"] == want["counts"] and got["rows_executed"] == want["rows_executed"] and got["n_windows"] == want["n_windows"], what


def assert_same_faces(got, want, what):
    assert got["faces"].shape == want["faces"].shape and np.array_equal(got["faces"], want["faces"]), what
    assert got["n_before_purge"] == want["n_before_purge"] and got["counts"] == want["counts"], what
    assert got["rows_executed"] == want["rows_executed"] and got["n_windows"] == want["n_windows"], what


def restated_loop(rig, small):
    """The stage loop restated on the host (as test_cascade.py::test_config3_full_pyramid_1080p): PIL-rule windows of ``small``, the
    device's features and regressions, the glue in numpy."""
    from pyfaceanalysis_amd.cascade import frame_windows
    boxes, level = frame_windows(small.shape[1], small.shape[0], SF, rig.pipe, SUB)
    stages = rig.stages

    def extract(coords, dang):
        return rig.pt.extract(small, coords, SUB, dtype=np.uint8, delta_angs=dang) if len(coords) else np.zeros((0, SUB[0] * SUB[1]), np.uint8)

    def execute(k, s):
        return rig.flow.execute(s, n_cols=K)

    def regress(k, sl):
        return stages[k].classifier.regression(np.ascontiguousarray(sl[:, :stages[k].classifier.input_dim]))
    return CR.run_cascade([s.name for s in stages], [s.flow is not None for s in stages], boxes, level, rig.pipe, extract, execute, regress)


def test_stream_of_mixed_sizes_against_fresh_objects(rig):
    """(a) Twenty frames of ten sizes through ONE DeviceCascade and ONE EyeLocator; after every frame ``detect_frame`` and
    ``detect_faces`` must return exactly what a cascade and a locator created for that frame alone return.  For three elements the
    fresh objects are themselves checked against PIL (prescale) and the restated stage loop.

    Survivors, from the fresh-object runs, so that the comparison is not one of empty arrays (asserted below; observed on an MI355X
    with KEEP / LATER_KEEP = 0.3 / 0.7, as (frame, cascade survivors, faces before the purge, faces)): 64x64 0/0/0, 2000x300 7/7/7,
    97x131 0/0/0, 320x240 1/1/1, 640x480 15/8/8, 3648x2736 294/113/113, 1920x1080 90/61/61, 1280x720 49/36/36, 1080x1920 89/53/53,
    1001x1000 51/32/32; second round 2000x300 7/7/7, 97x131 0/0/0, 320x240 1/1/1, 640x480 15/11/11, 3648x2736 270/115/115,
    1920x1080 69/45/44, 1280x720 54/39/39, 1080x1920 96/62/62, 1001x1000 64/50/49, 64x64 0/0/0 — 16 of 20 elements with survivors,
    the eye step at work on 8 frame sizes, 4 elements without a survivor.

    What it found when first run: ``hg_cascade_detect_faces_frame_device`` took the eye workspace's row and count pointers before the
    workspace was reserved.  On element 1 (2000x300, the first frame with survivors) the long-lived locator returned 7 rows of garbage
    and n_before_purge = 638665505, the fresh one 0 faces for 7 survivors; a later growth would have written rows into freed
    buffers.  test_eyes_gpu.py never saw it because its locator had run ``locate`` (which reserves) before ``detect_faces``."""
    import torch
    assert STREAM[0] == STREAM[-1] == (64, 64) and STREAM[1] == (2000, 300) and len(set(STREAM)) == 10
    assert all(STREAM.count(s) >= 2 for s in set(STREAM))                       # every size comes back: > 4 keys in rotation, twice
    i1308 = [i for i, s in enumerate(STREAM) if FRAME_STREAM[s][3] == 1308]
    assert i1308[:3] == [i1308[0], i1308[0] + 1, i1308[0] + 2] and len({STREAM[i] for i in i1308[:3]}) == 3
    assert all(STREAM[i + 1] == (1280, 720) for i, s in enumerate(STREAM) if s == (1920, 1080))
    alive, eye_sizes, log = [], set(), []
    first = None
    for i, (w, h) in enumerate(STREAM):
        frame = stream_frame(i)
        fdev = torch.from_numpy(frame).cuda()
        det = rig.dc.detect_frame(fdev, smallest_face=SF)
        faces = rig.dc.detect_faces(fdev, rig.loc, smallest_face=SF)
        want_det, want_faces = rig.fresh_answers(fdev, smallest_face=SF)
        print("element %2d  %4d x %4d  n = %4d  counts %s  before purge %d  faces %d" %
              (i, w, h, want_det["n_windows"], want_det["counts"], want_faces["n_before_purge"], len(want_faces["faces"])))
        assert want_det["n_windows"] == FRAME_STREAM[(w, h)][3]
        assert_same_detection(det, want_det, (i, w, h))
        assert_same_faces(faces, want_faces, (i, w, h))
        assert faces["counts"] == det["counts"]
        alive.append(want_det["counts"][-1])
        if want_faces["counts"][-1] > 0:
            eye_sizes.add((w, h))
        log.append((w, h, want_det["counts"][-1], want_faces["n_before_purge"], len(want_faces["faces"])))
        if i == 0:
            first = (det, faces)
        if i in ORACLE_ELEMENTS:
            small = pil_prescale(frame)
            got_small = rig.dc.prescale(fdev)
            assert tuple(got_small.shape) == (FRAME_STREAM[(w, h)][1], FRAME_STREAM[(w, h)][0])
            assert np.array_equal(got_small.cpu().numpy(), small), (i, "prescale against PIL")
            want = restated_loop(rig, small)
            known = [k for k, c in enumerate(want_det["counts"]) if c >= 0]
            assert [want_det["counts"][k] for k in known] == [want["counts"][k] for k in known], (i, want_det["counts"], want["counts"])
            assert np.array_equal(want_det["orig_index"], want["orig_index"]), i
            assert np.array_equal(want_det["coords"], want["coords"]) and np.array_equal(want_det["angles"], want["angles"]), i
    assert_same_detection(det, first[0], "the first frame again")
    assert_same_faces(faces, first[1], "the first frame again")
    print("survivors per element:", log)
    assert sum(a >= 1 for a in alive) * 2 >= len(STREAM), alive
    assert len(eye_sizes) >= 3, eye_sizes
    assert any(a == 0 for a in alive), alive


def test_prescale_size_changes_on_one_frame_size(rig):
    """(b) ``prescale`` with 1000 / 600 / 1000 on one frame size: every result is PIL's nearest resize, of the right shape (the cached
    output used to be keyed on the frame size alone: the 1000 call after a 600 call wrote past the smaller tensor)."""
    import torch
    for w, h in ((1920, 1080), (2000, 300)):
        frame = noise_frame(w, h, 8200 + w)
        fdev = torch.from_numpy(frame).cuda()
        for size in (1000, 600, 1000):
            pw, ph = grid.prescaled_size(w, h, size)
            got = rig.dc.prescale(fdev, size)
            assert tuple(got.shape) == (ph, pw), (w, h, size)
            assert np.array_equal(got.cpu().numpy(), pil_prescale(frame, size)), (w, h, size)
    assert grid.prescaled_size(2000, 300, 600) == FRAME_STREAM_600[(2000, 300)][:2]
    # the two live together: a 1000 result is not overwritten by a 600 call on the same frame size
    big = rig.dc.prescale(fdev, 1000)
    small = rig.dc.prescale(fdev, 600)
    assert big.data_ptr() != small.data_ptr() and np.array_equal(big.cpu().numpy(), pil_prescale(frame, 1000))
    assert np.array_equal(small.cpu().numpy(), pil_prescale(frame, 600))


def test_detect_frame_between_other_prescale_sizes_and_smallest_faces(rig):
    """(b) ``detect_frame`` with prescale_size 1000 / 600 / 1000 and with smallest_face 0.1 / 0.2 / 0.1 on one frame: the outer two
    agree, the middle one is a fresh cascade's answer (and so are the outer ones)."""
    import torch
    frame = noise_frame(2000, 300, 8301)
    fdev = torch.from_numpy(frame).cuda()
    a = rig.dc.detect_frame(fdev, smallest_face=SF, prescale_size=1000)
    b = rig.dc.detect_frame(fdev, smallest_face=SF, prescale_size=600)
    c = rig.dc.detect_frame(fdev, smallest_face=SF, prescale_size=1000)
    assert a["n_windows"] == 5148 and b["n_windows"] == FRAME_STREAM_600[(2000, 300)][3]
    assert_same_detection(c, a, "prescale 1000 again")
    assert_same_detection(b, rig.fresh_answers(fdev, faces=False, smallest_face=SF, prescale_size=600)[0], "prescale 600")
    assert_same_detection(a, rig.fresh_answers(fdev, faces=False, smallest_face=SF, prescale_size=1000)[0], "prescale 1000")
    frame = noise_frame(1920, 1080, 8302)
    fdev = torch.from_numpy(frame).cuda()
    a = rig.dc.detect_frame(fdev, smallest_face=0.1)
    b = rig.dc.detect_frame(fdev, smallest_face=0.2)
    c = rig.dc.detect_frame(fdev, smallest_face=0.1)
    assert a["n_windows"] == 1738 and b["n_windows"] == 386
    assert_same_detection(c, a, "smallest_face 0.1 again")
    assert_same_detection(b, rig.fresh_answers(fdev, faces=False, smallest_face=0.2)[0], "smallest_face 0.2")
    assert_same_detection(a, rig.fresh_answers(fdev, faces=False, smallest_face=0.1)[0], "smallest_face 0.1")


def test_detect_frame_checks_every_frame(rig):
    """(c) After a good uint8 frame of a shape, ``detect_frame`` (and ``prescale``) still refuse a float32 frame, a CPU tensor and a
    column-strided view of that shape — the check used to run on the first frame of a shape only — and answer as before afterwards."""
    import torch
    frame = noise_frame(1920, 1080, 8401)
    fdev = torch.from_numpy(frame).cuda()
    good = rig.dc.detect_frame(fdev, smallest_face=SF)
    strided = torch.empty((1920, 1080), dtype=torch.uint8, device=fdev.device).t()
    strided.copy_(fdev)
    assert strided.shape == (1080, 1920) and strided.stride(1) != 1
    for bad in (fdev.float(), torch.from_numpy(frame), strided):
        with pytest.raises(ValueError):
            rig.dc.detect_frame(bad, smallest_face=SF)
        with pytest.raises(ValueError):
            rig.dc.prescale(bad)
    assert_same_detection(rig.dc.detect_frame(fdev, smallest_face=SF), good, "after the bad frames")
    assert_same_detection(good, rig.fresh_answers(fdev, faces=False, smallest_face=SF)[0], "the good frame")


def test_keyed_ring_through_the_c_abi(rig):
    """(d) ``hg_patcher_extract_keyed_device`` on one patcher and one stream: six keys (six grids of different sizes, two of them with the
    same n) round-robin for three rounds through the ring of four slots — every call evicts — then one key reused with another n and
    with another output size, and the smallest table following the largest into the same slot.  Every output equals the un-keyed
    call (key = 0) on the same boxes and frame, bit for bit."""
    import torch
    from pyfaceanalysis_amd.cascade import frame_windows
    from pyfaceanalysis_amd.patches import Patcher
    L = _capi.lib()
    pt = Patcher()
    stream = torch.cuda.Stream()
    sizes = [(64, 64), (97, 131), (320, 240), (640, 480), (1000, 562), (1000, 150)]
    assert [FRAME_STREAM[s][3] for s in ((64, 64), (97, 131), (320, 240), (640, 480), (1920, 1080), (2000, 300))] == [99, 397, 1308, 1308, 1738, 5148]
    grids = []
    for j, (w, h) in enumerate(sizes):
        boxes, _ = frame_windows(w, h, SF, rig.pipe, SUB)
        frames = [torch.from_numpy(noise_frame(w, h, 8500 + 10 * j + r)).cuda() for r in range(3)]
        grids.append((0xC0FFEE00 + j, w, h, torch.from_numpy(boxes).cuda(), frames))
    assert [len(g[3]) for g in grids] == [99, 397, 1308, 1308, 1738, 5148]
    torch.cuda.synchronize()

    def call(key, frame, boxes, n, out_size):
        ow, oh = out_size
        out = torch.full((n, ow * oh), 0xA5, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        _capi.check(L.hg_patcher_extract_keyed_device(pt._handle(), key, C.c_void_p(frame.data_ptr()), _capi.HG_U8, int(frame.shape[0]),
                                                      int(frame.shape[1]), frame.stride(0), C.c_void_p(boxes.data_ptr()), n, ow, oh,
                                                      C.c_void_p(out.data_ptr()), _capi.HG_U8, ow * oh, C.c_void_p(stream.cuda_stream)))
        stream.synchronize()
        return out

    def check(key, frame, boxes, n, out_size, what):
        want = call(0, frame, boxes, n, out_size)
        got = call(key, frame, boxes, n, out_size)
        assert torch.equal(got, want), what
        return got
    for rnd in range(3):
        for key, w, h, boxes, frames in grids:
            check(key, frames[rnd], boxes, len(boxes), SUB, ("round", rnd, w, h))
    # a key that is still in the ring, twice in a row (the second call reuses the table) and on another frame of the size
    key, w, h, boxes, frames = grids[5]
    check(key, frames[0], boxes, len(boxes), SUB, "reuse")
    check(key, frames[1], boxes, len(boxes), SUB, "reuse, another frame")
    # one key, another n (the table must be rebuilt for the boxes given now), then the same n and another output size
    key, w, h, boxes, frames = grids[2]
    check(key, frames[0], boxes, len(boxes), SUB, "key 2")
    half = boxes[1::2].contiguous()
    check(key, frames[0], half, len(half), SUB, "key 2, another n")
    check(key, frames[0], half, len(half), (32, 32), "key 2, same n, another output size")
    check(key, frames[0], half, len(half), (48, 20), "key 2, same n, an output row that is no multiple of 16")
    check(key, frames[0], boxes, len(boxes), SUB, "key 2, the first n again")
    # the largest table, three keys never seen (the ring moves on by three), then the smallest: it lands in the largest one's slot,
    # whose buffer stays the large one
    big, small = grids[5], grids[0]
    check(0xB16B16, big[4][2], big[3], len(big[3]), SUB, "largest")
    for j in (1, 2, 3):
        check(0xABC000 + j, grids[j][4][0], grids[j][3], len(grids[j][3]), SUB, ("filler", j))
    check(0x5A5A11, small[4][2], small[3], len(small[3]), SUB, "smallest after largest")
    check(0xB16B16, big[4][1], big[3], len(big[3]), SUB, "largest again")
    check(0x5A5A11, small[4][1], small[3], len(small[3]), SUB, "smallest again")
    pt.close()


def test_flow_workspace_grows_and_shrinks(rig):
    """(e) One Flow handle, no ``reserve``, on a stream of its own: N = 1, 4096, 17, 8192, 16, 12000, 1 — the executor's ping-pong
    buffers are reallocated three times.  Every result equals the matching rows of ONE 12000-row call on a fresh handle (a row's
    features do not depend on the batch it travels in)."""
    import torch
    from pyfaceanalysis_amd import synth
    from pyfaceanalysis_amd.flow import Flow
    dev = torch.device("cuda", 0)
    x = torch.from_numpy(synth.make_subimages(12000, 64, dtype=np.uint8)).to(dev)
    ref_flow = Flow.from_blob(rig.blob, output_dtype=np.float32)
    ref = torch.full((12000, K), float("nan"), dtype=torch.float32, device=dev)
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    ref_flow.execute_device(x.data_ptr(), np.dtype(np.uint8), 12000, 4096, ref.data_ptr(), np.float32, K, K, stream=stream.cuda_stream)
    stream.synchronize()
    assert bool(torch.isfinite(ref).all())
    flow = Flow.from_blob(rig.blob, output_dtype=np.float32)
    for n in (1, 4096, 17, 8192, 16, 12000, 1):
        off = (12000 - n) // 3
        y = torch.full((n + 3, K), float("nan"), dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        flow.execute_device(x[off:].data_ptr(), np.dtype(np.uint8), n, 4096, y.data_ptr(), np.float32, K, K, stream=stream.cuda_stream)
        stream.synchronize()
        assert torch.equal(y[:n], ref[off:off + n]), n
        assert bool(torch.isnan(y[n:]).all()), n             # and nothing past the rows asked for
    flow.close()
    ref_flow.close()


def test_eye_workspace_grows_and_shrinks(rig):
    """(e) ``EyeLocator.locate`` with 3, then 300, then 1 face(s) on one locator (its workspace and its flow's grow at the second
    call): each result equals a locator's that was created for that call."""
    import torch
    from pyfaceanalysis_amd.eyes import EyeLocator
    from pyfaceanalysis_amd.flow import Flow
    small_dev = torch.from_numpy(rig.eye_small).cuda()

    def locator():
        f = Flow.from_blob(rig.blob, output_dtype=np.float32)
        return f, EyeLocator(f, rig.clf_x, f, rig.clf_y, contrast=CONTRAST)
    flow, loc = locator()
    seen_far = 0
    for n, start in ((3, 0), (300, 0), (1, 299)):
        boxes, angles = rig.face_boxes[start:start + n], rig.face_angles[start:start + n]
        got = loc.locate(small_dev, boxes, angles, return_patches=True)
        f2, fresh = locator()
        want = fresh.locate(small_dev, boxes, angles, return_patches=True)
        fresh.close()
        f2.close()
        for key in ("eye_coords", "too_far", "reg", "patches"):
            assert got[key].shape == want[key].shape and np.array_equal(got[key], want[key]), (n, key)
        assert got["patches"].shape == (2 * n, 4096) and np.isfinite(got["reg"]).all()
        seen_far += int(got["too_far"].sum())
    assert 0 < seen_far < 304
    loc.close()
    flow.close()
