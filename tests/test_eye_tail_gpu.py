"""GPU: the eye tail of hg_eyes.hip — k_eye_boxes, k_eye_contrast, k_eyes_glue, k_purge, the per-frame segment and purge kernels, and
the estimator's k_patch_contrast — past one 1024-face chunk and at its contrast and discard edges, against numpy (tests/eyes_restate.py,
oracle/pil_restate.py), never against another device call of the same kernel.  Cases and frame builders: tests/eye_tail_cases.py; what
they assume on the host: tests/test_eye_tail_host.py.  Everything runs on the T5L-16 network with 16 x 16 windows and eye patches.

A  ``locate`` on 4097 faces and on its prefixes at the chunk edges: too_far and the eye coordinates against ``shift_eyes`` fed the
   device regressions.
B  a cascade that accepts every window of a 2096-window frame: ``detect_faces`` against detect_frame -> locate -> numpy rows -> numpy
   purge, with more than 1024 rows and discards on both sides of face 1024.
C  the same through ``detect_faces_frames`` (three frames of one size), ``detect_faces_frame_list`` (three sizes, the small one in the
   middle) and one ``StreamSetTracker`` step of 1152 tracked windows, each frame held to the numpy composition / a tracker of its own.
D  eye stages of one class regress to their label: 9.0 on either axis discards every face, the double just below it none.
E  crafted frames: constant, two-level, all-zero, single-pixel and narrow-band patches through k_eye_contrast at 16 x 16, 64 x 64 and
   24 x 20, bit for bit; crafted crops through k_patch_contrast.

Figures of an MI355X run are in DESIGN.md §5 ("Eyes and purge"); every premise a case rests on is asserted where it is used."""
import numpy as np
import pytest

from tests import eye_tail_cases as TC
from tests import eyes_restate as ER
from tests.test_eyes_gpu import ulp_close

pytestmark = pytest.mark.gpu


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class Rig(object):
    """One T5L-16 flow for the faces and one for the eyes, the eye stages calibrated on the 4097 faces of A, the accept-all cascade, and
    a second cascade and eye handle on the same stages for the oracle trackers of the stream set."""

    def __init__(self, nets):
        from pyfaceanalysis_amd import synth_cascade
        from pyfaceanalysis_amd.flow import Flow
        from pyfaceanalysis_amd.patches import Patcher
        self.pipe = TC.pipeline()
        nodes = nets("T5L-16")
        self.flow, self.eye_flow = Flow(nodes, output_dtype=np.float32), Flow(nodes, output_dtype=np.float32)
        self.open = []
        self.frame_a = TC.noise_frame(TC.A_FRAME[0], TC.A_FRAME[1], TC.A_SEED)
        self.boxes, self.angles = TC.locate_faces()
        pt = Patcher()
        u8 = pt.extract(self.frame_a, ER.all_eye_boxes(self.boxes, self.angles), TC.SUB, dtype=np.uint8, delta_angs=-np.concatenate([self.angles] * 2))
        pt.close()
        _, self.clf_x, _, self.clf_y = synth_cascade.build_eye_stages(self.eye_flow, self.eye_flow.execute(ER.contrast(u8, *TC.CONTRAST)))
        rng = np.random.default_rng(3)
        accept_all = synth_cascade.quantile_classifier(rng.normal(size=(50, TC.K)), 9, [0.0, 0.1])      # every regression < the cut-off
        self.stages = [synth_cascade.Stage("Disc1", self.flow, accept_all)]
        self.dc, self.loc = self.cascade(), self.locator(self.clf_x, self.clf_y)

    def cascade(self):
        from pyfaceanalysis_amd.cascade import DeviceCascade
        dc = DeviceCascade(self.stages, TC.SUB, TC.K, self.pipe)
        self.open.append(dc)
        return dc

    def locator(self, clf_x, clf_y, flow=None, eye_size=TC.SUB, contrast=TC.CONTRAST):
        from pyfaceanalysis_amd.eyes import EyeLocator
        flow = self.eye_flow if flow is None else flow
        loc = EyeLocator(flow, clf_x, flow, clf_y, contrast=contrast, eye_size=eye_size, regression_size=TC.REG_SIZE)
        self.open.append(loc)
        return loc

    def close(self):
        import torch
        torch.cuda.synchronize()
        for o in self.open:
            o.close()
        self.eye_flow.close()
        self.flow.close()


@pytest.fixture(scope="module")
def rig(native_lib, nets):
    r = Rig(nets)
    yield r
    r.close()


# ---- A ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def located(rig):
    """The 4097-face call, its device eye boxes and numpy's answer from its regressions; computed once, left unchanged."""
    fdev = dev(rig.frame_a)
    full = rig.loc.locate(fdev, rig.boxes, rig.angles)
    eb = rig.loc.eye_boxes(rig.boxes, rig.angles)
    ec, far = ER.shift_eyes(eb, rig.angles, full["reg"], regression_size=TC.REG_SIZE)
    return dict(fdev=fdev, full=full, eb=eb, ec=ec, far=far)


@pytest.mark.parametrize("n", TC.A_SIZES)
def test_locate_past_one_chunk_against_numpy(rig, located, n):
    N = TC.A_N
    full, far = located["full"], located["far"]
    # the premise: every chunk of the long call keeps some faces and discards some; so do the one-face last chunks of 1025 / 2049 / 4097
    for lo in (0, TC.CHUNK, 3 * TC.CHUNK):
        assert 0 < far[lo:lo + TC.CHUNK + (lo == 3 * TC.CHUNK)].sum() < TC.CHUNK, lo
    singles = far[[TC.CHUNK, 2 * TC.CHUNK, 4 * TC.CHUNK]]
    assert singles.any() and not singles.all(), singles
    got = full if n == N else rig.loc.locate(located["fdev"], rig.boxes[:n], rig.angles[:n])
    ang = rig.angles[:n]
    eb = np.concatenate([located["eb"][:n], located["eb"][N:N + n]])
    assert np.array_equal(rig.loc.eye_boxes(rig.boxes[:n], ang), eb)
    ec, want_far = ER.shift_eyes(eb, ang, got["reg"], regression_size=TC.REG_SIZE)
    assert got["too_far"].shape == (n,) and np.array_equal(got["too_far"], want_far)
    zero = ang == 0.0
    assert np.array_equal(got["eye_coords"][zero], ec[zero])
    scale = np.abs(rig.boxes[:n]).max(axis=1, keepdims=True)
    assert ulp_close(got["eye_coords"], ec, scale)
    if n == N:
        off = (got["eye_coords"] != ec)[~zero]
        print("locate %d faces: %d too far (%s per chunk); %.2f %% of the %d coordinates at a non-zero angle differ from numpy (within 4 ulp)" %
              (n, far.sum(), [int(far[i:i + TC.CHUNK].sum()) for i in range(0, N, TC.CHUNK)], 100.0 * off.mean(), off.size))
        assert zero.sum() >= 500 and (~zero).sum() >= 3000 and np.abs(got["reg"]).max() <= 10.5 + 1e-9
    # every prefix is the long call's rows, bit for bit
    assert np.array_equal(got["eye_coords"], full["eye_coords"][:n]) and np.array_equal(got["too_far"], full["too_far"][:n])
    assert np.array_equal(got["reg"], np.concatenate([full["reg"][:, :n], full["reg"][:, N:N + n]], axis=1))
    assert got["eye_coords"].tobytes() == full["eye_coords"][:n].tobytes()


# ---- B, C: the numpy composition -------------------------------------------------------------------------------------------------------
def composed(rig, fdev, smallest_face, loc=None):
    """detect_frame -> locate on the frame the cascade read -> numpy's discard and rows -> numpy's purge.  ``locate`` itself is held to
    shift_eyes here (angles are 0 behind a Disc-only cascade: exact)."""
    from pyfaceanalysis_amd import eyes as E
    loc = rig.loc if loc is None else loc
    det = rig.dc.detect_frame(fdev, smallest_face=smallest_face)
    assert len(det["coords"]) == det["n_windows"] and not det["angles"].any()            # every window accepted, none turned
    out = loc.locate(rig.dc.prescale(fdev), det["coords"], det["angles"])
    if len(det["coords"]):
        ec, far = ER.shift_eyes(loc.eye_boxes(det["coords"], det["angles"]), det["angles"], out["reg"], regression_size=TC.REG_SIZE)
        assert np.array_equal(out["too_far"], far) and np.array_equal(out["eye_coords"], ec)
    rows = E.assemble_rows(det["coords"], det["angles"], det["confidence"], out["eye_coords"], out["too_far"])
    assert np.array_equal(rows, ER.assemble_rows(det["coords"], det["angles"], det["confidence"], out["eye_coords"], out["too_far"]))
    return dict(det=det, far=out["too_far"], reg=out["reg"], rows=rows, kept=ER.purge(rows))


def test_detect_faces_past_one_chunk_against_numpy(rig):
    fdev = dev(TC.noise_frame(TC.B_FRAME[0], TC.B_FRAME[1], TC.B_SEED))
    c = composed(rig, fdev, TC.B_SF)
    far, rows, want = c["far"], c["rows"], c["kept"]
    assert c["det"]["n_windows"] == TC.B_WINDOWS
    print("accept-all %dx%d: %d survivors, %d too far (%d below face 1024), %d rows before the purge, %d after" %
          (TC.B_FRAME + (len(far), far.sum(), far[:TC.CHUNK].sum(), len(rows), len(want))))
    # what makes the case tell: more than one chunk of rows, kept and discarded faces on both sides of the chunk edge, a purge drop
    assert len(rows) > TC.CHUNK
    assert far[:TC.CHUNK].any() and (~far[:TC.CHUNK]).any() and far[TC.CHUNK:].any() and (~far[TC.CHUNK:]).any()
    assert far[2 * TC.CHUNK:].any() and (~far[2 * TC.CHUNK:]).any()                      # the last, partial chunk too
    assert 0 < len(want) < len(rows)
    got = rig.dc.detect_faces(fdev, rig.loc, smallest_face=TC.B_SF)
    assert got["n_windows"] == TC.B_WINDOWS and got["counts"] == c["det"]["counts"] == [TC.B_WINDOWS]
    assert got["n_before_purge"] == len(rows)
    assert got["faces"].shape == want.shape and np.array_equal(got["faces"], want)


def check_pooled(rig, frames, got, what):
    """Every frame of a pooled call against its own numpy composition.  Returns the per-frame (rows before, rows after)."""
    assert len(got["faces"]) == len(got["n_before_purge"]) == len(frames), what
    seen = []
    for f, frame in enumerate(frames):
        c = composed(rig, frame, TC.B_SF)
        assert got["n_before_purge"][f] == len(c["rows"]), (what, f, got["n_before_purge"][f], len(c["rows"]))
        assert got["faces"][f].shape == c["kept"].shape and np.array_equal(got["faces"][f], c["kept"]), (what, f)
        seen.append((len(c["rows"]), len(c["kept"])))
    assert got["n_windows"] == sum(TC.n_windows((int(fr.shape[1]), int(fr.shape[0])), TC.B_SF) for fr in frames), what
    print("%s: rows before / after the purge per frame %s" % (what, seen))
    return seen


def test_stack_with_long_segments_against_numpy(rig):
    import torch
    w, h = TC.B_FRAME
    s = TC.C_STACK_SEEDS
    frames = [dev(TC.noise_frame(w, h, s[0])), dev(TC.sparse_frame(w, h, s[1])), dev(TC.noise_frame(w, h, s[2]))]
    got = rig.dc.detect_faces_frames(torch.stack(frames), rig.loc, smallest_face=TC.B_SF)
    seen = check_pooled(rig, frames, got, "stack")
    assert seen[0][0] > TC.CHUNK and seen[2][0] > TC.CHUNK and seen[1][0] < TC.SMALL_ROWS
    assert seen[0][1] < seen[0][0] and seen[2][1] < seen[2][0]                          # the per-frame purge drops rows of a long segment
    assert seen[0][1] > TC.CHUNK                                                         # and keeps more than one tile of them


def test_list_with_long_segments_against_numpy(rig):
    frames = [dev(TC.noise_frame(w, h, seed)) for (w, h), seed in zip(TC.C_LIST, TC.C_LIST_SEEDS)]
    got = rig.dc.detect_faces_frame_list(frames, rig.loc, smallest_face=TC.B_SF)
    seen = check_pooled(rig, frames, got, "list")
    assert seen[0][0] > TC.CHUNK and seen[1][0] < TC.SMALL_ROWS and seen[2][0] > seen[1][0]
    assert seen[0][1] < seen[0][0]
    # the small frame first and last: segments that begin at row 0 and end at the count
    for order in ((1, 0, 2), (0, 2, 1)):
        sub = [frames[i] for i in order]
        check_pooled(rig, sub, rig.dc.detect_faces_frame_list(sub, rig.loc, smallest_face=TC.B_SF), "list %s" % (order,))


def test_stream_set_step_with_more_tracked_rows_than_one_chunk(rig):
    """Sixteen streams that hold eight faces each: the tracked pass carries 16 x 8 x 9 = 1152 windows, all accepted, into ONE eye tail
    (k_eyes_glue over two chunks, k_frame_segments and k_purge_frames_kept over 16 segments), while each stream's own FaceTracker carries
    72 — inside one chunk, so the oracle is independent of the chunk loop."""
    import torch
    from tests import stream_set_cases as SC
    w, h = TC.S_FRAME
    stack = torch.stack([dev(TC.noise_frame(w, h, seed)) for seed in TC.S_SEEDS])
    pair = SC.Pair(rig.dc, rig.loc, rig.cascade(), rig.locator(rig.clf_x, rig.clf_y), TC.S_STREAMS, TC.S_SF, max_faces=TC.S_FACES)
    try:
        first = pair.step(stack, "grid step")
        assert first["n_grid"] == TC.S_STREAMS and all(st["n_held"] == TC.S_FACES for st in first["streams"])
        second = pair.step(stack, "tracked step")
        assert second["n_tracked"] == TC.S_STREAMS
        live = sum(st["n_windows"] for st in second["streams"])
        before = [st["n_before_purge"] for st in second["streams"]]
        print("stream set: %d tracked windows, rows before the purge per stream %s, kept %s" %
              (live, before, [len(st["faces"]) for st in second["streams"]]))
        assert live == 9 * TC.S_STREAMS * TC.S_FACES > TC.CHUNK
        assert sum(before) > 0 and max(st["n_windows"] for st in second["streams"]) < TC.CHUNK
        # rows of faces on both sides of face 1024 of the pooled pass: streams below and above 1024 / 72 both give rows
        edge = TC.CHUNK // (9 * TC.S_FACES)
        assert sum(before[:edge]) > 0 and sum(before[edge + 1:]) > 0
    finally:
        pair.close()


# ---- D ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", TC.D_CASES, ids=["x=%r,y=%r" % (x, y) for x, y, _ in TC.D_CASES])
def test_too_far_threshold_on_the_tolerance(rig, case):
    from pyfaceanalysis_amd import synth_cascade
    x, y, every_face_far = case
    rng = np.random.default_rng(5)
    feats = rng.normal(size=(50, TC.K))
    clf_x, clf_y = synth_cascade.quantile_classifier(feats, TC.K, [x]), synth_cascade.quantile_classifier(feats, TC.K, [y])
    loc = rig.locator(clf_x, clf_y)
    fdev = dev(TC.noise_frame(TC.D_FRAME[0], TC.D_FRAME[1], TC.D_SEED))
    det = rig.dc.detect_frame(fdev, smallest_face=TC.D_SF)
    assert len(det["coords"]) == TC.D_WINDOWS
    out = loc.locate(fdev, det["coords"], det["angles"])
    assert out["reg"].shape == (2, 2 * TC.D_WINDOWS)
    assert np.all(out["reg"][0] == x) and np.all(out["reg"][1] == y)                     # one class: the regression IS the label
    assert np.all(out["too_far"] == every_face_far)
    assert (max(abs(x), abs(y)) == TC.TOLERANCE) is every_face_far
    got = rig.dc.detect_faces(fdev, loc, smallest_face=TC.D_SF)
    if every_face_far:
        assert got["faces"].shape == (0, 10) and got["n_before_purge"] == 0
    else:
        c = composed(rig, fdev, TC.D_SF, loc)
        assert got["n_before_purge"] == TC.D_WINDOWS == len(c["rows"])
        assert got["faces"].shape == c["kept"].shape and np.array_equal(got["faces"], c["kept"]) and len(c["kept"]) > 0


# ---- E ---------------------------------------------------------------------------------------------------------------------------------
def two_layer_flow(eye_size, seed=21):
    from pyfaceanalysis_amd.flow import Flow
    from tests import helpers
    rng = np.random.default_rng(seed)
    return Flow([helpers.rand_pca(rng, eye_size[0] * eye_size[1], 12), helpers.rand_sfa(rng, 12, TC.K)], output_dtype=np.float32)


@pytest.mark.parametrize("target", TC.E_TARGETS, ids=["128-48", "ref"])
@pytest.mark.parametrize("eye_size", TC.E_EYE_SIZES, ids=["16x16", "64x64", "24x20"])
def test_contrast_edges_bit_for_bit(rig, eye_size, target):
    from oracle import pil_restate
    from pyfaceanalysis_amd import synth_cascade
    flow = None if eye_size == TC.SUB else two_layer_flow(eye_size)          # T5L-16 reads 16 x 16; a random two-layer net the others
    rng = np.random.default_rng(6)
    feats = rng.normal(size=(50, TC.K))
    labels = np.linspace(-10.5, 10.5, 5)
    loc = rig.locator(synth_cascade.quantile_classifier(feats, TC.K, labels), synth_cascade.quantile_classifier(feats, TC.K, labels, descending=True),
                      flow=flow, eye_size=eye_size, contrast=target)
    boxes, angles = TC.contrast_faces()
    eb = loc.eye_boxes(boxes, angles)
    dang = -np.concatenate([angles, angles])
    npix = eye_size[0] * eye_size[1]
    kinds = np.zeros(4, dtype=np.int64)
    try:
        for name, frame in TC.contrast_frames().items():
            out = loc.locate(dev(frame), boxes, angles, return_patches=True)
            u8 = pil_restate.extract_subimages_rotate(frame, eb, dang, eye_size)
            want = ER.contrast(u8, *target)
            assert out["patches"].shape == (2 * len(boxes), npix) and out["patches"].dtype == np.float32, name
            assert np.array_equal(out["patches"], want), (name, int((out["patches"] != want).sum()))
            assert np.isfinite(out["reg"]).all(), name
            kinds += np.array(TC.patch_kinds(u8, target))
    finally:
        if flow is not None:
            import torch
            torch.cuda.synchronize()
            rig.open.remove(loc)
            loc.close()
            flow.close()
    # the cases contain: a patch of std 0 (output target_mean everywhere), one clipped at 0, one clipped at 255, an all-zero one
    assert (kinds > 0).all(), kinds


def test_estimator_contrast_edges_bit_for_bit(native_lib):
    """k_patch_contrast (the estimator's patch step, composed and fused) on crops of the crafted frames: boxes inside the crop, over its
    left / top border (two-level patches) and wholly outside it (all zero), 8 x 8 and 13 x 11 patches (143 pixels: not a multiple of the
    kernel's thread count), both target pairs."""
    import torch
    from pyfaceanalysis_amd import analysis as A
    from pyfaceanalysis_amd.flow import Flow
    from tests import analysis_cases as AC
    cw, ch = AC.SMALL_CROP
    crops = np.ascontiguousarray(np.stack([f[:ch, :cw] for f in TC.contrast_frames().values()]))
    dense = torch.from_numpy(crops).cuda()
    kinds = np.zeros(4, dtype=np.int64)
    for patch_size in ((8, 8), (13, 11)):
        flow = Flow(AC.patch_flow(patch_size), output_dtype=np.float32)
        clf = AC.synthetic_classifier(5, np.zeros((2, 5)), 5, AC.GENDER_LABELS)
        for box in ((3.3, 2.1, 30.7, 41.9), (-9.4, -6.2, 27.3, 30.1), (-60.0, -60.0, -20.0, -16.0)):
            cut = AC.pil_cut(crops, patch_size, box, 0)
            for target in TC.E_TARGETS:
                want = ER.contrast(cut, *target)
                fa = A.FaceAnalyzer(flow, gender=clf, contrast=target, patch_size=patch_size, box=box, crop_size=AC.SMALL_CROP)
                try:
                    for flags in (0, A.FLAG_COMPOSED, A.FLAG_FUSED):
                        got = fa.patches(dense, flags=flags).cpu().numpy()
                        assert got.dtype == np.float32 and np.array_equal(got, want), (patch_size, box, target, flags)
                finally:
                    fa.close()
                kinds += np.array(TC.patch_kinds(cut, target))
        clf.close()
        flow.close()
    assert (kinds > 0).all(), kinds
