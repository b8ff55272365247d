"""GPU: pose normalisation and age / race / gender estimation for faces spread over a LIST of frames of different sizes
(hg_patcher_normalize_frame_list_device, hg_estimator_estimate_frame_list_device; ``FaceNormalizer.normalize_frame_list``,
``FaceAnalyzer.estimate_frame_list`` / ``estimate_faces_frame_list``, ``DeviceCascade.prescale_frame_list``) against the per-frame public
calls, which are their exact oracle: every face is normalised from its own record on its own frame, the patch kernels use one workgroup
per face, the network and the regressions are bit-identical across batch sizes.  Every comparison is ``==`` on bytes or bits (NaNs by
position), against objects created per frame; no tolerance anywhere.  The cases are in tests/estimate_frame_list_cases.py; the rigs and
helpers are those of tests/test_estimate_frames_gpu.py."""
import numpy as np
import pytest

from pyfaceanalysis_amd import analysis as A
from tests import analysis_cases as AC
from tests import estimate_frame_list_cases as LE
from tests import frame_batch_cases as BC
from tests import frame_list_cases as LC
from tests import normalize_cases as NC
from tests import test_estimate_frames_gpu as EF

pytestmark = pytest.mark.gpu

VALUE_KEYS, ALL_KEYS = EF.VALUE_KEYS, EF.ALL_KEYS
dev, normalizer, per_frame_images, assert_same, assert_dicts_equal = EF.dev, EF.normalizer, EF.per_frame_images, EF.assert_same, EF.assert_dicts_equal


@pytest.fixture(scope="module")
def rigs(native_lib):
    """The list of tests/frame_list_cases.py on the device — three views of one buffer of 255s —, its frames as dense tensors of their own
    (the per-frame oracle's), and normalizers by case."""
    import torch
    buf, frames, inside = LE.device_list(torch)
    host = LE.host_frames()
    assert all(np.array_equal(f.cpu().numpy(), h) for f, h in zip(frames, host))
    assert [f.stride(0) for f in frames] == [ld for _w, _h, ld, _s in LC.PATCH_FRAMES] and [tuple(f.shape) for f in frames] == [(h, w) for w, h in LE.SIZES]
    made = {}

    def norm(size, method, rotate=True):
        key = (size, method, rotate)
        if key not in made:
            made[key] = normalizer(size, method, rotate)
        return made[key]

    def untouched():
        return bool((buf.cpu().numpy()[~inside] == 255).all())
    yield dict(torch=torch, buf=buf, list=frames, host=host, frames=[dev(h) for h in host], norm=norm, untouched=untouched)
    torch.cuda.synchronize()
    for fn in made.values():
        fn.close()


# ---- normalise -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size,method,rotate", LE.NORMALIZE_CASES, ids=["%dx%d-%s" % (s[0], s[1], "rot" if r else "norot") for s, m, r in LE.NORMALIZE_CASES])
def test_normalize_frame_list_equals_normalize_per_frame(rigs, size, method, rotate):
    """Faces on three frames of different sizes and row strides cut from one buffer of 255s, not sorted by frame (asserted in
    ``spread_faces``): the nine eye sets, border faces over every edge of their OWN frame and the big faces of every frame; the default
    path choice and both forced ones.  The buffer's bytes outside the frames stay 255."""
    eyes, ff = LE.spread_faces(n_random=10 if size[0] < 100 else 2)
    fn = rigs["norm"](size, method, rotate)
    g, _ = fn.list_geometry(LE.SIZES, eyes, ff)
    staged, taps = LE.modes(g, size)
    if size[0] < 100:
        assert set(ff[taps]) == {1, 2} and set(ff[staged]) == {0, 1, 2}, "staged and tap-by-tap faces in one call"
    if not rotate:
        over = LE.overhang(g, ff)
        assert over[1] == (True,) * 4 and over[2] == (True,) * 4 and any(over[0]), over
    want, status = per_frame_images(rigs["frames"], eyes, ff, size, method, rotate)
    for flags in (0, 1, 2):
        img, st = fn.normalize_frame_list(rigs["list"], eyes, ff, flags=flags)
        assert tuple(img.shape) == want.shape and img.dtype == rigs["torch"].uint8 and st.dtype == np.int32
        got = img.cpu().numpy()
        assert np.array_equal(st, status) and np.count_nonzero(st == 0) >= len(ff) - 2
        assert np.array_equal(got, want), (flags, np.flatnonzero((got != want).any(axis=(1, 2))))
    assert all(want[ff == f].reshape(int((ff == f).sum()), -1).any(axis=1).sum() >= 6 for f in range(LE.N_FRAMES)), "the oracle's images are not empty, on any frame"
    assert (want == 0).any(), "crops reach over their frames: zeros, never the buffer's 255s"
    img, st = fn.normalize_frame_list(rigs["list"], geoms=g, face_frame=ff.astype(np.int64))      # the geoms in place of the eyes
    assert np.array_equal(img.cpu().numpy(), want) and np.array_equal(st, status)
    assert rigs["untouched"]()
    if rotate:
        assert not np.array_equal(want, per_frame_images(rigs["frames"], eyes, ff, size, method, False)[0])


def test_one_size_twice_and_one_tensor_twice(rigs):
    """[97 x 131, 7 x 5, another 97 x 131 with other pixels, the first tensor again, 40 x 61]: two frames of one size are two frames, a
    tensor listed twice is one frame under two indices; the 7 x 5 frame stands between the larger ones."""
    size, method = NC.SMALL_OUT_SIZES[0]
    w, h = LE.SIZES[1]
    other = dev(BC.noise_frame(w, h, 9177))
    frames = [rigs["list"][1], rigs["list"][0], other, rigs["list"][1], rigs["list"][2]]
    dense = [rigs["frames"][1], rigs["frames"][0], other, rigs["frames"][1], rigs["frames"][2]]
    sizes = [(int(f.shape[1]), int(f.shape[0])) for f in frames]
    assert sizes[0] == sizes[2] == sizes[3] and min(sizes) == sizes[1] == (7, 5)
    eyes, ff = LE.spread_faces(sizes=sizes, n_random=3, seed=2)
    want, status = per_frame_images(dense, eyes, ff, size, method)
    img, st = rigs["norm"](size, method).normalize_frame_list(frames, eyes, ff)
    got = img.cpu().numpy()
    assert np.array_equal(got, want) and np.array_equal(st, status)
    same_eyes = np.array([NC.eye_sets(w, h)[0][1]] * 3)
    got = rigs["norm"](size, method).normalize_frame_list(frames, same_eyes, [0, 2, 3])[0].cpu().numpy()
    assert np.array_equal(got[0], got[2]) and not np.array_equal(got[0], got[1]), "one tensor twice: equal images; one size twice: each its own pixels"


def test_a_frame_without_faces_and_all_faces_on_the_last_frame(rigs):
    size, method = NC.SMALL_OUT_SIZES[0]
    fn = rigs["norm"](size, method)
    for only in ((2, 0), (2,)):      # no face on frame 1 between frames with several; then all faces on the last frame
        eyes, ff = LE.spread_faces(only=only, seed=3)
        assert set(ff) == set(only)
        want, status = per_frame_images(rigs["frames"], eyes, ff, size, method)
        img, st = fn.normalize_frame_list(rigs["list"], eyes, ff)
        assert np.array_equal(img.cpu().numpy(), want) and np.array_equal(st, status) and want.any(), only
    assert rigs["untouched"]()


def test_refused_faces_and_frame_indices_outside_the_list(rigs):
    """Swapped and NaN eyes and frame indices -1, B and B + 5 between good faces: zero images, status 1 / 2 / 5, the neighbours' bytes
    those of a call without them.  On the list cut from the larger buffer, and on frames that ARE their allocations."""
    t = rigs["torch"]
    size, method = NC.SMALL_OUT_SIZES[0]
    fn = rigs["norm"](size, method)
    eyes0, ff0 = LE.spread_faces(n_random=3)
    eyes, ff, bad = LE.with_bad_rows(eyes0, ff0, LE.N_FRAMES)
    good = np.array([i not in bad for i in range(len(ff))])
    want0, _ = per_frame_images(rigs["frames"], eyes0, ff0, size, method)
    for frames in (rigs["list"], rigs["frames"]):
        for flags in (0, 1, 2):
            out = t.full((len(ff), size[1], size[0]), 7, dtype=t.uint8, device="cuda")
            img, st = fn.normalize_frame_list(frames, eyes, ff, out=out, flags=flags)
            got = img.cpu().numpy()
            assert img.data_ptr() == out.data_ptr() and {i: int(st[i]) for i in bad} == bad and not st[good].any()
            assert not got[~good].any()
            assert np.array_equal(got[good], want0), flags
    w, h = LE.SIZES[1]
    img, st = fn.normalize_frame_list([rigs["frames"][1]], np.array([NC.eye_sets(w, h)[0][1]] * 4), np.array([0, 1, 0, -1], dtype=np.int32))      # B = 1: index 1 is outside
    assert list(st) == [0, 5, 0, 5] and not img[1].any() and not img[3].any() and img[0].any() and bool((img[0] == img[2]).all())
    assert rigs["untouched"]()


def test_a_list_of_one_frame_and_a_list_cut_from_a_stack(rigs):
    """A list of one frame equals the single-frame entry; the frames of the stack of tests/estimate_frames_cases.py as a list equal
    ``normalize_frames`` on that stack."""
    from tests import estimate_frames_cases as EC
    size, method = NC.SMALL_OUT_SIZES[1]
    fn = rigs["norm"](size, method)
    for f, frame in enumerate(rigs["list"]):
        w, h = LE.SIZES[f]
        eyes = np.array([e for _, e in NC.eye_sets(w, h)] + LE.border_eyes(w, h))
        want, wst = fn.normalize(frame, eyes)
        got, gst = fn.normalize_frame_list([frame], eyes, np.zeros(len(eyes), dtype=np.int32))
        assert np.array_equal(got.cpu().numpy(), want.cpu().numpy()) and np.array_equal(gst, wst) and want.any()
    _buf, stack = EC.device_stack(rigs["torch"])
    eyes, ff = EC.spread_faces()
    want, wst = fn.normalize_frames(stack, eyes, ff)
    got, gst = fn.normalize_frame_list([stack[i] for i in range(EC.N_FRAMES)], eyes, ff)
    assert np.array_equal(got.cpu().numpy(), want.cpu().numpy()) and np.array_equal(gst, wst) and want.any()


def test_a_pitched_out_and_images_farther_apart_than_their_size(rigs):
    t = rigs["torch"]
    size, method = NC.SMALL_OUT_SIZES[0]
    fn = rigs["norm"](size, method)
    eyes, ff = LE.spread_faces(n_random=2)
    want, status = per_frame_images(rigs["frames"], eyes, ff, size, method)
    n, px, gap = len(ff), size[0] * size[1], 13
    buf = t.full((n, px + gap), 0xA5, dtype=t.uint8, device="cuda")      # a row stride above out_w * out_h: the gap bytes are untouched
    got, st = fn.normalize_frame_list(rigs["list"], eyes, ff, out=buf[:, :px].view(n, size[1], size[0]))
    assert got.data_ptr() == buf.data_ptr() and np.array_equal(st, status)
    b = buf.cpu().numpy()
    assert np.array_equal(b[:, :px].reshape(n, size[1], size[0]), want) and np.all(b[:, px:] == 0xA5)
    big = t.full((2 * n, size[1], size[0]), 0x5A, dtype=t.uint8, device="cuda")      # every second image of a larger tensor
    got, _ = fn.normalize_frame_list(rigs["list"], eyes, ff, out=big[::2])
    b = big.cpu().numpy()
    assert np.array_equal(b[::2], want) and np.all(b[1::2] == 0x5A)
    for bad in (big[:n].transpose(1, 2), big[:n - 1], big[:n].float()):
        with pytest.raises(ValueError, match="out must be"):
            fn.normalize_frame_list(rigs["list"], eyes, ff, out=bad)


def test_more_than_65535_faces(rigs):
    """65573 faces with a 2 x 2 output on the three frames: the face loop over gridDim.y with a resolved frame per face."""
    size, method = (2, 2), NC.AREA
    n = 65536 + 37
    ff = ((np.arange(n) * 7 + np.arange(n) // 5) % LE.N_FRAMES).astype(np.int32)
    base = [np.concatenate([NC.random_eyes(700, s, seed=k) for k in (21, 22)]) for s in LE.SIZES]
    eyes = np.stack([base[f][i % len(base[f])] for i, f in enumerate(ff)])
    ff[[100, 65535, 65536, n - 1]] = [-1, 3, 0, 2]
    eyes[65536], eyes[n - 1] = NC.eye_sets(*LE.SIZES[0])[0][1], NC.eye_sets(*LE.SIZES[2])[0][1]
    want, status = per_frame_images(rigs["frames"], eyes, ff, size, method)
    img, st = rigs["norm"](size, method).normalize_frame_list(rigs["list"], eyes, ff)
    got = img.cpu().numpy()
    assert np.array_equal(st, status) and list(st[[100, 65535]]) == [5, 5]
    assert np.array_equal(got, want), np.flatnonzero((got != want).any(axis=(1, 2)))[:10]
    assert want[65536:].any() and want.reshape(n, -1).any(axis=1).sum() > n // 10
    assert rigs["untouched"]()


def test_workspace_growth_and_reuse(rigs):
    """A small call, a larger one and a small one again through ONE long-lived normalizer — the face buffer and the scratch grow between
    them —, a stack call and a single-frame call between them, each against normalizers created per frame."""
    size, method = NC.SMALL_OUT_SIZES[0]
    one = normalizer(size, method)
    eyes, ff = LE.spread_faces(n_random=40)
    for n in (3, len(ff), 3):
        for flags in (0, 1):
            want, status = per_frame_images(rigs["frames"], eyes[:n], ff[:n], size, method)
            img, st = one.normalize_frame_list(rigs["list"], eyes[:n], ff[:n], flags=flags)
            assert np.array_equal(img.cpu().numpy(), want) and np.array_equal(st, status), (n, flags)
        idx = np.flatnonzero(ff[:n] == ff[0])
        frame = rigs["list"][int(ff[0])]
        assert np.array_equal(one.normalize(frame, eyes[:n][idx])[0].cpu().numpy(), want[idx])
        assert np.array_equal(one.normalize_frames(frame[None], eyes[:n][idx], np.zeros(len(idx), dtype=np.int32))[0].cpu().numpy(), want[idx])
    rigs["torch"].cuda.synchronize()
    one.close()


# ---- estimate ------------------------------------------------------------------------------------------------------------------------
class ListRig(EF.EstRig):
    """EF.EstRig's analyzers and per-frame oracle on the estimate list: 200 x 150, 97 x 131 and 160 x 120 noise frames."""

    def __init__(self, torch):
        EF.EstRig.__init__(self, torch)
        self.host = LE.est_frames()
        self.frames = [dev(h) for h in self.host]
        self.stack = None
        self.eyes, self.ff = LE.est_faces()


@pytest.fixture(scope="module")
def est(native_lib):
    import torch
    r = ListRig(torch)
    yield r
    r.close()


@pytest.mark.parametrize("clip,targets", ((True, AC.CONTRAST_STEEP), (False, AC.CONTRAST_UNCLIPPED)), ids=("clipped", "unclipped"))
@pytest.mark.parametrize("filt", sorted(AC.FILTERS))
def test_estimate_frame_list_equals_estimate_per_frame(est, filt, clip, targets):
    """Three frames of different sizes with 3, 2 and 4 faces, interleaved: every value key, the status, labels and confidences, the
    patches and the features — on the default patch path, the composed one and the fused kernel."""
    kw = dict(interpolation=filt, clip=clip, contrast=targets, box=LE.PATCH_BOX_OVER if filt == "BILINEAR" else LE.PATCH_BOX)
    keys = ALL_KEYS + ("patches", "features")
    want = est.per_frame(est.frames, est.eyes, est.ff, **kw)
    assert list(want["status"]) == [0] * 9 and len({float(v) for v in want["age"]}) >= 5 and len({p.tobytes() for p in want["patches"]}) == 9
    fa = est.analyzer(**kw)
    for flags in (0, A.FLAG_COMPOSED, A.FLAG_FUSED):
        got = fa.estimate_frame_list(est.frames, est.eyes, est.ff, return_intermediates=True, flags=flags)
        assert sorted(got) == sorted(keys)
        assert_same(got, want, keys, (filt, clip, flags))
    plain = fa.estimate_frame_list(est.frames, est.eyes, est.ff)
    assert "patches" not in plain and "features" not in plain
    assert_same(plain, want, ALL_KEYS)
    g, _ = fa._norm.list_geometry(LE.EST_SIZES, est.eyes, est.ff)
    assert_same(fa.estimate_frame_list(tuple(est.frames), geoms=g, face_frame=est.ff), want, ALL_KEYS)


def test_refused_and_outside_faces_leave_the_others_alone(est):
    eyes, ff, bad = LE.with_bad_rows(np.concatenate([est.eyes, est.eyes]), np.concatenate([est.ff, est.ff]), 3)
    good = np.array([i not in bad for i in range(len(ff))])
    fa = est.analyzer()
    got = fa.estimate_frame_list(est.frames, eyes, ff, return_intermediates=True)
    assert {i: int(got["status"][i]) for i in bad} == bad and not got["status"][good].any()
    for k in VALUE_KEYS + ("race_confidence", "gender_confidence"):
        assert np.isnan(got[k][~good]).all() and np.isfinite(got[k][good]).all(), k
    assert all(got[k][i] is None for i in bad for k in ("race_label", "gender_label")) and None not in [got["race_label"][i] for i in np.flatnonzero(good)]
    alone = fa.estimate_frame_list(est.frames, eyes[good], ff[good], return_intermediates=True)
    keys = ALL_KEYS + ("patches", "features")
    assert_same(got, EF._scatter(alone, good), keys, "neighbours", rows=np.flatnonzero(good))
    want = est.per_frame(est.frames, eyes, ff)
    assert_same(got, want, ALL_KEYS, "per frame")
    assert_same(got, want, ("patches", "features"), "per frame", rows=np.flatnonzero(good))


def test_absent_classifiers_keep_the_initial_values(est):
    want = est.per_frame(est.frames, est.eyes, est.ff, intermediates=False)
    ff = est.ff.copy()
    ff[3] = 3      # outside the list: NaN in the rows of absent classifiers too
    keep = np.arange(len(ff)) != 3
    for on, keys in ((dict(age=False, race=False), ("gender",)), (dict(race=False, gender=False), ("age", "age_std")), (dict(age=False, gender=False), ("race",))):
        fa = est.analyzer(n_features=5, **on)
        got = fa.estimate_frame_list(est.frames, est.eyes, est.ff)
        assert (set(got) & set(VALUE_KEYS)) == set(keys) and all(AC.same(got[k], want[k]) for k in keys), keys
        got = fa.estimate_frame_list(est.frames, est.eyes, ff)
        assert got["status"][3] == LE.STATUS_FRAME_RANGE and all(np.isnan(got[k][3]) and AC.same(got[k][keep], want[k][keep]) for k in keys), keys
    # the raw block: the rows of absent classifiers hold 0, 0, 10, 10
    import ctypes as C
    from pyfaceanalysis_amd import _capi, normalize as N
    t = est.torch
    only_race = est.analyzer(age=False, gender=False, n_features=5)
    g, ffc = only_race._norm.list_geometry(LE.EST_SIZES, est.eyes, ff)
    n = len(g)
    out = t.full((4, n + 1), -3.0, dtype=t.float64, device="cuda")
    refs = N.list_refs(est.frames)
    _capi.check(_capi.lib().hg_estimator_estimate_frame_list_device(only_race._handle(), 0, refs, 3, g.ctypes.data_as(C.c_void_p), ffc.ctypes.data_as(C.c_void_p), n,
                                                                    out.data_ptr(), n + 1, None, None, t.cuda.current_stream().cuda_stream))
    b = out.cpu().numpy()
    assert np.all(b[:, n] == -3.0) and np.isnan(b[:, 3]).all()
    assert np.all(b[0, :n][keep] == 0.0) and np.all(b[1, :n][keep] == 0.0) and AC.same(b[2, :n][keep], want["race"][keep]) and np.all(b[3, :n][keep] == 10.0)


def test_permuting_the_list_permutes_nothing_in_the_results(est):
    fa = est.analyzer()
    keys = ALL_KEYS + ("patches", "features")
    want = fa.estimate_frame_list(est.frames, est.eyes, est.ff, return_intermediates=True)
    perm = np.array([2, 0, 1])                       # new frame j is old frame perm[j]
    where = np.argsort(perm)                         # old frame f is new frame where[f]
    got = fa.estimate_frame_list([est.frames[p] for p in perm], est.eyes, where[est.ff].astype(np.int32), return_intermediates=True)
    assert_same(got, want, keys)
    assert_same(want, est.per_frame(est.frames, est.eyes, est.ff), keys)


# ---- prescale ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rig(native_lib, nets):
    from tests import test_frame_stream_gpu as FS
    r = FS.Rig(nets, keep=BC.KEEP, later_keep=BC.LATER_KEEP)
    yield r
    r.close()


def _colour(noise, fmt):
    if fmt == "L":
        return noise
    planes = {"RGB": (noise, 255 - noise, noise[::-1]), "BGRA": (noise[::-1], noise, 255 - noise, noise[:, ::-1])}[fmt]
    return np.ascontiguousarray(np.stack(planes, axis=2))


@pytest.mark.parametrize("fmt,filt", (("L", "NEAREST"), ("RGB", "BILINEAR"), ("BGRA", "NEAREST")))
def test_prescale_frame_list_equals_prescale_per_frame(rig, fmt, filt):
    """[640 x 480, 200 x 150, another 640 x 480 with other pixels, 97 x 131] at prescale_size 300: the two large frames shrink to 300 x 225,
    the small ones need no shrinking (a grey one comes back as the same tensor, a colour one converted).  Against ``prescale`` per frame
    on another cascade, cloned at once.  Then a longer list: the buffer grows."""
    import torch
    from pyfaceanalysis_amd.cascade import DeviceCascade
    from tests import test_frame_stream_gpu as FS
    sizes = [(640, 480), (200, 150), (640, 480), (97, 131)]
    host = [_colour(BC.noise_frame(w, h, 9500 + i), fmt) for i, (w, h) in enumerate(sizes)]
    dc = DeviceCascade(rig.stages, FS.SUB, FS.K, rig.pipe, frame_format=fmt, prescale_filter=filt)
    ref = DeviceCascade(rig.stages, FS.SUB, FS.K, rig.pipe, frame_format=fmt, prescale_filter=filt)
    try:
        fdev = [dev(x) for x in host]
        want = [ref.prescale(f, 300).clone().cpu().numpy() for f in fdev]
        assert want[0].shape == want[2].shape == (225, 300) and want[1].shape == (150, 200) and not np.array_equal(want[0], want[2])
        got = dc.prescale_frame_list(fdev, prescale_size=300)
        assert len(got) == 4 and all(g.dtype == torch.uint8 and g.dim() == 2 for g in got)
        assert all(np.array_equal(g.cpu().numpy(), w) for g, w in zip(got, want)), (fmt, filt)
        assert got[0].data_ptr() != got[2].data_ptr() and not torch.equal(got[0], got[2]), "two frames of one size come back as two frames"
        if fmt == "L":
            assert got[1] is fdev[1] and got[3] is fdev[3], "a grey frame that needs no shrinking is returned as it is"
        else:
            assert all(g.data_ptr() % 256 == 0 for g in got)
        # a longer list (the first one twice, a view with a row pitch among them): the buffer grows, the results are the oracle's again
        pitched = torch.full((480 + 4, (640 + 9) * fdev[0].shape[2] if fmt != "L" else 640 + 9), 255, dtype=torch.uint8, device="cuda")
        view = pitched[2:482, :640] if fmt == "L" else pitched[2:482, :640 * fdev[0].shape[2]].view(480, 640, fdev[0].shape[2])
        view.copy_(fdev[2])
        longer = fdev + [view] + fdev
        size_before = dc._list_pre.numel()
        got2 = dc.prescale_frame_list(longer, prescale_size=300)
        assert dc._list_pre.numel() > size_before
        assert all(np.array_equal(g.cpu().numpy(), w) for g, w in zip(got2, want + [want[2]] + want)), (fmt, filt, "longer")
        assert all(np.array_equal(g.cpu().numpy(), w) for g, w in zip(got, want)), "the first call's views still hold their frames (the old buffer lives with them)"
        again = dc.prescale_frame_list(fdev, prescale_size=300)      # the shorter list again, in the grown buffer
        assert all(np.array_equal(g.cpu().numpy(), w) for g, w in zip(again, want))
        assert dc.prescale_frame_list([], prescale_size=300) == []
    finally:
        torch.cuda.synchronize()
        dc.close()
        ref.close()


# ---- end to end ----------------------------------------------------------------------------------------------------------------------
def end_to_end(est, dc, loc, fdev, what):
    """detect_faces_frame_list -> prescale_frame_list -> estimate_faces_frame_list against detect_faces -> prescale -> estimate_faces per
    frame, dict for dict."""
    from tests import test_frame_stream_gpu as FS
    want = []
    for f in fdev:
        faces = dc.detect_faces(f, loc, smallest_face=FS.SF)["faces"]
        small = dc.prescale(f).clone()
        fa = est.analyzer()
        want.append((faces, small.cpu().numpy(), fa.estimate_faces(small, faces, return_intermediates=True)))
    n = [len(w[0]) for w in want]
    assert sum(1 for x in n if x > 0) >= 2 and 0 in n, (what, n)      # at least two frames have faces and one has none
    pooled = dc.detect_faces_frame_list(fdev, loc, smallest_face=FS.SF)["faces"]
    assert all(np.array_equal(p, w[0]) for p, w in zip(pooled, want)), what
    smalls = dc.prescale_frame_list(fdev)
    assert len(smalls) == len(want) and all(np.array_equal(s.cpu().numpy(), w[1]) for s, w in zip(smalls, want)), what
    got = est.analyzer().estimate_faces_frame_list(smalls, pooled, return_intermediates=True)
    assert len(got) == len(want)
    for f, (g, w) in enumerate(zip(got, want)):
        assert_dicts_equal(g, w[2], (what, f))
    return smalls, n


def test_end_to_end_on_the_mixed_grey_list(est, rig):
    """LC.MIXED: 97 x 131 and 320 x 240 frames in turn, faces 0 / 25 / 0 / 23 / 1 on an MI355X (tests/frame_batch_cases.py)."""
    from tests import test_frame_batch_gpu as FB
    dc, loc, close = rig.fresh()
    try:
        fdev = [dev(FB.frame_of(size, seed)) for size, seed in LC.MIXED]
        smalls, n = end_to_end(est, dc, loc, fdev, "mixed grey")
        assert all(s is f for s, f in zip(smalls, fdev)) and len({tuple(f.shape) for f in fdev}) == 2
    finally:
        close()


def test_end_to_end_on_an_rgb_list_behind_a_bilinear_prescale(est, rig):
    """LC.MIXED as RGB frames with three equal planes (PIL's "L" of (n, n, n) is n: the faces are the grey list's), and a 1280 x 720 frame
    (BC.hd_frame as (n, n, 255 - n)) that the BILINEAR prescale shrinks to 1000 x 562."""
    from pyfaceanalysis_amd.cascade import DeviceCascade
    from tests import test_frame_batch_gpu as FB
    from tests import test_frame_stream_gpu as FS
    grey = [FB.frame_of(size, seed) for size, seed in LC.MIXED]
    hd = BC.hd_frame(BC.HD_SEEDS[0])
    rgb = [dev(np.ascontiguousarray(np.stack([n, n, n], axis=2))) for n in grey[:3]] + [dev(np.ascontiguousarray(np.stack([hd, hd, 255 - hd], axis=2)))] + [
        dev(np.ascontiguousarray(np.stack([n, n, n], axis=2))) for n in grey[3:]]
    dc = DeviceCascade(rig.stages, FS.SUB, FS.K, rig.pipe, frame_format="RGB", prescale_filter="BILINEAR")
    try:
        smalls, n = end_to_end(est, dc, rig.loc, rgb, "rgb")
        assert tuple(smalls[3].shape) == (562, 1000) and [tuple(s.shape) for s in smalls[:3]] == [g.shape for g in grey[:3]]
        assert all(np.array_equal(s.cpu().numpy(), g) for s, g in zip(smalls[:3], grey[:3]))
    finally:
        dc.close()
