"""GPU: pose normalisation and age / race / gender estimation for faces spread over a stack of same-size frames
(hg_patcher_normalize_frames_device, hg_estimator_estimate_frames_device; ``FaceNormalizer.normalize_frames``,
``FaceAnalyzer.estimate_frames`` / ``estimate_faces_frames``, ``DeviceCascade.prescale_frames``) against the per-frame public calls, which
are their exact oracle: every face is normalised from its own record, the patch kernels use one workgroup per face, the network and the
regressions are bit-identical across batch sizes.  Every comparison is ``==`` on bytes or bits (NaNs by position), against objects
created per frame; no tolerance anywhere.  The cases are in tests/estimate_frames_cases.py."""
import ctypes as C

import numpy as np
import pytest

from pyfaceanalysis_amd import _capi, analysis as A, normalize as N
from tests import analysis_cases as AC
from tests import estimate_frames_cases as EC
from tests import frame_batch_cases as BC
from tests import normalize_cases as NC

pytestmark = pytest.mark.gpu

VALUE_KEYS = ("age", "age_std", "race", "gender")
ALL_KEYS = VALUE_KEYS + ("status", "race_confidence", "gender_confidence", "race_label", "gender_label")


def method_name(method):
    return "eyes_inferred-mouth_areaZ" if method == NC.AREAZ else "eyes_inferred-mouth_area"


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def normalizer(size, method, rotate=True):
    return N.FaceNormalizer(0, preset="pose", out_size=size, method=method_name(method), rotate=rotate)


def per_frame_images(frames_dev, eyes, ff, size, method, rotate=True, flags=0):
    """(images, status) of ``normalize`` on every frame for that frame's faces, each through a normalizer created for that frame; the
    faces whose frame is outside the list keep zero images and status 5."""
    import torch
    n, b = len(ff), len(frames_dev)
    want = np.zeros((n, size[1], size[0]), dtype=np.uint8)
    status = np.where((ff < 0) | (ff >= b), EC.STATUS_FRAME_RANGE, 0).astype(np.int32)
    for f, frame in enumerate(frames_dev):
        idx = np.flatnonzero(ff == f)
        fn = normalizer(size, method, rotate)
        img, st = fn.normalize(frame, eyes[idx], flags=flags)
        want[idx], status[idx] = img.cpu().numpy(), st
        torch.cuda.synchronize()
        fn.close()
    return want, status


@pytest.fixture(scope="module")
def rigs(native_lib):
    """The stack of tests/frame_batch_cases.py on the device, its frames as dense tensors of their own, and normalizers by case."""
    import torch
    buf, stack = EC.device_stack(torch)
    host = EC.host_frames()
    assert all(np.array_equal(stack[f].cpu().numpy(), host[f]) for f in range(BC.N_FRAMES)) and stack.stride() == (BC.FRAME_STRIDE, BC.LD, 1)
    made = {}

    def norm(size, method, rotate=True):
        key = (size, method, rotate)
        if key not in made:
            made[key] = normalizer(size, method, rotate)
        return made[key]
    yield dict(torch=torch, buf=buf, stack=stack, host=host, frames=[dev(h) for h in host], norm=norm)
    torch.cuda.synchronize()
    for fn in made.values():
        fn.close()


# ---- normalise -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size,method,rotate", EC.NORMALIZE_CASES, ids=["%dx%d-%s" % (s[0], s[1], "rot" if r else "norot") for s, m, r in EC.NORMALIZE_CASES])
def test_normalize_frames_equals_normalize_per_frame(rigs, size, method, rotate):
    """57 faces on three frames cut from one buffer of 255s (ld 144, frame stride no multiple of it), not sorted by frame."""
    eyes, ff = EC.spread_faces(n_random=10 if size[0] < 100 else 2)
    want, status = per_frame_images(rigs["frames"], eyes, ff, size, method, rotate)
    img, st = rigs["norm"](size, method, rotate).normalize_frames(rigs["stack"], eyes, ff)
    assert tuple(img.shape) == want.shape and img.dtype == rigs["torch"].uint8 and st.dtype == np.int32
    got = img.cpu().numpy()
    assert np.array_equal(st, status) and np.count_nonzero(st == 0) >= len(ff) - 2
    assert np.array_equal(got, want), np.flatnonzero((got != want).any(axis=(1, 2)))
    # (the seeded random eyes lie around the frame as often as on it; the nine named eye sets of every frame lie on it)
    assert (want.reshape(len(ff), -1).any(axis=1)).sum() >= 18, "the oracle's images are not empty"
    if rotate:
        assert not np.array_equal(want, per_frame_images(rigs["frames"], eyes, ff, size, method, False)[0])


def test_several_faces_on_one_frame_none_on_another(rigs):
    size, method = NC.SMALL_OUT_SIZES[0]
    eyes, ff = EC.spread_faces(only=(2, 0), seed=3)
    assert set(ff) == {0, 2}
    want, status = per_frame_images(rigs["frames"], eyes, ff, size, method)
    fn = rigs["norm"](size, method)
    img, st = fn.normalize_frames(rigs["stack"], eyes, ff)
    assert np.array_equal(img.cpu().numpy(), want) and np.array_equal(st, status)
    g = fn.geometry(eyes, EC.FRAME)      # the geoms in place of the eyes, and a list of frames in place of the tensor
    img, st = fn.normalize_frames([f for f in rigs["frames"]], geoms=g, face_frame=ff.astype(np.int64))
    assert np.array_equal(img.cpu().numpy(), want) and np.array_equal(st, status)


def test_border_faces_beside_frames_of_255(rigs):
    """A contiguous stack (frame_stride = H W): noise, all 255, noise.  Faces at the borders of the first and the last frame: a wrong
    inside test or offset reads a neighbour's 255s.  Against ``normalize`` per frame and against PIL."""
    t = rigs["torch"]
    w, h = EC.FRAME
    host = [rigs["host"][0], np.full((h, w), 255, np.uint8), rigs["host"][2]]
    stack = dev(np.stack(host))
    assert stack.stride() == (h * w, w, 1)
    border = [e for name, e in NC.eye_sets(w, h) if name in ("corners-down", "corners-up", "wider")] + [
        (1.0, 2.5, 14.0, 4.0), (w - 21.0, h - 6.0, w - 2.0, h - 9.5), (-3.0, h - 2.0, 9.0, h + 1.0), (w - 9.0, -1.0, w + 4.0, 1.5)]
    eyes = np.array(border + border, dtype=np.float64)
    ff = np.array([0] * len(border) + [2] * len(border), dtype=np.int32)
    for size, method in NC.SMALL_OUT_SIZES:
        fn = rigs["norm"](size, method)
        want, status = per_frame_images([stack[0].clone(), stack[1].clone(), stack[2].clone()], eyes, ff, size, method)
        for flags in (0, 1, 2):
            img, st = fn.normalize_frames(stack, eyes, ff, flags=flags)
            got = img.cpu().numpy()
            assert np.array_equal(got, want) and np.array_equal(st, status) and not st.any(), flags
        g = fn.geometry(eyes, EC.FRAME)
        for i in range(len(eyes)):
            assert np.array_equal(want[i], NC.pil_normalize(host[ff[i]], g[i], size)), i
        assert (want == 0).any() and want.any()      # the crops reach over the frame: zeros, never 255s


def test_both_paths_in_one_call_give_the_same_bytes(rigs):
    """(17, 13) areaZ: the "wider" faces are shrunk more than 4 x per axis and go tap by tap beside staged ones; flags 1 / 2 force either
    path on all faces."""
    size, method = (17, 13), NC.AREAZ
    eyes, ff = EC.spread_faces()
    fn = rigs["norm"](size, method)
    g = fn.geometry(eyes, EC.FRAME)
    np_ = g["rect"][:, 2].astype(np.int64) * g["rect"][:, 3]
    limit = 16 * size[0] * size[1]
    assert (np_ > limit).sum() >= 3 and ((np_ > 0) & (np_ <= limit)).sum() >= 10
    want, _ = per_frame_images(rigs["frames"], eyes, ff, size, method)
    for flags in (0, 1, 2):
        assert np.array_equal(fn.normalize_frames(rigs["stack"], eyes, ff, flags=flags)[0].cpu().numpy(), want), flags
        assert np.array_equal(per_frame_images(rigs["frames"], eyes, ff, size, method, flags=flags)[0], want), flags


def test_refused_faces_and_frame_indices_outside_the_stack(rigs):
    """Swapped and NaN eyes and frame indices -1, B and B + 5 between good faces: zero images, status 1 / 2 / 5, the neighbours'
    bytes those of a call without them.  On the stack cut from the larger buffer, and on a stack that IS its allocation."""
    t = rigs["torch"]
    size, method = NC.SMALL_OUT_SIZES[0]
    fn = rigs["norm"](size, method)
    eyes0, ff0 = EC.spread_faces(n_random=3)
    eyes, ff, bad = EC.with_bad_rows(eyes0, ff0, BC.N_FRAMES)
    good = np.array([i not in bad for i in range(len(ff))])
    want0, _ = per_frame_images(rigs["frames"], eyes0, ff0, size, method)
    whole = dev(np.stack(rigs["host"]))      # frame 0 starts the allocation, the last frame ends it
    for stack in (rigs["stack"], whole):
        for flags in (0, 1, 2):
            out = t.full((len(ff), size[1], size[0]), 7, dtype=t.uint8, device="cuda")
            img, st = fn.normalize_frames(stack, eyes, ff, out=out, flags=flags)
            got = img.cpu().numpy()
            assert {i: int(st[i]) for i in bad} == bad and not st[good].any()
            assert not got[~good].any()
            assert np.array_equal(got[good], want0), flags
    one = dev(rigs["host"][1])[None]      # B = 1: index 1 is outside
    img, st = fn.normalize_frames(one, eyes0[:4], np.array([0, 1, 0, -1], dtype=np.int32))
    assert list(st) == [0, 5, 0, 5] and not img[1].any() and not img[3].any()


def test_a_stack_of_one_frame_equals_the_single_frame_entry(rigs):
    size, method = NC.SMALL_OUT_SIZES[1]
    fn = rigs["norm"](size, method)
    eyes = np.array([e for _, e in NC.eye_sets(*EC.FRAME)])
    for f in range(BC.N_FRAMES):
        frame = rigs["stack"][f]
        assert not frame.is_contiguous()
        want, wst = fn.normalize(frame, eyes)
        got, gst = fn.normalize_frames(frame[None], eyes, np.zeros(len(eyes), dtype=np.int32))
        assert np.array_equal(got.cpu().numpy(), want.cpu().numpy()) and np.array_equal(gst, wst)


def test_every_second_frame_and_a_pitched_out(rigs):
    t = rigs["torch"]
    size, method = NC.SMALL_OUT_SIZES[0]
    fn = rigs["norm"](size, method)
    w, h = EC.FRAME
    big = t.full((2 * BC.N_FRAMES, h + 3, w + 37), 255, dtype=t.uint8, device="cuda")
    for f, fr in enumerate(rigs["frames"]):
        big[2 * f, 2:2 + h, 5:5 + w] = fr
    stack = big[::2, 2:2 + h, 5:5 + w]
    assert stack.stride() == (2 * (h + 3) * (w + 37), w + 37, 1)
    eyes, ff = EC.spread_faces(n_random=2)
    want, status = per_frame_images(rigs["frames"], eyes, ff, size, method)
    img, st = fn.normalize_frames(stack, eyes, ff)
    assert np.array_equal(img.cpu().numpy(), want) and np.array_equal(st, status)
    # images farther apart than their size: the gap bytes are untouched
    n, px, gap = len(ff), size[0] * size[1], 13
    buf = t.full((n, px + gap), 0xA5, dtype=t.uint8, device="cuda")
    got, _ = fn.normalize_frames(stack, eyes, ff, out=buf[:, :px].view(n, size[1], size[0]))
    assert got.data_ptr() == buf.data_ptr()
    b = buf.cpu().numpy()
    assert np.array_equal(b[:, :px].reshape(n, size[1], size[0]), want) and np.all(b[:, px:] == 0xA5)


def test_a_frame_stride_above_2_to_the_31(rigs):
    """Two frames 2^31 + 4099 bytes apart in ONE uninitialised allocation of which only the two frames are written: the 64-bit offset."""
    t = rigs["torch"]
    size, method = NC.SMALL_OUT_SIZES[0]
    w, h = EC.FRAME
    stride = (1 << 31) + 4099
    buf = t.empty(stride + h * BC.LD, dtype=t.uint8, device="cuda")
    stack = t.as_strided(buf, (2, h, w), (stride, BC.LD, 1), 0)
    stack[0], stack[1] = rigs["frames"][0], rigs["frames"][2]
    eyes, ff = EC.spread_faces(n_frames=2, n_random=2)
    want, status = per_frame_images([rigs["frames"][0], rigs["frames"][2]], eyes, ff, size, method)
    fn = rigs["norm"](size, method)
    for flags in (0, 2):
        img, st = fn.normalize_frames(stack, eyes, ff, flags=flags)
        assert np.array_equal(img.cpu().numpy(), want) and np.array_equal(st, status), flags
    assert not np.array_equal(want[ff == 0], want[ff == 1])
    del stack, buf
    t.cuda.empty_cache()


def test_more_than_65535_faces(rigs):
    """65573 faces with a 2 x 2 output: the face loop over gridDim.y with a frame per face."""
    size, method = (2, 2), NC.AREA
    base = np.concatenate([NC.random_eyes(700, EC.FRAME, seed=s) for s in (21, 22)])
    n = 65536 + 37
    eyes = base[np.arange(n) % len(base)]
    ff = ((np.arange(n) * 7 + np.arange(n) // 5) % BC.N_FRAMES).astype(np.int32)
    ff[[100, 65535, 65536, n - 1]] = [-1, 3, 0, 2]
    want, status = per_frame_images(rigs["frames"], eyes, ff, size, method)
    img, st = rigs["norm"](size, method).normalize_frames(rigs["stack"], eyes, ff)
    got = img.cpu().numpy()
    assert np.array_equal(st, status) and list(st[[100, 65535]]) == [5, 5]
    assert np.array_equal(got, want), np.flatnonzero((got != want).any(axis=(1, 2)))[:10]
    assert want[65536:].any() and want.reshape(n, -1).any(axis=1).sum() > n // 10


def test_workspace_growth_and_reuse(rigs):
    """A small call, a larger one and a small one again through ONE long-lived normalizer, a single-frame call between them, each against
    normalizers created per frame."""
    size, method = NC.SMALL_OUT_SIZES[0]
    one = normalizer(size, method)
    eyes, ff = EC.spread_faces(n_random=40)
    for n in (3, len(ff), 3):
        for flags in (0, 1):
            want, status = per_frame_images(rigs["frames"], eyes[:n], ff[:n], size, method)
            img, st = one.normalize_frames(rigs["stack"], eyes[:n], ff[:n], flags=flags)
            assert np.array_equal(img.cpu().numpy(), want) and np.array_equal(st, status), (n, flags)
        idx = np.flatnonzero(ff[:n] == ff[0])
        single = one.normalize(rigs["stack"][int(ff[0])], eyes[:n][idx])[0].cpu().numpy()
        assert np.array_equal(single, want[idx])
    rigs["torch"].cuda.synchronize()
    one.close()


# ---- estimate ------------------------------------------------------------------------------------------------------------------------
def merge_per_frame(results, ff):
    """The per-frame dicts of ``estimate`` (results[f]: the faces with ff == f, in their order) as one dict in face order.  A face whose
    frame is outside the list has status 5, NaN values, ``None`` labels and zero intermediates."""
    n, out = len(ff), {}
    for f, res in enumerate(results):
        idx = np.flatnonzero(ff == f)
        for k, v in res.items():
            if isinstance(v, list):
                col = out.setdefault(k, [None] * n)
                for i, x in zip(idx, v):
                    col[i] = x
            else:
                fill = np.nan if v.dtype.kind == "f" and v.ndim == 1 else 0
                out.setdefault(k, np.full((n,) + v.shape[1:], fill, dtype=v.dtype))[idx] = v
    out["status"][(ff < 0) | (ff >= len(results))] = EC.STATUS_FRAME_RANGE
    return out


class EstRig(object):
    """The small analyzers of tests/analysis_cases.py: a 40 x 44 crop, a 13 x 11 patch, patch_flow's linear node, three synthetic
    classifiers scattered over the features of the stack's own faces."""

    def __init__(self, torch):
        from pyfaceanalysis_amd.flow import Flow
        self.torch = torch
        self.flow = Flow(AC.patch_flow(EC.PATCH), output_dtype=np.float32)
        self.host = EC.est_frames()
        self.frames = [dev(h) for h in self.host]
        self.stack = torch.stack(self.frames)
        self.eyes, self.ff = EC.est_faces()
        self.made, self.clfs = [], None
        probe_clf = AC.synthetic_classifier(5, np.zeros((2, 5)), 5, AC.GENDER_LABELS)
        probe = A.FaceAnalyzer(self.flow, gender=probe_clf, contrast=AC.CONTRAST, patch_size=EC.PATCH, box=EC.PATCH_BOX, crop_size=AC.SMALL_CROP)
        feats = probe.estimate(self.frames[0], NC.random_eyes(40, EC.EST_FRAME, seed=3), return_intermediates=True)["features"]
        torch.cuda.synchronize()
        probe.close()
        probe_clf.close()
        self.clfs = AC.classifiers(feats, (4, 5, 5))

    def analyzer(self, age=True, race=True, gender=True, **kw):
        c = [clf if on else None for clf, on in zip(self.clfs, (age, race, gender))]
        fa = A.FaceAnalyzer(self.flow, *c, **dict(dict(contrast=AC.CONTRAST, patch_size=EC.PATCH, box=EC.PATCH_BOX, crop_size=AC.SMALL_CROP), **kw))
        self.made.append(fa)
        return fa

    def per_frame(self, frames, eyes, ff, intermediates=True, flags=0, **kw):
        """``estimate`` per frame on that frame's faces through an analyzer created for that frame, scattered back into face order."""
        results = []
        for f, frame in enumerate(frames):
            fa = self.analyzer(**kw)
            results.append(fa.estimate(frame, eyes[ff == f], return_intermediates=intermediates, flags=flags))      # (waits for the device)
            self.made.remove(fa)
            fa.close()
        return merge_per_frame(results, ff)

    def close(self):
        self.torch.cuda.synchronize()
        for fa in self.made:
            fa.close()
        for c in self.clfs:
            c.close()
        self.flow.close()


@pytest.fixture(scope="module")
def est(native_lib):
    import torch
    r = EstRig(torch)
    yield r
    r.close()


def assert_same(got, want, keys, what=None, rows=None):
    for k in keys:
        g, w = got[k], want[k]
        if rows is not None:
            g, w = ([g[i] for i in rows], [w[i] for i in rows]) if isinstance(g, list) else (g[rows], w[rows])
        assert (g == w) if isinstance(g, list) else AC.same(g, w), (what, k, g, w)


@pytest.mark.parametrize("clip,targets", ((True, AC.CONTRAST_STEEP), (False, AC.CONTRAST_UNCLIPPED)), ids=("clipped", "unclipped"))
@pytest.mark.parametrize("filt", sorted(AC.FILTERS))
def test_estimate_frames_equals_estimate_per_frame(est, filt, clip, targets):
    """Four 200 x 150 frames with 0, 1, 3 and 5 faces, interleaved: every value key, the status, labels and confidences, the patches and
    the features — on the default patch path, the composed one and the fused kernel."""
    kw = dict(interpolation=filt, clip=clip, contrast=targets, box=EC.PATCH_BOX_OVER if filt == "BILINEAR" else EC.PATCH_BOX)
    keys = ALL_KEYS + ("patches", "features")
    want = est.per_frame(est.frames, est.eyes, est.ff, **kw)
    assert list(want["status"]) == [0] * 9 and len({float(v) for v in want["age"]}) >= 5 and len({p.tobytes() for p in want["patches"]}) == 9
    fa = est.analyzer(**kw)
    for flags in (0, A.FLAG_COMPOSED, A.FLAG_FUSED):
        got = fa.estimate_frames(est.stack, est.eyes, est.ff, return_intermediates=True, flags=flags)
        assert sorted(got) == sorted(keys)
        assert_same(got, want, keys, (filt, clip, flags))
        assert_same(est.per_frame(est.frames, est.eyes, est.ff, flags=flags, **kw), want, keys, (filt, clip, flags, "per frame"))
    plain = fa.estimate_frames(est.stack, est.eyes, est.ff)
    assert "patches" not in plain and "features" not in plain
    assert_same(plain, want, ALL_KEYS)
    g = fa._norm.geometry(est.eyes, EC.EST_FRAME)
    assert_same(fa.estimate_frames(list(est.frames), geoms=g, face_frame=est.ff), want, ALL_KEYS)


def test_refused_and_outside_faces_leave_the_others_alone(est):
    eyes, ff, bad = EC.with_bad_rows(np.concatenate([est.eyes, est.eyes]), np.concatenate([est.ff, est.ff[::-1]]), 4)
    good = np.array([i not in bad for i in range(len(ff))])
    fa = est.analyzer()
    got = fa.estimate_frames(est.stack, eyes, ff, return_intermediates=True)
    assert {i: int(got["status"][i]) for i in bad} == bad and not got["status"][good].any()
    for k in VALUE_KEYS + ("race_confidence", "gender_confidence"):
        assert np.isnan(got[k][~good]).all() and np.isfinite(got[k][good]).all(), k
    assert all(got[k][i] is None for i in bad for k in ("race_label", "gender_label")) and None not in [got["race_label"][i] for i in np.flatnonzero(good)]
    alone = fa.estimate_frames(est.stack, eyes[good], ff[good], return_intermediates=True)
    keys = ALL_KEYS + ("patches", "features")
    assert_same(got, _scatter(alone, good), keys, "neighbours", rows=np.flatnonzero(good))
    want = est.per_frame(est.frames, eyes, ff)
    assert_same(got, want, ALL_KEYS, "per frame")
    assert_same(got, want, ("patches", "features"), "per frame", rows=np.flatnonzero(good))


def _scatter(res, mask):
    """The rows of ``res`` put where ``mask`` is True (other rows: None / zeros)."""
    idx, n = np.flatnonzero(mask), len(mask)
    out = {}
    for k, v in res.items():
        if isinstance(v, list):
            out[k] = [None] * n
            for i, x in zip(idx, v):
                out[k][i] = x
        else:
            out[k] = np.zeros((n,) + v.shape[1:], dtype=v.dtype)
            out[k][idx] = v
    return out


def raw_block(est, fa, eyes, ff, fill=-3.0):
    """hg_estimator_estimate_frames_device itself: the (4, n) block in rows one element farther apart than n."""
    t = est.torch
    g = fa._norm.geometry(eyes, EC.EST_FRAME)
    n = len(g)
    out = t.full((4, n + 1), fill, dtype=t.float64, device="cuda")
    b, h, w, ld, stride = N.stack_layout(est.stack)
    ffc = np.ascontiguousarray(ff, dtype=np.int32)
    _capi.check(_capi.lib().hg_estimator_estimate_frames_device(fa._handle(), 0, est.stack.data_ptr(), b, stride, h, w, ld, g.ctypes.data_as(C.c_void_p),
                                                                ffc.ctypes.data_as(C.c_void_p), n, out.data_ptr(), n + 1, None, None,
                                                                t.cuda.current_stream().cuda_stream))
    blk = out.cpu().numpy()
    assert np.all(blk[:, n] == fill)
    return blk[:, :n]


def test_absent_classifiers_keep_the_initial_values(est):
    want = est.per_frame(est.frames, est.eyes, est.ff, intermediates=False)
    only_gender = est.analyzer(age=False, race=False, n_features=5)
    got = only_gender.estimate_frames(est.stack, est.eyes, est.ff)
    assert sorted(got) == ["gender", "gender_confidence", "gender_label", "status"] and AC.same(got["gender"], want["gender"])
    b = raw_block(est, only_gender, est.eyes, est.ff)
    assert np.all(b[0] == 0.0) and np.all(b[1] == 0.0) and np.all(b[2] == 10.0) and AC.same(b[3], want["gender"])
    only_age = est.analyzer(race=False, gender=False, n_features=5)
    b = raw_block(est, only_age, est.eyes, est.ff)
    assert AC.same(b[0], want["age"]) and AC.same(b[1], want["age_std"]) and np.all(b[2] == 10.0) and np.all(b[3] == 10.0)
    only_race = est.analyzer(age=False, gender=False, n_features=5)
    ff = est.ff.copy()
    ff[3] = 4      # outside the stack: NaN in the rows of absent classifiers too
    b = raw_block(est, only_race, est.eyes, ff)
    keep = np.arange(len(ff)) != 3
    assert np.isnan(b[:, 3]).all() and np.all(b[0, keep] == 0.0) and np.all(b[1, keep] == 0.0) and AC.same(b[2, keep], want["race"][keep]) and np.all(b[3, keep] == 10.0)


def test_permuting_the_frames_permutes_nothing_in_the_results(est):
    fa = est.analyzer()
    keys = ALL_KEYS + ("patches", "features")
    want = fa.estimate_frames(est.stack, est.eyes, est.ff, return_intermediates=True)
    perm = np.array([2, 0, 3, 1])                    # new frame j is old frame perm[j]
    where = np.argsort(perm)                         # old frame f is new frame where[f]
    got = fa.estimate_frames(est.stack[est.torch.from_numpy(perm).cuda()], est.eyes, where[est.ff].astype(np.int32), return_intermediates=True)
    assert_same(got, want, keys)
    assert_same(want, est.per_frame(est.frames, est.eyes, est.ff), keys)


def test_the_reference_shape_once(est):
    """linearPCANetworkU11L on 96 x 96 patches of 256 x 260 crops, the default box: five faces on two 320 x 240 frames."""
    from pyfaceanalysis_amd.flow import Flow
    from tests import helpers
    t = est.torch
    flow = Flow(helpers.linear_u11l_96(0), output_dtype=np.float32)
    frames = [dev(NC.noise_frame(320, 240, seed=s)) for s in (0, 5)]
    eyes = AC.frame_eyes(320, 240)[[0, 1, 5, 2, 4]]
    ff = np.array([1, 0, 1, 0, 0], dtype=np.int32)
    clf0 = AC.synthetic_classifier(5, np.zeros((2, 8)), 8, AC.GENDER_LABELS)
    probe = A.FaceAnalyzer(flow, gender=clf0, contrast=AC.CONTRAST, n_features=30)
    feats = probe.estimate(frames[0], AC.frame_eyes(320, 240), return_intermediates=True)["features"]
    clfs = AC.classifiers(feats, (30, 12, 8), seed=21)
    keys = ALL_KEYS + ("patches", "features")
    made = [probe]
    results = []
    for f, frame in enumerate(frames):
        fa = A.FaceAnalyzer(flow, *clfs, contrast=AC.CONTRAST)
        made.append(fa)
        results.append(fa.estimate(frame, eyes[ff == f], return_intermediates=True))
    want = merge_per_frame(results, ff)
    fa = A.FaceAnalyzer(flow, *clfs, contrast=AC.CONTRAST)
    made.append(fa)
    assert fa.patch_size == (96, 96) and fa.crop_size == (256, 260) and fa.k == 30
    for flags in (0, A.FLAG_COMPOSED, A.FLAG_FUSED):
        assert_same(fa.estimate_frames(t.stack(frames), eyes, ff, return_intermediates=True, flags=flags), want, keys, flags)
    assert want["patches"].shape == (5, 9216) and np.isfinite(want["age"]).all()
    t.cuda.synchronize()
    for x in made:
        x.close()
    for c in clfs + (clf0,):
        c.close()
    flow.close()


# ---- end to end ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rig(native_lib, nets):
    from tests import test_frame_stream_gpu as FS
    r = FS.Rig(nets, keep=BC.KEEP, later_keep=BC.LATER_KEEP)
    yield r
    r.close()


def assert_dicts_equal(got, want, what):
    assert sorted(got) == sorted(want), what
    for k in want:
        assert (got[k] == want[k]) if isinstance(want[k], list) else AC.same(got[k], want[k]), (what, k, got[k], want[k])


def end_to_end(est, dc, loc, fdev, what, min_faces, need_empty=False):
    """detect_faces_frames -> prescale_frames -> estimate_faces_frames against detect_faces -> prescale -> estimate_faces per frame."""
    from tests import test_frame_stream_gpu as FS
    t = est.torch
    stack = t.stack(fdev)
    want = []
    for f in fdev:
        faces = dc.detect_faces(f, loc, smallest_face=FS.SF)["faces"]
        small = dc.prescale(f)
        fa = est.analyzer()
        want.append((faces, small.cpu().numpy(), fa.estimate_faces(small, faces, return_intermediates=True)))
    n = [len(w[0]) for w in want]
    assert sum(n) >= min_faces and (not need_empty or (0 in n and n[-1] > 0)), (what, n)
    pooled = dc.detect_faces_frames(stack, loc, smallest_face=FS.SF)["faces"]
    assert all(np.array_equal(p, w[0]) for p, w in zip(pooled, want)), what
    smalls = dc.prescale_frames(stack)
    assert smalls.dim() == 3 and smalls.dtype == t.uint8 and all(np.array_equal(smalls[f].cpu().numpy(), w[1]) for f, w in enumerate(want)), what
    got = est.analyzer().estimate_faces_frames(smalls, pooled, return_intermediates=True)
    assert len(got) == len(want)
    for f, (g, w) in enumerate(zip(got, want)):
        assert_dicts_equal(g, w[2], (what, f))
    return smalls


def test_end_to_end_on_a_grey_stack_without_prescale(est, rig):
    """B = 3 of 97 x 131 (BC.SMALL_SEEDS: a frame without a survivor between two that have some) and B = 3 of 320 x 240
    (BC.MEDIUM_SEEDS, 25 / 23 / 31 faces) with an empty frame added."""
    dc, loc, close = rig.fresh()
    try:
        fdev = [dev(BC.noise_frame(BC.SMALL[0], BC.SMALL[1], s)) for s in BC.SMALL_SEEDS]
        smalls = end_to_end(est, dc, loc, fdev, "small", 1, need_empty=True)
        assert tuple(smalls.shape) == (3, BC.SMALL[1], BC.SMALL[0])
        fdev = [dev(BC.noise_frame(BC.MEDIUM[0], BC.MEDIUM[1], s)) for s in BC.MEDIUM_SEEDS[:2]] + [dev(np.full((BC.MEDIUM[1], BC.MEDIUM[0]), 128, np.uint8))]
        stack = est.torch.stack(fdev)
        assert dc.prescale_frames(stack) is stack      # a grey stack that needs no shrinking is returned as it is
        end_to_end(est, dc, loc, fdev, "medium", 40)
    finally:
        close()


def test_end_to_end_on_an_rgb_stack_behind_a_bilinear_prescale(est, rig):
    """Two 1280 x 720 RGB frames (BC.HD_SEEDS; 1 and 2 faces) and a constant one, prescale_filter = "BILINEAR"."""
    from pyfaceanalysis_amd.cascade import DeviceCascade
    from tests import test_frame_stream_gpu as FS
    noise = [BC.hd_frame(s) for s in BC.HD_SEEDS] + [np.full((BC.HD[1], BC.HD[0]), 90, np.uint8)]
    rgb = [dev(np.stack([n, n, 255 - n], axis=2)) for n in noise]
    dc = DeviceCascade(rig.stages, FS.SUB, FS.K, rig.pipe, frame_format="RGB", prescale_filter="BILINEAR")
    try:
        smalls = end_to_end(est, dc, rig.loc, rgb, "rgb", 2)
        assert tuple(smalls.shape) == (3, 562, 1000)
    finally:
        dc.close()


@pytest.mark.parametrize("fmt", ("L", "RGB"))
@pytest.mark.parametrize("filt", ("NEAREST", "LANCZOS"))
def test_prescale_frames_equals_prescale_per_frame(rig, fmt, filt):
    """Grey and RGB stacks, the NEAREST gather and an antialiased filter, shrunk (640 x 480 -> 300 x 225) and not (a colour stack is
    converted whole); a strided stack; the same tensor again on the next call with the same key."""
    import torch
    from pyfaceanalysis_amd.cascade import DeviceCascade
    from tests import test_frame_stream_gpu as FS
    w, h = 640, 480
    noise = [BC.noise_frame(w, h, 9400 + i) for i in range(3)]
    host = noise if fmt == "L" else [np.ascontiguousarray(np.stack([n, 255 - n, n[::-1]], axis=2)) for n in noise]
    dc = DeviceCascade(rig.stages, FS.SUB, FS.K, rig.pipe, frame_format=fmt, prescale_filter=filt)
    ref = DeviceCascade(rig.stages, FS.SUB, FS.K, rig.pipe, frame_format=fmt, prescale_filter=filt)
    try:
        fdev = [dev(x) for x in host]
        big = torch.full((6,) + tuple(fdev[0].shape), 255, dtype=torch.uint8, device="cuda")
        big[::2] = torch.stack(fdev)
        for size in (300, 1000):
            want = [ref.prescale(f, size).cpu().numpy().copy() for f in fdev]
            for stack in (torch.stack(fdev), big[::2], fdev):
                got = dc.prescale_frames(stack, prescale_size=size)
                assert tuple(got.shape) == (3,) + want[0].shape and got.dtype == torch.uint8
                assert all(np.array_equal(got[f].cpu().numpy(), want[f]) for f in range(3)), (fmt, filt, size)
            if size == 300:
                assert want[0].shape == (225, 300) and dc.prescale_frames(torch.stack(fdev), prescale_size=size).data_ptr() == got.data_ptr()
            elif fmt == "L":
                st = torch.stack(fdev)
                assert dc.prescale_frames(st, prescale_size=size) is st
    finally:
        torch.cuda.synchronize()
        dc.close()
        ref.close()
