"""GPU: age, race and gender estimation on the device (pyfaceanalysis_amd/analysis.py, csrc/hg_estimate.hip).  The patch step against PIL's
own ``transform`` followed by the restated contrast (tests/analysis_cases.py), the whole chain against the composed public calls
(FaceNormalizer.normalize -> that oracle -> flow.execute -> regression), every comparison ``array_equal`` with NaNs by position."""
import ctypes as C

import numpy as np
import pytest

from pyfaceanalysis_amd import _capi, analysis as A, normalize as N
from tests import analysis_cases as AC, helpers, normalize_cases as NC
from tests.test_eyes_gpu import setup      # noqa: F401  (the synthetic frame, cascade and eye locator, built as that module builds them)

VALUE_KEYS = ("age", "age_std", "race", "gender")
FRAME = (200, 150)


@pytest.fixture(scope="module")
def dev(native_lib):
    """The small rig: the 8 x 8 linear net, a 200 x 150 frame, the "age" normaliser, three classifiers of input dims 4, 5, 5 scattered over
    the features of the frame's own faces, and the composed chain's result on the six eye pairs — computed once."""
    import torch
    from pyfaceanalysis_amd.flow import Flow
    flow = Flow(helpers.linear_net(0), output_dtype=np.float32)
    host = NC.noise_frame(*FRAME)
    frame = torch.from_numpy(host).cuda()
    norm = N.FaceNormalizer(0, preset="age")
    eyes = AC.frame_eyes(*FRAME)
    box = A.age_patch_box((256, 260), (8, 8))
    chain = lambda e, clfs, filt=0, clip=True, fr=None: AC.composed_chain(frame if fr is None else fr, e, norm, flow, clfs, (8, 8), box, filt, AC.CONTRAST, clip, 5)
    feats = chain(NC.random_eyes(40, FRAME, seed=3), (None, None, None))["features"]
    clfs = AC.classifiers(feats, (4, 5, 5))
    d = dict(torch=torch, flow=flow, host=host, frame=frame, norm=norm, eyes=eyes, box=box, chain=chain, clfs=clfs, want=chain(eyes, clfs), made=[])

    def analyzer(age=clfs[0], race=clfs[1], gender=clfs[2], **kw):
        fa = A.FaceAnalyzer(flow, age, race, gender, **dict(dict(contrast=AC.CONTRAST, patch_size=(8, 8)), **kw))
        d["made"].append(fa)
        return fa
    d["analyzer"] = analyzer
    yield d
    torch.cuda.synchronize()
    for fa in d["made"]:
        fa.close()
    for c in clfs:
        c.close()
    norm.close()
    flow.close()


def assert_same(got, want, keys):
    for k in keys:
        assert AC.same(got[k], want[k]), (k, got[k], want[k])


def patch_analyzer(made, torch, crop_size, patch_size, box, filt, clip, targets):
    from pyfaceanalysis_amd.flow import Flow
    flow = Flow(AC.patch_flow(patch_size), output_dtype=np.float32)
    clf = AC.synthetic_classifier(5, np.zeros((2, 5)), 5, AC.GENDER_LABELS)
    fa = A.FaceAnalyzer(flow, gender=clf, contrast=targets, clip=clip, patch_size=patch_size, box=box, interpolation=filt, crop_size=crop_size)
    made.append((fa, flow, clf))
    return fa


@pytest.fixture(scope="module")
def made(native_lib):
    import torch
    lst = []
    yield lst
    torch.cuda.synchronize()
    for fa, flow, clf in lst:
        fa.close()
        clf.close()
        flow.close()


def strided(torch, crops, gap=13):
    """The crops as a device tensor whose images are farther apart than their size."""
    n, h, w = crops.shape
    buf = torch.full((n, h * w + gap), 0x5A, dtype=torch.uint8, device="cuda")
    buf[:, :h * w] = torch.from_numpy(crops.reshape(n, -1)).cuda()
    return buf[:, :h * w].view(n, h, w)


@pytest.mark.gpu
@pytest.mark.parametrize("filt", sorted(AC.FILTERS))
@pytest.mark.parametrize("case", AC.PATCH_CASES, ids=[c[0] for c in AC.PATCH_CASES])
def test_patches_equal_pil_and_the_restated_contrast(made, case, filt):
    import torch
    name, crop_size, patch_size, box = case
    box = A.age_patch_box(crop_size, patch_size) if box is None else box
    npix = patch_size[0] * patch_size[1]
    crops = AC.noise_crops(70, crop_size)
    crops[5] = 0                    # a refused face's crop
    cut = AC.pil_cut(crops, patch_size, box, AC.FILTERS[filt])
    assert cut.any() and (name.find("over") < 0 or not cut[0].all())
    dense, far = torch.from_numpy(crops).cuda(), strided(torch, crops)
    assert far.stride(0) > crop_size[0] * crop_size[1]
    for clip, targets in ((True, AC.CONTRAST_STEEP), (False, AC.CONTRAST_UNCLIPPED)):
        want = AC.contrast(cut, targets[0], targets[1], clip)
        fa = patch_analyzer(made, torch, crop_size, patch_size, box, filt, clip, targets)
        for flags in (0, A.FLAG_COMPOSED, A.FLAG_FUSED):
            for n in (1, 3, 70):
                assert AC.same(fa.patches(dense[:n], flags=flags).cpu().numpy(), want[:n]), (name, filt, clip, flags, n)
            assert AC.same(fa.patches(far, flags=flags).cpu().numpy(), want), (name, filt, clip, flags, "crop_stride")
            buf = torch.full((70, npix + 7), -7.0, dtype=torch.float32, device="cuda")      # ldp > the row length: the gap is untouched
            got = fa.patches(dense, out=buf[:, :npix], flags=flags)
            assert got.data_ptr() == buf.data_ptr()
            b = buf.cpu().numpy()
            assert AC.same(np.ascontiguousarray(b[:, :npix]), want) and np.all(b[:, npix:] == -7.0), (name, filt, clip, flags, "ldp")
        assert tuple(fa.patches(dense[:0]).shape) == (0, npix)
    steep = AC.contrast(cut, *AC.CONTRAST_STEEP, clip=False)
    assert (steep < 0).any() or (steep > 255).any()       # the clip switch has something to switch


@pytest.mark.gpu
@pytest.mark.parametrize("filt", sorted(AC.FILTERS))
def test_a_patch_above_the_lds_cap_takes_the_composed_path(made, filt):
    import torch
    name, crop_size, patch_size, box = AC.ABOVE_THE_CAP
    assert patch_size[0] * patch_size[1] > 16384
    crops = AC.noise_crops(3, crop_size, seed=1)
    want = AC.patch_oracle(crops, patch_size, box, AC.FILTERS[filt], AC.CONTRAST, True)
    fa = patch_analyzer(made, torch, crop_size, patch_size, box, filt, True, AC.CONTRAST)
    dense = torch.from_numpy(crops).cuda()
    assert AC.same(fa.patches(dense).cpu().numpy(), want)
    assert AC.same(fa.patches(dense, flags=A.FLAG_COMPOSED).cpu().numpy(), want)
    with pytest.raises(ValueError, match="16384"):
        fa.patches(dense, flags=A.FLAG_FUSED)
    for flags in (3, 4, -1):
        with pytest.raises(ValueError, match="flags"):
            fa.patches(dense, flags=flags)


@pytest.mark.gpu
@pytest.mark.parametrize("filt", sorted(AC.FILTERS))
def test_a_constant_crop_becomes_the_target_mean(made, filt):
    import torch
    crops = np.full((2, 44, 40), 200, dtype=np.uint8)
    crops[1] = 0
    dense = torch.from_numpy(crops).cuda()
    inside, over = AC.PATCH_CASES[0][3], AC.PATCH_CASES[2][3]
    for clip, targets in ((True, AC.CONTRAST), (False, AC.CONTRAST_UNCLIPPED)):
        fa = patch_analyzer(made, torch, AC.SMALL_CROP, (8, 8), inside, filt, clip, targets)
        for flags in (0, A.FLAG_COMPOSED, A.FLAG_FUSED):
            got = fa.patches(dense, flags=flags).cpu().numpy()
            assert got.dtype == np.float32 and np.all(got == np.float32(targets[0])), (filt, clip, flags)
    # the same crop under a box that hangs over two edges: the zeros outside count in the statistics, the patch is not constant
    fa = patch_analyzer(made, torch, AC.SMALL_CROP, (13, 11), over, filt, True, AC.CONTRAST)
    want = AC.patch_oracle(crops, (13, 11), over, AC.FILTERS[filt], AC.CONTRAST, True)
    assert len(np.unique(want[0])) > 1 and np.all(want[1] == 128.0)
    for flags in (0, A.FLAG_COMPOSED, A.FLAG_FUSED):
        assert AC.same(fa.patches(dense, flags=flags).cpu().numpy(), want)


@pytest.mark.gpu
def test_chain_equals_the_composed_public_calls(dev):
    t = dev["torch"]
    want = dev["want"]
    assert list(want["status"]) == [0] * 6 and want["patches"].shape == (6, 64) and want["features"].shape == (6, 5)
    assert not want["crops"][4].all() and not want["crops"][5].all()      # the border faces' crops reach outside the frame
    assert len({float(v) for v in want["age"]}) > 1
    fa = dev["analyzer"]()
    assert fa.k == 5
    keys = VALUE_KEYS + ("status", "patches", "features")
    for flags in (0, A.FLAG_COMPOSED, A.FLAG_FUSED):
        got = fa.estimate(dev["frame"], dev["eyes"], return_intermediates=True, flags=flags)
        assert_same(got, want, keys)
        assert AC.same(got["race_confidence"], np.abs(want["race"]) / 2.0) and AC.same(got["gender_confidence"], np.abs(want["gender"]))
        assert got["race_label"] == A.race_strings(want["race"]) and got["gender_label"] == A.gender_strings(want["gender"])
    plain = fa.estimate(dev["frame"], dev["eyes"])
    assert "patches" not in plain and "features" not in plain
    assert_same(plain, want, VALUE_KEYS)
    assert_same(fa.estimate(dev["frame"], geoms=dev["norm"].geometry(dev["eyes"], FRAME)), want, VALUE_KEYS)
    # a pitched frame, and a crop view of a larger frame
    w, h = FRAME
    pitched = t.zeros((h, w + 11), dtype=t.uint8, device="cuda")[:, :w]
    larger = t.full((h + 9, w + 17), 255, dtype=t.uint8, device="cuda")[4:4 + h, 6:6 + w]
    for view in (pitched, larger):
        view.copy_(dev["frame"])
        assert not view.is_contiguous()
        assert_same(fa.estimate(view, dev["eyes"], return_intermediates=True), want, keys)
    # the other filters and the unclipped contrast, against the chain with the same choices
    for filt, clip in (("BILINEAR", True), ("BICUBIC", False)):
        fb = dev["analyzer"](interpolation=filt, clip=clip)
        wb = dev["chain"](dev["eyes"], dev["clfs"], AC.FILTERS[filt], clip)
        assert not AC.same(wb["patches"], want["patches"])
        for flags in (0, A.FLAG_COMPOSED):
            assert_same(fb.estimate(dev["frame"], dev["eyes"], return_intermediates=True, flags=flags), wb, keys)


@pytest.mark.gpu
def test_a_refused_face_in_the_middle_leaves_its_neighbours_alone(dev):
    e = dev["eyes"]
    swapped = (e[1, 2], e[1, 3], e[1, 0], e[1, 1])
    eyes = np.array([e[0], swapped, e[2], (7.0, 7.0, 7.0, 7.0), e[4]])
    fa = dev["analyzer"]()
    got = fa.estimate(dev["frame"], eyes, return_intermediates=True)
    assert list(got["status"]) == [0, 1, 0, 3, 0]
    for k in VALUE_KEYS + ("race_confidence", "gender_confidence"):
        assert np.isnan(got[k][[1, 3]]).all() and np.isfinite(got[k][[0, 2, 4]]).all(), k
    assert got["race_label"][1] is None and got["gender_label"][3] is None and None not in [got["race_label"][i] for i in (0, 2, 4)]
    alone = fa.estimate(dev["frame"], eyes[[0, 2, 4]], return_intermediates=True)
    for k in VALUE_KEYS + ("patches", "features"):
        assert AC.same(got[k][[0, 2, 4]], alone[k]), k
    assert_same(alone, {k: dev["want"][k][[0, 2, 4]] for k in VALUE_KEYS}, VALUE_KEYS)
    assert_same(got, dev["chain"](eyes, dev["clfs"]), VALUE_KEYS + ("status",))
    none = fa.estimate(dev["frame"], np.zeros((0, 4)), return_intermediates=True)
    for k in VALUE_KEYS + ("race_confidence", "gender_confidence"):
        assert none[k].shape == (0,) and none[k].dtype == np.float64
    assert none["status"].shape == (0,) and none["race_label"] == [] and none["patches"].shape == (0, 64) and none["features"].shape == (0, 5)


def raw_block(torch, fa, frame, eyes, fill=-3.0):
    """hg_estimator_estimate_device itself: the (4, n) block in rows one element farther apart than n."""
    g = fa._norm.geometry(eyes, (frame.shape[1], frame.shape[0]))
    n = len(g)
    out = torch.full((4, n + 1), fill, dtype=torch.float64, device="cuda")
    _capi.check(_capi.lib().hg_estimator_estimate_device(fa._handle(), 0, frame.data_ptr(), frame.shape[0], frame.shape[1], frame.stride(0), g.ctypes.data_as(C.c_void_p),
                                                         n, out.data_ptr(), n + 1, None, None, torch.cuda.current_stream().cuda_stream))
    b = out.cpu().numpy()
    assert np.all(b[:, n] == fill)
    return b[:, :n]


@pytest.mark.gpu
def test_absent_classifiers_keep_the_initial_values(dev):
    t, want, clfs = dev["torch"], dev["want"], dev["clfs"]
    only_gender = dev["analyzer"](age=None, race=None, n_features=5)
    got = only_gender.estimate(dev["frame"], dev["eyes"])
    assert sorted(got) == ["gender", "gender_confidence", "gender_label", "status"]
    assert AC.same(got["gender"], want["gender"])
    b = raw_block(t, only_gender, dev["frame"], dev["eyes"])
    assert np.all(b[0] == 0.0) and np.all(b[1] == 0.0) and np.all(b[2] == 10.0) and AC.same(b[3], want["gender"])
    only_age = dev["analyzer"](race=None, gender=None, n_features=5)
    got = only_age.estimate(dev["frame"], dev["eyes"])
    assert sorted(got) == ["age", "age_std", "status"]
    assert AC.same(got["age"], want["age"]) and AC.same(got["age_std"], want["age_std"])
    b = raw_block(t, only_age, dev["frame"], dev["eyes"])
    assert AC.same(b[0], want["age"]) and AC.same(b[1], want["age_std"]) and np.all(b[2] == 10.0) and np.all(b[3] == 10.0)
    only_race = dev["analyzer"](age=None, gender=None, n_features=5)
    b = raw_block(t, only_race, dev["frame"], dev["eyes"])
    assert np.all(b[0] == 0.0) and np.all(b[1] == 0.0) and AC.same(b[2], want["race"]) and np.all(b[3] == 10.0)
    # a refused face is NaN in the rows of absent classifiers too
    eyes = np.array([dev["eyes"][0], (7.0, 7.0, 7.0, 7.0)])
    b = raw_block(t, only_gender, dev["frame"], eyes)
    assert np.isnan(b[:, 1]).all() and list(b[:3, 0]) == [0.0, 0.0, 10.0] and b[3, 0] == want["gender"][0]
    assert only_age.k == 5 and dev["analyzer"](race=None, gender=None).k == 4      # n_features defaults to the widest classifier given


@pytest.mark.gpu
def test_the_reference_shape_once(dev):
    """linearPCANetworkU11L on 96 x 96 patches of 256 x 260 crops, the default box: three faces on a 320 x 240 frame."""
    t = dev["torch"]
    from pyfaceanalysis_amd.flow import Flow
    flow = Flow(helpers.linear_u11l_96(0), output_dtype=np.float32)
    host = NC.noise_frame(320, 240)
    frame = t.from_numpy(host).cuda()
    eyes = AC.frame_eyes(320, 240)[[0, 1, 5]]
    box = A.age_patch_box()
    feats = AC.composed_chain(frame, AC.frame_eyes(320, 240), dev["norm"], flow, (None, None, None), (96, 96), box, 0, AC.CONTRAST, True, 30)["features"]
    clfs = AC.classifiers(feats, (30, 12, 8), seed=21)
    want = AC.composed_chain(frame, eyes, dev["norm"], flow, clfs, (96, 96), box, 0, AC.CONTRAST, True, 30)
    fa = A.FaceAnalyzer(flow, *clfs, contrast=AC.CONTRAST)
    assert fa.box == box and fa.patch_size == (96, 96) and fa.crop_size == (256, 260) and fa.k == 30
    keys = VALUE_KEYS + ("status", "patches", "features")
    for flags in (0, A.FLAG_COMPOSED, A.FLAG_FUSED):
        assert_same(fa.estimate(frame, eyes, return_intermediates=True, flags=flags), want, keys)
    assert want["patches"].shape == (3, 9216) and np.isfinite(want["age"]).all()
    t.cuda.synchronize()
    fa.close()
    for c in clfs:
        c.close()
    flow.close()


@pytest.mark.gpu
def test_estimate_faces_on_detector_rows(setup, dev):      # noqa: F811
    """detect_faces rows -> estimate_faces on the prescaled frame the rows refer to."""
    from pyfaceanalysis_amd.flow import Flow
    s = setup
    faces = s["dc"].detect_faces(s["fdev"], s["loc"], smallest_face=0.1)["faces"]
    assert len(faces) > 0
    small = s["dc"].prescale(s["fdev"])
    flow = Flow(helpers.linear_u11l_96(0), output_dtype=np.float32)
    box = A.age_patch_box()
    chain = lambda clfs: AC.composed_chain(small, faces[:, 5:9], dev["norm"], flow, clfs, (96, 96), box, 0, AC.CONTRAST, True, 30)
    clfs = AC.classifiers(chain((None, None, None))["features"], (30, 12, 8), seed=31)
    fa = A.FaceAnalyzer(flow, *clfs, contrast=AC.CONTRAST)
    got = fa.estimate_faces(small, faces)
    direct = fa.estimate(small, faces[:, 5:9])
    assert np.any(got["status"] == 0)
    assert_same(got, direct, VALUE_KEYS + ("status", "race_confidence", "gender_confidence"))
    assert_same(got, chain(clfs), VALUE_KEYS + ("status",))
    ok = got["status"] == 0
    assert [l for l, o in zip(got["gender_label"], ok) if o] == A.gender_strings(got["gender"][ok])
    assert [l for l, o in zip(got["race_label"], ok) if o] == A.race_strings(got["race"][ok])
    assert all(l is None for l, o in zip(got["gender_label"] + got["race_label"], list(ok) * 2) if not o)
    dev["torch"].cuda.synchronize()
    fa.close()
    for c in clfs:
        c.close()
    flow.close()


@pytest.mark.gpu
def test_workspace_growth_and_reuse(dev):
    eyes = np.concatenate([dev["eyes"], NC.random_eyes(60, FRAME, seed=17)])[:40]
    one = dev["analyzer"]()
    keys = VALUE_KEYS + ("status", "patches", "features")
    for flags in (0, A.FLAG_COMPOSED):
        for n in (2, 40, 2):
            got = one.estimate(dev["frame"], eyes[:n], return_intermediates=True, flags=flags)
            fresh = dev["analyzer"]().estimate(dev["frame"], eyes[:n], return_intermediates=True, flags=flags)
            assert_same(got, fresh, keys)
            if n == 40:
                assert_same(got, dev["chain"](eyes, dev["clfs"]), keys)
                assert np.count_nonzero(got["status"] == 0) >= 20
