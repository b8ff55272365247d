"""CPU: the host side of age, race and gender estimation (pyfaceanalysis_amd/analysis.py, hg_estimator_create): the patch box against the
reference's expressions typed out, the label rules of map_real_gender_labels_to_strings / map_real_race_labels_to_strings at their edges,
and what the constructor and the C entry refuse before any device work."""
import ctypes as C

import numpy as np
import pytest

from pyfaceanalysis_amd import _capi, analysis as A
from pyfaceanalysis_amd.classifier import GaussianClassifier
from pyfaceanalysis_amd.flow import Flow
from tests import analysis_cases as AC, helpers


def test_age_patch_box_equals_the_reference_expressions():
    # face_analysis.py:1176-1197, literally (age_subimage_width = age_subimage_height = 96)
    out_size = (256, 260)
    age_image_width = out_size[0]
    age_image_height = out_size[1]
    age_subimage_width = age_subimage_height = 96
    age_base_scale = 1.14
    reduction_factor = 160.0 / 96
    age_sampling = age_base_scale * reduction_factor
    age_subimage_first_row = age_image_height / 2.0 - age_subimage_height * age_sampling / 2.0
    age_subimage_first_column = age_image_width / 2.0 - age_subimage_width * age_sampling / 2.0
    age_translations_x = 0.0 / reduction_factor
    age_translations_y = -6.0 / reduction_factor
    # the stated reading of trans_sampled=True: the translation is in sampled pixels
    tx, ty = age_translations_x * age_sampling, age_translations_y * age_sampling
    want = (age_subimage_first_column + tx, age_subimage_first_row + ty, age_subimage_first_column + tx + age_subimage_width * age_sampling,
            age_subimage_first_row + ty + age_subimage_height * age_sampling)
    got = A.age_patch_box()
    assert isinstance(got, tuple) and all(type(v) is float for v in got)
    assert got == want
    assert np.allclose(got, (36.8, 31.96, 219.2, 214.36), rtol=0, atol=1e-9)
    # trans_sampled=False: the translation as it stands
    want_raw = (age_subimage_first_column + age_translations_x, age_subimage_first_row + age_translations_y,
                age_subimage_first_column + age_translations_x + age_subimage_width * age_sampling,
                age_subimage_first_row + age_translations_y + age_subimage_height * age_sampling)
    assert A.age_patch_box(trans_sampled=False) == want_raw and want_raw != want
    # another patch and crop size, another translation
    s = 1.3 * (160.0 / 96)
    fc, fr = 40 / 2.0 - 13 * s / 2.0, 44 / 2.0 - 11 * s / 2.0
    t0, t1 = 2.0 / (160.0 / 96) * s, -3.0 / (160.0 / 96) * s
    assert A.age_patch_box((40, 44), (13, 11), base_scale=1.3, translation=(2.0, -3.0)) == (fc + t0, fr + t1, fc + t0 + 13 * s, fr + t1 + 11 * s)


def test_label_rules_at_their_edges():
    assert A.gender_strings([0.0, -0.0, 1e-9, -1.0, 1.0]) == ["Male", "Male", "Female", "Male", "Female"]
    assert A.race_strings([0.0, -0.0, 1e-9, -2.0, 2.0]) == ["Black", "Black", "White", "Black", "White"]
    assert A.gender_strings([-0.3, 0.3], long_text=False) == ["M", "F"]
    assert A.race_strings([-0.3, 0.3], long_text=False) == ["B", "W"]
    assert A.gender_strings([]) == [] and A.race_strings(np.zeros(0)) == []
    assert A.gender_strings([-1.000001, 1.000001]) == ["Male", "Female"]
    assert A.race_strings([-2.000001, 2.000001]) == ["Black", "White"]
    for fn, edge in ((A.gender_strings, 1.000001), (A.race_strings, 2.000001)):
        for v in (np.nextafter(edge, np.inf), np.nextafter(-edge, -np.inf), 10.0):
            with pytest.raises(ValueError, match="Unrecognized label: "):
                fn([0.5, v])
    g, r = np.array([-0.75, 0.0, 0.25]), np.array([-1.5, 0.0, 2.0])
    assert np.array_equal(A.gender_confidence(g), np.abs(g)) and np.array_equal(A.race_confidence(r), np.abs(r) / 2.0)


def consts(pw=8, ph=8, k=9, filt=0, std=48.0):
    c = _capi.HgEstimatorConsts()
    c.crop_w, c.crop_h, c.method, c.rotate = 40, 44, _capi.HG_NORM_AREAZ, 1
    c.patch_w, c.patch_h, c.filter, c.clip = pw, ph, filt, 1
    c.box[:] = (3.0, 2.0, 30.0, 40.0)
    c.target_mean, c.target_std = 128.0, std
    c.n_features, c.reserved = k, 0
    return c


def test_estimator_create_refuses_bad_arguments_on_the_host(native_lib):
    L = native_lib
    h = C.c_void_p()
    f = Flow(helpers.linear_net(0), output_dtype=np.float32)                  # 8 x 8 inputs, 9 outputs
    fh = f._handle(on_device=False).h
    create = lambda flow, cc: L.hg_estimator_create(flow, None, None, None, None if cc is None else C.byref(cc), None, 0, C.byref(h))
    assert create(fh, None) == _capi.HG_ERR_ARG and b"null constants" in L.hg_last_error()
    assert create(fh, consts(std=0.0)) == _capi.HG_ERR_ARG and b"target_std" in L.hg_last_error()
    assert create(fh, consts(std=-1.0)) == _capi.HG_ERR_ARG
    assert create(fh, consts(std=float("nan"))) == _capi.HG_ERR_ARG
    assert create(fh, consts(filt=1)) == _capi.HG_ERR_ARG and b"filter" in L.hg_last_error()      # 1 is LANCZOS in PIL: not a transform filter
    assert create(fh, consts(filt=4)) == _capi.HG_ERR_ARG
    bad = consts()
    bad.clip = 2
    assert create(fh, bad) == _capi.HG_ERR_ARG
    bad = consts()
    bad.box[2] = float("inf")
    assert create(fh, bad) == _capi.HG_ERR_ARG
    assert create(fh, consts(pw=300, ph=300)) == _capi.HG_ERR_ARG             # 90000 pixels
    assert create(None, consts()) == _capi.HG_ERR_ARG and b"null flow" in L.hg_last_error()
    assert create(fh, consts(pw=16, ph=16)) == _capi.HG_ERR_DIM and b"columns" in L.hg_last_error()      # patch width != flow input width
    assert create(fh, consts(k=10)) == _capi.HG_ERR_DIM and b"features" in L.hg_last_error()           # kept > outputs
    assert create(fh, consts()) == _capi.HG_ERR_ARG and b"at least one classifier" in L.hg_last_error()  # no classifier at all
    assert not h.value
    assert L.hg_estimator_patches_device(None, 0, None, 0, 1, None, 0, None) == _capi.HG_ERR_ARG
    assert L.hg_estimator_estimate_device(None, 0, None, 8, 8, 8, None, 1, None, 1, None, None, None) == _capi.HG_ERR_ARG
    L.hg_estimator_free(None)
    f.close()


def test_constructor_refusals_need_no_device():
    f = Flow(helpers.linear_net(0), output_dtype=np.float32)
    g5 = GaussianClassifier(np.zeros((2, 5)), np.stack([np.eye(5)] * 2), np.ones(2), np.ones(2) / 2, avg_labels=AC.GENDER_LABELS)
    g9 = GaussianClassifier(np.zeros((2, 9)), np.stack([np.eye(9)] * 2), np.ones(2), np.ones(2) / 2, avg_labels=AC.RACE_LABELS)
    kw = dict(contrast=AC.CONTRAST, patch_size=(8, 8))
    with pytest.raises(TypeError):
        A.FaceAnalyzer(f, gender=g5, patch_size=(8, 8))                        # the contrast targets are required
    with pytest.raises(ValueError, match="at least one classifier"):
        A.FaceAnalyzer(f, **kw)
    with pytest.raises(ValueError, match="target_std"):
        A.FaceAnalyzer(f, gender=g5, contrast=(128.0, 0.0), patch_size=(8, 8))
    with pytest.raises(ValueError, match="filter"):
        A.FaceAnalyzer(f, gender=g5, interpolation="LANCZOS", **kw)
    with pytest.raises(ValueError, match="filter"):
        A.FaceAnalyzer(f, gender=g5, interpolation=1, **kw)
    with pytest.raises(ValueError, match="columns"):
        A.FaceAnalyzer(f, gender=g5, contrast=AC.CONTRAST)                    # 96 x 96 patches into an 8 x 8 flow
    with pytest.raises(ValueError, match="kept"):
        A.FaceAnalyzer(f, gender=g5, race=g9, n_features=8, **kw)             # input_dim > n_features
    with pytest.raises(ValueError, match="kept"):
        A.FaceAnalyzer(f, gender=g5, n_features=10, **kw)                     # n_features > the flow's outputs
    with pytest.raises(ValueError, match="float32"):
        A.FaceAnalyzer(Flow(helpers.linear_net(0)), gender=g5, **kw)
    with pytest.raises(ValueError, match="avg_labels"):
        A.FaceAnalyzer(f, gender=GaussianClassifier(np.zeros((2, 5)), np.stack([np.eye(5)] * 2), np.ones(2), np.ones(2) / 2), **kw)
    with pytest.raises(ValueError, match="preset"):
        A.FaceAnalyzer(f, gender=g5, normalizer_preset="portrait", **kw)
    fa = A.FaceAnalyzer(f, gender=g5, race=g9, interpolation="BICUBIC", clip=False, **kw)
    c = fa.consts()
    assert (c.crop_w, c.crop_h, c.method, c.rotate) == (256, 260, _capi.HG_NORM_AREAZ, 1) and (c.patch_w, c.patch_h, c.filter, c.clip) == (8, 8, 3, 0)
    assert tuple(c.box) == A.age_patch_box((256, 260), (8, 8)) and (c.target_mean, c.target_std) == AC.CONTRAST and c.n_features == 9 and fa.k == 9
    assert C.sizeof(_capi.HgEstimatorConsts) == 88


def test_unclipped_contrast_restatement_differs_only_where_the_clip_acts():
    p = AC.noise_crops(2, (9, 7)).reshape(2, -1)
    a, b = AC.contrast(p, 128.0, 90.0, clip=True), AC.contrast(p, 128.0, 90.0, clip=False)
    inside = (b >= 0.0) & (b <= 255.0)
    assert np.array_equal(a[inside], b[inside]) and not inside.all() and np.array_equal(a[~inside], np.clip(b[~inside], 0.0, 255.0))
    z = AC.contrast(np.full((1, 12), 7, dtype=np.uint8), *AC.CONTRAST_UNCLIPPED, clip=False)      # std 0: every pixel the target mean
    assert z.dtype == np.float32 and np.all(z == 0.0)
