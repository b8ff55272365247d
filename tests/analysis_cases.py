"""Shared by tests/test_analysis_host.py and tests/test_analysis_gpu.py: the oracle of the age patch — PIL's own ``transform`` followed by
the restated contrast step (tests/eyes_restate.py, plus the unclipped variant) — the crops, boxes and synthetic classifiers of the
estimation tests, and the composed public calls the device chain is compared with."""
import numpy as np

from tests import eyes_restate as ER

FILTERS = {"NEAREST": 0, "BILINEAR": 2, "BICUBIC": 3}       # PIL's codes
CONTRAST = (128.0, 48.0)          # the build's contrast targets for these tests (pixel units)
CONTRAST_STEEP = (128.0, 110.0)   # a target std above the noise crops' own (about 74): values leave [0, 255], the clip acts
CONTRAST_UNCLIPPED = (0.0, 0.16)  # the reference's obj_avgs / obj_stds read as they stand: only meaningful without the clip


def contrast(patches_u8, target_mean, target_std, clip=True):
    """tests/eyes_restate.contrast, and the same without np.clip: exact statistics, float64 arithmetic, float32 result."""
    if clip:
        return ER.contrast(patches_u8, target_mean, target_std)
    p = np.asarray(patches_u8)
    out = np.empty(p.shape, dtype=np.float32)
    for i in range(len(p)):
        mean, std = ER.contrast_stats(p[i])
        x = p[i].astype(np.float64)
        x -= mean
        x /= (std / target_std) + 0.00000001
        x += target_mean
        out[i] = x.astype(np.float32)
    return out


def pil_cut(crops, patch_size, box, filt):
    """``Image.fromarray(crop).transform((pw, ph), Image.EXTENT, box, F)`` per crop: (n, pw * ph) uint8."""
    from PIL import Image
    pw, ph = patch_size
    box = tuple(float(v) for v in box)
    return np.stack([np.asarray(Image.fromarray(np.ascontiguousarray(c)).transform((pw, ph), Image.EXTENT, box, filt)).reshape(-1) for c in crops]
                    ) if len(crops) else np.zeros((0, pw * ph), dtype=np.uint8)


def patch_oracle(crops, patch_size, box, filt, targets, clip=True):
    return contrast(pil_cut(crops, patch_size, box, filt), targets[0], targets[1], clip)


def noise_crops(n, crop_size, seed=0):
    w, h = crop_size
    return np.random.default_rng(500 + 31 * w + h + seed).integers(0, 256, (n, h, w), dtype=np.uint8)


# (name, crop size, patch size, box or None for age_patch_box): fewer pixels than threads, an odd remainder, the reference's shape, a box
# hanging over the crop's left and top edges, one over its right and bottom edges
SMALL_CROP = (40, 44)
PATCH_CASES = [
    ("8x8", SMALL_CROP, (8, 8), (3.3, 2.1, 30.7, 41.9)),
    ("13x11", SMALL_CROP, (13, 11), (5.25, 7.5, 36.0, 39.75)),
    ("13x11-over-left-top", SMALL_CROP, (13, 11), (-9.4, -6.2, 27.3, 30.1)),
    ("13x11-over-right-bottom", SMALL_CROP, (13, 11), (12.6, 14.9, 51.0, 55.5)),
    ("96x96-reference", (256, 260), (96, 96), None),
]
ABOVE_THE_CAP = ("130x130", (256, 260), (130, 130), (10.5, 8.25, 250.0, 255.5))      # 16900 pixels > 16384


def patch_flow(patch_size, d_out=5, seed=3):
    """A linear network for patch sizes no hierarchy here reads: one node on all pixels where a node may be that wide (an affine node of the
    generic plan takes at most 16383 inputs), else a 10 x 10 grid of cloned fields under one node (sides that are multiples of 10)."""
    from pyfaceanalysis_amd import nodes as N
    from tests import helpers
    rng = np.random.default_rng(seed)
    pw, ph = patch_size
    if pw * ph <= 16383:
        return [helpers.rand_pca(rng, pw * ph, d_out)]
    assert pw % 10 == 0 and ph % 10 == 0
    sb0 = N.Rectangular2dSwitchboard((pw, ph), (pw // 10, ph // 10), (pw // 10, ph // 10), 1)
    l0 = N.CloneLayer(helpers.rand_pca(rng, (pw // 10) * (ph // 10), 2), 100)
    sb1 = N.Rectangular2dSwitchboard((10, 10), (10, 10), (10, 10), 2)
    return [sb0, l0, sb1, N.Layer([helpers.rand_pca(rng, 200, d_out)])]


def synthetic_classifier(seed, feats, d, avg_labels):
    """A GaussianClassifier on the first d feature columns: class means scattered over the spread of ``feats``, random SPD covariances."""
    from pyfaceanalysis_amd.classifier import GaussianClassifier
    rng = np.random.default_rng(seed)
    k = len(avg_labels)
    mu, sd = feats[:, :d].mean(axis=0), feats[:, :d].std(axis=0) + 1e-3
    means = mu + sd * rng.normal(size=(k, d))
    a = rng.normal(size=(k, d, d))
    covs = (a @ a.transpose(0, 2, 1) + d * np.eye(d)) * (sd[:, None] * sd[None, :])
    p = rng.uniform(0.5, 1.5, k)
    return GaussianClassifier(means, np.linalg.inv(covs), np.sqrt(np.linalg.det(covs)), p / p.sum(), avg_labels=avg_labels)


AGE_LABELS = [4.0, 11.0, 19.0, 28.0, 41.0, 63.0]
RACE_LABELS = [-2.0, 2.0]
GENDER_LABELS = [-1.0, 1.0]


def classifiers(feats, dims=(4, 5, 5), seed=11):
    """(age, race, gender) of input dims ``dims``."""
    return (synthetic_classifier(seed, feats, dims[0], AGE_LABELS), synthetic_classifier(seed + 1, feats, dims[1], RACE_LABELS),
            synthetic_classifier(seed + 2, feats, dims[2], GENDER_LABELS))


def frame_eyes(w, h):
    """Six eye pairs on a w x h frame, the last two near the border (their crops reach over it)."""
    return np.array([
        (0.40 * w, 0.45 * h, 0.55 * w, 0.47 * h),
        (0.30 * w, 0.60 * h, 0.42 * w, 0.52 * h),
        (0.60 * w, 0.30 * h, 0.85 * w, 0.36 * h),
        (0.50 * w, 0.50 * h, 0.53 * w, 0.50 * h),
        (1.0, 2.5, 14.0, 4.0),
        (w - 21.0, h - 6.0, w - 2.0, h - 9.5),
    ], dtype=np.float64)


def composed_chain(frame_dev, eyes, normalizer, flow, clfs, patch_size, box, filt, targets, clip, n_features):
    """The public calls one after the other: FaceNormalizer.normalize -> the patch oracle -> flow.execute -> regression.  ``clfs``:
    (age, race, gender), None where absent.  Refused faces (status != 0) come back NaN."""
    img, status = normalizer.normalize(frame_dev, eyes)
    crops = img.cpu().numpy()
    patches = patch_oracle(crops, patch_size, box, filt, targets, clip)
    n = len(crops)
    feats = flow.execute(patches)[:, :n_features] if n else np.zeros((0, n_features), dtype=np.float32)
    out = dict(status=status, crops=crops, patches=patches, features=feats)
    bad = status != 0
    age, race, gender = clfs
    if age is not None:
        a, s = age.regression(feats[:, :age.input_dim], estimate_std=True)
        out["age"], out["age_std"] = np.where(bad, np.nan, a), np.where(bad, np.nan, s)
    if race is not None:
        out["race"] = np.where(bad, np.nan, race.regression(feats[:, :race.input_dim]))
    if gender is not None:
        out["gender"] = np.where(bad, np.nan, gender.regression(feats[:, :gender.input_dim]))
    return out


def same(a, b):
    """array_equal with NaNs compared by position."""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")
