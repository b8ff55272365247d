"""Case tables, classifier and row builders and the long-double reference shared by tests/test_gauss_edges_gpu.py and
tests/test_gauss_host.py (the Gaussian soft-label regression of csrc/hg_gauss.hip / hg_gauss_dev.hpp at its edges).

The reference (``ref_ld``) restates the regression in ``np.longdouble`` from the inputs exactly as given (float32 rows are exact in
long double): log domain, posteriors normalised, reg = sum post a, std = sqrt(sum post (a - reg)^2) — the two-pass form of the
reference's estimate_std.  ``f64_two_pass`` is the same in plain float64; its error against the reference is the noise of a correct
float64 implementation of a case, and ``bounds`` turns that noise into what the device (and the C restatement) is held to.
``f64_one_pass`` is the formula the kernels had, sqrt(max(sum w a^2 / sum w - reg^2, 0)): kept as the negative control only."""
from __future__ import annotations

import ctypes as C
import functools
import types

import numpy as np

from tests.train_cases import CAP, EPS, FACTOR, FLOOR

LD = np.longdouble
F32, F64 = 1, 2                                   # HG_F32, HG_F64 (include/higsfa.h)

# ---------------------------------------------------------------------------------------------------------------- case tables
OFFSETS = (0.0, 2000.0, 1e6)                      # added to the labels: regression(x, avg_labels=...) takes any
# the form a single launch of a shape is sized for: "r4" workgroup form, four rows per workgroup from 256 rows on (K d <= 1536);
# "r1" workgroup form, one row per workgroup (K d <= 4096); "wave" one wave per row
LANE_SHAPES = [((k, 4), "r4") for k in (1, 2, 63, 64, 65, 128, 129)] + [((1023, 4), "r1"), ((1024, 4), "r1")]     # lane stride 64, 16 slots
FEATURE_SHAPES = [((10, d), "r4") for d in (1, 2, 63, 64)]                                                          # the xs[64] row
LDS_SHAPES = [((64, 24), "r4"), ((24, 64), "r4"), ((29, 53), "r1"), ((64, 64), "r1"), ((1024, 4), "r1"), ((256, 16), "r1"), ((241, 17), "wave"),
              ((65, 64), "wave"), ((1024, 5), "wave"), ((1024, 64), "wave")]
FEW_ROWS_ONLY = {(1024, 64): 8}                   # 32 MB of matrices: eight rows, no tiling
FORMS = dict(LANE_SHAPES + FEATURE_SHAPES + LDS_SHAPES)
SHAPES = list(FORMS)                              # (1024, 4) is in two tables: once
ROW_COUNTS = (1, 3, 4, 5, 255, 256, 257, 301)
N_TILE = max(ROW_COUNTS)
# the multi entry: (m, n) around n m = 128, and the classifier mixes; every group reads one (n, GROUP_LDX) matrix
GROUP_LDX = 24
GROUP_SIZES = ((2, 63), (2, 64), (3, 42), (3, 43), (4, 31), (4, 32), (4, 301))
GROUP_MIXES = {
    "small": ((10, 4), (50, 20), (39, 5), (2, 9)),           # every K d <= 1536: R = 4 from n m = 128 on
    "widths": ((64, 24), (10, 4), (10, 9), (50, 20)),        # d = 24, 4, 9, 20 on ldx = 24; LDS sized by the first (1536, the limit)
    "mid": ((10, 4), (100, 20), (39, 5), (2, 9)),            # one member in (1536, 4096]: R = 1 whatever n m
    "big": ((10, 4), (300, 20), (39, 5), (2, 9)),            # one member above 4096: single launches
}


def single_form(K, d, n, wave=False):
    """(form, R, grid_x, lds bytes) of a single launch as the shape's table entry sizes it."""
    cls = "wave" if wave else FORMS[(K, d)]
    if cls == "wave":
        return ("wave", 1, n, 64 * 8)
    R = 4 if cls == "r4" and n >= 256 else 1
    return ("wg", R, -(-n // R), R * (64 + K * d) * 8)


def group_forms(mix, m, n):
    """The launches of a multi call on the first m members of a mix: one "multi" line, or the members' single launches."""
    shapes = GROUP_MIXES[mix][:m]
    kd = [k * d for k, d in shapes]
    if max(kd) > 4096:
        out = []
        for (k, d), e in zip(shapes, kd):
            R = 4 if e <= 1536 and n >= 256 else 1
            out.append(("wave", 1, n, 1, 64 * 8) if e > 4096 else ("wg", R, -(-n // R), 1, R * (64 + e) * 8))
        return out
    R = 4 if mix in ("small", "widths") and n * m >= 128 else 1
    return [("multi", R, -(-n // R), m, R * (64 + max(kd)) * 8)]


def parse_launches(err):
    """[(form, R, grid_x, grid_y, lds)] from the "[gauss] form ..." lines of a HIGSFA_DEBUG run."""
    out = []
    for line in err.splitlines():
        if line.startswith("[gauss] "):
            w = line.split()
            gx, gy = w[w.index("grid") + 1].split("x")
            out.append((w[w.index("form") + 1], int(w[w.index("R") + 1]), int(gx), int(gy), int(w[w.index("lds") + 1])))
    return out


# ----------------------------------------------------------------------------------------------------------- inputs
@functools.lru_cache(maxsize=None)
def _drawn(K, d, seed):
    rng = np.random.default_rng([seed, K, d])
    means = rng.normal(size=(K, d)) * 2.0
    a = rng.normal(size=(K, d, d))
    inv_covs = a @ a.transpose(0, 2, 1) / d + 0.5 * np.eye(d)
    sqrt_det = np.exp(-0.5 * np.linalg.slogdet(inv_covs)[1])
    p = rng.random(K) + 0.1
    p /= p.sum()
    out = (means, inv_covs, sqrt_det, p, np.sort(rng.normal(size=K)) * 10.0)
    for v in out:
        v.setflags(write=False)
    return out


def classifier(K, d, seed=0, offset=0.0):
    """(means, inv_covs, sqrt_det, p, avg): random means, SPD inverse covariances A A'/d + I/2, their sqrt-determinants from slogdet,
    random priors, sorted normal labels x 10 + offset.  The offset changes the labels alone (the other arrays are shared, read-only)."""
    means, inv_covs, sqrt_det, p, labels = _drawn(K, d, seed)
    return means, inv_covs, sqrt_det, p, labels + offset


def rows(means, n_near=12, seed=0, ldx=None):
    """n_near rows near class means (0.3 sigma around seeded picks), one exactly on a mean, one at the midpoint of two means, one at
    least 40 units from every mean (the posterior is one-hot and every density underflows outside the log domain) and an all-zero row.
    ldx: width of the matrix (columns past d are filled with unrelated values)."""
    K, d = means.shape
    rng = np.random.default_rng([seed, K, d, 1])
    pick = rng.integers(0, K, n_near + 3)
    x = means[pick[:n_near]] + 0.3 * rng.normal(size=(n_near, d))
    u = rng.normal(size=d)
    far = u / np.linalg.norm(u) * (40.0 + np.linalg.norm(means, axis=1).max())
    x = np.concatenate([x, means[pick[n_near]][None], 0.5 * (means[pick[n_near + 1]] + means[(pick[n_near + 1] + 1) % K])[None], far[None], np.zeros((1, d))])
    if ldx is not None and ldx > d:
        x = np.concatenate([x, 7.0 * rng.normal(size=(len(x), ldx - d))], axis=1)
    return np.ascontiguousarray(x)


def tile(a, n):
    """The first n rows of the base rows repeated (as tests/test_gpu_parity.py builds its 301 rows)."""
    return np.ascontiguousarray(np.concatenate([a] * -(-n // len(a)))[:n])


# ----------------------------------------------------------------------------------------------------------------- reference
def _regress(x, means, inv_covs, sqrt_det, p, avg, dtype, one_pass=False):
    x, means, inv_covs, avg = (np.asarray(v).astype(dtype) for v in (x, means, inv_covs, avg))
    dx = x[:, None, :] - means[None]
    q = (np.einsum("cij,ncj->nci", inv_covs, dx) * dx).sum(axis=2)
    with np.errstate(divide="ignore"):
        lp = np.log(np.asarray(p).astype(dtype)) - np.log(np.asarray(sqrt_det).astype(dtype)) - q / 2
    w = np.exp(lp - lp.max(axis=1, keepdims=True))
    sw = w.sum(axis=1)
    reg = (w * avg).sum(axis=1) / sw
    if one_pass:
        return reg, np.sqrt(np.maximum((w * avg * avg).sum(axis=1) / sw - reg * reg, 0))
    return reg, np.sqrt((w * (avg[None] - reg[:, None]) ** 2).sum(axis=1) / sw)


def ref_ld(x, means, inv_covs, sqrt_det, p, avg):
    """(reg, std) in long double: log domain, normalised posteriors, two-pass std."""
    return _regress(x, means, inv_covs, sqrt_det, p, avg, LD)


def f64_two_pass(x, means, inv_covs, sqrt_det, p, avg):
    return _regress(x, means, inv_covs, sqrt_det, p, avg, np.float64)


def f64_one_pass(x, means, inv_covs, sqrt_det, p, avg):
    """What the kernels computed before: the negative control of tests/test_gauss_host.py."""
    return _regress(x, means, inv_covs, sqrt_det, p, avg, np.float64, one_pass=True)


def mdp_linear(x, means, inv_covs, sqrt_det, p, avg):
    """MDP's GaussianClassifier in the linear domain (densities, no log) with cuicuilco's regression / estimate_std on top, in long
    double: only for rows whose densities do not underflow."""
    x, means, inv_covs, sqrt_det, p, avg = (np.asarray(v).astype(LD) for v in (x, means, inv_covs, sqrt_det, p, avg))
    d = means.shape[1]
    dx = x[:, None, :] - means[None]
    q = (np.einsum("cij,ncj->nci", inv_covs, dx) * dx).sum(axis=2)
    prob = p * (2 * LD(np.pi)) ** (-LD(d) / 2) / sqrt_det * np.exp(-q / 2)
    with np.errstate(invalid="ignore"):                  # far rows: 0 / 0
        post = prob / prob.sum(axis=1, keepdims=True)
    reg = post @ avg
    return reg, np.sqrt((post * (avg[None] - reg[:, None]) ** 2).sum(axis=1))


def units(avg):
    """(A, S): reg errors are measured in A = max|avg|, std errors in the label spread S = max(avg) - min(avg)."""
    avg = np.asarray(avg, dtype=np.float64)
    return float(np.abs(avg).max()), float(avg.max() - avg.min())


def _tol(noise):
    return min(max(FACTOR * noise, FLOOR), CAP)


def bounds_for(x, params):
    """(reference reg, reference std, absolute bound on reg, absolute bound on std) of rows x under a classifier.  The bounds come
    from the float64 two-pass restatement's own error (the noise of a correct implementation) and never from a device result:
    reg within min(max(1000 noise, 1e-12), 1e-9) of A; std within the same rule of S plus 64 eps A, the rounding of reg itself (at
    most 16 serial and 6 butterfly adds, a multiply and a divide, doubled), which reaches std only where std is about 0."""
    reg, std = ref_ld(x, *params)
    r64, s64 = f64_two_pass(x, *params)
    A, S = units(params[4])
    noise_reg = float(np.abs(r64.astype(LD) - reg).max()) / A if A > 0 else 0.0
    noise_std = float(np.abs(s64.astype(LD) - std).max()) / S if S > 0 else 0.0
    return reg, std, _tol(noise_reg) * A, _tol(noise_std) * S + 64 * EPS * A


def errors(got_reg, got_std, ref_reg, ref_std):
    """Worst absolute errors in long double; a non-finite result is an infinite error."""
    def worst(got, ref):
        e = np.abs(np.asarray(got).astype(LD) - ref)
        return float("inf") if not np.all(np.isfinite(np.asarray(got))) else float(e.max())
    return worst(got_reg, ref_reg), (None if got_std is None else worst(got_std, ref_std))


def case_seed(K, d):
    return 100 + K * 65 + d


@functools.lru_cache(maxsize=None)
def case(K, d, offset):
    """One (shape, label offset): the classifier, its base rows as float64 and rounded to float32 (with five unrelated columns to the
    right: ldx = d + 5 reads the same rows), and per row type the reference and the bounds — computed once, shared, read-only."""
    c = types.SimpleNamespace(K=K, d=d, offset=offset, params=classifier(K, d, case_seed(K, d), offset))
    wide = rows(c.params[0], n_near=4 if (K, d) in FEW_ROWS_ONLY else 12, seed=case_seed(K, d), ldx=d + 5)
    c.x = {"f64": wide, "f32": wide.astype(np.float32)}
    c.n_tile = FEW_ROWS_ONLY.get((K, d), N_TILE)
    c.ref = {}
    for kind, xx in c.x.items():
        xx.setflags(write=False)
        c.ref[kind] = bounds_for(xx[:, :d], c.params)
    for a in c.params:
        a.setflags(write=False)
    return c


def bounds(c, kind="f64"):
    """(absolute bound on reg, absolute bound on std) of a case's rows of one type."""
    return c.ref[kind][2:]


def k1_exact(reg, std, avg):
    """K = 1: the posterior is 1 whatever the row: reg is avg[0] and std 0, exactly."""
    return np.all(np.asarray(reg) == avg[0]) and (std is None or np.all(np.asarray(std) == 0.0))


@functools.lru_cache(maxsize=None)
def group(mix):
    """The four classifiers of a mix (offsets 0, 2000, 1e6, 0 in turn) and N_TILE rows of GROUP_LDX columns: rows near the means of the
    members in turn (each member reads its first d columns), a zero row and a far row."""
    members = [classifier(k, d, 900 + i, OFFSETS[i % 3]) for i, (k, d) in enumerate(GROUP_MIXES[mix])]
    rng = np.random.default_rng([17, sorted(GROUP_MIXES).index(mix)])
    x = 2.0 * rng.normal(size=(N_TILE, GROUP_LDX))
    for r in range(N_TILE - 2):
        m = members[r % 4][0]
        x[r, :m.shape[1]] = m[rng.integers(0, len(m))] + 0.3 * rng.normal(size=m.shape[1])
    x[-2] = 0.0
    x[-1] = 60.0
    x.setflags(write=False)
    return members, x


# ---------------------------------------------------------------------------------------------------------------- the entries
def _vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def create(lib, means, inv_covs, sqrt_det, p, avg, K=None, d=None, device=0, out=True):
    """hg_gauss_create through the C ABI: (rc, handle).  K / d override the arrays' shape (the refusals)."""
    arrs = [None if a is None else np.ascontiguousarray(a, dtype=np.float64) for a in (means, inv_covs, sqrt_det, p, avg)]
    h = C.c_void_p()
    rc = lib.hg_gauss_create(arrs[0].shape[0] if K is None else K, arrs[0].shape[1] if d is None else d, *[_vp(a) for a in arrs], device,
                             C.byref(h) if out else None)
    return rc, h


def last_error(lib):
    return lib.hg_last_error().decode("utf-8", "replace")
