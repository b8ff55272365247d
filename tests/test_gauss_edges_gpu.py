"""GPU: the Gaussian soft-label regression (csrc/hg_gauss.hip: k_gauss_regression, k_gauss_regression_wg, k_gauss_regression_wg_multi
over hg_gauss_dev.hpp) in every launch form and at every size edge, against the long-double reference of tests/gauss_cases.py.

Bounds are not constants: per case the error of a plain float64 two-pass restatement against the reference is the noise of a correct
implementation; the device may have 1000 times that, at least 1e-12 and never more than 1e-9, of max|labels| for reg and of the label
spread for std (plus 64 eps max|labels|, the rounding of reg itself, which reaches std only near 0): gauss_cases.bounds_for.  The
one-pass std the kernels had misses these bounds (tests/test_gauss_host.py holds the formula to that; DESIGN.md §5 has the figures).
Every launch is held by its HIGSFA_DEBUG line to the form its case was sized for, so a moved threshold fails here instead of leaving
an edge unvisited.  Seeds are fixed; no case is chosen or dropped by a device result."""
import ctypes as C

import numpy as np
import pytest

from tests import gauss_cases as G

pytestmark = pytest.mark.gpu

HG_OK = 0
GUARD = 5
SENTINEL = -12345.678
DT = {"f64": G.F64, "f32": G.F32}
SHAPE_IDS = ["K%d-d%d" % s for s in G.SHAPES]


def _handle(lib, params):
    rc, h = G.create(lib, *params)
    assert rc == HG_OK, G.last_error(lib)
    return h


def _upload(x):
    import torch
    return torch.from_numpy(np.array(x, order="C")).cuda()      # (a copy: the cases' arrays are read-only)


def _run(lib, h, xd, n, ldx, kind, want_std=True):
    """hg_gauss_regression_device on the first n rows of a device matrix: (reg, std or None) as numpy; rows past n stay untouched."""
    import torch
    reg = torch.full((n + GUARD,), SENTINEL, dtype=torch.float64, device="cuda")
    std = torch.full((n + GUARD,), SENTINEL, dtype=torch.float64, device="cuda") if want_std else None
    torch.cuda.synchronize()
    rc = lib.hg_gauss_regression_device(h, C.c_void_p(xd.data_ptr()), DT[kind], n, ldx, C.c_void_p(reg.data_ptr()),
                                        C.c_void_p(std.data_ptr()) if want_std else None, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == HG_OK, G.last_error(lib)
    torch.cuda.synchronize()
    out = [None if t is None else t.cpu().numpy() for t in (reg, std)]
    for o in out:
        assert o is None or np.all(o[n:] == SENTINEL), "rows past the batch were written"
    return out[0][:n], None if out[1] is None else out[1][:n]


def _traced(capfd, fn, *a, **kw):
    """fn's result and the launches its debug lines name."""
    capfd.readouterr()
    res = fn(*a, **kw)
    return res, G.parse_launches(capfd.readouterr().err)


def _single(K, d, n, wave=False):
    form, R, gx, lds = G.single_form(K, d, n, wave)
    return [(form, R, gx, 1, lds)]


def _row_counts(c):
    return [n for n in G.ROW_COUNTS if n <= c.n_tile] + ([c.n_tile] if c.n_tile not in G.ROW_COUNTS else [])


def _hold(c, kind, reg, std, what):
    """A result on the first rows of the tiled base rows against the reference, within the case's bounds; K = 1 exact."""
    ref_reg, ref_std, tol_reg, tol_std = c.ref[kind]
    n = len(reg)
    e_reg, e_std = G.errors(reg, std, G.tile(ref_reg, n), G.tile(ref_std, n))
    assert e_reg <= tol_reg, "%s: reg error %.3e > %.3e" % (what, e_reg, tol_reg)
    assert std is None or e_std <= tol_std, "%s: std error %.3e > %.3e" % (what, e_std, tol_std)
    if c.K == 1:
        assert G.k1_exact(reg, std, c.params[4]), what
    return e_reg / tol_reg, (0.0 if std is None else e_std / tol_std)


# --------------------------------------------------------------------------------- 1. every shape, offset, row count, type, pitch
@pytest.mark.parametrize("K,d", G.SHAPES, ids=SHAPE_IDS)
def test_every_shape_against_the_reference(native_lib, capfd, monkeypatch, K, d):
    """Lane / slot edges (K = 1 ... 1024 at d = 4), feature edges (d = 1 ... 64), the LDS thresholds (K d = 1536 | 1537, 4096 | 4097) and
    the largest classifier, each with labels shifted by 0, 2000 and 1e6, at every row count (four rows per workgroup from 256 on, the
    ragged workgroups of 257 and 301), float32 and float64 rows, ldx = d and d + 5, with and without out_std: within the bounds;
    in the launch form the shape was sized for; and the same bits whatever n, the row's position, ldx and out_std."""
    monkeypatch.setenv("HIGSFA_DEBUG", "1")
    worst = [0.0, 0.0]
    for offset in G.OFFSETS:
        c = G.case(K, d, offset)
        h = _handle(native_lib, c.params)
        try:
            for kind in ("f64", "f32"):
                base = len(c.x[kind])
                canon = None
                for ldx in (d, d + 5):
                    xd = _upload(G.tile(c.x[kind][:, :ldx], c.n_tile))
                    for n in reversed(_row_counts(c)):
                        what = "K %d d %d offset %g %s ldx %d n %d" % (K, d, offset, kind, ldx, n)
                        (reg, std), got = _traced(capfd, _run, native_lib, h, xd, n, ldx, kind)
                        ratios = _hold(c, kind, reg, std, what)
                        worst = [max(a, b) for a, b in zip(worst, ratios)]
                        assert got == _single(K, d, n), what
                        if canon is None:
                            canon = (reg, std)
                            for a in canon:      # a row's bits do not depend on its position
                                assert a.tobytes() == G.tile(a[:base], len(a)).tobytes(), what
                        assert reg.tobytes() == canon[0][:n].tobytes() and std.tobytes() == canon[1][:n].tobytes(), what
                        (reg_only, none), got = _traced(capfd, _run, native_lib, h, xd, n, ldx, kind, want_std=False)
                        assert none is None and reg_only.tobytes() == reg.tobytes() and got == _single(K, d, n), what
                    del xd
        finally:
            native_lib.hg_gauss_free(h)
    print("K %d d %d: worst error / bound: reg %.3f std %.3f" % (K, d, worst[0], worst[1]))


# ------------------------------------------------------------------------------------------------------ 2. the same bits in every form
BOTH_FORMS = [s for s in G.SHAPES if G.FORMS[s] != "wave"]


@pytest.mark.parametrize("K,d", BOTH_FORMS, ids=["K%d-d%d" % s for s in BOTH_FORMS])
def test_same_bits_in_the_wave_and_workgroup_forms(native_lib, capfd, monkeypatch, K, d):
    """Shapes with K d <= 4096 run as one wave per row (HIGSFA_GAUSS_WAVE=1), one row per workgroup (255 rows) and, up to K d = 1536,
    four rows per workgroup (256 rows): reg and std have the same bits in all of them.  (Larger shapes exist in the wave form alone:
    test_every_shape_against_the_reference.)"""
    monkeypatch.setenv("HIGSFA_DEBUG", "1")
    for offset in (0.0, 1e6):
        c = G.case(K, d, offset)
        h = _handle(native_lib, c.params)
        try:
            for kind in ("f64", "f32"):
                xd = _upload(G.tile(c.x[kind], 256))
                runs = {}
                for n in (255, 256):
                    monkeypatch.delenv("HIGSFA_GAUSS_WAVE", raising=False)
                    runs["wg", n], got = _traced(capfd, _run, native_lib, h, xd, n, d + 5, kind)
                    assert got == _single(K, d, n)
                    monkeypatch.setenv("HIGSFA_GAUSS_WAVE", "1")
                    runs["wave", n], got = _traced(capfd, _run, native_lib, h, xd, n, d + 5, kind)
                    assert got == _single(K, d, n, wave=True)
                    monkeypatch.delenv("HIGSFA_GAUSS_WAVE")
                assert _single(K, d, 255)[0][1] == 1 and _single(K, d, 256)[0][1] == (4 if K * d <= 1536 else 1)
                _hold(c, kind, *runs["wave", 256], "wave form")
                for key, (reg, std) in runs.items():
                    assert reg.tobytes() == runs["wave", 256][0][:len(reg)].tobytes() and std.tobytes() == runs["wave", 256][1][:len(std)].tobytes(), key
        finally:
            native_lib.hg_gauss_free(h)


# ------------------------------------------------------------------------------------------------------------------ 3. the multi entry
@pytest.fixture(scope="module")
def groups(native_lib):
    made = {}

    def get(mix):
        if mix not in made:
            members, x = G.group(mix)
            made[mix] = ([_handle(native_lib, p) for p in members], {"f64": _upload(x), "f32": _upload(x.astype(np.float32))})
        return made[mix]
    yield get
    for hs, _ in made.values():
        for h in hs:
            native_lib.hg_gauss_free(h)


@pytest.mark.parametrize("m,n", G.GROUP_SIZES, ids=["m%d-n%d" % g for g in G.GROUP_SIZES])
@pytest.mark.parametrize("mix", list(G.GROUP_MIXES))
def test_multi_launch_against_single_launches(native_lib, groups, capfd, monkeypatch, mix, m, n):
    """hg_gauss_regression_multi_device on groups of unlike classifiers around n m = 127 | 128 (one row or four per workgroup), with LDS
    sized by the largest member, a member that forces R = 1 and a member that sends the group to single launches: the bits of one
    hg_gauss_regression_device launch per classifier (which the other tests hold to the reference), out_stride = n + 5 with the gap
    untouched, and the launch the group was sized for."""
    import torch
    monkeypatch.setenv("HIGSFA_DEBUG", "1")
    hs, xs = groups(mix)
    arr = (C.c_void_p * m)(*[h.value for h in hs[:m]])
    members = G.group(mix)[0]
    for kind in ("f64", "f32"):
        out = torch.full((m, n + GUARD), SENTINEL, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        rc, got = _traced(capfd, native_lib.hg_gauss_regression_multi_device, arr, m, C.c_void_p(xs[kind].data_ptr()), DT[kind], n, G.GROUP_LDX,
                          C.c_void_p(out.data_ptr()), n + GUARD, C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == HG_OK, G.last_error(native_lib)
        torch.cuda.synchronize()
        out = out.cpu().numpy()
        assert got == G.group_forms(mix, m, n)
        assert np.all(out[:, n:] == SENTINEL), "the gap between two classifiers' outputs was written"
        for s in range(m):
            reg, _ = _run(native_lib, hs[s], xs[kind], n, G.GROUP_LDX, kind, want_std=False)
            assert out[s, :n].tobytes() == reg.tobytes(), (mix, s, kind)
            if n == 301 or (m, n) == (2, 63):      # and the group's own rows against the reference (the last 40: the zero and far rows too)
                x, reg = xs[kind].cpu().numpy()[n - 40:n, :members[s][0].shape[1]], reg[n - 40:]
                ref_reg, ref_std, tol_reg, _ = G.bounds_for(x, members[s])
                assert G.errors(reg, None, ref_reg, ref_std)[0] <= tol_reg, (mix, s, kind)


# ------------------------------------------------------------------------------------------------------------------- 4. the host entry
@pytest.mark.parametrize("K,d", [(10, 4), (64, 24), (241, 17)])
def test_host_entry_on_a_pitched_array(native_lib, K, d):
    """hg_gauss_regression on a host array of d + 5 columns: the bits of the device entry, float32 and float64."""
    c = G.case(K, d, 2000.0)
    h = _handle(native_lib, c.params)
    try:
        for kind in ("f64", "f32"):
            x = G.tile(c.x[kind], 257)
            reg, std = np.full(257, SENTINEL), np.full(257, SENTINEL)
            vp = lambda a: a.ctypes.data_as(C.c_void_p)
            assert native_lib.hg_gauss_regression(h, vp(x), DT[kind], 257, d + 5, vp(reg), vp(std)) == HG_OK, G.last_error(native_lib)
            _hold(c, kind, reg, std, "host entry")
            dev = _run(native_lib, h, _upload(x), 257, d + 5, kind)
            assert reg.tobytes() == dev[0].tobytes() and std.tobytes() == dev[1].tobytes()
            reg2 = np.full(257, SENTINEL)
            assert native_lib.hg_gauss_regression(h, vp(x), DT[kind], 257, d + 5, vp(reg2), None) == HG_OK
            assert reg2.tobytes() == reg.tobytes()
    finally:
        native_lib.hg_gauss_free(h)


def test_classifier_object_with_shifted_labels(native_lib):
    """GaussianClassifier.regression(x, avg_labels=...) rebuilds its handle when the labels change: each call is held to the reference
    of the labels it was given, and going back gives the first call's bits."""
    from pyfaceanalysis_amd.classifier import GaussianClassifier
    cases = [G.case(64, 24, o) for o in G.OFFSETS]
    means, inv_covs, sqrt_det, p, avg = cases[0].params
    clf = GaussianClassifier(means, inv_covs, sqrt_det, p, avg_labels=avg)
    try:
        x = cases[0].x["f64"][:, :24]
        first = clf.regression(x, estimate_std=True)
        _hold(cases[0], "f64", *first, "own labels")
        for c in cases[1:]:
            _hold(c, "f64", *clf.regression(x, avg_labels=c.params[4], estimate_std=True), "labels + %g" % c.offset)
            _hold(c, "f32", *clf.regression(c.x["f32"][:, :24], avg_labels=c.params[4], estimate_std=True), "labels + %g, float32" % c.offset)
        again = clf.regression(x, estimate_std=True)
        assert again[0].tobytes() == first[0].tobytes() and again[1].tobytes() == first[1].tobytes()
    finally:
        clf.close()


# ---------------------------------------------------------------------------------------------------------------- 5. metamorphic checks
META_SHAPES = [(2, 4), (63, 4), (64, 4), (129, 4), (10, 64), (29, 53), (241, 17)]


@pytest.mark.parametrize("K,d", META_SHAPES, ids=["K%d-d%d" % s for s in META_SHAPES])
def test_shifted_labels_shift_reg_and_leave_std(native_lib, K, d):
    """Labels + C give reg + C and the same std, each side to its own bound (C = 2000 and 1e6 against 0)."""
    res = {}
    for offset in G.OFFSETS:
        c = G.case(K, d, offset)
        h = _handle(native_lib, c.params)
        try:
            res[offset] = _run(native_lib, h, _upload(c.x["f64"]), len(c.x["f64"]), d + 5, "f64")
        finally:
            native_lib.hg_gauss_free(h)
    c0 = G.case(K, d, 0.0)
    for offset in G.OFFSETS[1:]:
        c = G.case(K, d, offset)
        d_reg = np.abs((res[offset][0].astype(G.LD) - G.LD(offset)) - res[0.0][0].astype(G.LD)).max()
        d_std = np.abs(res[offset][1].astype(G.LD) - res[0.0][1].astype(G.LD)).max()
        # (the shifted labels are the sums rounded to float64: half an ulp of the shifted label each, inside the floor of the bound)
        assert d_reg <= c.ref["f64"][2] + c0.ref["f64"][2] and d_std <= c.ref["f64"][3] + c0.ref["f64"][3]


@pytest.mark.parametrize("K,d", [(10, 4), (63, 4), (64, 4), (128, 4), (29, 53), (241, 17)])
def test_a_class_with_prior_zero_changes_nothing(native_lib, K, d):
    """A class with prior exactly 0 (log weight -inf) put in the middle of the table — on the mean row of the fixture, where it would
    win with any positive prior, and with a label far outside the others: the result of the classifier without it, to the same bounds.
    K + 1 crosses the lane stride at 64 and the slot count at 128, (29, 53) and (241, 17) run it in the one-row workgroup form and the wave form."""
    for offset in (0.0, 1e6):
        c = G.case(K, d, offset)
        means, inv_covs, sqrt_det, p, avg = c.params
        x = c.x["f64"]
        j = K // 2
        ins = lambda a, v: np.concatenate([a[:j], np.asarray(v)[None], a[j:]])
        with_zero = (ins(means, x[12, :d]), ins(inv_covs, inv_covs[0]), ins(sqrt_det, sqrt_det[0]), ins(p, 0.0), ins(avg, avg.max() + 1000.0))
        h = _handle(native_lib, with_zero)
        try:
            for kind in ("f64", "f32"):
                _hold(c, kind, *_run(native_lib, h, _upload(c.x[kind]), len(x), d + 5, kind), "prior 0 among %d classes" % (K + 1))
        finally:
            native_lib.hg_gauss_free(h)


# ------------------------------------------------------------------------------------------------------------------ 6. non-finite rows
@pytest.mark.parametrize("K,d", [(10, 4), (64, 24), (10, 1)])
def test_a_non_finite_row_stays_in_its_row(native_lib, capfd, monkeypatch, K, d):
    """A NaN row and an Inf row, one inside a full four-row workgroup (row 5 of 303) and one in the ragged last one (row 301 of rows
    300 ... 302): that row comes back NaN in reg and std, every other row keeps the bits of the run without it."""
    monkeypatch.setenv("HIGSFA_DEBUG", "1")
    n = 303
    c = G.case(K, d, 2000.0)
    h = _handle(native_lib, c.params)
    try:
        for kind in ("f64", "f32"):
            x = G.tile(c.x[kind], n)
            clean = _run(native_lib, h, _upload(x), n, d + 5, kind)
            _hold(c, kind, *clean, "clean rows")
            for bad in ((np.nan, np.inf), (-np.inf, np.nan)):
                y = x.copy()
                y[5, :d], y[301, :d] = bad
                (reg, std), got = _traced(capfd, _run, native_lib, h, _upload(y), n, d + 5, kind)
                assert got == [("wg", 4, 76, 1, 4 * (64 + K * d) * 8)]
                keep = np.ones(n, dtype=bool)
                keep[[5, 301]] = False
                for a, b in ((reg, clean[0]), (std, clean[1])):
                    assert np.isnan(a[5]) and np.isnan(a[301])
                    assert a[keep].tobytes() == b[keep].tobytes()
    finally:
        native_lib.hg_gauss_free(h)
