"""No GPU: what tests/test_gauss_edges_gpu.py leans on.  The C restatement (oracle/ref_c.c, the two-pass std) against the long-double
reference of tests/gauss_cases.py within the bounds the device is held to, on every case: a plain float64 implementation stays inside
them.  The one-pass formula the kernels had violates them (the negative control: a bound that lets it through is too loose).  The
reference against MDP's linear-domain formula.  And the refusals of hg_gauss_create, which are all checked before the device is
looked for, so each is HG_ERR_ARG with its text on any machine."""
import os

import numpy as np
import pytest

from oracle import ref_c
from tests import gauss_cases as G

HG_ERR_ARG = -1
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
AGE = 2          # classifiers.npz: the 39 x 4 age classifier, labels 16.5 ... 57.5


def _golden(i):
    g = np.load(os.path.join(GOLD, "classifiers.npz"))
    return tuple(g["c%d_%s" % (i, k)] for k in ("means", "inv_covs", "sqrt_def_covs", "p", "avg_labels")), g["c%d_x" % i], g["c%d_reg" % i], g["c%d_std" % i]


@pytest.mark.parametrize("K,d", G.SHAPES, ids=["K%d-d%d" % s for s in G.SHAPES])
def test_c_restatement_within_bounds(K, d):
    """oracle/ref_c.c on every shape and offset, float64 rows and float32-rounded rows: inside the device's bounds; K = 1 exact."""
    for offset in G.OFFSETS:
        c = G.case(K, d, offset)
        for kind in ("f64", "f32"):
            ref_reg, ref_std, tol_reg, tol_std = c.ref[kind]
            reg, std = ref_c.gauss_regression(c.x[kind][:, :d].astype(np.float64), *c.params)
            e_reg, e_std = G.errors(reg, std, ref_reg, ref_std)
            print("K %d d %d offset %g %s: reg %.2e / %.2e  std %.2e / %.2e" % (K, d, offset, kind, e_reg, tol_reg, e_std, tol_std))
            assert e_reg <= tol_reg and e_std <= tol_std
            if K == 1:
                assert G.k1_exact(reg, std, c.params[4])
            assert np.array_equal(ref_c.gauss_regression(c.x[kind][:, :d].astype(np.float64), *c.params, want_std=False), reg)


CONTROL = [(K, d, o) for (K, d) in G.SHAPES for o in G.OFFSETS[1:] if K >= 2 and 20 <= K * d <= 4096]


@pytest.mark.parametrize("K,d,offset", CONTROL, ids=["K%d-d%d-%g" % c for c in CONTROL])
def test_one_pass_formula_violates_the_std_bound(K, d, offset):
    """The negative control: sqrt(max(sum w a^2 / sum w - reg^2, 0)) in float64 misses the std bound on every shifted case with K >= 2
    and 20 <= K d <= 4096 (its reg, the same operations as the two-pass form's, does not)."""
    c = G.case(K, d, offset)
    ref_reg, ref_std, tol_reg, tol_std = c.ref["f64"]
    reg, std = G.f64_one_pass(c.x["f64"][:, :d], *c.params)
    e_reg, e_std = G.errors(reg, std, ref_reg, ref_std)
    print("K %d d %d offset %g: one-pass std error %.2e, bound %.2e" % (K, d, offset, e_std, tol_std))
    assert e_reg <= tol_reg and e_std > tol_std


def test_one_pass_formula_violates_the_bound_on_the_age_classifier():
    """The shipped age classifier on its own fixture rows (labels 16.5 ... 57.5, no shift): the one-pass form is off by 2.2e-7 where
    the true std is 1.9e-8 — 5e-9 of the label spread, above the cap — and the stored std is the reference's."""
    params, x, gold_reg, gold_std = _golden(AGE)
    ref_reg, ref_std, tol_reg, tol_std = G.bounds_for(x, params)
    _, e_std = G.errors(*G.f64_one_pass(x, *params), ref_reg, ref_std)
    A, S = G.units(params[4])
    assert params[0].shape == (39, 4) and abs(A - 57.5) < 0.05 and abs(S - 41.0) < 0.05
    assert e_std > 1e-7 and e_std / S > G.CAP and e_std > tol_std
    e_reg, e_two = G.errors(*G.f64_two_pass(x, *params), ref_reg, ref_std)
    assert e_reg <= tol_reg and e_two <= tol_std
    assert np.array_equal(gold_std, ref_std.astype(np.float64))


def test_reference_against_the_linear_domain_formula():
    """ref_ld against MDP's formula as published (densities with the (2 pi)^(-d/2) factor, normalised, no log) on the near rows of the
    seven golden classifiers, and the two-pass float64 form against it on all their rows."""
    for i in range(7):
        params, x, gold_reg, gold_std = _golden(i)
        reg, std = G.ref_ld(x, *params)
        lin_reg, lin_std = G.mdp_linear(x, *params)
        ok = np.isfinite(lin_reg.astype(np.float64))             # rows far from every class: 0 / 0 outside the log domain
        assert ok.sum() >= 20
        A, S = G.units(params[4])
        assert float(np.abs(reg - lin_reg)[ok].max()) <= 1e-15 * A and float(np.abs(std - lin_std)[ok].max()) <= 1e-15 * S
        assert np.array_equal(gold_std, std.astype(np.float64))
        assert np.allclose(gold_reg, reg.astype(np.float64), rtol=1e-12)
        r64, s64 = G.f64_two_pass(x, *params)
        assert np.allclose(s64, gold_std, rtol=1e-9, atol=1e-12)


def test_case_tables_reach_what_they_claim():
    """The thresholds the tables are built around, restated: K d at 1536 | 1537 and 4096 | 4097, every form, the row counts around 256,
    the groups around n m = 128, and rows that are what rows() says."""
    kd = {k * d: f for (k, d), f in G.FORMS.items()}
    assert kd[1536] == "r4" and kd[1537] == "r1" and kd[4096] == "r1" and kd[4097] == "wave"
    assert all((f == "r4") == (k * d <= 1536) and (f == "wave") == (k * d > 4096) for (k, d), f in G.FORMS.items())
    assert {255, 256} <= set(G.ROW_COUNTS) and sorted(m * n for m, n in G.GROUP_SIZES)[:6] == [124, 126, 126, 128, 128, 129]
    assert G.single_form(64, 24, 256) == ("wg", 4, 64, 4 * 1600 * 8) and G.single_form(64, 24, 255) == ("wg", 1, 255, 1600 * 8)
    assert G.group_forms("small", 2, 63) == [("multi", 1, 63, 2, 1064 * 8)] and G.group_forms("small", 2, 64) == [("multi", 4, 16, 2, 4 * 1064 * 8)]
    assert G.group_forms("mid", 4, 301) == [("multi", 1, 301, 4, 2064 * 8)] and [f[0] for f in G.group_forms("big", 3, 43)] == ["wg", "wave", "wg"]
    for K, d in ((10, 4), (65, 64)):
        c = G.case(K, d, 0.0)
        means, x = c.params[0], c.x["f64"][:, :d]
        dist = np.linalg.norm(x[:, None] - means[None], axis=2)
        assert x.shape == (16, d) and dist[12].min() == 0 and dist[14].min() >= 40 and not x[15].any()
        assert np.min(np.diff(np.sort(dist[13]))) <= 1e-12                              # two means at the same distance: their midpoint
        post_far = np.exp(-0.5 * dist[14].min() ** 2 * 0.5)
        assert post_far == 0.0 or post_far < 1e-170        # the largest density of the far row (smallest eigenvalue 1/2)
    assert G.case(1024, 64, 0.0).x["f64"].shape == (8, 69)


def _good():
    return list(G.classifier(3, 2, 1))


REFUSALS = {
    "K=0": (dict(K=0), "n_classes must be 1..1024"), "K=1025": (dict(K=1025), "n_classes must be 1..1024"),
    "d=0": (dict(d=0), "dim must be 1..64"), "d=65": (dict(d=65), "dim must be 1..64"),
    "means null": (dict(null=0), "null parameter array"), "inv_covs null": (dict(null=1), "null parameter array"),
    "sqrt_det null": (dict(null=2), "null parameter array"), "priors null": (dict(null=3), "null parameter array"),
    "avg null": (dict(null=4), "null parameter array"), "out null": (dict(out=False), "null output handle pointer"),
    "sqrt_det zero": (dict(poke=(2, 1, 0.0)), "class 1: non-positive sqrt-det or negative prior"),
    "sqrt_det negative": (dict(poke=(2, 2, -1.0)), "class 2: non-positive sqrt-det or negative prior"),
    "sqrt_det nan": (dict(poke=(2, 0, float("nan"))), "class 0: non-positive sqrt-det or negative prior"),
    "prior negative": (dict(poke=(3, 1, -1e-300)), "class 1: non-positive sqrt-det or negative prior"),
}


@pytest.mark.parametrize("name", list(REFUSALS))
def test_create_refuses_bad_arguments(native_lib, name):
    """Every argument check of hg_gauss_create runs before the device count is asked for (the class checks were moved there with this
    test): HG_ERR_ARG and the message, no handle, on a machine with or without a GPU."""
    how, text = REFUSALS[name]
    a = _good()
    if "null" in how:
        K, d = a[0].shape
        a[how["null"]] = None
        how = dict(K=K, d=d)
    if "poke" in how:
        i, c, v = how["poke"]
        a[i] = a[i].copy()
        a[i][c] = v
        how = {}
    rc, h = G.create(native_lib, *a, **how)
    assert rc == HG_ERR_ARG and h.value is None
    assert G.last_error(native_lib) == text
