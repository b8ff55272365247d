"""No GPU: the argument checks of hg_sfa_train_layer / hg_pca_train_layer / hg_train_apply_device run before the device is looked
for, so each refusal below is HG_ERR_ARG with a text in hg_last_error on any machine.  Plus the reference of
tests/train_cases.py against itself: what the GPU tests lean on."""
import ctypes as C

import numpy as np
import pytest

from tests import train_cases as T

HG_ERR_ARG = -1
U8, F64 = 0, 2


def _vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _train_args(**over):
    d = over.get("d", 4)
    x = np.zeros((8, 8), dtype=np.float64)
    a = dict(x=x, on_host=1, dtype=F64, n=8, ldx=8, conn=np.zeros((1, max(1, min(d, 128))), dtype=np.int32), n_nodes=1, d=d,
             evals=np.zeros(200), evecs=np.zeros(200 * 200), mean=np.zeros(200))
    a.update(over)
    return a


TRAIN_REFUSALS = {
    "n=2": dict(n=2), "d=0": dict(d=0), "d=129": dict(d=129), "dtype=3": dict(dtype=3), "dtype=-1": dict(dtype=-1),
    "x null": dict(x=None), "conn null": dict(conn=None), "evals null": dict(evals=None), "evecs null": dict(evecs=None),
    "mean null": dict(mean=None), "no nodes": dict(n_nodes=0),
}


@pytest.mark.parametrize("entry", ["hg_sfa_train_layer", "hg_pca_train_layer"])
@pytest.mark.parametrize("case", list(TRAIN_REFUSALS))
def test_train_layer_refuses_bad_arguments(native_lib, entry, case):
    a = _train_args(**TRAIN_REFUSALS[case])
    rc = getattr(native_lib, entry)(_vp(a["x"]), a["on_host"], a["dtype"], a["n"], a["ldx"], _vp(a["conn"]), a["n_nodes"], a["d"], 0,
                                    _vp(a["evals"]), _vp(a["evecs"]), _vp(a["mean"]), None)
    assert rc == HG_ERR_ARG
    assert native_lib.hg_last_error().decode().strip()


def _apply_args(**over):
    # 2 nodes x 3 inputs -> p = 2, two functions: width 8.  The "device" pointers are never dereferenced: the checks come first.
    a = dict(x=np.zeros((4, 6)), dtype=F64, n=4, ldx=6, conn=np.arange(6, dtype=np.int32).reshape(2, 3), n_nodes=2, d=3, mean=np.zeros((2, 3)),
             w=np.zeros((2, 3, 2)), p=2, n_funcs=2, kinds=np.array([0, 1] + [0] * 7, dtype=np.int32), expos=np.array([1.0, 0.8] + [1.0] * 7),
             out=np.zeros((4, 8)), ldo=8)
    a.update(over)
    return a


APPLY_REFUSALS = {
    "ldo one short": dict(ldo=7), "ldo one short, no function": dict(n_funcs=0, kinds=None, expos=None, ldo=3), "n_funcs=9": dict(n_funcs=9, ldo=100),
    "n_funcs=-1": dict(n_funcs=-1), "kind 3": dict(kinds=np.array([0, 3], dtype=np.int32)), "kind -1": dict(kinds=np.array([-1, 0], dtype=np.int32)),
    "abs power without exponents": dict(expos=None), "signed power without exponents": dict(kinds=np.array([0, 2], dtype=np.int32), expos=None),
    "functions without kinds": dict(kinds=None), "dtype=3": dict(dtype=3), "n=0": dict(n=0), "d=0": dict(d=0), "p=0": dict(p=0), "no nodes": dict(n_nodes=0),
    "x null": dict(x=None), "conn null": dict(conn=None), "mean null": dict(mean=None), "w null": dict(w=None), "out null": dict(out=None),
}


@pytest.mark.parametrize("case", list(APPLY_REFUSALS))
def test_train_apply_refuses_bad_arguments(native_lib, case):
    a = _apply_args(**APPLY_REFUSALS[case])
    rc = native_lib.hg_train_apply_device(_vp(a["x"]), a["dtype"], a["n"], a["ldx"], _vp(a["conn"]), a["n_nodes"], a["d"], _vp(a["mean"]), _vp(a["w"]),
                                          a["p"], a["n_funcs"], _vp(a["kinds"]), _vp(a["expos"]), _vp(a["out"]), a["ldo"], 0)
    assert rc == HG_ERR_ARG
    assert native_lib.hg_last_error().decode().strip()
    assert not a["out"].any() if a["out"] is not None else True


def test_reference_agrees_with_numpy_and_sees_a_dropped_difference():
    """stats_ref against np.cov and the definition; a float64 restatement's noise is orders below the cap, and the signal of one
    dropped difference orders above it: the margin the tolerance rule stands on."""
    x, conn, ref = T.walk_case(16, 3000, "u8")
    xk = x[:, conn[1]].astype(np.float64)
    m_r, b_r, a_r, noise = ref[1]
    assert T.rel_err(np.cov(xk.T), b_r) < 1e-12 and T.rel_err(xk.mean(axis=0), m_r) < 1e-14
    dx = np.diff(xk, axis=0)
    assert T.rel_err(dx.T @ dx / 2999, a_r) < 1e-13
    assert noise["sfa"] is not None and max(noise.values()) < 1e-12 and T.tolerance(max(noise.values())) <= T.CAP
    dropped = np.delete(dx, 64, axis=0)
    assert T.rel_err(dropped.T @ dropped / 2999, a_r) > 1e-5 > 1e3 * T.CAP


def test_constructed_spectra_are_what_they_claim():
    for d, s in T.SPECTRUM_CASES:
        x = T.spectrum_input(d, s)
        w = np.linalg.eigvalsh(T.stats_ref(x, T.block_conn(1, d))[0][1].astype(np.float64))
        if s == "singular":
            assert x.shape[0] == d - 2 and np.abs(w[:3]).max() < 1e-12 * w[-1]
        elif s == "graded":
            assert abs(w[0] / 1e-6 - 1) < 1e-3 and (d == 1 or abs(w[-1] / 1e6 - 1) < 1e-9)
        elif s in ("equal", "clusters"):
            assert np.abs(w - 1).max() < 2e-9
    for d in T.SFA_CLUSTER_WIDTHS:
        import scipy.linalg
        x, tau = T.sfa_cluster_input(d)
        _, b, a = (m.astype(np.float64) for m in T.stats_ref(x, T.block_conn(1, d))[0])
        w = scipy.linalg.eigh(a, b, eigvals_only=True)
        assert np.linalg.cond(b) < 10 and np.abs(w[:d // 2] / tau - 1).max() < 1e-12 and np.abs(w[d // 2:] / tau - 1 - 1e-9).max() < 1e-12


def test_apply_reference_layout_and_bound():
    """apply_ref against a float64 restatement written the slow way: layout node-major, then function, then component."""
    rng = np.random.default_rng(0)
    x = rng.integers(0, 256, size=(5, 9)).astype(np.uint8)
    conn = np.array([[8, 0, 3], [2, 7, 1]], dtype=np.int32)
    mean, w = rng.normal(size=(2, 3)) + 128, rng.normal(size=(2, 3, 2))
    funcs = T.APPLY_FUNCS["sgn08_sq_id"]
    ref, bound = T.apply_ref(x, conn, mean, w, funcs)
    assert ref.shape == (5, 12) and np.all(bound > 0)
    for t in range(5):
        for k in range(2):
            z = (x[t, conn[k]].astype(np.float64) - mean[k]) @ w[k]
            want = np.concatenate([np.sign(z) * np.abs(z) ** 0.8, np.abs(z) ** 2.0, z])
            got = ref[t, k * 6:(k + 1) * 6].astype(np.float64)
            assert np.all(np.abs(got - want) <= bound[t, k * 6:(k + 1) * 6] + 1e-300)
