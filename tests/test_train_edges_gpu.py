"""GPU: the five kernels of csrc/hg_train.hip (k_sfa_stats16, k_sfa_stats, k_sfa_finish, k_sygv16, k_train_apply) and the two
rocSOLVER routes behind them, at the edges of their code, against the long-double reference of tests/train_cases.py.

The statistics have no entry of their own; they are observed through the public calls: B = V diag(lambda) V' from PCA mode (any
n >= 3, singular or not), A = (B_ref W) diag(lambda) (B_ref W)' from SFA mode (W' B W = I; where cond(B) < 1e4).  Tolerances are
not constants: per case the error of a plain float64 restatement (numpy one-pass sums, LAPACK eigh, the same reconstruction)
against the reference is the noise of a correct float64 implementation; the device may have 1000 times that, at least 1e-12 and
never more than 1e-9, of max|reference| (train_cases.tolerance).  An indexing or counting error moves a statistic by 1/n of its
size at least: 6e-5 at the largest n here.  Every node of every layer is checked.  Measured ratios: DESIGN.md §8,
profiles/r18_train_edges.txt."""
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.linalg

from tests import train_cases as T
from tests.train_cases import PCA, SFA

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HG_OK, HG_ERR_ARG, HG_ERR_STATE = 0, -1, -6


def _report(what, err, tol):
    print("%-28s err %.2e  tol %.2e  ratio %.3f" % (what, err, tol, err / tol))


def _check_layer(x, conn, ref, modes=(PCA, SFA), on_host=1, n=None, ldx=None, dtype=None, tag=""):
    """Run the layer in each mode and hold EVERY node to its reference.  Returns {mode: (evals, evecs, mean)}."""
    out = {}
    for mode in modes:
        rc, evals, evecs, mean = T.run_layer(mode, x, conn, n=n, ldx=ldx, dtype=dtype, on_host=on_host)
        assert rc == HG_OK, T.last_error()
        assert np.all(np.diff(evals, axis=1) >= 0)
        worst = {"mean": (0.0, 1.0), "stat": (0.0, 1.0)}
        for k, (m_r, b_r, a_r, noise) in enumerate(ref):
            key = "pca" if mode == PCA else "sfa"
            assert noise[key] is not None, "case unfit for SFA mode: cond(B) above %g at node %d" % (T.COND_MAX, k)
            got = T.recon_pca(evals[k], evecs[k]) if mode == PCA else T.recon_sfa(evals[k], evecs[k], b_r)
            e_stat, t_stat = T.rel_err(got, b_r if mode == PCA else a_r), T.tolerance(noise[key])
            e_mean, t_mean = T.rel_err(mean[k], m_r), T.tolerance(noise["mean"])
            if e_stat / t_stat >= worst["stat"][0] / worst["stat"][1]:
                worst["stat"] = (e_stat, t_stat)
            if e_mean / t_mean >= worst["mean"][0] / worst["mean"][1]:
                worst["mean"] = (e_mean, t_mean)
            assert e_mean <= t_mean, "node %d mean: %.3e > %.3e" % (k, e_mean, t_mean)
            assert e_stat <= t_stat, "node %d %s: %.3e > %.3e" % (k, "B (PCA)" if mode == PCA else "A (SFA)", e_stat, t_stat)
        _report("%s %s mean" % (tag, "pca" if mode == PCA else "sfa"), *worst["mean"])
        _report("%s %s %s" % (tag, "pca" if mode == PCA else "sfa", "B" if mode == PCA else "A"), *worst["stat"])
        out[mode] = (evals, evecs, mean)
    return out


# ------------------------------------------------------------------------------------------- 1. statistics at every kernel edge
@pytest.mark.parametrize("d,kind", T.WIDTH_CASES, ids=["d%d-%s" % c for c in T.WIDTH_CASES])
def test_stats_at_every_width(native_lib, d, kind):
    """Matrix-core kernel d = 1 ... 16, vector kernel at its pass edges (64|65, 90|91, 110|111), a three-pass node, the largest
    node (128: 16384 entries) and the raised LDS limit (127, 128): PCA mode on 200 samples, SFA mode on d + 150."""
    x, conn, ref = T.walk_case(d, 200, kind)
    _check_layer(x, conn, ref, (PCA,), tag="d%d %s n200" % (d, kind))
    x, conn, ref = T.walk_case(d, d + 150, kind)
    _check_layer(x, conn, ref, (SFA,), tag="d%d %s n%d" % (d, kind, d + 150))


@pytest.mark.parametrize("d,n,kind", T.COUNT_CASES, ids=["d%d-n%d-%s" % c for c in T.COUNT_CASES])
def test_stats_at_sample_count_edges(native_lib, d, n, kind):
    """n at the staging-chunk edges (32 rows for float64 on the matrix cores, 64 otherwise) and the split edges (n / 256): the
    difference that crosses a chunk or a split is fetched one row ahead.  Three nodes; PCA always, SFA wherever n >= d + 20."""
    x, conn, ref = T.walk_case(d, n, kind, 3)
    _check_layer(x, conn, ref, (PCA, SFA) if T.sfa_legal(n, d) else (PCA,), tag="d%d n%d %s" % (d, n, kind))


@pytest.mark.parametrize("d", [16, 20])
def test_stats_at_the_split_ceiling(native_lib, d):
    """n = 16385 with a single chunk (d = 16) or node (d = 20): 64 splits, the ceiling, of 257 rows (the last one 194)."""
    x, conn, ref = T.walk_case(d, 16385, "f64", 1)
    _check_layer(x, conn, ref, tag="d%d n16385" % d)


@pytest.mark.parametrize("d,n_nodes,kind", T.NODE_CASES, ids=["d%d-k%d-%s" % c for c in T.NODE_CASES])
def test_stats_with_ragged_node_counts(native_lib, d, n_nodes, kind):
    """16 nodes per workgroup and two per wave on the matrix-core kernel: layers of 1, 2, 15, 16, 17 and 33 nodes."""
    x, conn, ref = T.walk_case(d, 300, kind, n_nodes)
    _check_layer(x, conn, ref, tag="d%d k%d %s" % (d, n_nodes, kind))


def test_stats_with_overlapping_fields(native_lib):
    """4 x 4 fields at stride 2 on a 12 x 12 image: 25 nodes in two chunks, every interior column shared by four nodes."""
    from pyfaceanalysis_amd import nodes as N
    conn = N.Rectangular2dSwitchboard((12, 12), (4, 4), (2, 2), 1).connections.reshape(-1, 16)
    assert conn.shape == (25, 16)
    for kind in ("u8", "f64"):
        x = T.walk(300, 144, kind, 77)
        _check_layer(x, conn, T.layer_reference(x, conn), tag="overlap %s" % kind)


@pytest.mark.parametrize("d", [16, 20])
def test_stats_with_scattered_columns(native_lib, d):
    """conn a seeded random choice out of ldx = 1000 columns, unsorted within a node and shared between the nodes of a chunk —
    from a host array, and through a device pointer whose ldx (1000) is wider than any column used (< 600)."""
    import torch
    for kind in ("u8", "f64"):
        x = T.walk(300, 1000, kind, 78)
        conn = T.scattered_conn(33, d, 1000, 150, 5)
        ref = T.layer_reference(x, conn)
        host = _check_layer(x, conn, ref, tag="scattered d%d %s host" % (d, kind))
        conn_low = T.scattered_conn(33, d, 600, 150, 6)
        assert conn_low.max() < 600
        xd = torch.from_numpy(x).cuda()
        dev = _check_layer(xd.data_ptr(), conn_low, T.layer_reference(x, conn_low), n=300, ldx=1000, dtype=x.dtype, on_host=0,
                           tag="scattered d%d %s device" % (d, kind))
        again = _check_layer(xd.data_ptr(), conn, ref, n=300, ldx=1000, dtype=x.dtype, on_host=0, tag="scattered d%d %s device" % (d, kind))
        for mode in (PCA, SFA):         # host array and device pointer of the same data: the same bytes
            for a, b in zip(host[mode], again[mode]):
                assert a.tobytes() == b.tobytes()
        del dev


def test_results_are_deterministic(native_lib):
    """Fixed-order sums: two calls give the same bytes — evals, evecs and mean on the d <= 16 route, mean on every route."""
    for d, bits_of in ((16, (0, 1, 2)), (9, (0, 1, 2)), (20, (2,)), (128, (2,))):
        for kind in ("u8", "f64"):
            x, conn, _ = T.walk_case(d, 769, kind, 3 if d <= 20 else 1)
            for mode in (PCA, SFA):
                a, b = T.run_layer(mode, x, conn), T.run_layer(mode, x, conn)
                assert a[0] == HG_OK and b[0] == HG_OK, T.last_error()
                for i in bits_of:
                    assert a[1 + i].tobytes() == b[1 + i].tobytes(), (d, kind, mode, i)


# --------------------------------------------------------------------------------------------- 2. the solvers on hard spectra
def _pca_spectrum_errors(x, evals, evecs):
    """(eigenvalue error, residual, orthogonality) of a PCA result against the long-double covariance, and the same three for
    numpy's eigh on the float64 one-pass covariance: the noise."""
    d = x.shape[1]
    conn = T.block_conn(1, d)
    c = T.stats_ref(x, conn)[0][1].astype(np.float64)
    w = np.linalg.eigvalsh(c)
    nrm = np.abs(w).max()
    errs = lambda lam, v: (float(np.abs(lam - w).max() / nrm), float(np.abs(c @ v - v * lam).max() / nrm), float(np.abs(v.T @ v - np.eye(d)).max()))
    return errs(evals, evecs), errs(*np.linalg.eigh(T.stats_f64(x, conn)[0][1]))


def _assert_spectrum(tag, got, noise):
    for name, e, nz in zip(("eigenvalues", "residual", "orthogonality"), got, noise):
        tol = T.tolerance(nz)
        _report("%s %s" % (tag, name), e, tol)
        assert e <= tol, "%s %s: %.3e > %.3e" % (tag, name, e, tol)


@pytest.mark.parametrize("d,spectrum", T.SPECTRUM_CASES, ids=["d%d-%s" % c for c in T.SPECTRUM_CASES])
def test_pca_on_hard_spectra(native_lib, d, spectrum):
    """Repeated, clustered (1 | 1 + 1e-9), graded (1e-6 ... 1e6), already diagonal and singular (n = d - 2) covariances: d = 1, 5, 16
    on k_sygv16, d = 17, 40 on rocSOLVER.  Eigenvectors of a cluster are not unique, so: eigenvalues against eigvalsh of the
    long-double covariance relative to its norm, the residual C V - V diag(lambda), V' V - I, ascending order."""
    x = T.spectrum_input(d, spectrum)
    rc, evals, evecs, _ = T.run_layer(PCA, x, T.block_conn(1, d))
    assert rc == HG_OK, T.last_error()
    assert np.all(np.diff(evals[0]) >= 0)
    _assert_spectrum("pca d%d %s" % (d, spectrum), *_pca_spectrum_errors(x, evals[0], evecs[0]))


def _sfa_errors(x, evals, evecs):
    """(eigenvalue error, residual A W - B W diag(lambda), W' B W - I), each relative, and scipy's own on the float64 statistics."""
    d = x.shape[1]
    conn = T.block_conn(1, d)
    _, b, a = (m.astype(np.float64) for m in T.stats_ref(x, conn)[0])
    w_ref = scipy.linalg.eigh(a, b, eigvals_only=True)

    def errs(lam, w):
        bw = b @ w
        return (float(np.abs(lam - w_ref).max() / np.abs(w_ref).max()), float(np.abs(a @ w - bw * lam).max() / np.abs(a @ w).max()),
                float(np.abs(w.T @ bw - np.eye(d)).max()))
    _, bf, af = T.stats_f64(x, conn)[0]
    return errs(evals, evecs), errs(*scipy.linalg.eigh(af, bf))


@pytest.mark.parametrize("d", T.SFA_CLUSTER_WIDTHS)
def test_sfa_on_clustered_eigenvalues(native_lib, d):
    """A well-conditioned B (cond 9) with the generalized eigenvalues in two clusters tau | tau (1 + 1e-9)."""
    x, tau = T.sfa_cluster_input(d)
    rc, evals, evecs, _ = T.run_layer(SFA, x, T.block_conn(1, d))
    assert rc == HG_OK, T.last_error()
    assert np.all(np.diff(evals[0]) >= 0) and np.abs(evals[0] / tau - 1).max() < 2e-9
    _assert_spectrum("sfa d%d clusters" % d, *_sfa_errors(x, evals[0], evecs[0]))


_child_died = []


@pytest.mark.parametrize("var", ["HIGSFA_SYGVJ", "HIGSFA_SYGVD"])
def test_forced_rocsolver_routes(native_lib, tmp_path, var):
    """HIGSFA_SYGVJ=1 / HIGSFA_SYGVD=1 send nodes of <= 16 inputs to rocSOLVER.  The variable is read once per process, so each
    route runs in one fresh child; the parent holds its results to the same reference by the same bound, and to the own solver."""
    assert not _child_died, "not started: the child of %s died" % _child_died[0]
    out = str(tmp_path / "forced.npz")
    env = {k: v for k, v in os.environ.items() if k not in ("HIGSFA_SYGVJ", "HIGSFA_SYGVD")}
    env[var] = "1"
    try:
        r = subprocess.run([sys.executable, "-m", "tests.train_cases", out], cwd=ROOT, env=env, timeout=120, stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT)
    except subprocess.TimeoutExpired:
        _child_died.append(var)
        raise
    if r.returncode != 0:
        _child_died.append(var)
    assert r.returncode == 0, "child exit %d:\n%s" % (r.returncode, r.stdout.decode(errors="replace")[-2000:])
    res = np.load(out)
    for i, (kind, args) in enumerate(T.FORCED_CASES):
        x, conn = T.forced_input(kind, args)
        for mode in T.forced_modes(kind, args, x):
            evals, evecs, mean = (res["%d_%d_%s" % (i, mode, s)] for s in ("evals", "evecs", "mean"))
            rc, own_evals, own_evecs, own_mean = T.run_layer(mode, x, conn)
            assert rc == HG_OK, T.last_error()
            assert mean.tobytes() == own_mean.tobytes()
            tag = "%s %s %s" % (var[-5:], kind, args)
            if kind == "walk":
                ref = T.walk_case(*args)[2]
                for k, (m_r, b_r, a_r, noise) in enumerate(ref):
                    key, target = ("pca", b_r) if mode == PCA else ("sfa", a_r)
                    tol = T.tolerance(noise[key])
                    rec = lambda lam, v: T.recon_pca(lam, v) if mode == PCA else T.recon_sfa(lam, v, b_r)
                    e_ref, e_own = T.rel_err(rec(evals[k], evecs[k]), target), T.rel_err(rec(evals[k], evecs[k]), rec(own_evals[k], own_evecs[k]))
                    _report("%s %s node %d" % (tag, key, k), e_ref, tol)
                    assert e_ref <= tol and e_own <= tol, (tag, k, e_ref, e_own, tol)
            else:
                got, noise = (_pca_spectrum_errors if mode == PCA else _sfa_errors)(x, evals[0], evecs[0])
                _assert_spectrum(tag, got, noise)
                e_own = float(np.abs(evals - own_evals).max() / np.abs(own_evals).max())
                assert e_own <= T.tolerance(noise[0]), (tag, e_own)


# ------------------------------------------------------------------------------------- 3. hg_train_apply_device against apply_ref
def _apply_inputs(kind, d, p, n_nodes, seed=0):
    """x (37 rows; one row equal to the integer mean, so z = 0 there), a permuted conn over an ldx wider than needed, mean, W."""
    rng = np.random.default_rng([seed, d, p, n_nodes])
    ldx = n_nodes * d + 7
    conn = rng.permutation(ldx)[:n_nodes * d].reshape(n_nodes, d).astype(np.int32)
    mean = rng.integers(100, 151, size=(n_nodes, d)).astype(np.float64)
    x = rng.integers(0, 256, size=(T.APPLY_N, ldx)).astype(np.float64)
    if kind != "u8":
        x += rng.normal(size=x.shape)
    x = x.astype(T.DTYPES[kind])
    for k in range(n_nodes):
        x[5, conn[k]] = mean[k].astype(x.dtype)
    return np.ascontiguousarray(x), conn, mean, rng.normal(size=(n_nodes, d, p)) / np.sqrt(d)


def _run_apply(x, conn, mean, w, funcs, pad=3, sentinel=-7.25):
    import torch
    from pyfaceanalysis_amd.train import train_apply
    width = conn.shape[0] * max(1, len(funcs)) * w.shape[2]
    xd = torch.from_numpy(x).cuda()
    out = torch.full((x.shape[0], width + pad), sentinel, dtype=torch.float64, device="cuda")
    train_apply(xd.data_ptr(), x.dtype, x.shape[0], x.shape[1], conn, mean, w, funcs, out.data_ptr(), width + pad)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.all(got[:, width:] == sentinel), "padding columns of ldo written"
    return got[:, :width]


@pytest.mark.parametrize("funcs", list(T.APPLY_FUNCS))
@pytest.mark.parametrize("d,p,n_nodes", T.APPLY_SHAPES, ids=["d%d-p%d-k%d" % s for s in T.APPLY_SHAPES])
@pytest.mark.parametrize("kind", list(T.DTYPES))
def test_train_apply_against_reference(native_lib, kind, d, p, n_nodes, funcs):
    """uint8 / float32 / float64 input, no function, identity, [identity, |z|^0.8], [sgn|z|^0.8, |z|^2, identity], a work size
    (37 rows) that is no multiple of 256, p = 1, ldo = width + 3 with untouched padding, and one row with z exactly 0."""
    fl = T.APPLY_FUNCS[funcs]
    x, conn, mean, w = _apply_inputs(kind, d, p, n_nodes)
    got = _run_apply(x, conn, mean, w, fl)
    ref, bound = T.apply_ref(x, conn, mean, w, fl)
    assert got.shape == ref.shape
    err = np.abs(got.astype(np.longdouble) - ref).astype(np.float64)
    assert np.all(ref[5] == 0) and np.all(got[5] == 0)
    live = bound > 0
    print("apply %s d%d p%d k%d %s: worst err / bound %.3f" % (kind, d, p, n_nodes, funcs, float((err[live] / bound[live]).max()) if live.any() else 0.0))
    assert np.all(err <= bound), "worst err / bound %.3f at %s" % (float((err[live] / bound[live]).max()), np.unravel_index(np.argmax(err - bound), err.shape))


# --------------------------------------------------------------------------------------------------------------- 4. refusals
def _after_refusal_still_right():
    x, conn, ref = T.walk_case(16, 129, "u8", 3)
    _check_layer(x, conn, ref, tag="after a refusal")
    x, conn, ref = T.walk_case(20, 129, "u8", 3)
    _check_layer(x, conn, ref, tag="after a refusal")


@pytest.mark.parametrize("bad", [-1, "ldx"])
def test_connection_out_of_range_is_refused(native_lib, bad):
    import torch
    from pyfaceanalysis_amd import _capi
    x, conn, _ = T.walk_case(16, 129, "u8", 3)
    conn = conn.copy()
    conn[1, 7] = x.shape[1] if bad == "ldx" else bad
    for mode in (PCA, SFA):
        rc = T.run_layer(mode, x, conn)[0]
        assert rc == HG_ERR_ARG and "out of range" in T.last_error()
    xd = torch.from_numpy(x.copy()).cuda()
    out = torch.zeros((129, 3 * 2), dtype=torch.float64, device="cuda")
    vp = lambda a: a.ctypes.data_as(_capi.C.c_void_p)
    mean, w = np.zeros((3, 16)), np.ones((3, 16, 2))
    rc = native_lib.hg_train_apply_device(xd.data_ptr(), _capi.HG_U8, 129, x.shape[1], vp(conn), 3, 16, vp(mean), vp(w), 2, 0, None, None,
                                          out.data_ptr(), 6, 0)
    assert rc == HG_ERR_ARG and "out of range" in T.last_error()
    assert float(out.abs().max()) == 0.0
    _after_refusal_still_right()


@pytest.mark.parametrize("d", [16, 20])
@pytest.mark.parametrize("defect", ["constant", "twice"])
def test_singular_covariance_is_refused_by_sfa_and_taken_by_pca(native_lib, d, defect):
    """A constant input column, and a column listed twice in a node: SFA mode names the node in HG_ERR_STATE; PCA mode accepts the
    same input and meets the reconstruction bound; the next call is right."""
    x, conn, _ = T.walk_case(d, 129, "u8", 3)
    x, conn = x.copy(), conn.copy()
    if defect == "constant":
        x[:, conn[1, 4]] = 128
    else:
        conn[1, 9] = conn[1, 2]
    rc = T.run_layer(SFA, x, conn)[0]
    assert rc == HG_ERR_STATE and "node 1" in T.last_error(), (rc, T.last_error())
    _check_layer(x, conn, T.layer_reference(x, conn), (PCA,), tag="%s d%d" % (defect, d))
    _after_refusal_still_right()


@pytest.mark.parametrize("mode", [SFA, PCA])
def test_nan_input_is_reported(native_lib, mode):
    """A single NaN in a float32 input reaches every eigenvalue of its node: k_sygv16's ranking stays a permutation (NaN sorts
    last) and the call reports HG_ERR_STATE — a failed Cholesky in SFA mode, Jacobi sweeps that cannot converge in PCA mode."""
    x, conn, _ = T.walk_case(16, 129, "f32", 3)
    x = x.copy()
    x[40, conn[2, 3]] = np.nan
    rc = T.run_layer(mode, x, conn)[0]
    assert rc == HG_ERR_STATE and "node 2" in T.last_error(), (rc, T.last_error())
    _after_refusal_still_right()
