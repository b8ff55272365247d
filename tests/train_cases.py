"""Case tables, input builders and the long-double reference shared by tests/test_train_edges_gpu.py and
tests/test_train_host.py (the training kernels of csrc/hg_train.hip at their edges).

The reference (``stats_ref``, ``apply_ref``) restates k_sfa_finish / k_train_apply in ``np.longdouble`` per node from the input
exactly as given (uint8 and float32 values are exact in long double).  ``stats_f64`` is the plain float64 restatement — one-pass
sums — whose error against the reference is the noise of a correct float64 implementation of a case; ``tolerance`` turns that
noise into the bound the device result is held to.

Run as a module (``python -m tests.train_cases OUT.npz``) this file is the child process of the forced-solver test: the solver
route is read from the environment once per process."""
from __future__ import annotations

import ctypes as C
import functools
import sys

import numpy as np

SFA, PCA = 0, 1
EPS = float(np.finfo(np.float64).eps)
FACTOR, FLOOR, CAP = 1000.0, 1e-12, 1e-9       # device error <= FACTOR x float64 noise, at least FLOOR, never above CAP (relative)
COND_MAX = 1e4                                 # SFA mode is observed through B_ref W: only where cond(B) stays below this
DTYPES = {"u8": np.uint8, "f32": np.float32, "f64": np.float64}

# ---------------------------------------------------------------------------------------------------------------- case tables
MFMA_WIDTHS = (1, 2, 4, 15, 16)                                         # k_sfa_stats16
VECTOR_WIDTHS = (17, 63, 64, 65, 90, 91, 110, 111, 126, 127, 128)       # k_sfa_stats: pass edges 64|65, 90|91, 110|111; LDS limit 127, 128
TYPED_WIDTHS = (4, 16, 17, 65, 128)
WIDTH_CASES = [(d, "f64") for d in MFMA_WIDTHS + VECTOR_WIDTHS] + [(d, t) for d in TYPED_WIDTHS for t in ("u8", "f32")]
COUNT_EDGES = (3, 4, 5, 31, 32, 33, 63, 64, 65, 127, 128, 129, 511, 512, 513, 767, 768, 769)
COUNT_CASES = [(d, n, t) for d in (16, 20) for t in ("u8", "f32", "f64") for n in COUNT_EDGES]
NODE_COUNTS = (1, 2, 15, 16, 17, 33)
NODE_CASES = [(d, k, t) for d in (16, 9) for k in NODE_COUNTS for t in ("u8", "f64")]
SPECTRA = ("equal", "clusters", "graded", "diagonal", "singular")
SPECTRUM_CASES = [(d, s) for d in (1, 5, 16, 17, 40) for s in SPECTRA if not (d == 1 and s == "singular")]
SFA_CLUSTER_WIDTHS = (5, 16, 17, 40)
APPLY_SHAPES = ((1, 1, 1), (16, 3, 5), (120, 20, 2))                    # (d, p, n_nodes)
APPLY_FUNCS = {"none": [], "id": [(0, 1.0)], "id_abs08": [(0, 1.0), (1, 0.8)], "sgn08_sq_id": [(2, 0.8), (1, 2.0), (0, 1.0)]}
APPLY_N = 37
# what each forced-solver child runs (all d <= 16, both modes where SFA is legal): (kind, args)
FORCED_CASES = [("walk", (4, 200, "u8")), ("walk", (16, 65, "f64")), ("walk", (15, 165, "f32")), ("walk", (1, 151, "f64")),
                ("spectrum", (16, "clusters")), ("spectrum", (5, "graded")), ("sfa_clusters", (16,))]


# -------------------------------------------------------------------------------------------------------------------- inputs
def walk(n, ncols, kind, seed):
    """Random walk plus noise (so that the difference covariance is not the covariance) around a large mean: uint8 around 128,
    the float types the same signal unrounded."""
    rng = np.random.default_rng(seed)
    w = rng.normal(size=(n, ncols)).cumsum(axis=0)
    w = (w - w.mean(axis=0)) / np.maximum(w.std(axis=0), 1e-30)
    x = 128.0 + 20.0 * w + 30.0 * rng.normal(size=(n, ncols))
    if kind == "u8":
        return np.clip(np.rint(x), 0, 255).astype(np.uint8)
    return np.ascontiguousarray(x.astype(DTYPES[kind]))


def block_conn(n_nodes, d):
    return np.arange(n_nodes * d, dtype=np.int32).reshape(n_nodes, d)


def scattered_conn(n_nodes, d, ldx, pool, seed):
    """Seeded random columns out of ``ldx``: unsorted within a node, and — drawn from a pool of ``pool`` columns — shared between
    the nodes of a chunk of 16."""
    rng = np.random.default_rng(seed)
    cols = rng.choice(ldx, size=pool, replace=False)
    conn = np.stack([rng.choice(cols, size=d, replace=False) for _ in range(n_nodes)]).astype(np.int32)
    assert len(np.unique(conn[:min(16, n_nodes)])) < min(16, n_nodes) * d and np.any(np.diff(conn, axis=1) < 0)
    return conn


def _orthonormal_centred(n, d, rng):
    q, _ = np.linalg.qr(rng.normal(size=(n, d)))
    q, _ = np.linalg.qr(q - q.mean(axis=0))
    return q


def spectrum_input(d, spectrum, seed=0):
    """x (float64) whose covariance has a chosen spectrum: x = q sqrt(lambda (n-1)) U' with centred orthonormal q."""
    rng = np.random.default_rng([seed, d, SPECTRA.index(spectrum)])
    if spectrum == "singular":                  # fewer samples than inputs: rank n - 1
        n = d - 2
        return np.ascontiguousarray(rng.normal(size=(n, d)) * np.linspace(0.5, 2.0, d))
    n = 3 * d + 20
    lam = {"equal": np.ones(d), "clusters": np.where(np.arange(d) < d // 2, 1.0, 1.0 + 1e-9), "graded": np.logspace(-6, 6, d),
           "diagonal": np.linspace(1.0, 2.0, d)}[spectrum]
    u = np.eye(d) if spectrum == "diagonal" else np.linalg.qr(rng.normal(size=(d, d)))[0]
    return np.ascontiguousarray(_orthonormal_centred(n, d, rng) * np.sqrt(lam * (n - 1)) @ u.T)


def sfa_cluster_input(d, n=400, seed=0):
    """x with a well-conditioned covariance whose generalized eigenvalues form two clusters, tau and tau (1 + 1e-9).  The
    DCT-II vectors c_k diagonalise D'D (D: first difference) with eigenvalues mu_k = 2 - 2 cos(pi k / n) and are centred; a unit
    combination a c_k + b c_m has the Rayleigh quotient a^2 mu_k + b^2 mu_m, and combinations of disjoint pairs are orthogonal
    in both forms.  So every column gets its own pair and the weights that hit its target; a mixing matrix of condition ~10 and
    a mean leave the generalized eigenvalues alone."""
    rng = np.random.default_rng([seed, d, n])
    t = np.arange(n) + 0.5
    mu = lambda k: 2.0 - 2.0 * np.cos(np.pi * k / n)
    tau = mu(n / 4.0)
    q = np.empty((n, d))
    for j in range(d):
        k, m = 1 + j, n - 1 - j                                      # mu_k < tau < mu_m
        target = tau if j < d // 2 else tau * (1.0 + 1e-9)
        a2 = (mu(m) - target) / (mu(m) - mu(k))
        q[:, j] = (np.sqrt(a2) * np.cos(np.pi * k * t / n) + np.sqrt(1.0 - a2) * np.cos(np.pi * m * t / n)) * np.sqrt(2.0 / n)
    u1, u2 = np.linalg.qr(rng.normal(size=(d, d)))[0], np.linalg.qr(rng.normal(size=(d, d)))[0]
    mix = u1 * np.linspace(1.0, 3.0, d) @ u2.T
    return np.ascontiguousarray(q * np.sqrt(n - 1.0) @ mix + 3.0), tau


# ----------------------------------------------------------------------------------------------------------------- reference
def stats_ref(x, conn):
    """Per node k: mean, B = Cov(x[:, conn[k]]) (two-pass, / (n-1)) and A = sum dx dx' / (n-1) (not mean-centred), long double."""
    n = x.shape[0]
    out = []
    for cols in np.asarray(conn):
        xk = x[:, cols].astype(np.longdouble)
        mean = xk.sum(axis=0) / n
        c = xk - mean
        dx = xk[1:] - xk[:-1]
        out.append((mean, c.T @ c / (n - 1), dx.T @ dx / (n - 1)))
    return out


def stats_f64(x, conn):
    """The same in plain float64 with numpy's one-pass sums: what a correct float64 implementation gives."""
    n = x.shape[0]
    out = []
    for cols in np.asarray(conn):
        xk = x[:, cols].astype(np.float64)
        s = xk.sum(axis=0)
        dx = xk[1:] - xk[:-1]
        out.append((s / n, (xk.T @ xk - np.outer(s, s) / n) / (n - 1), dx.T @ dx / (n - 1)))
    return out


def apply_ref(x, conn, mean, w, funcs):
    """out[t, node * width + f * p + j] = func_f(((x[t, conn[node]] - mean[node]) W[node])_j) in long double, and the derived bound
    per element: 2 d eps (|x - mean| @ |W|) for the chain of fused multiply-adds, pushed through the function (times
    e |z|^(e-1) where z != 0), plus 8 eps |value| for pow."""
    n_nodes, d = conn.shape
    p = w.shape[2]
    nf = max(1, len(funcs))
    ref = np.empty((x.shape[0], n_nodes * nf * p), dtype=np.longdouble)
    bound = np.empty(ref.shape)
    for k in range(n_nodes):
        c = x[:, conn[k]].astype(np.longdouble) - mean[k].astype(np.longdouble)
        z = c @ w[k].astype(np.longdouble)
        dz = 2.0 * d * EPS * (np.abs(c).astype(np.float64) @ np.abs(w[k]))
        for f, (kind, expo) in enumerate(funcs or [(0, 1.0)]):
            sl = slice((k * nf + f) * p, (k * nf + f + 1) * p)
            if kind == 0:
                ref[:, sl], bound[:, sl] = z, dz
                continue
            az = np.abs(z)
            v = np.power(az, np.longdouble(expo))
            slope = np.zeros(z.shape)
            nz = az > 0
            slope[nz] = (expo * np.power(az[nz], np.longdouble(expo - 1.0))).astype(np.float64)
            ref[:, sl] = v if kind == 1 else np.copysign(v, z)
            bound[:, sl] = dz * slope + 8.0 * EPS * v.astype(np.float64)
    return ref, bound


def rel_err(got, ref):
    """max |got - ref| / max |ref| (long double difference, float result)."""
    ref = np.asarray(ref, dtype=np.longdouble)
    scale = float(np.abs(ref).max())
    return float(np.abs(np.asarray(got, dtype=np.longdouble) - ref).max()) / (scale if scale > 0 else 1.0)


def tolerance(noise):
    """The bound for a device result from the float64 noise of its case; a case whose noise needs more than CAP is a bad case."""
    assert FACTOR * noise <= CAP, "case too ill-conditioned for its reference: float64 noise %.2e" % noise
    return max(FLOOR, FACTOR * noise)


def recon_pca(evals, evecs):
    """B from what PCA mode returns: V diag(lambda) V'."""
    return (evecs * evals) @ evecs.T


def recon_sfa(evals, evecs, b_ref):
    """A from what SFA mode returns: W' B W = I, so A = (B W) diag(lambda) (B W)'."""
    bw = np.asarray(b_ref, dtype=np.float64) @ evecs
    return (bw * evals) @ bw.T


def sfa_legal(n, d):
    """SFA mode is run wherever n >= d + 20 (PCA mode everywhere: n <= d is legal there)."""
    return n >= d + 20


@functools.lru_cache(maxsize=None)
def walk_case(d, n, kind, n_nodes=2, seed=0):
    """A block layer on a walk, its reference and its float64 noise, computed once per case and shared (read-only)."""
    x = walk(n, n_nodes * d, kind, seed + 1000 * d + n)
    conn = block_conn(n_nodes, d)
    x.setflags(write=False)
    return x, conn, layer_reference(x, conn)


def layer_reference(x, conn):
    """Per node: the reference statistics, and the float64 noise of mean, of B through PCA and of A through SFA (None where
    cond(B) is too large to observe A through B_ref W, or B is singular)."""
    import scipy.linalg
    out = []
    for (m_r, b_r, a_r), (m_f, b_f, a_f) in zip(stats_ref(x, conn), stats_f64(x, conn)):
        lam, vec = np.linalg.eigh(b_f)
        noise = {"mean": rel_err(m_f, m_r), "pca": rel_err(recon_pca(lam, vec), b_r), "sfa": None}
        ev = np.linalg.eigvalsh(b_r.astype(np.float64))
        if sfa_legal(x.shape[0], len(conn[0])) and ev[0] > 0 and ev[-1] / ev[0] < COND_MAX:
            lam2, w2 = scipy.linalg.eigh(a_f, b_f)
            noise["sfa"] = rel_err(recon_sfa(lam2, w2, b_r), a_r)
        out.append((m_r, b_r, a_r, noise))
    return out


# ---------------------------------------------------------------------------------------------------------------- the entries
def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def run_layer(mode, x, conn, n=None, ldx=None, dtype=None, on_host=1, device=0):
    """hg_sfa_train_layer (mode SFA) / hg_pca_train_layer (PCA) through the C ABI.  x: a numpy array (on_host=1) or a device
    pointer with n / ldx / dtype.  Returns (rc, evals (k, d), evecs (k, d, d) with evecs[k][:, i] the i-th vector, mean (k, d))."""
    from pyfaceanalysis_amd import _capi
    conn = np.ascontiguousarray(conn, dtype=np.int32)
    n_nodes, d = conn.shape
    if isinstance(x, np.ndarray):
        x = np.ascontiguousarray(x)
        n, ldx, dtype, ptr = x.shape[0], x.shape[1], x.dtype, x.ctypes.data
    else:
        ptr = int(x)
    evals, evecs_cm, mean = np.full((n_nodes, d), np.nan), np.full((n_nodes, d, d), np.nan), np.full((n_nodes, d), np.nan)
    fn = _capi.lib().hg_pca_train_layer if mode == PCA else _capi.lib().hg_sfa_train_layer
    rc = fn(C.c_void_p(ptr), int(on_host), _capi.np_dtype_code(dtype), int(n), int(ldx), _vp(conn), n_nodes, d, int(device), _vp(evals),
            _vp(evecs_cm), _vp(mean), None)
    return rc, evals, np.swapaxes(evecs_cm, 1, 2).copy(), mean


def last_error():
    from pyfaceanalysis_amd import _capi
    return _capi.lib().hg_last_error().decode("utf-8", "replace")


def forced_input(kind, args):
    if kind == "walk":
        d, n, t = args
        x, conn, _ = walk_case(d, n, t)
        return x, conn
    x = spectrum_input(*args) if kind == "spectrum" else sfa_cluster_input(*args)[0]
    return x, block_conn(1, x.shape[1])


def forced_modes(kind, args, x):
    if kind == "spectrum":
        return (PCA,)
    if kind == "sfa_clusters":
        return (SFA,)
    return (PCA, SFA) if sfa_legal(x.shape[0], x.shape[1]) else (PCA,)


def _child(out_path):
    res = {}
    for i, (kind, args) in enumerate(FORCED_CASES):
        x, conn = forced_input(kind, args)
        for mode in forced_modes(kind, args, x):
            rc, evals, evecs, mean = run_layer(mode, x, conn)
            if rc != 0:
                raise SystemExit("case %d mode %d: rc %d: %s" % (i, mode, rc, last_error()))
            res["%d_%d_evals" % (i, mode)], res["%d_%d_evecs" % (i, mode)], res["%d_%d_mean" % (i, mode)] = evals, evecs, mean
    np.savez(out_path, **res)


if __name__ == "__main__":
    _child(sys.argv[1])
