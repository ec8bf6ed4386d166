"""fp64 NumPy/SciPy definition of the inducing-point GP (include/gpx.h, gpx_sparse_*; SparseGP): the collapsed variational
bound of Titsias 2009 ("SGPR").  With s_n^2 = sn2 w_n (w = 1 without weights), S = diag(s^2), yt = S^-1/2 y:

    Kuu = sf2 k(Z, Z) + jitter I      L  = chol(Kuu)                (m x m)
    A   = L^-1 sf2 k(Z, X) S^-1/2     B  = I + A A^T,  LB = chol(B)
    c   = LB^-1 A yt                  (m x k)
    ELBO_c = -N/2 log 2 pi - sum log LB_ii - 1/2 sum log s_n^2 - 1/2 |yt_c|^2 + 1/2 |c_c|^2 - 1/2 sum sf2 / s_n^2 + 1/2 tr(A A^T)
    predict: T1 = L^-1 sf2 k(Z, Xs), T2 = LB^-1 T1
             mean = T2^T c,  var = sf2 - colsumsq(T1) + colsumsq(T2),  cov = sf2 k(Xs, Xs) - T1^T T1 + T2^T T2

The order is part of the definition: A is whitened by L^-1 BEFORE the contraction over the N points (``SparseRef``).
``CheapOrder`` is the other order, Phi = K_uf S^-1 K_fu first and L^-1 Phi L^-T after it — half the N m^2 work, and it loses
the result (test_sparse_ref.py measures by how much); nothing else uses it.

Kernel distances come from coordinate DIFFERENCES, not from |a|^2 + |b|^2 - 2 a.b: the expansion leaves r ~ 1e-8 on
coincident points, which spoils the Z = X identities for Matern-1/2 (an ELBO error of 9e-5).  Shared by the CPU and GPU tests."""
import numpy as np
from scipy.linalg import cholesky, solve_triangular

LOG_2PI = float(np.log(2.0 * np.pi))
SQRT3, SQRT5 = np.sqrt(3.0), np.sqrt(5.0)
KERNELS = ("rbf", "matern52", "matern32", "matern12")


def kernel_matrix(A, B, kernel, ls, sf2, block=2048):
    """sf2 k(A, B), (na, nb), from coordinate differences of the scaled points (row blocks bound the temporaries)"""
    A, B = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
    l = np.broadcast_to(np.atleast_1d(np.asarray(ls, dtype=np.float64)), (A.shape[1],))
    As, Bs = A / l, B / l
    K = np.empty((len(A), len(B)))
    for i in range(0, len(A), block):
        D = As[i:i + block, None, :] - Bs[None, :, :]
        r2 = np.sum(D * D, axis=2)
        if kernel == "rbf":
            K[i:i + block] = np.exp(-0.5 * r2)
        elif kernel == "matern52":
            s = SQRT5 * np.sqrt(r2)
            K[i:i + block] = (1.0 + s + s * s / 3.0) * np.exp(-s)
        elif kernel == "matern32":
            s = SQRT3 * np.sqrt(r2)
            K[i:i + block] = (1.0 + s) * np.exp(-s)
        elif kernel == "matern12":
            K[i:i + block] = np.exp(-np.sqrt(r2))
        else:
            raise ValueError(f"sparse_ref: unknown kernel {kernel!r}")
    return sf2 * K


class SparseRef:
    """The model above with SciPy's Cholesky and triangular solves."""

    def __init__(self, kernel, ls, sf2, sn2, jitter):
        self.kernel, self.ls, self.sf2, self.sn2, self.jitter = kernel, ls, float(sf2), float(sn2), float(jitter)

    def _kuu_factor(self, Z):
        Kuu = kernel_matrix(Z, Z, self.kernel, self.ls, self.sf2)
        Kuu[np.diag_indices_from(Kuu)] += self.jitter
        return cholesky(Kuu, lower=True)

    def _whitened(self, X, s):
        """A = L^-1 K_uf S^-1/2 (m x N)"""
        Kuf = kernel_matrix(self.Z, X, self.kernel, self.ls, self.sf2)
        return solve_triangular(self.L, Kuf, lower=True) / s[None, :]

    def fit(self, X, y, Z, w=None):
        X, self.Z = np.asarray(X, dtype=np.float64), np.asarray(Z, dtype=np.float64)
        N, m = len(X), len(self.Z)
        self.y1d = np.ndim(y) == 1
        Y = np.asarray(y, dtype=np.float64).reshape(N, -1)
        s2 = self.sn2 * (np.ones(N) if w is None else np.asarray(w, dtype=np.float64))
        s = np.sqrt(s2)
        Yt = Y / s[:, None]
        self.L = self._kuu_factor(self.Z)
        A = self._whitened(X, s)
        AAt = A @ A.T
        self.LB = cholesky(np.eye(m) + AAt, lower=True)
        self.c = solve_triangular(self.LB, A @ Yt, lower=True)
        self.elbo = (-0.5 * N * LOG_2PI - np.sum(np.log(np.diag(self.LB))) - 0.5 * np.sum(np.log(s2))
                     - 0.5 * np.sum(Yt * Yt, axis=0) + 0.5 * np.sum(self.c * self.c, axis=0)
                     - 0.5 * np.sum(self.sf2 / s2) + 0.5 * np.trace(AAt))
        return self

    def _t12(self, Xs):
        T1 = solve_triangular(self.L, kernel_matrix(self.Z, Xs, self.kernel, self.ls, self.sf2), lower=True)
        return T1, solve_triangular(self.LB, T1, lower=True)

    def predict(self, Xs):
        """mean ((M,) for a 1-D y, else (M, k)) and the latent variance (M,)"""
        T1, T2 = self._t12(Xs)
        mean = T2.T @ self.c
        var = self.sf2 - np.sum(T1 * T1, axis=0) + np.sum(T2 * T2, axis=0)
        return (mean[:, 0] if self.y1d else mean), var

    def predict_cov(self, Xs):
        T1, T2 = self._t12(Xs)
        mean = T2.T @ self.c
        cov = kernel_matrix(Xs, Xs, self.kernel, self.ls, self.sf2) - T1.T @ T1 + T2.T @ T2
        return (mean[:, 0] if self.y1d else mean), cov


class CheapOrder(SparseRef):
    """The order the model must NOT be computed in: contract first, whiten the m x m result afterwards."""

    def fit(self, X, y, Z, w=None):
        X, self.Z = np.asarray(X, dtype=np.float64), np.asarray(Z, dtype=np.float64)
        N, m = len(X), len(self.Z)
        self.y1d = np.ndim(y) == 1
        Y = np.asarray(y, dtype=np.float64).reshape(N, -1)
        s2 = self.sn2 * (np.ones(N) if w is None else np.asarray(w, dtype=np.float64))
        Yt = Y / np.sqrt(s2)[:, None]
        self.L = self._kuu_factor(self.Z)
        Kuf = kernel_matrix(self.Z, X, self.kernel, self.ls, self.sf2) / np.sqrt(s2)[None, :]
        Phi = Kuf @ Kuf.T
        AAt = solve_triangular(self.L, solve_triangular(self.L, Phi, lower=True).T, lower=True)
        AAt = 0.5 * (AAt + AAt.T)
        self.LB = cholesky(np.eye(m) + AAt, lower=True)
        self.c = solve_triangular(self.LB, solve_triangular(self.L, Kuf @ Yt, lower=True), lower=True)
        self.elbo = (-0.5 * N * LOG_2PI - np.sum(np.log(np.diag(self.LB))) - 0.5 * np.sum(np.log(s2))
                     - 0.5 * np.sum(Yt * Yt, axis=0) + 0.5 * np.sum(self.c * self.c, axis=0)
                     - 0.5 * np.sum(self.sf2 / s2) + 0.5 * np.trace(AAt))
        return self


def exact_gp(X, y, Xs, kernel, ls, sf2, sn2, w=None):
    """The exact GP of the same data by the same kernel code: (mean, latent variance, LML summed over the targets)"""
    X = np.asarray(X, dtype=np.float64)
    N = len(X)
    Y = np.asarray(y, dtype=np.float64).reshape(N, -1)
    K = kernel_matrix(X, X, kernel, ls, sf2)
    K[np.diag_indices_from(K)] += sn2 * (np.ones(N) if w is None else np.asarray(w, dtype=np.float64))
    L = cholesky(K, lower=True)
    z = solve_triangular(L, Y, lower=True)
    V = solve_triangular(L, kernel_matrix(X, Xs, kernel, ls, sf2), lower=True)
    mean = V.T @ z
    lml = float(-0.5 * np.sum(z * z) - Y.shape[1] * np.sum(np.log(np.diag(L))) - 0.5 * N * Y.shape[1] * LOG_2PI)
    return (mean[:, 0] if np.ndim(y) == 1 else mean), sf2 - np.sum(V * V, axis=0), lml


def path_grid_problem(P, steps, seed, noise=0.05):
    """P paths on a shared grid of `steps` times in [0, 1]: X (P steps, 1) path-major, y (P steps, 2), the grid (steps, 1)"""
    rng = np.random.default_rng(seed)
    t = np.linspace(0.0, 1.0, steps)
    X = np.tile(t, P).reshape(-1, 1)
    base = np.stack([np.sin(2.0 * np.pi * t), np.cos(1.5 * np.pi * t) * t], axis=1)
    y = np.tile(base, (P, 1)) + noise * rng.standard_normal((P * steps, 2))
    return X, y, t.reshape(-1, 1)


def problem(N, d, M, k, seed, weighted):
    """seeded inputs in [0, 1]^d, k smooth targets with noise, query points, weights in [0.5, 2] (or None)"""
    rng = np.random.default_rng(seed)
    X = rng.uniform(0.0, 1.0, (N, d))
    Xs = rng.uniform(0.0, 1.0, (M, d))
    ph = rng.uniform(0.0, 2.0 * np.pi, (k,))
    y = np.sin(2.0 * np.pi * X[:, :1] + ph[None, :]) + 0.5 * np.cos(3.0 * X.sum(axis=1))[:, None] + 0.1 * rng.standard_normal((N, k))
    w = rng.uniform(0.5, 2.0, N) if weighted else None
    return X, (y[:, 0] if k == 1 else y), Xs, w


# The parity cases of tests/test_sparse_gpu.py (and the ELBO <= LML cases of tests/test_sparse_ref.py).  Every value of
# every axis appears: m in {1, 63, 64, 130, 257}, N in {1, 130, 512, 700, 2100}, chunk in {256, 0} (N = 700: three chunks,
# the last with 188 rows; N = 512: two full ones; N = 130: one partial), d in {1, 3, 5}, scalar and ARD lengthscales,
# k in {1, 2, 8}, with and without weights, four families, jitter 1e-6 and, for one RBF case, 1e-8.
CASES = [
    dict(id="rbf-d1-N700-m130", kernel="rbf", N=700, d=1, m=130, k=1, ard=False, weighted=False, chunk=256, jitter=1e-6),
    dict(id="rbf-d1-N2100-m257-j1e-8", kernel="rbf", N=2100, d=1, m=257, k=2, ard=False, weighted=True, chunk=0, jitter=1e-8),
    dict(id="m52-d3-N512-m64-k8", kernel="matern52", N=512, d=3, m=64, k=8, ard=True, weighted=True, chunk=256, jitter=1e-6),
    dict(id="m32-d5-N130-m63", kernel="matern32", N=130, d=5, m=63, k=1, ard=True, weighted=False, chunk=256, jitter=1e-6),
    dict(id="m12-d3-N1-m1", kernel="matern12", N=1, d=3, m=1, k=2, ard=False, weighted=False, chunk=0, jitter=1e-6),
    dict(id="m12-d1-N700-m257", kernel="matern12", N=700, d=1, m=257, k=1, ard=False, weighted=True, chunk=0, jitter=1e-6),
    dict(id="m52-d3-N2100-m130", kernel="matern52", N=2100, d=3, m=130, k=1, ard=False, weighted=False, chunk=256, jitter=1e-6),
    dict(id="rbf-d5-N512-m63", kernel="rbf", N=512, d=5, m=63, k=2, ard=True, weighted=True, chunk=0, jitter=1e-6),
]
SF2, SN2 = 1.3, 0.04


def case_data(case, seed=0):
    """-> dict(X, y, Xs, w, Z, ls) of a case: seeded; Z equally spaced for d = 1, uniform points otherwise"""
    d, m = case["d"], case["m"]
    X, y, Xs, w = problem(case["N"], d, 96, case["k"], 1000 + seed + 17 * CASES.index(case), case["weighted"])
    rng = np.random.default_rng(77 + seed)
    Z = np.linspace(0.0, 1.0, m).reshape(m, 1) if d == 1 and m > 1 else rng.uniform(0.0, 1.0, (m, d))
    base = 0.3 if d == 1 else 0.6
    ls = base * (1.0 + 0.25 * np.arange(d)) if case["ard"] else base
    return dict(X=X, y=y, Xs=Xs, w=w, Z=Z, ls=ls)
