"""fp64 NumPy/SciPy reference of the GP with per-observation noise weights (include/gpx.h, gpx_set_noise_weights):

    K = sf2 k(X, X) + diag(sn2 w_i + jitter),    w_i >= 0 fixed data, sn2 the level that is learnt.

Dense fit (alpha, logdet, LML), predict (mean, latent variance), the LML gradient by R&W eq. 5.9 with
dK / dlog sn2 = sn2 diag(w), i.e. the noise entry 1/2 sn2 sum_i w_i (sum_c alpha_ic^2 - k (K^-1)_ii), and the weighted block
score S_g = K(X_g, X_g) - V_g^T V_g + diag_add diag(wq_g) built on tests/score_ref.py.  All four kernel families through
score_ref.kernel_matrix.  Shared by the CPU and GPU tests."""
import os
import sys

import numpy as np
from scipy.linalg import cho_solve, cholesky, solve_triangular

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import matern_ref  # noqa: E402
from score_ref import LOG_2PI, kernel_matrix  # noqa: E402

SQRT5 = np.sqrt(5.0)


def noise_diag(w, sn2, jitter):
    return sn2 * np.asarray(w, dtype=np.float64) + jitter


def kernel_dlog_ls(X, kernel, ls, sf2):
    """[dK / dlog l_c], one per entry of ls (a scalar ls: one matrix), each (N, N): kd(r) d_c^2 with d = u_i - u_j"""
    X = np.asarray(X, dtype=np.float64)
    l = matern_ref.lengthscales(ls, X.shape[1])
    D = X[:, None, :] / l - X[None, :, :] / l
    r2 = np.sum(D ** 2, axis=2)
    if kernel == "rbf":
        kd = sf2 * np.exp(-0.5 * r2)
    elif kernel == "matern52":
        s = SQRT5 * np.sqrt(r2)
        kd = sf2 * (5.0 / 3.0) * (1.0 + s) * np.exp(-s)
    else:
        kd = matern_ref.kd_factor(np.sqrt(r2), kernel, sf2)
    dl = [kd * D[:, :, c] ** 2 for c in range(X.shape[1])]
    return [sum(dl)] if np.atleast_1d(ls).size == 1 else dl


class HeteroGP:
    """Exact GP with SciPy's Cholesky and a noise weight per observation (w None: ones)."""

    def __init__(self, kernel, ls, sf2, sn2, jitter=0.0):
        self.kernel, self.ls, self.sf2, self.sn2, self.jitter = kernel, ls, float(sf2), float(sn2), float(jitter)

    def gram(self, X, w):
        K = kernel_matrix(X, X, self.kernel, self.ls, self.sf2)
        K[np.diag_indices_from(K)] += noise_diag(w, self.sn2, self.jitter)
        return K

    def fit(self, X, y, w=None):
        self.X = np.asarray(X, dtype=np.float64)
        self.y1d = np.ndim(y) == 1
        self.Y = np.asarray(y, dtype=np.float64).reshape(len(self.X), -1)
        self.w = np.ones(len(self.X)) if w is None else np.asarray(w, dtype=np.float64)
        self.L = cholesky(self.gram(self.X, self.w), lower=True)
        self.z = solve_triangular(self.L, self.Y, lower=True)
        self.alpha = solve_triangular(self.L, self.z, lower=True, trans="T")
        self.logdet = 2.0 * float(np.sum(np.log(np.diag(self.L))))
        return self

    @property
    def alpha_(self):
        return self.alpha[:, 0] if self.y1d else self.alpha

    def lml(self):
        n, k = self.Y.shape
        return float(-0.5 * np.sum(self.Y * self.alpha) - 0.5 * k * self.logdet - 0.5 * n * k * LOG_2PI)

    def predict(self, Xs):
        """mean ((M,) for a 1-D y, else (M, k)) and latent variance (M,)"""
        Ks = kernel_matrix(Xs, self.X, self.kernel, self.ls, self.sf2)
        V = solve_triangular(self.L, Ks.T, lower=True)
        mean = V.T @ self.z
        return (mean[:, 0] if self.y1d else mean), self.sf2 - np.einsum("nm,nm->m", V, V)

    def lml_gradient(self):
        """d LML / d log theta, theta = (lengthscales..., sf2, sn2), summed over the targets (R&W eq. 5.9)"""
        n, k = self.Y.shape
        W = self.alpha @ self.alpha.T - k * cho_solve((self.L, True), np.eye(n))
        g = [0.5 * np.sum(W * dK) for dK in kernel_dlog_ls(self.X, self.kernel, self.ls, self.sf2)]
        g.append(0.5 * np.sum(W * kernel_matrix(self.X, self.X, self.kernel, self.ls, self.sf2)))
        g.append(0.5 * self.sn2 * float(np.sum(self.w * np.diag(W))))
        return np.array(g)

    def score(self, Xq, Yq, Lg, diag_add, wq=None):
        """the weighted block score -> dict(logp (G, k), maha (G, k), logdet (G,), kappa (G,), dmin (G,)): dmin the
        smallest per-point diagonal value diag_add wq_i of the block"""
        Xq = np.asarray(Xq, dtype=np.float64)
        Yq = np.asarray(Yq, dtype=np.float64).reshape(len(Xq), -1)
        M, k = Yq.shape
        G = M // Lg
        wq = np.ones(M) if wq is None else np.asarray(wq, dtype=np.float64)
        Ks = kernel_matrix(Xq, self.X, self.kernel, self.ls, self.sf2)
        V = solve_triangular(self.L, Ks.T, lower=True)
        mean = V.T @ self.z
        out = {"logp": np.empty((G, k)), "maha": np.empty((G, k)), "logdet": np.empty(G), "kappa": np.empty(G),
               "dmin": np.empty(G)}
        for g in range(G):
            sl = slice(g * Lg, (g + 1) * Lg)
            S = kernel_matrix(Xq[sl], Xq[sl], self.kernel, self.ls, self.sf2) - V[:, sl].T @ V[:, sl]
            S = 0.5 * (S + S.T)
            S[np.diag_indices(Lg)] += diag_add * wq[sl]
            Ls = cholesky(S, lower=True)
            r = solve_triangular(Ls, Yq[sl] - mean[sl], lower=True)
            ev = np.linalg.eigvalsh(S)
            out["kappa"][g] = ev[-1] / ev[0]
            out["dmin"][g] = diag_add * wq[sl].min()
            out["maha"][g] = np.sum(r * r, axis=0)
            out["logdet"][g] = 2.0 * np.sum(np.log(np.diag(Ls)))
            out["logp"][g] = -0.5 * out["maha"][g] - 0.5 * out["logdet"][g] - 0.5 * Lg * LOG_2PI
        return out


# ---- the standard inputs of the fp64 tests -------------------------------------------------------------------------------
SF2, SN2, LS = 1.5, 1e-2, 0.3


def ard(d):
    """scalar 0.3 spread into d slightly different length scales"""
    return tuple(LS * (1.0 + 0.15 * (c - (d - 1) / 2.0)) for c in range(d))


def weights(N, seed, lo=0.1, hi=10.0, zeros=True):
    """log-uniform in [lo, hi]; every 97th weight 0 (an exact observation)"""
    rng = np.random.default_rng(seed)
    w = np.exp(rng.uniform(np.log(lo), np.log(hi), N))
    if zeros:
        w[::97] = 0.0
    return w


def problem(N, d, M, k, seed):
    """X uniform in [0, 1]^d, k smooth targets plus noise whose size follows the weights' model only loosely, M queries"""
    rng = np.random.default_rng(seed)
    X = rng.uniform(0.0, 1.0, (N, d))
    Xs = rng.uniform(-0.05, 1.05, (M, d))
    a = rng.uniform(2.0, 5.0, (d, k))

    def f(A):
        return np.sin(A @ a) + 0.3 * np.cos(2.0 * A.sum(axis=1, keepdims=True))

    Y = f(X) + 0.1 * rng.standard_normal((N, k))
    return X, (Y[:, 0] if k == 1 else Y), Xs
