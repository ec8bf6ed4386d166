"""fp64 NumPy/SciPy reference of gpx_score_blocks (include/gpx.h): the joint log predictive density of blocks of query
points under an exact GP.  K from ``oracle.gp_oracle.kernel_matrix`` (Matern-3/2 and Matern-1/2, which the oracle does not
know, from ``matern_ref``), the Cholesky of K, and per block S_g with its own Cholesky.  Also returns each block's 2-norm
condition number, which the error bounds of the tests are written in.  Shared by the CPU and GPU tests."""
import os
import sys

import numpy as np
from scipy.linalg import cholesky, solve_triangular

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import matern_ref  # noqa: E402
from oracle.gp_oracle import kernel_matrix as _oracle_kernel  # noqa: E402

LOG_2PI = float(np.log(2.0 * np.pi))


def kernel_matrix(A, B, kernel, ls, sf2):
    if kernel in matern_ref.KERNELS:
        return matern_ref.kernel_matrix(A, B, kernel, ls, sf2)
    return _oracle_kernel(A, B, kernel=kernel, lengthscale=ls, variance=sf2)


def kappa_bound(Lg, sf2, diag_add):
    """kappa_g <= (Lg sf2 + diag_add) / diag_add: the posterior covariance of a block is PSD (lambda_min(S_g) >= diag_add)
    and its trace is at most the prior's, Lg sf2 (lambda_max(S_g) <= Lg sf2 + diag_add)."""
    return (Lg * sf2 + diag_add) / diag_add


def score_ref(X, Y, Xq, Yq, Lg, kernel, ls, sf2, sn2, diag_add, jitter=0.0):
    """-> dict(logp (G, k), maha (G, k), logdet (G,), kappa (G,), mean (M, k), S (G, Lg, Lg))"""
    X, Xq = np.asarray(X, dtype=np.float64), np.asarray(Xq, dtype=np.float64)
    Y = np.asarray(Y, dtype=np.float64).reshape(len(X), -1)
    Yq = np.asarray(Yq, dtype=np.float64).reshape(len(Xq), -1)
    M, k = Yq.shape
    assert M % Lg == 0 and Y.shape[1] == k
    G = M // Lg
    K = kernel_matrix(X, X, kernel, ls, sf2)
    K[np.diag_indices_from(K)] += sn2 + jitter
    L = cholesky(K, lower=True)
    z = solve_triangular(L, Y, lower=True)
    Ks = kernel_matrix(Xq, X, kernel, ls, sf2)
    V = solve_triangular(L, Ks.T, lower=True)            # (N, M)
    mean = V.T @ z
    out = {"logp": np.empty((G, k)), "maha": np.empty((G, k)), "logdet": np.empty(G), "kappa": np.empty(G), "mean": mean,
           "S": np.empty((G, Lg, Lg))}
    for g in range(G):
        sl = slice(g * Lg, (g + 1) * Lg)
        S = kernel_matrix(Xq[sl], Xq[sl], kernel, ls, sf2) - V[:, sl].T @ V[:, sl]
        S = 0.5 * (S + S.T)
        S[np.diag_indices(Lg)] += diag_add
        Ls = cholesky(S, lower=True)
        w = solve_triangular(Ls, Yq[sl] - mean[sl], lower=True)
        ev = np.linalg.eigvalsh(S)
        out["S"][g] = S
        out["kappa"][g] = ev[-1] / ev[0]
        out["maha"][g] = np.sum(w * w, axis=0)
        out["logdet"][g] = 2.0 * np.sum(np.log(np.diag(Ls)))
        out["logp"][g] = -0.5 * out["maha"][g] - 0.5 * out["logdet"][g] - 0.5 * Lg * LOG_2PI
    return out


def problem(N, d, k, G, Lg, seed, box=10.0):
    """A seeded regression problem with G blocks of Lg query points: training inputs uniform in [0, box]^d, each block a
    short straight walk through [-1, box + 1]^d (some points outside the data), targets a smooth function plus noise."""
    rng = np.random.default_rng(seed)
    X = rng.uniform(0.0, box, (N, d))
    w = rng.uniform(0.5, 1.5, (d, k))

    def f(A):
        return np.sin(A @ w) + 0.3 * np.cos(0.7 * A.sum(axis=1, keepdims=True))

    Y = f(X) + 0.1 * rng.standard_normal((N, k))      # X, Y depend on (N, d, k, seed) only
    start = rng.uniform(-1.0, box + 1.0, (G, 1, d))
    step = rng.uniform(-0.12, 0.12, (G, 1, d))
    Xq = (start + step * np.arange(Lg)[None, :, None] + 0.01 * rng.standard_normal((G, Lg, d))).reshape(G * Lg, d)
    Yq = f(Xq) + 0.1 * rng.standard_normal((G * Lg, k))
    return X, Y, Xq, Yq
