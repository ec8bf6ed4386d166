"""fp64 reference of the posterior gradient (include/gpx.h, gpx_predict_grad): the closed forms of the kernel
derivatives, with SciPy's Cholesky and triangular solves.  Shared by the CPU and GPU tests."""
import numpy as np
from scipy.linalg import cholesky, solve_triangular

from oracle.gp_oracle import kernel_matrix


def lengthscales(ls, d):
    return np.broadcast_to(np.atleast_1d(np.asarray(ls, dtype=np.float64)), (d,)).copy()


def kernel_grad(A, B, kernel, ls, sf2):
    """G (d, na, nb)[j][a][b] = d k(A_a, B_b) / d A_aj"""
    A, B = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
    d = A.shape[1]
    l = lengthscales(ls, d)
    diffs = [A[:, j, None] / l[j] - B[None, :, j] / l[j] for j in range(d)]
    r2 = sum(e * e for e in diffs)
    if kernel == "rbf":
        g = sf2 * np.exp(-0.5 * r2)
    else:
        s = np.sqrt(5.0 * r2)
        g = sf2 * (5.0 / 3.0) * (1.0 + s) * np.exp(-s)
    return np.stack([-(g * diffs[j]) / l[j] for j in range(d)])


def prior_grad_var(kernel, ls, sf2, d):
    """Var[d f / d x_j] of the prior, (d,)"""
    return (1.0 if kernel == "rbf" else 5.0 / 3.0) * sf2 / lengthscales(ls, d) ** 2


def grad_ref(X, y, Xs, kernel, ls, sf2, sn2, jitter):
    """dmean (M, d, k) and the latent derivative variance dvar (M, d) of the posterior at Xs"""
    X, Xs = np.asarray(X, dtype=np.float64), np.asarray(Xs, dtype=np.float64)
    K = kernel_matrix(X, X, kernel, ls, sf2)
    K[np.diag_indices_from(K)] += sn2 + jitter
    L = cholesky(K, lower=True)
    z = solve_triangular(L, np.asarray(y, dtype=np.float64).reshape(len(X), -1), lower=True)
    G = kernel_grad(Xs, X, kernel, ls, sf2)
    d = X.shape[1]
    prior = prior_grad_var(kernel, ls, sf2, d)
    dmean = np.empty((len(Xs), d, z.shape[1]))
    dvar = np.empty((len(Xs), d))
    for j in range(d):
        V = solve_triangular(L, G[j].T, lower=True)
        dmean[:, j, :] = V.T @ z
        dvar[:, j] = prior[j] - np.einsum("nm,nm->m", V, V)
    return dmean, dvar
