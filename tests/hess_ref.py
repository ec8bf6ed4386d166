"""fp64 reference of the posterior second derivatives (include/gpx.h, gpx_predict_hess): the closed forms of the kernel's
second and third derivatives, with SciPy's Cholesky and triangular solves.  With u = (x* - x) / l per dimension and
v, g, h, p of the family (csrc/gpx_cov.h),

    d^2 k / d x*_i d x*_j        = (h u_i u_j - g delta_ij) / (l_i l_j)
    d^3 k / d x*_i d x*_j d x_c  = (p u_i u_j u_c - h (delta_ic u_j + delta_jc u_i + delta_ij u_c)) / (l_i l_j l_c)
    Var_prior[d_i d_j f]         = h(0) / (l_i^2 l_j^2)  (i != j),   3 h(0) / l_i^4  (i == j)

for the twice differentiable families, RBF (g = h = p = v, h(0) = sf2) and Matern-5/2 (h(0) = 25 sf2 / 3).  The pairs
(i, j), i <= j, are numbered row-major.  Variants for fits with derivative rows (on tests/dobs_ref.py) and with path ids
(on tests/within_predict_ref.py).  Shared by the CPU and GPU tests."""
import os
import sys

import numpy as np
from scipy.linalg import cholesky, solve_triangular

from oracle.gp_oracle import kernel_matrix

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from deriv_ref import lengthscales  # noqa: E402

H0 = {"rbf": 1.0, "matern52": 25.0 / 3.0}   # h(0) / sf2


def pairs(d):
    """the (i, j), i <= j, row-major: two index arrays of d (d + 1) / 2 entries"""
    return np.triu_indices(d)


def ghp(r2, kernel, sf2):
    """g, h, p of the family at squared scaled distances r2 (p u_i u_j u_c of Matern-5/2 -> 0 at r = 0: p = 0 there)"""
    if kernel == "rbf":
        v = sf2 * np.exp(-0.5 * r2)
        return v, v, v
    if kernel != "matern52":
        raise ValueError(f"{kernel} is not twice differentiable")
    s = np.sqrt(5.0 * r2)
    e = np.exp(-s)
    with np.errstate(divide="ignore", invalid="ignore"):
        p = np.where(s > 0, sf2 * (125.0 / 3.0) * e / s, 0.0)
    return sf2 * (5.0 / 3.0) * (1.0 + s) * e, sf2 * (25.0 / 3.0) * e, p


def _scaled(A, B, ls):
    A, B = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
    l = lengthscales(ls, A.shape[1])
    U = A[:, None, :] / l - B[None, :, :] / l                        # (na, nb, d)
    return U, l, np.sum(U * U, axis=2)


def kernel_hess(A, B, kernel, ls, sf2):
    """H (D2, na, nb)[(i, j)][a][b] = d^2 k(A_a, B_b) / d A_ai d A_aj"""
    U, l, r2 = _scaled(A, B, ls)
    g, h, _ = ghp(r2, kernel, sf2)
    return np.stack([(h * U[:, :, i] * U[:, :, j] - (g if i == j else 0.0)) / (l[i] * l[j]) for i, j in zip(*pairs(len(l)))])


def kernel_third(A, B, kinds, kernel, ls, sf2):
    """T (D2, na, nb)[(i, j)][a][b] = d^3 k(A_a, B_b) / d A_ai d A_aj d B_bc with c = kinds[b] (every entry >= 0)"""
    U, l, r2 = _scaled(A, B, ls)
    _, h, p = ghp(r2, kernel, sf2)
    c = np.asarray(kinds, dtype=np.int64)
    uc = np.take_along_axis(U, np.broadcast_to(c[None, :, None], U.shape[:2] + (1,)), axis=2)[:, :, 0]
    out = []
    for i, j in zip(*pairs(len(l))):
        ui, uj = U[:, :, i], U[:, :, j]
        s = (c == i)[None, :] * uj + (c == j)[None, :] * ui + (uc if i == j else 0.0)
        out.append((p * ui * uj * uc - h * s) / (l[i] * l[j] * l[c][None, :]))
    return np.stack(out)


def kinds_hess(A, B, kinds, kernel, ls, sf2):
    """(D2, na, nb): the second derivative by A_a of the covariance of f(A_a) with the observation b of kind kinds[b]
    (-1: a value, c >= 0: d f / d x_c)"""
    kinds = np.asarray(kinds, dtype=np.int64)
    return np.where((kinds >= 0)[None, None, :], kernel_third(A, B, np.maximum(kinds, 0), kernel, ls, sf2),
                    kernel_hess(A, B, kernel, ls, sf2))


def path_hess(A, ga, B, gb, kernel, ls, sf2, ls_path, sg2):
    """(D2, na, nb): the second derivative by A_a of ``within_ref.path_cov(A, ga, B, gb, ...)``"""
    H = kernel_hess(A, B, kernel, ls, sf2)
    ga, gb = np.asarray(ga), np.asarray(gb)
    same = (ga[:, None] == gb[None, :]) & (ga[:, None] >= 0)
    if sg2 > 0 and same.any():
        H = H + np.where(same[None, :, :], kernel_hess(A, B, kernel, ls_path, sg2), 0.0)
    return H


def prior_hess_var(kernel, ls, sf2, d):
    """Var[d_i d_j f] of the prior, (D2,)"""
    l = lengthscales(ls, d)
    i, j = pairs(d)
    return np.where(i == j, 3.0, 1.0) * H0[kernel] * sf2 / (l[i] ** 2 * l[j] ** 2)


def solved(L, z, H, prior):
    """hmean (M, D2, k) and hvar (M, D2) from the row blocks H (D2, M, N) and their priors ((D2,) or (M, D2))"""
    D2, M, _ = H.shape
    prior = np.broadcast_to(prior, (M, D2))
    hmean, hvar = np.empty((M, D2, z.shape[1])), np.empty((M, D2))
    for b in range(D2):
        V = solve_triangular(L, H[b].T, lower=True)
        hmean[:, b, :] = V.T @ z
        hvar[:, b] = prior[:, b] - np.einsum("nm,nm->m", V, V)
    return hmean, hvar


def hess_ref(X, y, Xs, kernel, ls, sf2, sn2, jitter, w=None):
    """hmean (M, D2, k) and the latent variance hvar (M, D2) of the posterior's second derivatives at Xs; w: noise weights"""
    X, Xs = np.asarray(X, dtype=np.float64), np.asarray(Xs, dtype=np.float64)
    K = kernel_matrix(X, X, kernel, ls, sf2)
    K[np.diag_indices_from(K)] += sn2 * (1.0 if w is None else np.asarray(w, dtype=np.float64)) + jitter
    L = cholesky(K, lower=True)
    z = solve_triangular(L, np.asarray(y, dtype=np.float64).reshape(len(X), -1), lower=True)
    return solved(L, z, kernel_hess(Xs, X, kernel, ls, sf2), prior_hess_var(kernel, ls, sf2, X.shape[1]))


def hess_ref_kinds(ref, Xs):
    """the same for a fitted ``dobs_ref.DobsGP`` (a fit with derivative rows)"""
    H = kinds_hess(Xs, ref.X, ref.kinds, ref.kernel, ref.ls, ref.sf2)
    return solved(ref.L, ref.z, H, prior_hess_var(ref.kernel, ref.ls, ref.sf2, ref.d))


def hess_ref_paths(fit, Xq, gq):
    """the same for a ``within_ref.fit_ref`` fit and query points with path ids gq (an int: the same for all): the second
    derivatives of f + g_p where gq >= 0, whose prior gains the formula in sg2 and l_path"""
    Xq = np.asarray(Xq, dtype=np.float64)
    M, d = Xq.shape
    gq = np.full(M, int(gq)) if np.ndim(gq) == 0 else np.asarray(gq)
    sg2 = fit["sg2"] if fit["grouped"] else 0.0
    H = path_hess(Xq, gq, fit["X"], fit["ids"], fit["kernel"], fit["ls"], fit["sf2"], fit["ls_path"], sg2)
    prior = prior_hess_var(fit["kernel"], fit["ls"], fit["sf2"], d)[None, :] + np.where(
        (gq >= 0)[:, None], prior_hess_var(fit["kernel"], fit["ls_path"], sg2, d)[None, :], 0.0)
    return solved(fit["L"], fit["z"], H, prior)


def expand(h, d):
    """(M, D2, ...) over the pairs -> the symmetric (M, d, d, ...)"""
    idx = np.zeros((d, d), dtype=np.int64)
    idx[pairs(d)] = np.arange(d * (d + 1) // 2)
    idx = np.maximum(idx, idx.T)
    return np.asarray(h)[:, idx.reshape(-1)].reshape((len(h), d, d) + np.shape(h)[2:])
