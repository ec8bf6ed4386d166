"""Dense fp64 NumPy reference of predicting an observed path itself under the hierarchical model (include/gpx.h,
gpx_predict_paths and its three siblings): a query point x* comes with a path id p*,

    p* = -1:  value = f(x*)                     p* >= 0:  value = f(x*) + g_{p*}(x*)
    Cov[value(x*, p*), y_i]           = sf2 k(x*, x_i; l) + [p* == p_i >= 0] sg2 k(x*, x_i; l_path)
    Cov[value(x*, p*), value(x', p')] = sf2 k(x*, x'; l)  + [p* == p'  >= 0] sg2 k(x*, x'; l_path)

both lines being ``within_ref.path_cov``.  Built on ``within_ref.fit_ref``: mean, variance, joint covariance, and the gradient
of mean and variance with respect to x* from the analytic derivative of both terms (d k / d x*_j = -g (u*_j - u_j) / l_j with
u = x / l and g of the family's table in csrc/gpx_cov.h).  Shared by the CPU and GPU tests."""
import os
import sys

import numpy as np
from scipy.linalg import solve_triangular

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import within_ref as wr  # noqa: E402

GRAD_PRIOR = {"rbf": 1.0, "matern52": 5.0 / 3.0, "matern32": 3.0}   # dpoly(0): Var[d f / d x_j] = GRAD_PRIOR sf2 / l_j^2


def _query_ids(gq, M):
    gq = np.asarray(gq)
    return np.full(M, int(gq)) if gq.ndim == 0 else gq


def kernel_dx(A, B, kernel, ls, sf2):
    """(d, m, n): d / d A_aj of sf2 k(A_a, B_b; l) for the differentiable families"""
    A, B = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
    d = A.shape[1]
    l = wr._ls(ls, d)
    u = (A[:, None, :] - B[None, :, :]) / l                      # (m, n, d)
    r = np.sqrt(np.sum(u * u, axis=2))
    if kernel == "rbf":
        g = sf2 * np.exp(-0.5 * r * r)
    elif kernel == "matern52":
        s = np.sqrt(5.0) * r
        g = sf2 * (5.0 / 3.0) * (1.0 + s) * np.exp(-s)
    elif kernel == "matern32":
        g = 3.0 * sf2 * np.exp(-np.sqrt(3.0) * r)
    else:
        raise ValueError(f"{kernel} is not differentiable")
    return np.moveaxis(-g[:, :, None] * u / l, 2, 0)


def path_cov_dx(A, ga, B, gb, kernel, ls, sf2, ls_path, sg2):
    """(d, m, n): d / d A_aj of ``within_ref.path_cov(A, ga, B, gb, ...)``"""
    G = kernel_dx(A, B, kernel, ls, sf2)
    if ga is None or gb is None or not sg2 > 0:
        return G
    ga, gb = np.asarray(ga), np.asarray(gb)
    same = (ga[:, None] == gb[None, :]) & (ga[:, None] >= 0)
    if same.any():
        G = G + np.where(same[None, :, :], kernel_dx(A, B, kernel, ls_path, sg2), 0.0)
    return G


def predict_path(fit, Xq, gq):
    """posterior of value(x*, p*) at Xq with ids gq (an int: the same for all): mean (M, k), cov (M, M); var = diag(cov)"""
    Xq = np.asarray(Xq, dtype=np.float64)
    gq = _query_ids(gq, len(Xq))
    a = (fit["kernel"], fit["ls"], fit["sf2"], fit["ls_path"], fit["sg2"] if fit["grouped"] else 0.0)
    Ks = wr.path_cov(Xq, gq, fit["X"], fit["ids"], *a)
    V = solve_triangular(fit["L"], Ks.T, lower=True)
    cov = wr.path_cov(Xq, gq, Xq, gq, *a) - V.T @ V
    return V.T @ fit["z"], 0.5 * (cov + cov.T)


def grad_priors(fit, gq, d):
    """(M, d): the prior variance of d value / d x_j, c sf2 / l_j^2 + [p* >= 0] c sg2 / l_path,j^2"""
    c = GRAD_PRIOR[fit["kernel"]]
    pf = c * fit["sf2"] / wr._ls(fit["ls"], d) ** 2
    pg = c * (fit["sg2"] if fit["grouped"] else 0.0) / wr._ls(fit["ls_path"], d) ** 2
    return pf[None, :] + np.where(np.asarray(gq)[:, None] >= 0, pg[None, :], 0.0)


def predict_path_grad(fit, Xq, gq):
    """-> dmean (M, d, k), dvar (M, d): the gradient of the posterior mean with respect to x*, and the posterior variance of
    each partial derivative of the value (prior minus the squared norm of L^-1 d K*^T)"""
    Xq = np.asarray(Xq, dtype=np.float64)
    M, d = Xq.shape
    gq = _query_ids(gq, M)
    dK = path_cov_dx(Xq, gq, fit["X"], fit["ids"], fit["kernel"], fit["ls"], fit["sf2"], fit["ls_path"],
                     fit["sg2"] if fit["grouped"] else 0.0)
    prior = grad_priors(fit, gq, d)
    dmean, dvar = np.empty((M, d, fit["z"].shape[1])), np.empty((M, d))
    for j in range(d):
        V = solve_triangular(fit["L"], dK[j].T, lower=True)
        dmean[:, j, :] = V.T @ fit["z"]
        dvar[:, j] = prior[:, j] - np.sum(V * V, axis=0)
    return dmean, dvar
