"""fp64 NumPy definition of the gradient of the inducing-point bound (include/gpx.h, gpx_sparse_elbo_grad;
SparseGP.elbo_gradient), on top of tests/sparse_ref.py.  F = SparseRef(...).elbo.sum() over the k target columns; the
gradient is with respect to the LOG parameters in gpx_lml_grad's order: n_ls lengthscales, sf2, sn2.

With the notation of sparse_ref (A = L^-1 Kuf S^-1/2 with columns a_n, B = I + A A^T = LB LB^T, c = LB^-1 A yt):

    ch  = LB^-T c                                              (m x k)
    H   = k (I - B^-1) - ch ch^T                               (m x m)
    Guu = 1/2 L^-T [ k (2 I - B^-1 - B) - ch ch^T ] L^-1        (m x m)
    t_n = L^-T ( H a_n + ch yt_n^T ) / s_n                      row n of T = (dF / dKuf)^T,  N x m

    dF / dlog l_c = sum T . dKfu / dlog l_c + sum Guu . dKuu / dlog l_c
    dF / dlog sf2 = sum T . Kfu + sum Guu . (Kuu - jitter I) - 1/2 k sf2 sum_n 1 / s_n^2
    dF / dlog sn2 = 1/2 k (m - tr B^-1) - 1/2 k N + 1/2 |yt|^2 - |c|^2 + 1/2 (|c|^2 - |ch|^2) + 1/2 k sf2 sum 1 / s_n^2
                    - 1/2 k tr(A A^T)

dK / dlog l_c = kd u_c^2, u = (x - z) / l, kd the family's own (gpx_cov.h: RBF k, Matern-5/2 (5/3)(1 + s) e^-s, Matern-3/2
3 e^-s, Matern-1/2 e^-r / r and 0 at r = 0; each times sf2); one lengthscale for all dimensions sums over c.

``fd_gradient`` is the five-point central difference of the bound in the same parameters.  Shared by the CPU and GPU tests."""
import numpy as np
from scipy.linalg import solve_triangular

import sparse_ref

SQRT3, SQRT5 = np.sqrt(3.0), np.sqrt(5.0)
FD_STEPS = (1e-2, 3e-3, 1e-3, 3e-4)


def kernel_dl(A, B, kernel, ls, sf2):
    """-> (K, dK) with K = sf2 k(A, B) (na, nb) and dK (d, na, nb)[c] = kd u_c^2, from coordinate differences"""
    A, B = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
    l = np.broadcast_to(np.atleast_1d(np.asarray(ls, dtype=np.float64)), (A.shape[1],))
    D = (A / l)[:, None, :] - (B / l)[None, :, :]
    U2 = D * D
    r2 = np.sum(U2, axis=2)
    r = np.sqrt(r2)
    if kernel == "rbf":
        K = np.exp(-0.5 * r2)
        kd = K
    elif kernel == "matern52":
        s = SQRT5 * r
        e = np.exp(-s)
        K, kd = (1.0 + s + s * s / 3.0) * e, (5.0 / 3.0) * (1.0 + s) * e
    elif kernel == "matern32":
        s = SQRT3 * r
        e = np.exp(-s)
        K, kd = (1.0 + s) * e, 3.0 * e
    elif kernel == "matern12":
        K = np.exp(-r)
        kd = np.divide(K, r, out=np.zeros_like(r), where=r > 0)
    else:
        raise ValueError(f"sparse_grad_ref: unknown kernel {kernel!r}")
    return sf2 * K, sf2 * kd[None, :, :] * np.moveaxis(U2, 2, 0)


def contract(W, A, B, kernel, ls, sf2):
    """sum_ij W_ij (dK / dlog theta_t)_ij for theta = (lengthscales..., sf2): what gpx_cross_dtheta_contract computes,
    and the scale sum_ij |W_ij| |dK_ij| per entry that its error is measured against"""
    K, dK = kernel_dl(A, B, kernel, ls, sf2)
    if np.ndim(ls) == 0 or np.size(ls) == 1:
        dK = dK.sum(axis=0, keepdims=True)
    terms = np.concatenate([dK, K[None]], axis=0)
    return np.sum(W[None] * terms, axis=(1, 2)), np.sum(np.abs(W)[None] * np.abs(terms), axis=(1, 2))


def gradient(kernel, ls, sf2, sn2, jitter, X, y, Z, w=None):
    """-> (F, grad): the bound summed over the targets and its analytic gradient in (log l..., log sf2, log sn2)"""
    X, Z = np.asarray(X, dtype=np.float64), np.asarray(Z, dtype=np.float64)
    N, m = len(X), len(Z)
    Y = np.asarray(y, dtype=np.float64).reshape(N, -1)
    k = Y.shape[1]
    ref = sparse_ref.SparseRef(kernel, ls, sf2, sn2, jitter).fit(X, y, Z, w)
    s2 = sn2 * (np.ones(N) if w is None else np.asarray(w, dtype=np.float64))
    s = np.sqrt(s2)
    Yt = Y / s[:, None]
    L, LB, c = ref.L, ref.LB, ref.c
    A = ref._whitened(X, s)
    B = np.eye(m) + A @ A.T
    LBinv = solve_triangular(LB, np.eye(m), lower=True)
    Binv = LBinv.T @ LBinv
    ch = solve_triangular(LB, c, lower=True, trans="T")
    H = k * (np.eye(m) - Binv) - ch @ ch.T
    Muu = k * (2.0 * np.eye(m) - Binv - B) - ch @ ch.T
    Guu = 0.5 * solve_triangular(L, solve_triangular(L, Muu, lower=True, trans="T").T, lower=True, trans="T")
    T = solve_triangular(L, H @ A + ch @ Yt.T, lower=True, trans="T").T / s[:, None]
    gx, _ = contract(T, X, Z, kernel, ls, sf2)
    gu, _ = contract(Guu, Z, Z, kernel, ls, sf2)
    sum_inv = float(np.sum(1.0 / s2))
    g = gx + gu
    g[-1] -= 0.5 * k * sf2 * sum_inv
    cc, chh = float(np.sum(c * c)), float(np.sum(ch * ch))
    gn = (0.5 * k * (m - np.trace(Binv)) - 0.5 * k * N + 0.5 * float(np.sum(Yt * Yt)) - cc + 0.5 * (cc - chh)
          + 0.5 * k * sf2 * sum_inv - 0.5 * k * float(np.sum(A * A)))
    return float(ref.elbo.sum()), np.concatenate([g, [gn]])


def bound(theta, n_ls, kernel, jitter, X, y, Z, w=None):
    """the bound summed over the targets at the log parameters theta = (log l..., log sf2, log sn2)"""
    p = np.exp(theta)
    ls = p[0] if n_ls == 1 else p[:n_ls]
    return float(sparse_ref.SparseRef(kernel, ls, p[n_ls], p[n_ls + 1], jitter).fit(X, y, Z, w).elbo.sum())


def fd_gradient(kernel, ls, sf2, sn2, jitter, X, y, Z, w=None, h=1e-3):
    """five-point central differences of the bound in the log parameters, step h"""
    l = np.atleast_1d(np.asarray(ls, dtype=np.float64))
    theta = np.log(np.concatenate([l, [sf2, sn2]]))
    f = lambda t: bound(t, l.size, kernel, jitter, X, y, Z, w)  # noqa: E731
    g = np.empty_like(theta)
    for i in range(theta.size):
        e = np.zeros_like(theta)
        e[i] = h
        g[i] = (-f(theta + 2 * e) + 8.0 * f(theta + e) - 8.0 * f(theta - e) + f(theta - 2 * e)) / (12.0 * h)
    return g


def metric(g, f):
    """max_i |g_i - f_i| / (|f_i| + 1e-3 max_j |f_j|)"""
    g, f = np.asarray(g, dtype=np.float64), np.asarray(f, dtype=np.float64)
    return float(np.max(np.abs(g - f) / (np.abs(f) + 1e-3 * np.max(np.abs(f)))))


def exact_lml_gradient(kernel, ls, sf2, sn2, X, y, w=None):
    """gradient of the exact GP's log marginal likelihood (summed over the targets) in the same parameters:
    1/2 sum (alpha alpha^T - k K^-1) . dK / dlog theta"""
    X = np.asarray(X, dtype=np.float64)
    N = len(X)
    Y = np.asarray(y, dtype=np.float64).reshape(N, -1)
    k = Y.shape[1]
    wv = np.ones(N) if w is None else np.asarray(w, dtype=np.float64)
    K, dK = kernel_dl(X, X, kernel, ls, sf2)
    Ky = K + np.diag(sn2 * wv)
    Kinv = np.linalg.inv(Ky)
    Kinv = 0.5 * (Kinv + Kinv.T)
    al = Kinv @ Y
    Wm = 0.5 * (al @ al.T - k * Kinv)
    if np.ndim(ls) == 0 or np.size(ls) == 1:
        dK = dK.sum(axis=0, keepdims=True)
    g = [float(np.sum(Wm * D)) for D in dK]
    g.append(float(np.sum(Wm * K)))
    g.append(float(np.sum(np.diag(Wm) * sn2 * wv)))
    return np.array(g)
