"""fp64 NumPy/SciPy reference of the leave-one-out predictions of a GP (gpx_loo / GP.loo; Rasmussen & Williams §5.4.2).

``K`` is the covariance of the observations as the fit holds it — noise, weights, jitter, derivative rows and the path term
included; it comes from the dense builders the suite already has (oracle.gp_oracle.kernel_matrix, matern_ref,
dobs_ref.mixed_gram + noise_diag, within_ref.path_cov).  ``H`` (N, p), or None: basis functions whose coefficients are
marginalised under a flat prior (basis_ref.basis_matrix; R&W §2.7).

    loo_closed   the closed form: the explicit inverse Q = K^-1 (with H: Q' = Q - Q H (H^T Q H)^-1 H^T Q), then
                 var_i = 1 / Q_ii, mean_i = y_i - (Q y)_i / Q_ii, logp_i the Gaussian log-density of y_i
    loo_refit    what the closed form stands for: delete row i, factorise the other rows, predict observation i from them
                 (with H: the predictive equations of R&W 2.41-2.42).  It shares no step with loo_closed.

Both return dict(mean (N, k), var (N,), logp (N, k), total (k,)).  A row that the basis coefficients alone determine
(closed form: Q'_ii <= 64 * 2^-52 * Q_ii; refit: fewer than p other rows) is undetermined: var +inf, mean NaN, logp -inf."""
import numpy as np
from scipy.linalg import cho_solve, cholesky

LOG_2PI = float(np.log(2.0 * np.pi))
UNDETERMINED = 64.0 * 2.0 ** -52


def _pack(mean, var, logp):
    return {"mean": mean, "var": var, "logp": logp, "total": logp.sum(axis=0)}


def loo_closed(K, Y, H=None):
    K = np.asarray(K, dtype=np.float64)
    Y = np.asarray(Y, dtype=np.float64).reshape(len(K), -1)
    Q = np.linalg.inv(K)
    Q = 0.5 * (Q + Q.T)
    q0 = np.diag(Q).copy()
    if H is not None:
        B = Q @ np.asarray(H, dtype=np.float64)
        A = H.T @ B
        Q = Q - B @ np.linalg.solve(0.5 * (A + A.T), B.T)
    q = np.diag(Q).copy()
    alpha = Q @ Y
    bad = q <= UNDETERMINED * q0
    with np.errstate(divide="ignore", invalid="ignore"):
        var = np.where(bad, np.inf, 1.0 / q)
        mean = np.where(bad[:, None], np.nan, Y - alpha / q[:, None])
        logp = np.where(bad[:, None], -np.inf, -0.5 * np.log(2.0 * np.pi / q)[:, None] - alpha ** 2 / (2.0 * q[:, None]))
    return _pack(mean, var, logp)


def loo_refit(K, Y, H=None):
    K = np.asarray(K, dtype=np.float64)
    N = len(K)
    Y = np.asarray(Y, dtype=np.float64).reshape(N, -1)
    mean, var, logp = np.empty_like(Y), np.empty(N), np.empty_like(Y)
    for i in range(N):
        rest = np.delete(np.arange(N), i)
        if H is not None and len(rest) < H.shape[1]:
            mean[i], var[i], logp[i] = np.nan, np.inf, -np.inf
            continue
        c = (cholesky(K[np.ix_(rest, rest)], lower=True), True)
        ks = K[rest, i]
        Kik = cho_solve(c, ks)
        if H is None:
            m = Kik @ Y[rest]
            v = K[i, i] - ks @ Kik
        else:
            Hr = H[rest]
            KiH = cho_solve(c, Hr)
            A = Hr.T @ KiH
            beta = np.linalg.solve(A, KiH.T @ Y[rest])
            r = H[i] - Hr.T @ Kik
            m = Kik @ (Y[rest] - Hr @ beta) + H[i] @ beta
            v = K[i, i] - ks @ Kik + r @ np.linalg.solve(A, r)
        mean[i], var[i] = m, v
        logp[i] = -0.5 * (LOG_2PI + np.log(v)) - (Y[i] - m) ** 2 / (2.0 * v)
    return _pack(mean, var, logp)


# ---- K of the five kinds of fit, from the suite's dense builders -----------------------------------------------------
def plain_gram(X, kernel, ls, sf2, sn2, w=None, jitter=0.0):
    """sf2 k(X, X) + diag(sn2 w_i + jitter): the oracle's builder for "rbf" / "matern52", matern_ref's for the other two"""
    if kernel in ("rbf", "matern52"):
        from oracle.gp_oracle import kernel_matrix
    else:
        from matern_ref import kernel_matrix
    K = np.array(kernel_matrix(X, X, kernel, ls, sf2), dtype=np.float64)
    K[np.diag_indices_from(K)] += sn2 * (np.ones(len(X)) if w is None else np.asarray(w, dtype=np.float64)) + jitter
    return K


def dobs_gram(c):
    """a case of dobs_ref (value and derivative rows in the fit's order, ``derivative_noise`` on the latter)"""
    from dobs_ref import mixed_gram, noise_diag
    K = mixed_gram(c["Xall"], c["kinds"], c["Xall"], c["kinds"], c["kernel"], c["ls"], c["sf2"])
    K[np.diag_indices_from(K)] += noise_diag(c["kinds"], c["w"], c["sn2"], c["sn2_deriv"], c["jitter"])
    return K


def within_gram(X, ids, kernel, ls, sf2, sn2, ls_path, sg2, w=None, jitter=0.0):
    from within_ref import path_cov
    K = np.array(path_cov(X, ids, X, ids, kernel, ls, sf2, ls_path, sg2), dtype=np.float64)
    K[np.diag_indices_from(K)] += sn2 * (np.ones(len(X)) if w is None else np.asarray(w, dtype=np.float64)) + jitter
    return K


def errors(got, ref):
    """the four figures every test prints and bounds: mean with floor 1e-6, var purely relative (it is at least the row's
    noise), logp with floor 1, total relative; rows that are undetermined in the reference must be so in `got` (inf)"""
    gm, rm = np.asarray(got["mean"]).reshape(ref["mean"].shape), ref["mean"]
    gl, rl = np.asarray(got["logp"]).reshape(ref["logp"].shape), ref["logp"]
    gv, rv = np.asarray(got["var"]), ref["var"]
    ok = np.isfinite(rv)
    if not (np.array_equal(np.isfinite(gv), ok) and np.all(gv[~ok] == np.inf) and np.all(np.isnan(gm[~ok]))
            and np.all(gl[~ok] == -np.inf)):
        return {"mean": np.inf, "var": np.inf, "logp": np.inf, "total": np.inf}
    out = {"mean": 0.0, "var": 0.0, "logp": 0.0, "total": 0.0}
    if ok.any():
        out["mean"] = float(np.max(np.abs(gm[ok] - rm[ok]) / np.maximum(np.abs(rm[ok]), 1e-6)))
        out["var"] = float(np.max(np.abs(gv[ok] - rv[ok]) / rv[ok]))
        out["logp"] = float(np.max(np.abs(gl[ok] - rl[ok]) / np.maximum(np.abs(rl[ok]), 1.0)))
    gt, rt = np.asarray(got["total"], dtype=np.float64).reshape(-1), ref["total"]
    if ok.all():
        out["total"] = float(np.max(np.abs(gt - rt) / np.abs(rt)))
    elif not np.all(gt == -np.inf):
        out["total"] = np.inf
    return out
