"""Dense fp64 NumPy/SciPy reference of the hierarchical path model (include/gpx.h, gpx_set_path_groups):

    y_p(t) = f(t) + g_p(t) + noise,     K[(x, p), (x', p')] = sf2 k(x, x'; l) + [p == p' and p >= 0] sg2 k(x, x'; l_path)

The family values come from ``score_ref.kernel_matrix``.  Fit (alpha, logdet, the predict of f), the block score with the
extra within-path term, and the forecast of partly observed new paths computed TWO ways:

* ``forecast_schur``: what the library does — the joint posterior-of-f-plus-g covariance S of a block's Lo + Lp points,
  conditioned on the first Lo through the Schur complement;
* ``forecast_refit``: the independent way — refit the training set plus the block's observed points under a fresh path id,
  then predict the block's remaining points as members of that path; the prefix log-density is the difference of the two
  log marginal likelihoods.

Both return each block's 2-norm condition number ``kappa`` of S_oo + diag_add I, in which the tests' bounds are written.
Shared by the CPU and GPU tests."""
import os
import sys

import numpy as np
from scipy.linalg import cho_solve, cholesky, solve_triangular

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from score_ref import LOG_2PI, kernel_matrix  # noqa: E402


def _ls(ls, d):
    ls = np.atleast_1d(np.asarray(ls, dtype=np.float64))
    return np.full(d, ls[0]) if ls.size == 1 else ls


def path_cov(A, ga, B, gb, kernel, ls, sf2, ls_path, sg2):
    """(m, n) covariance of observations A with path ids ga against B with ids gb (None: no ids, f alone)"""
    A, B = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
    d = A.shape[1]
    K = kernel_matrix(A, B, kernel, _ls(ls, d), sf2)
    if ga is None or gb is None or not sg2 > 0:
        return K
    ga, gb = np.asarray(ga), np.asarray(gb)
    same = (ga[:, None] == gb[None, :]) & (ga[:, None] >= 0)
    if same.any():
        K = K + np.where(same, kernel_matrix(A, B, kernel, _ls(ls_path, d), sg2), 0.0)
    return K


def kappa_bound(Lo, sf2, sg2, diag_add):
    """kappa(S_oo + diag_add I) <= (Lo (sf2 + sg2) + diag_add) / diag_add: S_oo is PSD with a trace of at most the prior's"""
    return (Lo * (sf2 + sg2) + diag_add) / diag_add


def fit_ref(X, ids, Y, kernel, ls, sf2, sn2, ls_path, sg2, w=None, jitter=0.0, extra_diag=None):
    """-> dict(L, z, alpha (N, k), logdet, lml (k,)); diagonal sn2 w_i + jitter (extra_diag (N,) replaces it where not NaN)"""
    X = np.asarray(X, dtype=np.float64)
    Y = np.asarray(Y, dtype=np.float64).reshape(len(X), -1)
    K = path_cov(X, ids, X, ids, kernel, ls, sf2, ls_path, sg2)
    dg = sn2 * (np.ones(len(X)) if w is None else np.asarray(w, dtype=np.float64)) + jitter
    if extra_diag is not None:
        dg = np.where(np.isnan(extra_diag), dg, extra_diag)
    K[np.diag_indices_from(K)] += dg
    L = cholesky(K, lower=True)
    z = solve_triangular(L, Y, lower=True)
    alpha = solve_triangular(L.T, z, lower=False)
    logdet = 2.0 * np.sum(np.log(np.diag(L)))
    lml = -0.5 * np.sum(z * z, axis=0) - 0.5 * logdet - 0.5 * len(X) * LOG_2PI
    grouped = ids is not None and sg2 > 0 and bool(np.any(np.asarray(ids) >= 0))  # else: the plain model (as the library)
    return {"X": X, "ids": ids, "grouped": grouped, "L": L, "z": z, "alpha": alpha, "logdet": logdet, "lml": lml,
            "kernel": kernel, "ls": ls, "sf2": sf2, "ls_path": ls_path, "sg2": sg2}


def predict_f(fit, Xq):
    """posterior of the cluster mean f at Xq: mean (M, k), cov (M, M), V = L^-1 K*^T (N, M)"""
    Xq = np.asarray(Xq, dtype=np.float64)
    d = Xq.shape[1]
    Ks = kernel_matrix(Xq, fit["X"], fit["kernel"], _ls(fit["ls"], d), fit["sf2"])
    V = solve_triangular(fit["L"], Ks.T, lower=True)
    cov = kernel_matrix(Xq, Xq, fit["kernel"], _ls(fit["ls"], d), fit["sf2"]) - V.T @ V
    return V.T @ fit["z"], 0.5 * (cov + cov.T), V


def block_cov(fit, Xb):
    """joint covariance of one NEW path at Xb under the fit, without noise: posterior(f) [+ sg2 k(., .; l_path)], and the mean"""
    mean, S, _ = predict_f(fit, Xb)
    if fit["grouped"]:
        d = Xb.shape[1]
        S = S + kernel_matrix(Xb, Xb, fit["kernel"], _ls(fit["ls_path"], d), fit["sg2"])
    return mean, 0.5 * (S + S.T)


def score_ref_within(fit, Xq, Yq, Lg, diag_add):
    """score_ref with the extra block term, in score_ref's own operation order (one solve for all the queries), so that a
    fit without effective path ids reproduces it exactly -> dict(logp (G, k), maha (G, k), logdet (G,), kappa (G,))"""
    Xq = np.asarray(Xq, dtype=np.float64)
    Yq = np.asarray(Yq, dtype=np.float64).reshape(len(Xq), -1)
    G, k, d = len(Xq) // Lg, Yq.shape[1], Xq.shape[1]
    Ks = kernel_matrix(Xq, fit["X"], fit["kernel"], fit["ls"], fit["sf2"])
    V = solve_triangular(fit["L"], Ks.T, lower=True)
    mean = V.T @ fit["z"]
    out = {"logp": np.empty((G, k)), "maha": np.empty((G, k)), "logdet": np.empty(G), "kappa": np.empty(G)}
    for g in range(G):
        sl = slice(g * Lg, (g + 1) * Lg)
        S = kernel_matrix(Xq[sl], Xq[sl], fit["kernel"], fit["ls"], fit["sf2"]) - V[:, sl].T @ V[:, sl]
        S = 0.5 * (S + S.T)
        if fit["grouped"]:
            S += kernel_matrix(Xq[sl], Xq[sl], fit["kernel"], _ls(fit["ls_path"], d), fit["sg2"])
        S[np.diag_indices(Lg)] += diag_add
        Ls = cholesky(S, lower=True)
        w = solve_triangular(Ls, Yq[sl] - mean[sl], lower=True)
        ev = np.linalg.eigvalsh(S)
        out["kappa"][g] = ev[-1] / ev[0]
        out["maha"][g] = np.sum(w * w, axis=0)
        out["logdet"][g] = 2.0 * np.sum(np.log(np.diag(Ls)))
        out["logp"][g] = -0.5 * out["maha"][g] - 0.5 * out["logdet"][g] - 0.5 * Lg * LOG_2PI
    return out


def _blocks(Xo, Yo, Xp, G):
    Xo, Xp = np.asarray(Xo, dtype=np.float64), np.asarray(Xp, dtype=np.float64)
    Yo = np.asarray(Yo, dtype=np.float64).reshape(len(Xo), -1)
    Lo, Lp = len(Xo) // G, len(Xp) // G
    assert Lo * G == len(Xo) and Lp * G == len(Xp)
    return Xo, Yo, Xp, Lo, Lp


def schur_block(mean, S, Lo, yo, diag_add):
    """One block of the Schur form from its joint prior: ``mean`` (Lo + Lp, k) and ``S`` (Lo + Lp, Lo + Lp) without noise,
    the first Lo points observed as ``yo`` with noise diag_add -> dict(mean (Lp, k), cov (Lp, Lp), logp (k,), maha (k,),
    kappa = cond(S_oo + diag_add I), resid = max |yo - mean_o|)"""
    Soo = S[:Lo, :Lo].copy()
    Soo[np.diag_indices(Lo)] += diag_add
    Loo = cholesky(Soo, lower=True)
    B = solve_triangular(Loo, S[:Lo, Lo:], lower=True).T                 # S_po L_oo^-T
    r = yo - mean[:Lo]
    w = solve_triangular(Loo, r, lower=True)
    ev = np.linalg.eigvalsh(Soo)
    c = S[Lo:, Lo:] - B @ B.T
    maha = np.sum(w * w, axis=0)
    return {"mean": mean[Lo:] + B @ w, "cov": 0.5 * (c + c.T), "maha": maha,
            "logp": -0.5 * maha - np.sum(np.log(np.diag(Loo))) - 0.5 * Lo * LOG_2PI, "kappa": ev[-1] / ev[0],
            "resid": np.max(np.abs(r))}


def forecast_schur(fit, Xo, Yo, Xp, G, diag_add, prior=None):
    """-> dict(mean (G Lp, k), cov (G, Lp, Lp), logp (G, k), maha (G, k), kappa (G,), resid (G,) = max |yo - mean_o|).
    ``prior(Xb) -> (mean, S)`` replaces the reference's own joint prior of a block (``block_cov``) when given: a test that
    isolates the block algebra feeds the posterior of f that the handle under test itself reports."""
    Xo, Yo, Xp, Lo, Lp = _blocks(Xo, Yo, Xp, G)
    k = Yo.shape[1]
    out = {"mean": np.empty((G * Lp, k)), "cov": np.empty((G, Lp, Lp)), "logp": np.empty((G, k)), "maha": np.empty((G, k)),
           "kappa": np.empty(G), "resid": np.empty(G)}
    for g in range(G):
        Xb = np.concatenate([Xo[g * Lo:(g + 1) * Lo], Xp[g * Lp:(g + 1) * Lp]])
        mean, S = prior(Xb) if prior is not None else block_cov(fit, Xb)
        b = schur_block(mean, S, Lo, Yo[g * Lo:(g + 1) * Lo], diag_add)
        out["mean"][g * Lp:(g + 1) * Lp] = b["mean"]
        for n in ("cov", "logp", "maha", "kappa", "resid"):
            out[n][g] = b[n]
    return out


def forecast_refit(train, Xo, Yo, Xp, G, diag_add):
    """The independent route.  ``train`` = dict(X, ids (None: a plain fit), Y, kernel, ls, sf2, sn2, ls_path, sg2, w, jitter):
    per block, the training set plus its observed points under a fresh path id (noise diag_add on them) is fitted anew and
    the points to forecast are predicted as members of that path.  -> dict(mean, cov, logp) shaped as forecast_schur's."""
    Xo, Yo, Xp, Lo, Lp = _blocks(Xo, Yo, Xp, G)
    X = np.asarray(train["X"], dtype=np.float64)
    Y = np.asarray(train["Y"], dtype=np.float64).reshape(len(X), -1)
    N, k = Y.shape
    grouped = train.get("ids") is not None and train["sg2"] > 0 and bool(np.any(np.asarray(train["ids"]) >= 0))
    ids = np.asarray(train["ids"]) if grouped else np.full(N, -1)
    fresh = int(ids.max()) + 1 if grouped else -1       # a plain fit: the block has no deviation of its own either
    kw = dict(kernel=train["kernel"], ls=train["ls"], sf2=train["sf2"], sn2=train["sn2"], ls_path=train["ls_path"],
              sg2=train["sg2"] if grouped else 0.0, jitter=train.get("jitter", 0.0))
    w = train.get("w")
    base = fit_ref(X, ids if grouped else None, Y, w=w, **kw)
    out = {"mean": np.empty((G * Lp, k)), "cov": np.empty((G, Lp, Lp)), "logp": np.empty((G, k))}
    for g in range(G):
        xo, yo, xp = Xo[g * Lo:(g + 1) * Lo], Yo[g * Lo:(g + 1) * Lo], Xp[g * Lp:(g + 1) * Lp]
        Xa = np.concatenate([X, xo])
        ia = np.concatenate([ids, np.full(Lo, fresh)])
        wa = np.concatenate([np.ones(N) if w is None else np.asarray(w, dtype=np.float64), np.ones(Lo)])
        extra = np.concatenate([np.full(N, np.nan), np.full(Lo, diag_add)])
        big = fit_ref(Xa, ia if grouped else None, np.concatenate([Y, yo]), w=wa, extra_diag=extra, **kw)
        gp_ids = np.full(Lp, fresh)
        Ks = path_cov(xp, gp_ids, Xa, ia, kw["kernel"], kw["ls"], kw["sf2"], kw["ls_path"], kw["sg2"])
        Kpp = path_cov(xp, gp_ids, xp, gp_ids, kw["kernel"], kw["ls"], kw["sf2"], kw["ls_path"], kw["sg2"])
        out["mean"][g * Lp:(g + 1) * Lp] = Ks @ big["alpha"]
        c = Kpp - Ks @ cho_solve((big["L"], True), Ks.T)
        out["cov"][g] = 0.5 * (c + c.T)
        out["logp"][g] = big["lml"] - base["lml"]
    return out


def problem(P=12, L=33, G=5, Lo=20, Lp=13, k=2, kernel="matern32", ls=0.25, sf2=1.5, ls_path=0.1, sg2=0.4, sn2=1e-2,
            seed=0, d=1):
    """P training paths of L points and G new paths of Lo + Lp points, all drawn jointly from the model itself: one f for
    all, one g per path, noise sn2.  Inputs: sorted uniform times in [0, 1] (d > 1: further columns a smooth function of
    the time plus a little scatter).  -> dict(X, ids, Y, Xo, Yo, Xp, Yp)"""
    rng = np.random.default_rng(seed)

    def times(n_paths, n):
        t = np.sort(rng.uniform(0.0, 1.0, (n_paths, n)), axis=1)
        cols = [t] + [np.sin((c + 1.0) * t) + 0.02 * rng.standard_normal(t.shape) for c in range(1, d)]
        return np.stack(cols, axis=-1).reshape(n_paths * n, d)

    X, Xb = times(P, L), times(G, Lo + Lp)
    ids = np.repeat(np.arange(P), L)
    idb = np.repeat(np.arange(P, P + G), Lo + Lp)
    Xa, ia = np.concatenate([X, Xb]), np.concatenate([ids, idb])
    K = path_cov(Xa, ia, Xa, ia, kernel, ls, sf2, ls_path, sg2)
    K[np.diag_indices_from(K)] += 1e-10
    Ya = cholesky(K, lower=True) @ rng.standard_normal((len(Xa), k)) + np.sqrt(sn2) * rng.standard_normal((len(Xa), k))
    Yb = Ya[len(X):].reshape(G, Lo + Lp, k)
    Xb3 = Xb.reshape(G, Lo + Lp, d)
    return {"X": X, "ids": ids.astype(np.int32), "Y": Ya[:len(X)], "Xo": Xb3[:, :Lo].reshape(G * Lo, d),
            "Yo": Yb[:, :Lo].reshape(G * Lo, k), "Xp": Xb3[:, Lo:].reshape(G * Lp, d), "Yp": Yb[:, Lo:].reshape(G * Lp, k)}
