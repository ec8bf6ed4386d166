"""fp64 NumPy/SciPy reference of the GP with explicit basis functions (include/gpx.h, gpx_set_basis; Rasmussen & Williams
§2.7, eqs. 2.41-2.42): y = f(x) + h(x)^T beta + noise with a flat prior on beta, marginalised.

    H = h(X) (N x p),  K = sf2 k(X, X) + diag(sn2 w_i + jitter) = L L^T
    A = H^T K^-1 H,   beta = A^-1 H^T K^-1 y,   alpha' = K^-1 (y - H beta)           (H^T alpha' = 0)
    mean(x*) = k*^T alpha' + h(x*)^T beta
    cov(x*, x') = k(x*, x') - k*^T K^-1 k' + r*^T A^-1 r',   r* = h(x*) - H^T K^-1 k*
    profile LML = -1/2 (y - H beta)^T alpha' - k/2 log|K| - N k / 2 log 2 pi,  gradient at fixed beta: R&W eq. 5.9 with alpha'

h is evaluated on the raw inputs: [1] | [1, x_1..x_d] | [1, x_1..x_d, x_1^2..x_d^2].  Dense algebra only (cho_solve on K; no
step is shared with the library's bordered-row form).  Block scores and forecasts are the dense Gaussian formulas on the
joint posterior of a block's rows.  Shared by the CPU and GPU tests."""
import os
import sys

import numpy as np
from scipy.linalg import cho_solve, cholesky, solve_triangular

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from hetero_ref import kernel_dlog_ls  # noqa: E402
from score_ref import LOG_2PI, kernel_matrix  # noqa: E402

BASES = ("constant", "linear", "quadratic")


def basis_matrix(X, basis):
    """h(X): (n, p), p = 1 | 1 + d | 1 + 2 d"""
    X = np.asarray(X, dtype=np.float64)
    cols = [np.ones((len(X), 1))]
    if basis in ("linear", "quadratic"):
        cols.append(X)
    if basis == "quadratic":
        cols.append(X ** 2)
    if basis not in BASES:
        raise ValueError(basis)
    return np.concatenate(cols, axis=1)


class BasisGP:
    def __init__(self, kernel, ls, sf2, sn2, basis, jitter=0.0):
        self.kernel, self.ls, self.sf2, self.sn2, self.basis, self.jitter = kernel, ls, float(sf2), float(sn2), basis, jitter

    def gram(self, X, w=None):
        K = kernel_matrix(X, X, self.kernel, self.ls, self.sf2)
        K[np.diag_indices_from(K)] += self.sn2 * (1.0 if w is None else np.asarray(w, dtype=np.float64)) + self.jitter
        return K

    def fit(self, X, y, w=None):
        self.X = np.asarray(X, dtype=np.float64)
        self.y1d = np.ndim(y) == 1
        self.Y = np.asarray(y, dtype=np.float64).reshape(len(self.X), -1)
        self.w = w
        self.H = basis_matrix(self.X, self.basis)
        self.cK = (cholesky(self.gram(self.X, w), lower=True), True)
        self.KiH = cho_solve(self.cK, self.H)
        self.KiY = cho_solve(self.cK, self.Y)
        self.A = self.H.T @ self.KiH
        self.A = 0.5 * (self.A + self.A.T)
        self.beta_cov = np.linalg.inv(self.A)
        self.beta = np.linalg.solve(self.A, self.H.T @ self.KiY)          # (p, k)
        self.alpha = cho_solve(self.cK, self.Y - self.H @ self.beta)       # alpha'
        self.logdet = 2.0 * float(np.sum(np.log(np.diag(self.cK[0]))))
        return self

    def out(self, a):
        return a[:, 0] if self.y1d else a

    def lml(self):
        n, k = self.Y.shape
        r = self.Y - self.H @ self.beta
        return float(-0.5 * np.sum(r * self.alpha) - 0.5 * k * self.logdet - 0.5 * n * k * LOG_2PI)

    def lml_gradient(self):
        """d profile LML / d log (lengthscales..., sf2, sn2) at fixed beta (the term through beta vanishes: H^T alpha' = 0)"""
        n, k = self.Y.shape
        W = self.alpha @ self.alpha.T - k * cho_solve(self.cK, np.eye(n))
        g = [0.5 * np.sum(W * dK) for dK in kernel_dlog_ls(self.X, self.kernel, self.ls, self.sf2)]
        g.append(0.5 * np.sum(W * kernel_matrix(self.X, self.X, self.kernel, self.ls, self.sf2)))
        w = np.ones(n) if self.w is None else np.asarray(self.w, dtype=np.float64)
        g.append(0.5 * self.sn2 * float(np.sum(w * np.diag(W))))
        return np.array(g)

    def joint(self, Xs):
        """mean (M, k) and the joint covariance (M, M) of the latent function at Xs"""
        Xs = np.asarray(Xs, dtype=np.float64)
        Ks = kernel_matrix(Xs, self.X, self.kernel, self.ls, self.sf2)
        R = basis_matrix(Xs, self.basis) - Ks @ self.KiH                   # (M, p)
        mean = Ks @ self.alpha + basis_matrix(Xs, self.basis) @ self.beta
        cov = kernel_matrix(Xs, Xs, self.kernel, self.ls, self.sf2) - Ks @ cho_solve(self.cK, Ks.T) + R @ self.beta_cov @ R.T
        return mean, 0.5 * (cov + cov.T)

    def predict(self, Xs):
        mean, cov = self.joint(Xs)
        return self.out(mean), np.diag(cov).copy()

    def score(self, Xq, Yq, Lg, diag_add):
        """-> dict(logp (G, k), maha (G, k), logdet (G,), kappa (G,)): joint density of blocks of Lg query points"""
        Xq = np.asarray(Xq, dtype=np.float64)
        Yq = np.asarray(Yq, dtype=np.float64).reshape(len(Xq), -1)
        G, k = len(Xq) // Lg, Yq.shape[1]
        out = {"logp": np.empty((G, k)), "maha": np.empty((G, k)), "logdet": np.empty(G), "kappa": np.empty(G)}
        for g in range(G):
            sl = slice(g * Lg, (g + 1) * Lg)
            mean, S = self.joint(Xq[sl])
            S[np.diag_indices(Lg)] += diag_add
            Ls = cholesky(S, lower=True)
            r = solve_triangular(Ls, Yq[sl] - mean, lower=True)
            ev = np.linalg.eigvalsh(S)
            out["kappa"][g] = ev[-1] / ev[0]
            out["maha"][g] = np.sum(r * r, axis=0)
            out["logdet"][g] = 2.0 * np.sum(np.log(np.diag(Ls)))
            out["logp"][g] = -0.5 * out["maha"][g] - 0.5 * out["logdet"][g] - 0.5 * Lg * LOG_2PI
        return out

    def forecast(self, Xo, Yo, Xp, G, diag_add):
        """Blocks of Lo observed rows (Xo, Yo) then Lp rows to forecast (Xp): the posterior of the Lp rows given the
        block's own observations (noise diag_add on them) -> dict(mean (G, Lp, k), cov (G, Lp, Lp), logp (G, k),
        kappa (G,) of S_oo + diag_add I, resid (G,) = max |yo - mean_o|, maha (G, k), scale (G,) = max diag of the joint S)"""
        Xo, Xp = np.asarray(Xo, dtype=np.float64), np.asarray(Xp, dtype=np.float64)
        Yo = np.asarray(Yo, dtype=np.float64).reshape(len(Xo), -1)
        Lo, Lp, k = len(Xo) // G, len(Xp) // G, Yo.shape[1]
        out = {"mean": np.empty((G, Lp, k)), "cov": np.empty((G, Lp, Lp)), "logp": np.empty((G, k)), "kappa": np.empty(G),
               "resid": np.empty(G), "maha": np.empty((G, k)), "scale": np.empty(G)}
        for g in range(G):
            xo, xp, yo = Xo[g * Lo:(g + 1) * Lo], Xp[g * Lp:(g + 1) * Lp], Yo[g * Lo:(g + 1) * Lo]
            mean, S = self.joint(np.concatenate([xo, xp]))
            Soo = S[:Lo, :Lo] + diag_add * np.eye(Lo)
            c = (cholesky(Soo, lower=True), True)
            r = yo - mean[:Lo]
            out["mean"][g] = mean[Lo:] + S[Lo:, :Lo] @ cho_solve(c, r)
            out["cov"][g] = S[Lo:, Lo:] - S[Lo:, :Lo] @ cho_solve(c, S[:Lo, Lo:])
            wv = solve_triangular(c[0], r, lower=True)
            ev = np.linalg.eigvalsh(Soo)
            out["kappa"][g] = ev[-1] / ev[0]
            out["resid"][g] = np.abs(r).max()
            out["maha"][g] = np.sum(wv * wv, axis=0)
            out["scale"][g] = np.diag(S).max()
            out["logp"][g] = -0.5 * out["maha"][g] - np.sum(np.log(np.diag(c[0]))) - 0.5 * Lo * LOG_2PI
        return out


def absorbed_predict(X, y, Xs, kernel, ls, sf2, sn2, basis, b2):
    """The zero-mean GP with kernel k + b2 h h^T (beta ~ N(0, b2 I) absorbed into the covariance): its mean (M, k) and
    variance (M,) tend to the marginalised ones as b2 -> infinity (R&W eq. 2.40 -> 2.41)."""
    X, Xs = np.asarray(X, dtype=np.float64), np.asarray(Xs, dtype=np.float64)
    Y = np.asarray(y, dtype=np.float64).reshape(len(X), -1)
    H, Hs = basis_matrix(X, basis), basis_matrix(Xs, basis)
    K = kernel_matrix(X, X, kernel, ls, sf2) + b2 * H @ H.T
    K[np.diag_indices_from(K)] += sn2
    c = (cholesky(K, lower=True), True)
    Ks = kernel_matrix(Xs, X, kernel, ls, sf2) + b2 * Hs @ H.T
    prior = sf2 + b2 * np.sum(Hs * Hs, axis=1)
    return Ks @ cho_solve(c, Y), prior - np.einsum("mn,nm->m", Ks, cho_solve(c, Ks.T))


def block_queries(G, Lg, d, k, seed):
    """G blocks of Lg query points, each a short straight walk through [-0.2, 1.2]^d (some points outside the data of
    trend_problem), and targets for them"""
    rng = np.random.default_rng(seed)
    start = rng.uniform(-0.2, 1.2, (G, 1, d))
    step = rng.uniform(-0.012, 0.012, (G, 1, d))
    Xq = (start + step * np.arange(Lg)[None, :, None] + 0.002 * rng.standard_normal((G, Lg, d))).reshape(G * Lg, d)
    Yq = 2.0 + Xq @ rng.uniform(-3.0, 3.0, (d, k)) + 0.3 * rng.standard_normal((G * Lg, k))
    return Xq, Yq


def trend_problem(N, d, k, M, seed):
    """X uniform in [0, 1]^d; targets a linear trend plus a smooth term plus noise; M queries, a quarter of them outside
    the data's box"""
    rng = np.random.default_rng(seed)
    X = rng.uniform(0.0, 1.0, (N, d))
    Xs = rng.uniform(0.0, 1.0, (M, d))
    Xs[::4] = rng.uniform(-0.5, 1.5, (len(Xs[::4]), d))
    a, b = rng.uniform(2.0, 5.0, (d, k)), rng.uniform(-3.0, 3.0, (d, k))

    def f(A):
        return 2.0 + A @ b + 0.5 * np.sin(A @ a)

    Y = f(X) + 0.1 * rng.standard_normal((N, k))
    return X, (Y[:, 0] if k == 1 else Y), Xs
