"""fp64 NumPy reference of the Matern-3/2 and Matern-1/2 kernels (include/gpx.h, GPX_KERNEL_MATERN32 / _MATERN12):
the kernel matrix, its derivative with respect to the first argument, its derivatives with respect to the log
hyper-parameters, and a dense exact GP (fit, predict, joint covariance, LML and LML gradient).  The oracle knows only
"rbf" and "matern52"; these two families are restated here.  Shared by the CPU and GPU tests."""
import numpy as np
from scipy.linalg import cho_solve, cholesky, solve_triangular

KERNELS = ("matern32", "matern12")
SQRT3 = np.sqrt(3.0)


def lengthscales(ls, d):
    return np.broadcast_to(np.atleast_1d(np.asarray(ls, dtype=np.float64)), (d,)).copy()


def _diffs(A, B, ls):
    A, B = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
    l = lengthscales(ls, A.shape[1])
    return A[:, None, :] / l - B[None, :, :] / l          # (na, nb, d): u_a - u_b


def kernel_matrix(A, B, kernel, ls, sf2):
    """sf2 k(A, B), (na, nb)"""
    r = np.sqrt(np.sum(_diffs(A, B, ls) ** 2, axis=2))
    if kernel == "matern32":
        s = SQRT3 * r
        return sf2 * ((1.0 + s) * np.exp(-s))
    if kernel == "matern12":
        return sf2 * np.exp(-r)
    raise ValueError(f"matern_ref: unknown kernel {kernel!r}")


def kd_factor(r, kernel, sf2):
    """kd with dK/dlog l_c = kd d_c^2; Matern-1/2: 0 at r = 0"""
    if kernel == "matern32":
        return 3.0 * sf2 * np.exp(-SQRT3 * r)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(r > 0.0, sf2 * np.exp(-r) / np.where(r > 0.0, r, 1.0), 0.0)


def kernel_grad(A, B, kernel, ls, sf2):
    """G (d, na, nb)[j][a][b] = d k(A_a, B_b) / d A_aj (Matern-3/2 only: Matern-1/2 has no derivative)"""
    if kernel != "matern32":
        raise ValueError("only Matern-3/2 is differentiable")
    D = _diffs(A, B, ls)
    l = lengthscales(ls, D.shape[2])
    g = 3.0 * sf2 * np.exp(-SQRT3 * np.sqrt(np.sum(D ** 2, axis=2)))
    return np.stack([-(g * D[:, :, j]) / l[j] for j in range(D.shape[2])])


def prior_grad_var(ls, sf2, d):
    """Var[d f / d x_j] of the Matern-3/2 prior, (d,)"""
    return 3.0 * sf2 / lengthscales(ls, d) ** 2


def kernel_dtheta(X, kernel, ls, sf2, sn2):
    """[dK/dlog l_0, ... (one per entry of ls, scalar ls: one), dK/dlog sf2, dK/dlog sn2], each (N, N)"""
    n_ls = np.atleast_1d(ls).size
    D = _diffs(X, X, ls)
    r = np.sqrt(np.sum(D ** 2, axis=2))
    kd = kd_factor(r, kernel, sf2)
    dl = [kd * D[:, :, c] ** 2 for c in range(D.shape[2])]
    if n_ls == 1:
        dl = [sum(dl)]
    return dl + [kernel_matrix(X, X, kernel, ls, sf2), sn2 * np.eye(len(X))]


class DenseGP:
    """Exact GP with SciPy's Cholesky: K = sf2 k(X, X) + (sn2 + jitter) I."""

    def __init__(self, kernel, ls, sf2, sn2, jitter=0.0):
        self.kernel, self.ls, self.sf2, self.sn2, self.jitter = kernel, ls, float(sf2), float(sn2), float(jitter)

    def fit(self, X, y):
        self.X = np.asarray(X, dtype=np.float64)
        self.Y = np.asarray(y, dtype=np.float64).reshape(len(self.X), -1)
        K = kernel_matrix(self.X, self.X, self.kernel, self.ls, self.sf2)
        K[np.diag_indices_from(K)] += self.sn2 + self.jitter
        self.L = cholesky(K, lower=True)
        self.alpha = cho_solve((self.L, True), self.Y)
        return self

    def predict(self, Xs):
        """mean (M, k) and latent variance (M,)"""
        Ks = kernel_matrix(Xs, self.X, self.kernel, self.ls, self.sf2)
        V = solve_triangular(self.L, Ks.T, lower=True)
        return Ks @ self.alpha, self.sf2 - np.einsum("nm,nm->m", V, V)

    def predict_cov(self, Xs):
        Ks = kernel_matrix(Xs, self.X, self.kernel, self.ls, self.sf2)
        V = solve_triangular(self.L, Ks.T, lower=True)
        return Ks @ self.alpha, kernel_matrix(Xs, Xs, self.kernel, self.ls, self.sf2) - V.T @ V

    def predict_grad(self, Xs):
        """Matern-3/2: dmean (M, d, k) and latent dvar (M, d)"""
        G = kernel_grad(Xs, self.X, self.kernel, self.ls, self.sf2)
        d = G.shape[0]
        prior = prior_grad_var(self.ls, self.sf2, d)
        dmean = np.stack([G[j] @ self.alpha for j in range(d)], axis=1)
        dvar = np.empty((len(Xs), d))
        for j in range(d):
            V = solve_triangular(self.L, G[j].T, lower=True)
            dvar[:, j] = prior[j] - np.einsum("nm,nm->m", V, V)
        return dmean, dvar

    def lml(self):
        n, k = self.Y.shape
        return float(-0.5 * np.sum(self.Y * self.alpha) - k * np.sum(np.log(np.diag(self.L)))
                     - 0.5 * n * k * np.log(2.0 * np.pi))

    def lml_grad(self):
        """d LML / d log theta, theta = (lengthscales..., sf2, sn2), summed over the target columns"""
        k = self.Y.shape[1]
        W = self.alpha @ self.alpha.T - k * cho_solve((self.L, True), np.eye(len(self.X)))
        return np.array([0.5 * np.sum(W * dK) for dK in kernel_dtheta(self.X, self.kernel, self.ls, self.sf2,
                                                                        self.sn2)])
