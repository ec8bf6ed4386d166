"""fp64 NumPy/SciPy reference of the GP conditioned on derivative observations (include/gpx.h, gpx_set_observation_kinds).

Row i of a fit is an observation at x_i with a kind: -1 a value of f, j a value of d f / d x_j.  With u = (x_a - x_b) / l per
dimension, r^2 = sum u^2 and v, g, h of the family (csrc/gpx_cov.h) the Gram entry for kinds (a, b) is

    (-1, -1)  v               ( i, -1)  -g u_i / l_i
    (-1,  j)  g u_j / l_j     ( i,  j)  (g delta_ij - h u_i u_j) / (l_i l_j)

and the diagonal gets (kind_i < 0 ? sn2 : sn2_deriv) w_i + jitter.  Dense: the mixed Gram, alpha, the log-determinant, the
LML, the posterior mean / variance / covariance at value queries, the posterior gradient mean and variance, and the block
scores.  v, g and h are written out here (not taken from the oracle), so that tests/test_dobs_ref.py can hold them against
differences of ``oracle.gp_oracle.kernel_matrix``.  Also the table of the GPU test cases: the CPU and GPU tests share inputs."""
import numpy as np
from scipy.linalg import cholesky, solve_triangular

LOG_2PI = float(np.log(2.0 * np.pi))
KERNELS = ("rbf", "matern52", "matern32")
GRAD_PRIOR = {"rbf": 1.0, "matern52": 5.0 / 3.0, "matern32": 3.0}


def lengthscales(ls, d):
    return np.broadcast_to(np.atleast_1d(np.asarray(ls, dtype=np.float64)), (d,)).copy()


def vgh(r2, kernel, sf2):
    """v, g, h of the family at squared scaled distances r2 (h u_i u_j of Matern-3/2 is taken as 0 at r = 0: h = 0 there)"""
    r = np.sqrt(r2)
    if kernel == "rbf":
        v = sf2 * np.exp(-0.5 * r2)
        return v, v, v
    if kernel == "matern52":
        s = np.sqrt(5.0) * r
        e = np.exp(-s)
        return sf2 * (1.0 + s + s * s / 3.0) * e, sf2 * (5.0 / 3.0) * (1.0 + s) * e, sf2 * (25.0 / 3.0) * e
    if kernel == "matern32":
        s = np.sqrt(3.0) * r
        e = np.exp(-s)
        with np.errstate(divide="ignore", invalid="ignore"):
            h = np.where(s > 0, 9.0 * sf2 * e / s, 0.0)
        return sf2 * (1.0 + s) * e, 3.0 * sf2 * e, h
    raise ValueError(f"no derivative observations for kernel {kernel!r}")


def mixed_gram(A, ka, B, kb, kernel, ls, sf2):
    """(na, nb): the covariance of observations of kinds ka (na,) at A with observations of kinds kb (nb,) at B"""
    A, B = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
    ka, kb = np.asarray(ka, dtype=np.int64), np.asarray(kb, dtype=np.int64)
    d = A.shape[1]
    l = lengthscales(ls, d)
    U = A[:, None, :] / l - B[None, :, :] / l                       # (na, nb, d)
    v, g, h = vgh(np.sum(U * U, axis=2), kernel, sf2)
    ia, ib = np.maximum(ka, 0), np.maximum(kb, 0)
    ua = np.take_along_axis(U, np.broadcast_to(ia[:, None, None], U.shape[:2] + (1,)), axis=2)[:, :, 0]   # u_{ka}
    ub = np.take_along_axis(U, np.broadcast_to(ib[None, :, None], U.shape[:2] + (1,)), axis=2)[:, :, 0]   # u_{kb}
    la, lb = l[ia][:, None], l[ib][None, :]
    da, db = (ka >= 0)[:, None], (kb >= 0)[None, :]
    same = ka[:, None] == kb[None, :]
    out = np.where(~da & ~db, v, 0.0)
    out = np.where(da & ~db, -g * ua / la, out)
    out = np.where(~da & db, g * ub / lb, out)
    return np.where(da & db, (g * same - h * (ua * ub)) / (la * lb), out)


def noise_diag(kinds, w, sn2, sn2_deriv, jitter):
    kinds = np.asarray(kinds)
    w = np.ones(len(kinds)) if w is None else np.asarray(w, dtype=np.float64)
    return np.where(kinds < 0, sn2, sn2_deriv) * w + jitter


class DobsGP:
    """Exact GP on value and derivative observations, with SciPy's Cholesky."""

    def __init__(self, kernel, ls, sf2, sn2, sn2_deriv=0.0, jitter=0.0):
        self.kernel, self.ls, self.sf2 = kernel, ls, float(sf2)
        self.sn2, self.sn2_deriv, self.jitter = float(sn2), float(sn2_deriv), float(jitter)

    def gram(self, X, kinds, w=None):
        K = mixed_gram(X, kinds, X, kinds, self.kernel, self.ls, self.sf2)
        K[np.diag_indices_from(K)] += noise_diag(kinds, w, self.sn2, self.sn2_deriv, self.jitter)
        return K

    def fit(self, X, kinds, y, w=None):
        self.X = np.asarray(X, dtype=np.float64)
        self.kinds = np.asarray(kinds, dtype=np.int64)
        self.d = self.X.shape[1]
        self.y1d = np.ndim(y) == 1
        self.Y = np.asarray(y, dtype=np.float64).reshape(len(self.X), -1)
        self.K = self.gram(self.X, self.kinds, w)
        self.L = cholesky(self.K, lower=True)
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

    def _solved_cross(self, Xs, kq):
        Ks = mixed_gram(Xs, kq, self.X, self.kinds, self.kernel, self.ls, self.sf2)
        return solve_triangular(self.L, Ks.T, lower=True)           # (N, M)

    def _squeeze(self, mean):
        return mean[:, 0] if self.y1d else mean

    def predict(self, Xs):
        """mean ((M,) for a 1-D y, else (M, k)) and latent variance (M,) of f at Xs"""
        V = self._solved_cross(Xs, np.full(len(Xs), -1))
        return self._squeeze(V.T @ self.z), self.sf2 - np.einsum("nm,nm->m", V, V)

    def predict_cov(self, Xs):
        """mean and the joint (M, M) covariance of f at Xs"""
        none = np.full(len(Xs), -1)
        V = self._solved_cross(Xs, none)
        return self._squeeze(V.T @ self.z), mixed_gram(Xs, none, Xs, none, self.kernel, self.ls, self.sf2) - V.T @ V

    def prior_grad_var(self):
        return GRAD_PRIOR[self.kernel] * self.sf2 / lengthscales(self.ls, self.d) ** 2

    def predict_grad(self, Xs):
        """dmean (M, d, k) and the latent derivative variance dvar (M, d) of the posterior at Xs"""
        M = len(Xs)
        prior = self.prior_grad_var()
        dmean, dvar = np.empty((M, self.d, self.z.shape[1])), np.empty((M, self.d))
        for j in range(self.d):
            V = self._solved_cross(Xs, np.full(M, j))
            dmean[:, j, :] = V.T @ self.z
            dvar[:, j] = prior[j] - np.einsum("nm,nm->m", V, V)
        return dmean, dvar

    def score(self, Xq, Yq, Lg, diag_add):
        """block scores -> dict(logp (G, k), maha (G, k), logdet (G,), kappa (G,)) (tests/score_ref.py's, value queries)"""
        Xq = np.asarray(Xq, dtype=np.float64)
        Yq = np.asarray(Yq, dtype=np.float64).reshape(len(Xq), -1)
        M, k = Yq.shape
        G = M // Lg
        none = np.full(M, -1)
        V = self._solved_cross(Xq, none)
        mean = V.T @ self.z
        out = {"logp": np.empty((G, k)), "maha": np.empty((G, k)), "logdet": np.empty(G), "kappa": np.empty(G)}
        for g in range(G):
            sl = slice(g * Lg, (g + 1) * Lg)
            S = mixed_gram(Xq[sl], none[sl], Xq[sl], none[sl], self.kernel, self.ls, self.sf2) - V[:, sl].T @ V[:, sl]
            S = 0.5 * (S + S.T)
            S[np.diag_indices(Lg)] += diag_add
            Ls = cholesky(S, lower=True)
            r = solve_triangular(Ls, Yq[sl] - mean[sl], lower=True)
            ev = np.linalg.eigvalsh(S)
            out["kappa"][g] = ev[-1] / ev[0]
            out["maha"][g] = np.sum(r * r, axis=0)
            out["logdet"][g] = 2.0 * np.sum(np.log(np.diag(Ls)))
            out["logp"][g] = -0.5 * out["maha"][g] - 0.5 * out["logdet"][g] - 0.5 * Lg * LOG_2PI
        return out


# ---- the inputs of the GPU tests (tests/test_dobs_gpu.py), conditioned by tests/test_dobs_ref.py -------------------------------
SF2, SN2, SN2_DERIV = 1.5, 1e-2, 5e-2
N_VAL, N_DER, M_QUERY, BLOCK = 200, 70, 130, 128   # 270 rows: no multiple of 64 or 128, the kind boundary inside the tile
SCORE_G, SCORE_LG = 4, 33                          # [192, 256); block=128: three panels at the padded size 384
LS = {1: 0.3, 3: (0.3, 0.25, 0.4), 5: (0.5, 0.4, 0.6, 0.45, 0.55)}   # d = 1: a scalar; 3: ARD; 5: ARD, the generic-D kernels
TARGETS = {1: 1, 3: 2, 5: 1}
JITTER = 1e-10 * SF2


def _curve(rng, d, k):
    a = rng.uniform(2.0, 5.0, (d, k))

    def f(A):
        return np.sin(A @ a) + 0.3 * np.cos(2.0 * A.sum(axis=1, keepdims=True))

    def df(A, dims):
        return np.cos(A @ a) * a[dims, :] - 0.6 * np.sin(2.0 * A.sum(axis=1, keepdims=True))
    return f, df


def problem(kernel, d, order, seed):
    """One parity case: dict(kernel, ls, sf2, sn2, sn2_deriv, jitter, X (N, d), y, Xd (Nd, d), dims (Nd,), yd, Xs (M, d),
    Xq / Yq (G * Lg rows: the scored blocks), and the fitted rows in the order of the fit: Xall, yall, kinds, w = None).
    order "last": values then derivative rows (what GP.fit(derivatives=) builds); "mixed": the same rows interleaved at
    random (kinds through the C call)."""
    rng = np.random.default_rng(seed)
    k = TARGETS[d]
    f, df = _curve(rng, d, k)
    X = rng.uniform(0.0, 1.0, (N_VAL, d))
    Xd = rng.uniform(0.0, 1.0, (N_DER, d))
    dims = rng.integers(0, d, N_DER)
    y = f(X) + 0.1 * rng.standard_normal((N_VAL, k))
    yd = df(Xd, dims) + 0.2 * rng.standard_normal((N_DER, k))
    Xs = rng.uniform(-0.05, 1.05, (M_QUERY, d))
    t = np.linspace(0.0, 1.0, SCORE_LG)[None, :, None]
    p0, p1 = rng.uniform(0.0, 1.0, (SCORE_G, 1, d)), rng.uniform(0.0, 1.0, (SCORE_G, 1, d))
    Xq = (p0 + t * (p1 - p0)).reshape(-1, d)                         # every block a straight path through the box
    Yq = f(Xq) + 0.1 * rng.standard_normal((len(Xq), k))
    if k == 1:
        y, yd, Yq = y[:, 0], yd[:, 0], Yq[:, 0]
    Xall, yall = np.concatenate([X, Xd]), np.concatenate([y, yd])
    kinds = np.concatenate([np.full(N_VAL, -1), dims]).astype(np.int32)
    if order == "mixed":
        perm = rng.permutation(N_VAL + N_DER)
        Xall, yall, kinds = Xall[perm], yall[perm], kinds[perm]
    return dict(kernel=kernel, ls=LS[d], sf2=SF2, sn2=SN2, sn2_deriv=SN2_DERIV, jitter=JITTER, X=X, y=y, Xd=Xd, dims=dims, yd=yd,
                Xs=Xs, Xq=Xq, Yq=Yq, Xall=Xall, yall=yall, kinds=kinds, w=None)


WAYPOINT_T = np.array([0.1, 0.3, 0.5, 0.7, 0.9])


def waypoint_problem(seed=77):
    """The constraint case, d = 1: 30 noisy values, then five waypoints (w = 0) with exact velocities (sn2_deriv = 0) at the
    same five well-separated times — "pass through here with this velocity" as two exact observations each."""
    rng = np.random.default_rng(seed)
    f, df = _curve(rng, 1, 1)
    tw = WAYPOINT_T[:, None]
    Xn = rng.uniform(0.0, 1.0, (30, 1))
    X = np.concatenate([Xn, tw])
    y = np.concatenate([f(Xn)[:, 0] + 0.1 * rng.standard_normal(30), f(tw)[:, 0]])
    w = np.concatenate([np.ones(30), np.zeros(5)])
    dims = np.zeros(5, dtype=np.int64)
    yd = df(tw, dims)[:, 0]
    Xs = np.concatenate([tw, rng.uniform(0.0, 1.0, (20, 1))])         # the five times first
    kinds = np.concatenate([np.full(35, -1), dims]).astype(np.int32)
    return dict(kernel="matern52", ls=0.15, sf2=SF2, sn2=SN2, sn2_deriv=0.0, jitter=JITTER, X=X, y=y, Xd=tw, dims=dims, yd=yd, Xs=Xs,
                Xall=np.concatenate([X, tw]), yall=np.concatenate([y, yd]), kinds=kinds, w=np.concatenate([w, np.ones(5)]),
                w_values=w)


DIMS = (1, 3, 5)
ORDERS = ("last", "mixed")
CASES = {f"{kernel}_d{d}_{order}": (lambda kernel=kernel, d=d, order=order, i=i: problem(kernel, d, order, 1000 + i))
         for i, (kernel, d, order) in enumerate((kn, d, o) for kn in KERNELS for d in DIMS for o in ORDERS)}
CASES["waypoints"] = waypoint_problem

_cache = {}


def case(name):
    """the inputs of case `name` and its fitted reference, computed once and shared: (dict, DobsGP)"""
    if name not in _cache:
        c = CASES[name]()
        ref = DobsGP(c["kernel"], c["ls"], c["sf2"], c["sn2"], c["sn2_deriv"], c["jitter"])
        _cache[name] = (c, ref.fit(c["Xall"], c["kinds"], c["yall"], c["w"]))
    return _cache[name]
