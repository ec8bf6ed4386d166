"""fp64 NumPy/SciPy reference of the LML gradient of a GP with derivative observations (gpx_lml_grad_full), on top of
tests/dobs_ref.py.

With u = (x_a - x_b) / l per dimension, r^2 = sum u^2, v, g, h of the family (dobs_ref.vgh) and p = -2 d h / d (r^2)

    RBF         p = v
    Matern-5/2  p = sf2 (125/3) e^-s / s,           s = sqrt5 r, 0 at r = 0
    Matern-3/2  p = 27 sf2 e^-s (1 + s) / s^3,      s = sqrt3 r, 0 at r = 0

the derivative of the Gram entry E of kinds (ka, kb) is  d E / d log l_c = A u_c^2 + (delta(ka, c) + delta(kb, c)) B  with

    (-1, -1)  A = g                                  B = 0
    (-1,  j)  A = h u_j / l_j                        B = -2 g u_j / l_j
    ( i, -1)  A = -h u_i / l_i                       B = +2 g u_i / l_i
    ( i,  j)  A = (h delta_ij - p u_i u_j) / (l_i l_j)    B = (2 h u_i u_j - g delta_ij) / (l_i l_j)

(one lengthscale for every dimension: the sum over c).  d K / d log sf2 is the noise-free mixed Gram, d K / d log sn2 =
sn2 w_i on the value rows and d K / d log sn2_deriv = sn2_deriv w_i on the derivative rows.  The gradient
1/2 (sum_c alpha_c^T dK alpha_c - k tr(K^-1 dK)) is formed two ways, with an explicit inverse and with triangular solves;
tests/test_dobs_grad_ref.py holds every piece against central differences.  Also the N = 1100 case of the GPU tests."""
import numpy as np
from scipy.linalg import solve_triangular

import dobs_ref
from dobs_ref import DobsGP, lengthscales, mixed_gram


def vghp(r2, kernel, sf2):
    v, g, h = dobs_ref.vgh(r2, kernel, sf2)
    if kernel == "rbf":
        return v, g, h, v
    s = np.sqrt((5.0 if kernel == "matern52" else 3.0) * r2)
    e = np.exp(-s)
    with np.errstate(divide="ignore", invalid="ignore"):
        if kernel == "matern52":
            p = np.where(s > 0, sf2 * (125.0 / 3.0) * e / s, 0.0)
        else:
            p = np.where(s > 0, 27.0 * sf2 * e * (1.0 + s) / s ** 3, 0.0)
    return v, g, h, p


def mixed_gram_dl(A, ka, B, kb, kernel, ls, sf2):
    """(n_ls, na, nb): d mixed_gram / d log lengthscale[c]; n_ls = 1 for a scalar ``ls``"""
    A, B = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
    ka, kb = np.asarray(ka, dtype=np.int64), np.asarray(kb, dtype=np.int64)
    d = A.shape[1]
    n_ls = np.atleast_1d(np.asarray(ls)).size
    l = lengthscales(ls, d)
    U = A[:, None, :] / l - B[None, :, :] / l
    r2 = np.sum(U * U, axis=2)
    v, g, h, p = vghp(r2, kernel, sf2)
    ia, ib = np.maximum(ka, 0), np.maximum(kb, 0)
    ua = np.take_along_axis(U, np.broadcast_to(ia[:, None, None], U.shape[:2] + (1,)), axis=2)[:, :, 0]
    ub = np.take_along_axis(U, np.broadcast_to(ib[None, :, None], U.shape[:2] + (1,)), axis=2)[:, :, 0]
    la, lb = l[ia][:, None], l[ib][None, :]
    da, db = (ka >= 0)[:, None], (kb >= 0)[None, :]
    same = ka[:, None] == kb[None, :]
    Am = np.where(~da & ~db, g, 0.0)
    Bm = np.zeros_like(Am)
    Am = np.where(~da & db, h * ub / lb, Am)
    Bm = np.where(~da & db, -2.0 * g * ub / lb, Bm)
    Am = np.where(da & ~db, -h * ua / la, Am)
    Bm = np.where(da & ~db, 2.0 * g * ua / la, Bm)
    Am = np.where(da & db, (h * same - p * ua * ub) / (la * lb), Am)
    Bm = np.where(da & db, (2.0 * h * ua * ub - g * same) / (la * lb), Bm)
    if n_ls == 1:
        return (Am * r2 + (da.astype(float) + db.astype(float)) * Bm)[None]
    out = np.empty((d,) + Am.shape)
    for c in range(d):
        out[c] = Am * U[:, :, c] ** 2 + ((ka == c)[:, None].astype(float) + (kb == c)[None, :].astype(float)) * Bm
    return out


def dK(gp, w=None):
    """the n_ls + 3 matrices d K / d log theta of a fitted DobsGP, theta = (lengthscales.., sf2, sn2, sn2_deriv)"""
    X, kinds = gp.X, gp.kinds
    w = np.ones(len(X)) if w is None else np.asarray(w, dtype=np.float64)
    out = list(mixed_gram_dl(X, kinds, X, kinds, gp.kernel, gp.ls, gp.sf2))
    out.append(mixed_gram(X, kinds, X, kinds, gp.kernel, gp.ls, gp.sf2))
    out.append(np.diag(np.where(kinds < 0, gp.sn2 * w, 0.0)))
    out.append(np.diag(np.where(kinds >= 0, gp.sn2_deriv * w, 0.0)))
    return out


def lml_grad_inverse(gp, w=None):
    """1/2 sum_ij (alpha alpha^T - k K^-1)_ij dK_ij with the explicit inverse"""
    k = gp.Y.shape[1]
    Kinv = np.linalg.inv(gp.K)
    Q = gp.alpha @ gp.alpha.T - k * Kinv
    return np.array([0.5 * np.sum(Q * D) for D in dK(gp, w)])


def lml_grad_solves(gp, w=None):
    """the same through triangular solves: tr(K^-1 dK) = tr(L^-1 dK L^-T)"""
    k = gp.Y.shape[1]
    out = []
    for D in dK(gp, w):
        V = solve_triangular(gp.L, D, lower=True)
        tr = np.trace(solve_triangular(gp.L, V.T, lower=True))
        out.append(0.5 * (np.sum(gp.alpha * (D @ gp.alpha)) - k * tr))
    return np.array(out)


def dl_problem(d, seed=10):
    """inputs of the element-wise test of d gram / d log l: 70 x 50 rows of mixed kinds in d dimensions, the first 20 pairs
    (i, i) coincident — values against derivative rows, and derivative rows of one dimension against each other"""
    rng = np.random.default_rng(seed + d)
    na, nb = 70, 50
    A, B = rng.uniform(size=(na, d)), rng.uniform(size=(nb, d))
    B[:20] = A[:20]
    ka, kb = rng.integers(-1, d, na).astype(np.int32), rng.integers(-1, d, nb).astype(np.int32)
    ka[:10], kb[:10] = -1, np.arange(10) % d
    ka[10:15], kb[10:15] = 0, 0
    return A, ka, B, kb


# ---- the N = 1100 case: nine 128-tiles (the second super-tile of the triangular map), the D = 2 instantiation ------------------
BIG_N_VAL, BIG_N_DER = 800, 300
BIG_LS = (0.3, 0.25)


def big_problem(seed=4242):
    rng = np.random.default_rng(seed)
    d, k = 2, 1
    f, df = dobs_ref._curve(rng, d, k)
    X = rng.uniform(0.0, 1.0, (BIG_N_VAL, d))
    Xd = rng.uniform(0.0, 1.0, (BIG_N_DER, d))
    dims = rng.integers(0, d, BIG_N_DER)
    y = (f(X) + 0.1 * rng.standard_normal((BIG_N_VAL, k)))[:, 0]
    yd = (df(Xd, dims) + 0.2 * rng.standard_normal((BIG_N_DER, k)))[:, 0]
    kinds = np.concatenate([np.full(BIG_N_VAL, -1), dims]).astype(np.int32)
    return dict(kernel="matern52", ls=BIG_LS, sf2=dobs_ref.SF2, sn2=dobs_ref.SN2, sn2_deriv=dobs_ref.SN2_DERIV,
                jitter=dobs_ref.JITTER, X=X, y=y, Xd=Xd, dims=dims, yd=yd, Xall=np.concatenate([X, Xd]),
                yall=np.concatenate([y, yd]), kinds=kinds, w=None)


# the weighted case (weights != 1 on both kinds of rows) on the inputs of one table case
WEIGHTED_CASE = "matern32_d3_last"


def weighted_problem():
    c = dict(dobs_ref.CASES[WEIGHTED_CASE]())
    rng = np.random.default_rng(99)
    c["w"] = rng.uniform(0.3, 3.0, len(c["kinds"]))
    return c


GPU_CASES = dict(dobs_ref.CASES)
GPU_CASES["big_d2"] = big_problem
GPU_CASES["weighted"] = weighted_problem

_cache = {}


def case(name):
    """(inputs, fitted DobsGP, lml, gradient (n_ls + 3)) of GPU case `name`, computed once and shared"""
    if name not in _cache:
        c = GPU_CASES[name]()
        ref = DobsGP(c["kernel"], c["ls"], c["sf2"], c["sn2"], c["sn2_deriv"], c["jitter"]).fit(c["Xall"], c["kinds"], c["yall"],
                                                                                             c["w"])
        _cache[name] = (c, ref, ref.lml(), lml_grad_solves(ref, c["w"]))
    return _cache[name]
