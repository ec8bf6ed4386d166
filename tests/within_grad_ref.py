"""Dense fp64 NumPy/SciPy reference of the LML gradient of the hierarchical path model (gpx_lml_grad_paths), on top of
tests/within_ref.py (``fit_ref``) and ``score_ref.kernel_matrix``.

With e_c = (x_ic - x_jc) / l_c, r^2 = sum_c e_c^2, u_c = (x_ic - x_jc) / l_path,c, r_p^2 = sum_c u_c^2, m_ij = [id_i == id_j
and id_i >= 0] and kd the family's function (``value_kd`` below, written out here, not taken from the library)

    K_ij = sf2 k(r) + m_ij sg2 k(r_p) + (sn2 w_i + jitter) delta_ij

    theta      (dK / dlog theta)_ij
    l_c        kd(r; sf2) e_c^2            (the path term does not depend on l)
    sf2        sf2 k(r)                    (the f part only)
    sn2        sn2 w_i delta_ij
    sg2        m_ij sg2 k(r_p)
    l_path,c   m_ij kd(r_p; sg2) u_c^2

(one lengthscale for every dimension: the sum over c).  The gradient 1/2 (sum_c alpha_c^T dK alpha_c - k tr(K^-1 dK)) is
formed two ways, with an explicit inverse and with triangular solves; tests/test_within_grad_ref.py holds every piece
against central differences.  Also the cases of the GPU tests (``GPU_CASES``, ``PAIRS``)."""
import os
import sys

import numpy as np
from scipy.linalg import solve_triangular

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import within_ref as wr  # noqa: E402
from score_ref import kernel_matrix  # noqa: E402

KERNELS = ("rbf", "matern52", "matern32", "matern12")
SF2, SG2, SN2 = 1.5, 0.4, 1e-2
JITTER = 1e-10 * SF2        # GP's default
K_TARGETS = 2


def _ls(ls, d):
    ls = np.atleast_1d(np.asarray(ls, dtype=np.float64))
    return np.full(d, ls[0]) if ls.size == 1 else ls


def value_kd(r2, kernel, s2):
    """(s2 k(r), kd): d (s2 k) / d log l_c = kd e_c^2"""
    if kernel == "rbf":
        v = s2 * np.exp(-0.5 * r2)
        return v, v
    if kernel == "matern52":
        s = np.sqrt(5.0 * r2)
        e = np.exp(-s)
        return s2 * (1.0 + s + s * s / 3.0) * e, s2 * (5.0 / 3.0) * (1.0 + s) * e
    if kernel == "matern32":
        s = np.sqrt(3.0 * r2)
        e = np.exp(-s)
        return s2 * (1.0 + s) * e, 3.0 * s2 * e
    r = np.sqrt(r2)
    v = s2 * np.exp(-r)
    with np.errstate(divide="ignore", invalid="ignore"):
        return v, np.where(r > 0, v / r, 0.0)


def _scaled_sq(A, B, ls):
    """(d, na, nb): ((a_c - b_c) / l_c)^2"""
    A, B = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
    U = (A[:, None, :] - B[None, :, :]) / _ls(ls, A.shape[1])
    return (U * U).transpose(2, 0, 1)


def _same(ga, gb):
    ga, gb = np.asarray(ga), np.asarray(gb)
    return (ga[:, None] == gb[None, :]) & (ga[:, None] >= 0)


def path_dtheta_ref(A, ga, B, gb, kernel, ls_path, sg2):
    """(1 + n_ls_path, na, nb): [0] m sg2 k(r_p), [1 + c] its derivative by log l_path,c — gpx_kernel_path_dtheta_matrix"""
    E2 = _scaled_sq(A, B, ls_path)
    v, kd = value_kd(E2.sum(axis=0), kernel, sg2)
    m = _same(ga, gb)
    n_lsp = np.atleast_1d(np.asarray(ls_path)).size
    out = [np.where(m, v, 0.0)]
    out += [np.where(m, kd * E2.sum(axis=0), 0.0)] if n_lsp == 1 else [np.where(m, kd * E2[c], 0.0) for c in range(n_lsp)]
    return np.stack(out)


def dK(p, kernel):
    """the matrices d K / d log theta of case p, theta = (l.., sf2, sn2, sg2, l_path..)"""
    X, ids = p["X"], p["ids"]
    n_ls = np.atleast_1d(np.asarray(p["ls"])).size
    E2 = _scaled_sq(X, X, p["ls"])
    _, kd = value_kd(E2.sum(axis=0), kernel, SF2)
    out = [kd * E2.sum(axis=0)] if n_ls == 1 else [kd * E2[c] for c in range(n_ls)]
    out.append(kernel_matrix(X, X, kernel, _ls(p["ls"], X.shape[1]), SF2))
    out.append(np.diag(SN2 * (np.ones(len(X)) if p["w"] is None else p["w"])))
    out.extend(path_dtheta_ref(X, ids, X, ids, kernel, p["lsp"], SG2))
    return out


def fit_case(p, kernel, ls=None, sf2=SF2, sn2=SN2, lsp=None, sg2=SG2):
    return wr.fit_ref(p["X"], p["ids"], p["Y"], kernel, p["ls"] if ls is None else ls, sf2, sn2,
                      p["lsp"] if lsp is None else lsp, sg2, w=p["w"], jitter=JITTER)


def full_K(fit):
    return fit["L"] @ fit["L"].T


def lml_grad_solves(p, kernel, fit):
    """1/2 (sum_c alpha_c^T dK alpha_c - k tr(L^-1 dK L^-T)) through triangular solves"""
    k, out = fit["alpha"].shape[1], []
    for D in dK(p, kernel):
        V = solve_triangular(fit["L"], D, lower=True)
        tr = np.trace(solve_triangular(fit["L"], V.T, lower=True))
        out.append(0.5 * (np.sum(fit["alpha"] * (D @ fit["alpha"])) - k * tr))
    return np.array(out)


def weight_matrix(fit):
    """W = sum_c alpha_c alpha_c^T - k K^-1, with the explicit inverse"""
    return fit["alpha"] @ fit["alpha"].T - fit["alpha"].shape[1] * np.linalg.inv(full_K(fit))


def lml_grad_inverse(p, kernel, fit):
    W = weight_matrix(fit)
    return np.array([0.5 * np.sum(W * D) for D in dK(p, kernel)])


def wrong_variance_entry(p, kernel, fit):
    """the whole-K contraction 1/2 sum W (K - diag): what the variance entry must NOT be on a fit with path ids"""
    K = full_K(fit)
    return 0.5 * np.sum(weight_matrix(fit) * (K - np.diag(np.diag(K) - (SF2 + SG2 * (np.asarray(p["ids"]) >= 0)))))


# ---- the cases of the GPU tests: all k = 2, sf2 = 1.5, sg2 = 0.4, sn2 = 1e-2, drawn with within_ref.problem(seed=3) -------------
def _draw(P=12, d=1, ls=0.25, lsp=0.1):
    p = wr.problem(P=P, L=33, k=K_TARGETS, ls=ls, sf2=SF2, ls_path=lsp, sg2=SG2, sn2=SN2, seed=3, d=d)
    p.update(ls=np.atleast_1d(np.asarray(ls, dtype=np.float64)), lsp=np.atleast_1d(np.asarray(lsp, dtype=np.float64)), w=None)
    return p


def sorted_d1():
    """N = 396: four 128-tiles with a ragged last one, paths straddle tile borders, off-diagonal tiles have no same-path pair"""
    return _draw()


def shuffled_d3():
    """the same P and L at d = 3, ARD both; rows permuted and every 17th id -1: every tile holds same-path pairs"""
    p = _draw(d=3, ls=np.linspace(0.25, 0.4, 3), lsp=np.linspace(0.1, 0.15, 3))
    perm = np.random.default_rng(17).permutation(len(p["X"]))
    ids = p["ids"][perm].copy()
    ids[::17] = -1
    p.update(X=np.ascontiguousarray(p["X"][perm]), Y=np.ascontiguousarray(p["Y"][perm]), ids=ids.astype(np.int32))
    return p


def nine_tiles_d2():
    """N = 1122, sorted: nine 128-tiles, the second super-tile of the triangular map; the D = 2 instantiation"""
    return _draw(P=34, d=2, ls=np.linspace(0.25, 0.4, 2), lsp=np.linspace(0.1, 0.15, 2))


def ls_d_path_1():
    return _draw(d=2, ls=np.linspace(0.25, 0.4, 2), lsp=0.1)


def ls_1_path_d():
    return _draw(d=2, ls=0.25, lsp=np.linspace(0.1, 0.15, 2))


def weighted():
    p = _draw()
    w = np.random.default_rng(99).uniform(0.5, 2.0, len(p["X"]))
    w[200] = 0.0
    p["w"] = w
    return p


def sorted_d4():
    """d = 4, ARD both: the run-time-d instantiation of the trace kernel (d = 1, 2, 3 have instantiations of their own)"""
    return _draw(d=4, ls=np.linspace(0.25, 0.4, 4), lsp=np.linspace(0.1, 0.15, 4))


GPU_CASES = {"sorted_d1": sorted_d1, "shuffled_d3": shuffled_d3, "nine_tiles_d2": nine_tiles_d2, "ls_d_path_1": ls_d_path_1,
             "ls_1_path_d": ls_1_path_d, "weighted": weighted, "sorted_d4": sorted_d4}
# all four families on the first two, Matern-3/2 on the others
PAIRS = [(n, k) for n in ("sorted_d1", "shuffled_d3") for k in KERNELS] + \
        [(n, "matern32") for n in GPU_CASES if n not in ("sorted_d1", "shuffled_d3")]

_problems, _cache = {}, {}


def problem(name):
    if name not in _problems:
        _problems[name] = GPU_CASES[name]()
    return _problems[name]


def case(name, kernel="matern32"):
    """(inputs, fit_ref's fit, lml summed over the targets, gradient (n_ls + 3 + n_ls_path)), computed once and shared"""
    if (name, kernel) not in _cache:
        p = problem(name)
        fit = fit_case(p, kernel)
        _cache[name, kernel] = (p, fit, float(np.sum(fit["lml"])), lml_grad_solves(p, kernel, fit))
    return _cache[name, kernel]
