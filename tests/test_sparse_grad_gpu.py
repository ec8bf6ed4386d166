"""GPU: the gradient of the inducing-point bound (SparseGP.elbo_gradient, gpx_sparse_elbo_grad) against its NumPy
definition (tests/sparse_grad_ref.py), against the dense GP's LML gradient where the bound IS the LML, its contraction
kernel alone (gpx_cross_dtheta_contract) inside its rounding bound, and SparseGP.optimize.

Bars.  The gradient metric is max_i |g_i - f_i| / (|f_i| + 1e-3 max_j |f_j|) (sparse_grad_ref.metric).  BAR = 1e-6 is the
project's parity bar; TIGHT_BAR is one decade above the largest metric measured over the eight parity cases on one MI355X
(profiles/sparse_grad_parity.json, written by tools/sparse_grad_parity.py) — measured against the NumPy definition, never
against the GPU's own output.  KERNEL_BAR = 1e-10 of sum |W_ij| |dK_ij| for the kernel alone: its sums have at most 130 * 130
terms, so the summation error is below 130 * 130 * 2^-53 = 2e-12 of that scale, and the rest is a few ulp of exp / sqrt.
Every test prints its figures before it asserts."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import sparse_grad_ref  # noqa: E402
import sparse_ref  # noqa: E402
from gaussianprocesspathmodelling_amd import GP, SparseGP, _abi  # noqa: E402

pytestmark = pytest.mark.gpu

BAR, KERNEL_BAR = 1e-6, 1e-10
TIGHT_BAR = 6.84e-8       # measured at most 6.84e-09 ("rbf-d1-N2100-m257-j1e-8"; profiles/sparse_grad_parity.json)
SF2, SN2 = sparse_ref.SF2, sparse_ref.SN2
_PD = C.POINTER(C.c_double)


# ---- 1. the contraction kernel alone ---------------------------------------------------------------------------------

def contract(gpx, kernel, A, B, W, ls, sf2):
    ls = np.atleast_1d(np.asarray(ls, dtype=np.float64))
    out = np.full(ls.size + 1, np.nan)
    A, B, W = (np.ascontiguousarray(a, dtype=np.float64) for a in (A, B, W))
    rc = gpx.gpx_cross_dtheta_contract(_abi.KERNEL_IDS[kernel], _abi.dptr(A), A.shape[0], _abi.dptr(B), B.shape[0], A.shape[1],
                                       _abi.dptr(W), _abi.dptr(ls), ls.size, sf2, _abi.dptr(out))
    assert rc == 0, gpx.gpx_last_error(None)
    return out


def kernel_ratio(gpx, kernel, A, B, W, ls, sf2):
    """max_t |out_t - ref_t| / sum |W_ij| |dK_ij|, after checking that a second call returns the same bits"""
    out = contract(gpx, kernel, A, B, W, ls, sf2)
    assert np.array_equal(out, contract(gpx, kernel, A, B, W, ls, sf2))
    ref, scale = sparse_grad_ref.contract(W, A, B, kernel, ls, sf2)
    assert np.all(np.isfinite(out)) and out.shape == ref.shape
    return float(np.max(np.abs(out - ref) / np.maximum(scale, np.finfo(float).tiny)))


def kernel_shapes():
    return [(na, nb, d) for na in (1, 63, 64, 130) for nb in (1, 64, 130) for d in (1, 3, 5)]


def kernel_case(kernel, ard, na, nb, d):
    rng = np.random.default_rng(1000 * na + 10 * nb + d + (500 if ard else 0))
    A, B = rng.uniform(0.0, 1.0, (na, d)), rng.uniform(0.0, 1.0, (nb, d))
    W = rng.standard_normal((na, nb))                       # mixed signs
    ls = 0.4 * (1.0 + 0.3 * np.arange(d)) if ard else 0.5
    return A, B, W, ls


def largest_kernel_ratio(gpx):
    """over every family, scalar and ARD lengthscales and every shape (also what profiles/sparse_grad_parity.json records)"""
    return max(kernel_ratio(gpx, kernel, *kernel_case(kernel, ard, na, nb, d), 1.3)
               for kernel in sparse_ref.KERNELS for ard in (False, True) for na, nb, d in kernel_shapes())


@pytest.mark.parametrize("ard", [False, True], ids=["scalar", "ard"])
@pytest.mark.parametrize("kernel", sparse_ref.KERNELS)
def test_contraction_kernel_inside_its_rounding_bound(gpx, kernel, ard):
    worst = 0.0
    for na, nb, d in kernel_shapes():
        ratio = kernel_ratio(gpx, kernel, *kernel_case(kernel, ard, na, nb, d), 1.3)
        worst = max(worst, ratio)
        assert ratio < KERNEL_BAR, (kernel, ard, na, nb, d, ratio)
    print(f"{kernel} ard={ard}: largest |out - ref| / sum |W| |dK| = {worst:.2e}")


@pytest.mark.parametrize("kernel", sparse_ref.KERNELS)
def test_contraction_kernel_with_coincident_points(gpx, kernel):
    """several rows of A are rows of B (Z drawn from X; the Kuu diagonal): finite, and inside the same bound"""
    rng = np.random.default_rng(7)
    B = rng.uniform(0.0, 1.0, (130, 3))
    A = rng.uniform(0.0, 1.0, (70, 3))
    A[::5] = B[3:3 + 14 * 9:9]
    W = rng.standard_normal((70, 130))
    for ls in (0.5, np.array([0.4, 0.5, 0.7])):
        ratio = kernel_ratio(gpx, kernel, A, B, W, ls, 1.3)
        print(f"{kernel} coincident, n_ls={np.size(ls)}: {ratio:.2e}")
        assert ratio < KERNEL_BAR
    Z = rng.uniform(0.0, 1.0, (65, 3))                       # Z against Z: the whole diagonal coincides
    G = rng.standard_normal((65, 65))
    ratio = kernel_ratio(gpx, kernel, Z, Z, G + G.T, 0.5, 1.3)
    print(f"{kernel} Z against Z: {ratio:.2e}")
    assert ratio < KERNEL_BAR


def test_contraction_refusals(gpx):
    out = np.full(2, 7.0)
    one = np.ones(1)
    p = _abi.dptr(one)
    assert gpx.gpx_cross_dtheta_contract(0, p, 0, p, 1, 1, p, p, 1, 1.0, _abi.dptr(out)) == _abi.E_ARG
    assert gpx.gpx_cross_dtheta_contract(9, p, 1, p, 1, 1, p, p, 1, 1.0, _abi.dptr(out)) == _abi.E_ARG
    assert gpx.gpx_cross_dtheta_contract(0, p, 1, p, 1, 2, p, p, 3, 1.0, _abi.dptr(out)) == _abi.E_ARG
    assert list(out) == [7.0, 7.0]


# ---- 2. end-to-end parity with the NumPy definition ------------------------------------------------------------------

def fit_case(case, chunk=None):
    D = sparse_ref.case_data(case)
    gp = SparseGP(case["kernel"], D["ls"], SF2, SN2, jitter=case["jitter"], chunk=case["chunk"] if chunk is None else chunk)
    gp.fit(D["X"], D["y"], inducing=D["Z"], noise_weights=D["w"])
    return gp, D


_REF = {}


def reference(case):
    """(F, grad) of the NumPy definition, computed once per case"""
    if case["id"] not in _REF:
        D = sparse_ref.case_data(case)
        _REF[case["id"]] = sparse_grad_ref.gradient(case["kernel"], D["ls"], SF2, SN2, case["jitter"], D["X"], D["y"], D["Z"],
                                                    D["w"])
    return _REF[case["id"]]


def parity_figures(case):
    """the figures of one case (also what profiles/sparse_grad_parity.json records)"""
    gp, D = fit_case(case)
    with gp:
        F, g = gp.elbo_gradient()
        assert F == float(gp.elbo().sum())
    Fr, gr = reference(case)
    assert g.shape == gr.shape == (np.size(D["ls"]) + 2,)
    return {"grad": sparse_grad_ref.metric(g, gr), "elbo": abs(F - Fr) / max(abs(Fr), 1.0)}


@pytest.mark.parametrize("case", sparse_ref.CASES, ids=[c["id"] for c in sparse_ref.CASES])
def test_gradient_parity_with_the_numpy_definition(case):
    fig = parity_figures(case)
    print(case["id"], {k: f"{v:.2e}" for k, v in fig.items()})
    assert fig["grad"] < BAR and fig["elbo"] < BAR, fig
    assert fig["grad"] < TIGHT_BAR, fig


def test_the_tight_bar_is_one_decade_above_the_measurement():
    rec = json.load(open(os.path.join(ROOT, "profiles", "sparse_grad_parity.json")))
    assert {f["case"] for f in rec["fits"]} == {c["id"] for c in sparse_ref.CASES}
    largest = max(f["grad"] for f in rec["fits"])
    assert largest == rec["largest"] and largest < TIGHT_BAR <= 10.0 * largest * (1.0 + 1e-12) and TIGHT_BAR <= BAR
    assert rec["kernel_largest"] < KERNEL_BAR


# ---- 3. identity with the dense library ------------------------------------------------------------------------------

def dense_identity_figure(kernel):
    """Z = the shared grid, jitter = 0: the bound is the LML for every theta, so elbo_gradient() is GP.lml_gradient()"""
    X, y, grid = sparse_ref.path_grid_problem(40, 33, 5)
    with SparseGP(kernel, 0.25, SF2, SN2, jitter=0.0) as sp, GP(kernel, 0.25, SF2, SN2, jitter=0.0, max_tries=1) as gp:
        F, g = sp.fit(X, y, inducing=grid).elbo_gradient()
        lml, gd = gp.fit(X, y).lml_gradient()
    return sparse_grad_ref.metric(g, gd), abs(F - lml) / max(abs(lml), 1.0)


@pytest.mark.parametrize("kernel", ["matern32", "matern12"])
def test_gradient_is_the_dense_gps_where_the_bound_is_the_lml(kernel):
    fig, felbo = dense_identity_figure(kernel)
    print(f"{kernel}: gradient {fig:.2e}, bound against LML {felbo:.2e}")
    assert fig < BAR and felbo < BAR


# ---- 4. what may and may not change ----------------------------------------------------------------------------------

@pytest.mark.parametrize("case", [sparse_ref.CASES[0], sparse_ref.CASES[2]], ids=lambda c: c["id"])
def test_chunk_size_changes_rounding_only(case):
    a, _ = fit_case(case, chunk=256)
    b, _ = fit_case(case, chunk=0)
    with a, b:
        other = b.chunk_
        assert a.chunk_ == 256 and other != 256
        (_, ga), (_, gb) = a.elbo_gradient(), b.elbo_gradient()
    fig = sparse_grad_ref.metric(ga, gb)
    print(case["id"], f"chunk 256 against {other}: {fig:.2e}")
    assert fig < BAR


def test_two_calls_are_bit_identical_and_predict_keeps_its_bits():
    case = sparse_ref.CASES[6]
    gp, D = fit_case(case)
    with gp:
        m0, v0 = gp.predict(D["Xs"])
        e0 = gp.elbo()
        F1, g1 = gp.elbo_gradient()
        m1, v1 = gp.predict(D["Xs"])
        F2, g2 = gp.elbo_gradient()
        assert F1 == F2 and np.array_equal(g1, g2)
        assert np.array_equal(m0, m1) and np.array_equal(v0, v1) and np.array_equal(e0, gp.elbo())
        _, c0 = gp.predict(D["Xs"], return_cov=True)
    other, _ = fit_case(case)                                # a fresh handle: the same bits again
    with other:
        F3, g3 = other.elbo_gradient()
        _, c3 = other.predict(D["Xs"], return_cov=True)
    assert F3 == F1 and np.array_equal(g3, g1) and np.array_equal(c0, c3)


def test_device_tensors_give_the_same_bits():
    import torch
    case = sparse_ref.CASES[2]
    gp, D = fit_case(case)
    with gp:
        F0, g0 = gp.elbo_gradient()
    dev = torch.device("cuda", 0)
    t = lambda a: torch.as_tensor(a, device=dev)  # noqa: E731
    with SparseGP(case["kernel"], D["ls"], SF2, SN2, jitter=case["jitter"], chunk=case["chunk"]) as gp:
        gp.fit(t(D["X"]), t(D["y"]), inducing=t(D["Z"]), noise_weights=t(D["w"]))
        F1, g1 = gp.elbo_gradient()
    assert F1 == F0 and np.array_equal(g1, g0)


def test_refusals_leave_the_fit_valid(gpx):
    case = sparse_ref.CASES[3]
    gp, D = fit_case(case)
    with gp:
        _, g0 = gp.elbo_gradient()
        m0, v0 = gp.predict(D["Xs"])
        X, y = np.ascontiguousarray(D["X"]), np.ascontiguousarray(D["y"])
        grad, elbo = np.full(g0.size, 7.0), np.full(1, 7.0)
        px, py = C.c_void_p(X.ctypes.data), C.c_void_p(y.ctypes.data)
        call = lambda h, n, g=grad: gpx.gpx_sparse_elbo_grad(h, px, py, None, n, 0, _abi.dptr(elbo), _abi.dptr(g))  # noqa: E731
        assert call(gp._h, len(X) - 1) == _abi.E_ARG and b"N differs" in gpx.gpx_last_error(gp._h)
        assert call(gp._h, len(X) + 1) == _abi.E_ARG
        assert gpx.gpx_sparse_elbo_grad(gp._h, None, py, None, len(X), 0, None, _abi.dptr(grad)) == _abi.E_ARG
        assert gpx.gpx_sparse_elbo_grad(gp._h, px, py, None, len(X), 5, None, _abi.dptr(grad)) == _abi.E_ARG
        assert np.all(grad == 7.0) and elbo[0] == 7.0        # a refused call writes nothing
        m1, v1 = gp.predict(D["Xs"])
        assert np.array_equal(m0, m1) and np.array_equal(v0, v1)
        assert np.array_equal(gp.elbo_gradient()[1], g0)
    with GP(kernel="rbf", lengthscale=0.5) as dense:         # a dense-fitted handle, then an unfitted one
        dense.fit(D["X"], D["y"])
        assert call(dense._h, len(X)) == _abi.E_ARG and b"dense fit" in gpx.gpx_last_error(dense._h)
        assert dense.predict(D["Xs"])[0].shape == (len(D["Xs"]),)
    with SparseGP("rbf", 0.5) as fresh:
        assert call(fresh._h, len(X)) == _abi.E_ARG and b"no successful gpx_sparse_fit" in gpx.gpx_last_error(fresh._h)
        with pytest.raises(RuntimeError):
            fresh.elbo_gradient()
    assert np.all(grad == 7.0) and elbo[0] == 7.0


# ---- 5. optimize -----------------------------------------------------------------------------------------------------

def test_optimize_learns_on_the_bound():
    X, y, grid = sparse_ref.path_grid_problem(20, 33, 9)
    start = dict(kernel="matern52", lengthscale=2.1, variance=1.0, noise=0.01)   # 3x too long: the bound peaks at 0.71
    with SparseGP(**start) as gp:
        f0 = float(gp.fit(X, y, inducing=grid).elbo().sum())
        res = gp.optimize(X, y, inducing=grid)
        f1 = float(gp.elbo().sum())
        print(f"analytic: bound {f0:.4f} -> {f1:.4f} in {res.nit} iterations, {res.nfev} evaluations; lengthscale "
              f"{gp.lengthscale}, variance {gp.variance:.4g}, noise {gp.noise:.4g}")
        assert f1 >= f0 and res.fun == -f1
        assert np.array_equal(res.x, np.log([gp.lengthscale[0], gp.variance, gp.noise]))
        assert gp.lengthscale[0] != 2.1 and gp.variance != 1.0 and gp.noise != 0.01
        assert gp.jitter == 1e-8 * gp.variance               # the default jitter follows the variance
        assert gp.predict(grid)[0].shape == (33, 2)
    with SparseGP(**start) as gp:
        res3 = gp.optimize(X, y, inducing=grid, jac="3-point")
        f3 = float(gp.elbo().sum())
        print(f"3-point: bound {f3:.4f} in {res3.nit} iterations, {res3.nfev} evaluations")
        assert res3.fun == -f3 and abs(f3 - f1) < 1e-3
    with SparseGP(**start, jitter=1e-7) as gp:               # a jitter that was given stays; an int is resolved once
        gp.optimize(X, y, inducing=33, params=("lengthscale",), maxiter=5)
        assert gp.jitter == 1e-7 and gp.variance == 1.0 and gp.noise == 0.01 and gp.lengthscale[0] != 2.1
        assert np.array_equal(gp.inducing_, grid)
        with pytest.raises(ValueError):
            gp.optimize(X, y, inducing=grid, params=("lengthscale", "jitter"))
