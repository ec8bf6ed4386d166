"""GPU: the inducing-point GP (SparseGP, gpx_sparse_*) against its NumPy definition (tests/sparse_ref.py), against the
library's own dense GP where the two models coincide, and the TN kernel alone inside its rounding bound.

Bars.  BAR = 1e-6 is the project's parity bar (tests/test_loo_gpu.py): mean with floor 1e-6, variance purely relative, the
bound with floor 1.  TIGHT_BAR is one decade above the largest of those ratios measured over the parity cases on one
MI355X (profiles/sparse_parity.json, written by tools/sparse_parity.py).  FRESH_BAR = 1e-9 is the project's bar for one
quantity by two routes.  Every test prints its figures before it asserts."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import sparse_ref  # noqa: E402
from gaussianprocesspathmodelling_amd import GP, GpxError, SparseGP, _abi  # noqa: E402

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
BAR, FRESH_BAR = 1e-6, 1e-9
TIGHT_BAR = 2.28e-8       # measured at most 2.28e-09 (variance of "rbf-d1-N2100-m257-j1e-8"; profiles/sparse_parity.json)
SF2, SN2 = sparse_ref.SF2, sparse_ref.SN2


def rel_mean(a, b):
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-6)))


def rel_var(a, b):
    return float(np.max(np.abs(a - b) / np.abs(b)))


def rel_floor1(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b)) / np.maximum(np.abs(b), 1.0)))


# ---- 1. the TN kernel alone ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("rows", [1, 63, 64, 1000])
@pytest.mark.parametrize("n", [64, 192, 320])
def test_tn_kernel_inside_its_rounding_bound(gpx, n, rows, accumulate):
    """|out - ref| <= (rows + 16) 2^-53 (|C| + |X|^T |X|) per element of the lower triangle: worst-case summation of the
    `rows` products (and the term that was there); nothing above the diagonal is written"""
    rng = np.random.default_rng(1000 * n + rows)
    X = rng.standard_normal((rows, n))
    C0 = rng.standard_normal((n, n))
    out = C0.copy()
    rc = gpx.gpx_syrk_tn(_abi.dptr(out), n, _abi.dptr(X), rows, accumulate)
    assert rc == 0, gpx.gpx_last_error(None)
    ref = X.T @ X + (C0 if accumulate else 0.0)
    bound = (rows + 16) * U * (np.abs(X).T @ np.abs(X) + (np.abs(C0) if accumulate else 0.0))
    low = np.tril(np.ones((n, n), dtype=bool))
    ratio = float(np.max(np.abs(out - ref)[low] / bound[low]))
    print(f"n={n} rows={rows} accumulate={accumulate}: max |out - ref| / bound = {ratio:.3f}")
    assert ratio <= 1.0
    assert np.array_equal(out[~low], C0[~low])


def test_tn_kernel_twice_is_bit_identical(gpx):
    rng = np.random.default_rng(3)
    X = rng.standard_normal((1000, 192))
    a, b = np.zeros((192, 192)), np.zeros((192, 192))
    assert gpx.gpx_syrk_tn(_abi.dptr(a), 192, _abi.dptr(X), 1000, 0) == 0
    assert gpx.gpx_syrk_tn(_abi.dptr(b), 192, _abi.dptr(X), 1000, 0) == 0
    assert np.array_equal(a, b)


# ---- 2. end-to-end parity with the NumPy definition ------------------------------------------------------------------

def fit_case(case, chunk=None, seed=0):
    D = sparse_ref.case_data(case, seed)
    gp = SparseGP(case["kernel"], D["ls"], SF2, SN2, jitter=case["jitter"], chunk=case["chunk"] if chunk is None else chunk)
    gp.fit(D["X"], D["y"], inducing=D["Z"], noise_weights=D["w"])
    return gp, D


def parity_figures(case):
    """the figures of one case (also what profiles/sparse_parity.json records)"""
    gp, D = fit_case(case)
    with gp:
        mean, var = gp.predict(D["Xs"])
        elbo = gp.elbo()
        _, cov = gp.predict(D["Xs"], return_cov=True)
    ref = sparse_ref.SparseRef(case["kernel"], D["ls"], SF2, SN2, case["jitter"]).fit(D["X"], D["y"], D["Z"], D["w"])
    mr, vr = ref.predict(D["Xs"])
    _, cr = ref.predict_cov(D["Xs"])
    assert mean.shape == mr.shape and var.shape == vr.shape and elbo.shape == ref.elbo.shape
    return {"mean": rel_mean(mean, mr), "var": rel_var(var, vr), "elbo": rel_floor1(elbo, ref.elbo),
            "cov": float(np.max(np.abs(cov - cr)) / SF2)}


@pytest.mark.parametrize("case", sparse_ref.CASES, ids=[c["id"] for c in sparse_ref.CASES])
def test_parity_with_the_numpy_definition(case):
    fig = parity_figures(case)
    print(case["id"], {k: f"{v:.2e}" for k, v in fig.items()})
    assert fig["mean"] < BAR and fig["var"] < BAR and fig["elbo"] < BAR and fig["cov"] < BAR, fig
    assert max(fig["mean"], fig["var"], fig["elbo"]) < TIGHT_BAR, fig


def test_the_tight_bar_is_one_decade_above_the_measurement():
    rec = json.load(open(os.path.join(ROOT, "profiles", "sparse_parity.json")))
    assert {f["case"] for f in rec["fits"]} == {c["id"] for c in sparse_ref.CASES}
    largest = max(max(f["mean"], f["var"], f["elbo"]) for f in rec["fits"])
    assert largest == rec["largest"] and largest < TIGHT_BAR <= 10.0 * largest * (1.0 + 1e-12) and TIGHT_BAR <= BAR


def test_device_tensors_in_device_tensors_out():
    import torch
    case = sparse_ref.CASES[2]
    gp, D = fit_case(case)
    with gp:
        m0, v0 = gp.predict(D["Xs"])
        e0 = gp.elbo()
    dev = torch.device("cuda", 0)
    t = lambda a: torch.as_tensor(a, device=dev)  # noqa: E731
    with SparseGP(case["kernel"], D["ls"], SF2, SN2, jitter=case["jitter"], chunk=case["chunk"]) as gp:
        gp.fit(t(D["X"]), t(D["y"]), inducing=t(D["Z"]), noise_weights=t(D["w"]))
        m1, v1 = gp.predict(t(D["Xs"]))
        assert m1.is_cuda and v1.is_cuda and gp.inducing_.is_cuda
        assert np.array_equal(m1.cpu().numpy(), m0) and np.array_equal(v1.cpu().numpy(), v0) and np.array_equal(gp.elbo(), e0)


def test_inducing_as_a_count():
    X, y, Xs, _ = sparse_ref.problem(400, 1, 50, 1, 4, False)
    with SparseGP("matern52", 0.3, SF2, SN2) as gp:
        gp.fit(X, y, inducing=40)
        assert gp.inducing_.shape == (40, 1) and np.allclose(gp.inducing_[:, 0], np.linspace(X.min(), X.max(), 40))
        assert gp.jitter == 1e-8 * SF2
        mean, var = gp.predict(Xs, include_noise=True)
        ref = sparse_ref.SparseRef("matern52", 0.3, SF2, SN2, 1e-8 * SF2).fit(X, y, gp.inducing_)
        mr, vr = ref.predict(Xs)
        assert rel_mean(mean, mr) < BAR and rel_var(var, vr + SN2) < BAR
    X, y, Xs, _ = sparse_ref.problem(300, 3, 50, 1, 5, False)
    X[150:] = X[:150]                                        # 150 distinct rows
    with SparseGP("rbf", 0.6, SF2, SN2) as gp:
        a = gp.fit(X, y, inducing=60, random_state=3).inducing_.copy()
        b = gp.fit(X, y, inducing=60, random_state=3).inducing_
        assert a.shape == (60, 3) and np.array_equal(a, b) and len(np.unique(a, axis=0)) == 60
        assert all(any(np.array_equal(z, x) for x in X[:150]) for z in a)
        assert gp.fit(X, y, inducing=500).inducing_.shape == (150, 3)


# ---- 3. against the library's own dense GP ---------------------------------------------------------------------------

def dense_figures(kernel, X, y, Xs, Z, ls, w):
    with SparseGP(kernel, ls, SF2, SN2, jitter=0.0) as sp:
        sp.fit(X, y, inducing=Z, noise_weights=w)
        mean, var = sp.predict(Xs)
        elbo = float(sp.elbo().sum())
    with GP(kernel, ls, SF2, SN2, jitter=0.0, max_tries=1) as gp:
        md, vd = gp.fit(X, y, noise_weights=w).predict(Xs)
        lml = gp.log_marginal_likelihood(y)
    return {"mean": rel_mean(mean, md), "var": rel_var(var, vd), "elbo_vs_lml": abs(elbo - lml) / max(1.0, abs(lml))}


@pytest.mark.parametrize("kernel", ["matern32", "matern12"])
def test_inducing_points_at_the_data_give_the_dense_gp(kernel):
    X, y, Xs, w = sparse_ref.problem(300, 2, 64, 2, 5, True)
    fig = dense_figures(kernel, X, y, Xs, X, np.array([0.5, 0.8]), w)
    print(kernel, {k: f"{v:.2e}" for k, v in fig.items()})
    assert max(fig.values()) < FRESH_BAR, fig


@pytest.mark.parametrize("kernel", ["matern32", "matern12"])
def test_a_shared_time_grid_gives_the_dense_gp(kernel):
    X, y, grid = sparse_ref.path_grid_problem(40, 33, 3)
    Xs = np.linspace(-0.05, 1.05, 57).reshape(-1, 1)
    fig = dense_figures(kernel, X, y, Xs, grid, 0.3, None)
    print(kernel, {k: f"{v:.2e}" for k, v in fig.items()})
    assert max(fig.values()) < FRESH_BAR, fig


# ---- 4. determinism and state ----------------------------------------------------------------------------------------

def test_two_fits_and_predicts_around_a_covariance_are_bit_identical():
    case = sparse_ref.CASES[0]                               # three chunks
    gp, D = fit_case(case)
    with gp:
        m0, v0 = gp.predict(D["Xs"])
        e0 = gp.elbo()
        mc, cov = gp.predict(D["Xs"], return_cov=True)
        m1, v1 = gp.predict(D["Xs"])
        assert np.array_equal(m0, m1) and np.array_equal(v0, v1) and np.array_equal(mc, m0)
        assert np.array_equal(cov, cov.T)
        d = float(np.max(np.abs(np.diag(cov) - v0) / np.abs(v0)))
        print(f"diag(cov) against var: {d:.2e}")
        assert d < TIGHT_BAR
        gp.fit(D["X"], D["y"], inducing=D["Z"], noise_weights=D["w"])
        m2, v2 = gp.predict(D["Xs"])
        assert np.array_equal(m0, m2) and np.array_equal(v0, v2) and np.array_equal(e0, gp.elbo())
    gp2, _ = fit_case(case)
    with gp2:
        m3, v3 = gp2.predict(D["Xs"])
        assert np.array_equal(m0, m3) and np.array_equal(v0, v3) and np.array_equal(e0, gp2.elbo())


@pytest.mark.parametrize("case", [sparse_ref.CASES[0], sparse_ref.CASES[2]], ids=lambda c: c["id"])
def test_the_chunk_size_changes_rounding_only(case):
    a, D = fit_case(case, chunk=256)
    b, _ = fit_case(case, chunk=0)
    with a, b:
        assert a.chunk_ == 256 and b.chunk_ >= 1024
        (ma, va), (mb, vb) = a.predict(D["Xs"]), b.predict(D["Xs"])
        fig = {"mean": rel_mean(ma, mb), "var": rel_var(va, vb), "elbo": rel_floor1(a.elbo(), b.elbo())}
    print(case["id"], {k: f"{v:.2e}" for k, v in fig.items()})
    assert max(fig.values()) < TIGHT_BAR, fig


def _raw_sparse_fit(lib, h, X, y, Z, ls, jitter=1e-6):
    info = C.c_int64(-1)
    X, y, Z = (np.ascontiguousarray(a, dtype=np.float64) for a in (X, y, Z))
    ls = np.ascontiguousarray(np.atleast_1d(ls), dtype=np.float64)
    k = 1 if y.ndim == 1 else y.shape[1]
    rc = lib.gpx_sparse_fit(h, X.ctypes.data, y.ctypes.data, None, len(X), X.shape[1], k, Z.ctypes.data, len(Z), _abi.dptr(ls),
                            ls.size, SF2, SN2, jitter, 0, _abi.MEM_HOST, C.byref(info))
    return rc, info.value


def test_a_dense_fit_after_a_sparse_one_is_a_fresh_handle_and_the_two_families_refuse_each_other(gpx):
    X, y, Xs, _ = sparse_ref.problem(500, 2, 40, 1, 8, False)
    Z = X[:70]
    with GP("matern52", 0.5, SF2, SN2) as fresh:
        m0, v0 = fresh.fit(X, y).predict(Xs)
        ld0 = fresh.log_det_
        # a dense-fitted handle refuses the sparse calls and keeps its fit
        out = np.zeros(len(Xs))
        for rc in (gpx.gpx_sparse_predict(fresh._h, Xs.ctypes.data, len(Xs), out.ctypes.data, None, _abi.MEM_HOST),
                   gpx.gpx_sparse_predict_cov(fresh._h, Xs.ctypes.data, 4, None, out.ctypes.data, _abi.MEM_HOST),
                   gpx.gpx_sparse_elbo(fresh._h, _abi.dptr(out)), gpx.gpx_sparse_info(fresh._h, None, None, None, None)):
            assert rc == _abi.E_ARG and b"dense fit" in gpx.gpx_last_error(fresh._h)
        assert not out.any()
        m1, v1 = fresh.predict(Xs)
        assert np.array_equal(m0, m1) and np.array_equal(v0, v1)
    with GP("matern52", 0.5, SF2, SN2) as gp:
        rc, info = _raw_sparse_fit(gpx, gp._h, X, y, Z, 0.5)
        assert (rc, info) == (0, 0)
        ms = np.zeros(len(Xs))
        assert gpx.gpx_sparse_predict(gp._h, Xs.ctypes.data, len(Xs), ms.ctypes.data, None, _abi.MEM_HOST) == 0
        # a sparse-fitted handle refuses the dense calls, says where its fit is served, and keeps it
        out = np.zeros(len(Xs))
        ld = C.c_double(0.0)
        for rc in (gpx.gpx_predict(gp._h, Xs.ctypes.data, len(Xs), out.ctypes.data, None, _abi.MEM_HOST),
                   gpx.gpx_predict_cov(gp._h, Xs.ctypes.data, 4, None, out.ctypes.data, _abi.MEM_HOST),
                   gpx.gpx_logdet(gp._h, C.byref(ld)), gpx.gpx_get_alpha(gp._h, out.ctypes.data),
                   gpx.gpx_loo(gp._h, _abi.dptr(out), None, None, None), gpx.gpx_remove_rows(gp._h, 0, 1, C.byref(C.c_int64())),
                   gpx.gpx_lml_grad(gp._h, _abi.dptr(out), _abi.dptr(out))):
            assert rc == _abi.E_ARG and b"gpx_sparse_" in gpx.gpx_last_error(gp._h), gpx.gpx_last_error(gp._h)
        assert not out.any()
        ms2 = np.zeros(len(Xs))
        assert gpx.gpx_sparse_predict(gp._h, Xs.ctypes.data, len(Xs), ms2.ctypes.data, None, _abi.MEM_HOST) == 0
        assert np.array_equal(ms, ms2)
        # the dense fit that follows replaces it: the bits of the fresh handle
        m2, v2 = gp.fit(X, y).predict(Xs)
        assert np.array_equal(m0, m2) and np.array_equal(v0, v2) and gp.log_det_ == ld0
        assert gpx.gpx_sparse_elbo(gp._h, _abi.dptr(out)) == _abi.E_ARG


# ---- 5. failures and refusals ----------------------------------------------------------------------------------------

def test_identical_inducing_points_without_jitter_report_the_second_one(gpx):
    """(the first two points, variance 1: the second pivot is 1 - 1 * 1 = 0 exactly, whatever the rounding elsewhere)"""
    X, y, Xs, _ = sparse_ref.problem(200, 2, 10, 1, 2, False)
    Z = X[:20].copy()
    Z[1] = Z[0]
    with SparseGP("rbf", 0.5, 1.0, SN2, jitter=0.0) as gp:
        with pytest.raises(np.linalg.LinAlgError):
            gp.fit(X, y, inducing=Z)
        assert gp.info_ == 2
        with pytest.raises(RuntimeError):
            gp.predict(Xs)
        out = np.zeros(len(Xs))
        assert gpx.gpx_sparse_predict(gp._h, Xs.ctypes.data, len(Xs), out.ctypes.data, None, _abi.MEM_HOST) == _abi.E_ARG
        assert gp.fit(X, y, inducing=X[:20]).info_ == 0     # the handle is usable afterwards


def test_bad_weights_and_unsupported_handles_are_refused(gpx):
    X, y, Xs, w = sparse_ref.problem(200, 2, 10, 1, 2, True)
    with SparseGP("rbf", 0.5, SF2, SN2) as gp:
        gp.fit(X, y, inducing=X[:20], noise_weights=w)
        m0 = gp.predict(Xs, return_var=False)
        for bad in (0.0, -1.0, np.nan, np.inf):
            wb = w.copy()
            wb[77] = bad
            with pytest.raises(GpxError) as e:
                gp.fit(X, y, inducing=X[:20], noise_weights=wb)
            assert e.value.code == _abi.E_ARG
        with pytest.raises(ValueError):
            gp.fit(X, np.tile(y[:, None], (1, 9)), inducing=X[:20])
        assert np.array_equal(gp.fit(X, y, inducing=X[:20], noise_weights=w).predict(Xs, return_var=False), m0)
    for kw in ({"dtype": "float32"}, {"dtype": "mixed"}, {"devices": [0], "transport": "local"}):
        with GP("rbf", 0.5, SF2, SN2, **kw) as g:
            rc, _ = _raw_sparse_fit(gpx, g._h, X, y, X[:20], 0.5)
            assert rc == _abi.E_UNSUPPORTED, kw
            out = np.zeros(len(Xs))
            assert gpx.gpx_sparse_predict(g._h, Xs.ctypes.data, len(Xs), out.ctypes.data, None, _abi.MEM_HOST) == _abi.E_UNSUPPORTED
    assert m0.shape == (10,)


def test_nan_in_the_inducing_points_never_gives_a_fit(gpx):
    X, y, Xs, _ = sparse_ref.problem(200, 2, 10, 1, 2, False)
    Z = X[:20].copy()
    Z[7, 1] = np.nan
    with SparseGP("matern32", 0.5, SF2, SN2) as gp:
        with pytest.raises((np.linalg.LinAlgError, GpxError)):
            gp.fit(X, y, inducing=Z)
        out = np.zeros(len(Xs))
        assert gpx.gpx_sparse_predict(gp._h, Xs.ctypes.data, len(Xs), out.ctypes.data, None, _abi.MEM_HOST) == _abi.E_ARG
        assert not out.any()
