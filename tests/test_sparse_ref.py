"""The NumPy definition of the inducing-point GP (tests/sparse_ref.py) against what must hold of it, on the CPU.

* Z = X with jitter 0 is the exact GP: the posterior and the LML of the suite's exact references (oracle/gp_oracle.py for
  the unweighted Matern-5/2 case, tests/hetero_ref.py — the same textbook algorithm with a noise weight per observation and
  the two further Matern families — for the weighted ones).  Measured: mean 1.7e-14, variance 1.2e-12 relative,
  ELBO - LML 6.1e-12; the bar is 1e-9, the project's bar for one quantity by two routes.
* ELBO <= LML on every parity case of the GPU test.
* Q_ff = K_ff when Z covers the distinct inputs: 40 paths on a shared 33-step grid with Z = the grid.
* Permuting the observations changes nothing beyond 1e-8 (measured: 8.4e-10 relative variance).
* The order the model is defined in matters: contracting before whitening loses the result."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sparse_ref  # noqa: E402
from hetero_ref import HeteroGP  # noqa: E402
from oracle.gp_oracle import OracleGP  # noqa: E402

SF2, SN2 = sparse_ref.SF2, sparse_ref.SN2
BAR = 1e-9


def rel_mean(a, b):
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-6)))


def rel_var(a, b):
    return float(np.max(np.abs(a - b) / np.abs(b)))


def rel_floor1(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b)) / np.maximum(np.abs(b), 1.0)))


@pytest.mark.parametrize("kernel", ["matern52", "matern32", "matern12"])
def test_inducing_points_at_the_data_give_the_exact_weighted_posterior_and_lml(kernel):
    X, y, Xs, w = sparse_ref.problem(300, 2, 64, 2, 5, True)
    ls = np.array([0.5, 0.8])
    sp = sparse_ref.SparseRef(kernel, ls, SF2, SN2, 0.0).fit(X, y, X, w)
    mean, var = sp.predict(Xs)
    ex = HeteroGP(kernel, ls, SF2, SN2, 0.0).fit(X, y, w)
    me, ve = ex.predict(Xs)
    print(f"{kernel}: mean {rel_mean(mean, me):.2e} var {rel_var(var, ve):.2e} elbo-lml {sp.elbo.sum() - ex.lml():.2e}")
    assert rel_mean(mean, me) <= BAR and rel_var(var, ve) <= BAR
    assert abs(sp.elbo.sum() - ex.lml()) <= BAR * max(1.0, abs(ex.lml()))
    _, cov = sp.predict_cov(Xs)
    assert rel_var(np.diag(cov), ve) <= BAR and np.max(np.abs(cov - cov.T)) <= 1e-12 * SF2


def test_inducing_points_at_the_data_give_the_oracle_posterior_and_lml():
    X, y, Xs, _ = sparse_ref.problem(300, 2, 64, 1, 6, False)
    sp = sparse_ref.SparseRef("matern52", 0.6, SF2, SN2, 0.0).fit(X, y, X)
    ref = OracleGP("matern52", 0.6, SF2, SN2, jitter=0.0).fit(X, y)
    me, ve = ref.predict(Xs)
    mean, var = sp.predict(Xs)
    assert rel_mean(mean, me) <= BAR and rel_var(var, ve) <= BAR
    assert abs(sp.elbo.sum() - ref.log_marginal_likelihood()) <= BAR * max(1.0, abs(ref.log_marginal_likelihood()))


@pytest.mark.parametrize("case", sparse_ref.CASES, ids=[c["id"] for c in sparse_ref.CASES])
def test_the_bound_is_below_the_exact_lml(case):
    D = sparse_ref.case_data(case)
    sp = sparse_ref.SparseRef(case["kernel"], D["ls"], SF2, SN2, case["jitter"]).fit(D["X"], D["y"], D["Z"], D["w"])
    _, _, lml = sparse_ref.exact_gp(D["X"], D["y"], D["Xs"], case["kernel"], D["ls"], SF2, SN2, D["w"])
    # (the rounding of either side is orders below 1e-9 |LML|: see the identities above)
    assert np.all(np.isfinite(sp.elbo)) and sp.elbo.sum() <= lml + BAR * max(1.0, abs(lml))


@pytest.mark.parametrize("kernel", ["matern52", "matern32", "matern12"])
def test_a_shared_time_grid_with_the_grid_as_inducing_points_is_exact(kernel):
    X, y, grid = sparse_ref.path_grid_problem(40, 33, 3)
    Xs = np.linspace(-0.05, 1.05, 57).reshape(-1, 1)
    sp = sparse_ref.SparseRef(kernel, 0.3, SF2, SN2, 0.0).fit(X, y, grid)
    mean, var = sp.predict(Xs)
    me, ve, lml = sparse_ref.exact_gp(X, y, Xs, kernel, 0.3, SF2, SN2)
    print(f"{kernel}: mean {rel_mean(mean, me):.2e} var {rel_var(var, ve):.2e} elbo-lml {sp.elbo.sum() - lml:.2e}")
    assert rel_mean(mean, me) <= BAR and rel_var(var, ve) <= BAR and abs(sp.elbo.sum() - lml) <= BAR * max(1.0, abs(lml))
    moved = sparse_ref.SparseRef(kernel, 0.3, SF2, SN2, 1e-6).fit(X, y, grid).predict(Xs)[1]
    assert rel_var(moved, ve) > 1e-6   # jitter on Kuu is a change of MODEL: 1e-6 is visible far above rounding


@pytest.mark.parametrize("kernel,N,m,jitter", [("rbf", 2100, 257, 1e-8), ("matern52", 4000, 130, 1e-6)])
def test_permuting_the_observations_and_reversing_the_inducing_points_changes_nothing(kernel, N, m, jitter):
    X, y, Xs, w = sparse_ref.problem(N, 1, 64, 2, 9, True)
    Z = np.linspace(0.0, 1.0, m).reshape(m, 1)
    a = sparse_ref.SparseRef(kernel, 0.3, SF2, SN2, jitter).fit(X, y, Z, w)
    p = np.random.default_rng(1).permutation(N)
    b = sparse_ref.SparseRef(kernel, 0.3, SF2, SN2, jitter).fit(X[p], y[p], Z[::-1], w[p])
    (ma, va), (mb, vb) = a.predict(Xs), b.predict(Xs)
    print(f"{kernel}: mean {rel_mean(mb, ma):.2e} var {rel_var(vb, va):.2e} elbo {rel_floor1(b.elbo, a.elbo):.2e}")
    assert rel_mean(mb, ma) <= 1e-8 and rel_var(vb, va) <= 1e-8 and rel_floor1(b.elbo, a.elbo) <= 1e-8


def test_contracting_before_whitening_loses_the_result():
    """RBF, d = 1, N = 2100, m = 257, jitter 1e-8 (measured: the cheap order's bound differs by 0.67 and its variance by
    2.3e-7 relative, the whitened order agrees with itself to 1.5e-10 / 4.2e-11)."""
    X, y, Xs, w = sparse_ref.problem(2100, 1, 64, 1, 9, False)
    Z = np.linspace(0.0, 1.0, 257).reshape(-1, 1)
    good = sparse_ref.SparseRef("rbf", 0.3, SF2, SN2, 1e-8).fit(X, y, Z)
    p = np.random.default_rng(2).permutation(2100)
    again = sparse_ref.SparseRef("rbf", 0.3, SF2, SN2, 1e-8).fit(X[p], y[p], Z[::-1])
    own = abs(again.elbo[0] - good.elbo[0])
    try:
        cheap = sparse_ref.CheapOrder("rbf", 0.3, SF2, SN2, 1e-8).fit(X, y, Z)
    except np.linalg.LinAlgError:
        return  # (lost altogether)
    lost = abs(cheap.elbo[0] - good.elbo[0])
    print(f"whitened order vs itself {own:.2e}, cheap order vs whitened {lost:.2e}")
    assert own <= 1e-8 * abs(good.elbo[0]) and lost >= 1e3 * max(own, 1e-12)
