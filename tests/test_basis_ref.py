"""CPU: the fp64 reference of the GP with explicit basis functions (tests/basis_ref.py) checked against itself — the
identities the library's form rests on.  N = 300, d = 2, k = 2, 64 queries of which a quarter lie outside the data's box."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import basis_ref as br  # noqa: E402

KERNEL, LS, SF2, SN2 = "rbf", (0.3, 0.4), 1.5, 1e-2


@pytest.fixture(scope="module")
def data():
    return br.trend_problem(300, 2, 2, 64, seed=3)


@pytest.mark.parametrize("basis", br.BASES)
def test_the_residual_coefficients_are_orthogonal_to_the_basis(data, basis):
    X, Y, _ = data
    ref = br.BasisGP(KERNEL, LS, SF2, SN2, basis).fit(X, Y)
    got, scale = np.abs(ref.H.T @ ref.alpha).max(), np.abs(ref.H.T @ ref.KiY).max()
    print(f"{basis}: max|H^T alpha'| = {got:.3e}, max|H^T K^-1 y| = {scale:.3e}, cond(A) = {np.linalg.cond(ref.A):.3g}")
    assert got <= 1e-10 * scale


@pytest.mark.parametrize("basis", br.BASES)
def test_a_vague_prior_on_beta_absorbed_into_the_kernel_gives_the_same_posterior(data, basis):
    """b^2 = 1e7: the remaining gap is a property of the finite b^2 (O(1 / b^2) times the size of A^-1), not of the code"""
    X, Y, Xs = data
    mean, var = br.BasisGP(KERNEL, LS, SF2, SN2, basis).fit(X, Y).predict(Xs)
    m2, v2 = br.absorbed_predict(X, Y, Xs, KERNEL, LS, SF2, SN2, basis, 1e7)
    gm, gv = np.abs(mean - m2).max(), np.max(np.abs(var - v2) / var)
    print(f"{basis}: mean gap {gm:.3e} (absolute), variance gap {gv:.3e} (relative)")
    assert gm <= 1e-3 and gv <= 1e-3


@pytest.mark.parametrize("basis", br.BASES)
def test_the_fixed_beta_gradient_is_the_gradient_of_the_profile_likelihood(data, basis):
    X, Y, _ = data
    grad = br.BasisGP(KERNEL, LS, SF2, SN2, basis).fit(X, Y).lml_gradient()
    theta = np.log(np.array(LS + (SF2, SN2)))
    h = 1e-4
    for i in range(len(theta)):
        f = []
        for s in (+1.0, -1.0):
            t = theta.copy()
            t[i] += s * h
            e = np.exp(t)
            f.append(br.BasisGP(KERNEL, tuple(e[:2]), e[2], e[3], basis).fit(X, Y).lml())
        fd = (f[0] - f[1]) / (2 * h)
        assert abs(fd - grad[i]) <= 2e-5 * np.abs(grad).max(), (basis, i, fd, grad[i])


@pytest.mark.parametrize("basis", br.BASES)
def test_far_from_the_data_the_mean_is_the_trend(data, basis):
    X, Y, _ = data
    ref = br.BasisGP(KERNEL, LS, SF2, SN2, basis).fit(X, Y)
    far = np.array([[40.0, -35.0], [-50.0, 60.0]])       # the RBF covariance with the data underflows to 0
    mean, _ = ref.predict(far)
    want = br.basis_matrix(far, basis) @ ref.beta
    assert np.max(np.abs(mean - want)) <= 1e-9 * np.abs(want).max()


def test_score_and_forecast_of_the_reference_agree_with_each_other(data):
    """the forecast's logp is the score of the observed rows alone; a forecast with no noise on a repeated point returns it"""
    X, Y, Xs = data
    ref = br.BasisGP(KERNEL, LS, SF2, SN2, "linear").fit(X, Y)
    Xo, Xp = Xs[:40].copy(), Xs[40:60].copy()
    Yo = np.sin(Xo @ np.ones((2, 2)))
    fc = ref.forecast(Xo, Yo, Xp, 4, SN2)
    sc = ref.score(Xo, Yo, 10, SN2)
    assert np.max(np.abs(fc["logp"] - sc["logp"])) <= 1e-9 * np.abs(sc["logp"]).max()
    assert fc["mean"].shape == (4, 5, 2) and np.all(np.einsum("gii->gi", fc["cov"]) > 0)
