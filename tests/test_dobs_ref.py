"""CPU: the dense reference of the GP with derivative observations (tests/dobs_ref.py) against what it does not share code
with — differences of ``oracle.gp_oracle.kernel_matrix``, the oracle's posterior, and a GP conditioned on difference
quotients as linear observations — and the conditioning of every case the GPU tests compare against it."""
import os
import sys

import numpy as np
import pytest

from oracle.gp_oracle import OracleGP

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dobs_ref  # noqa: E402
from dobs_ref import DobsGP, mixed_gram  # noqa: E402
from score_ref import kernel_matrix  # noqa: E402  (the oracle's; Matern-3/2, which the oracle does not know, from matern_ref)

LS3 = np.array([0.3, 0.7, 1.1])
SF2 = 1.7


@pytest.mark.parametrize("kernel", dobs_ref.KERNELS)
def test_gram_elements_are_differences_of_the_kernel(kernel):
    """(a) every kind pair, d = 3, ARD: central (one derivative) and mixed second (two) differences of k at step 1e-4"""
    rng = np.random.default_rng(0)
    d, eps, n = 3, 1e-4, 60
    A, B = rng.normal(size=(n, d)), 0.5 * rng.normal(size=(n, d))

    def k(da, ja, db, jb):
        Aa, Bb = A.copy(), B.copy()
        if ja >= 0:
            Aa[:, ja] += da
        if jb >= 0:
            Bb[:, jb] += db
        return kernel_matrix(Aa, Bb, kernel, LS3, SF2)

    worst, largest = 0.0, 0.0
    for ja in range(-1, d):
        for jb in range(-1, d):
            if ja < 0 and jb < 0:
                fd = k(0, ja, 0, jb)
            elif jb < 0:
                fd = (k(eps, ja, 0, jb) - k(-eps, ja, 0, jb)) / (2 * eps)
            elif ja < 0:
                fd = (k(0, ja, eps, jb) - k(0, ja, -eps, jb)) / (2 * eps)
            else:
                fd = (k(eps, ja, eps, jb) - k(eps, ja, -eps, jb) - k(-eps, ja, eps, jb) + k(-eps, ja, -eps, jb)) / (4 * eps * eps)
            got = mixed_gram(A, np.full(n, ja), B, np.full(n, jb), kernel, LS3, SF2)
            worst, largest = max(worst, np.max(np.abs(got - fd))), max(largest, np.max(np.abs(got)))
    print(f"{kernel}: worst |element - difference| {worst:.2e}, largest entry {largest:.3g}")
    assert worst <= 1e-4 * largest


@pytest.mark.parametrize("kernel", dobs_ref.KERNELS)
def test_gram_is_symmetric_positive_definite_with_the_prior_on_its_diagonal(kernel):
    """(b) 40 rows of mixed kinds"""
    rng = np.random.default_rng(1)
    n, d = 40, 3
    X, kinds = rng.uniform(size=(n, d)), rng.integers(-1, d, size=n)
    G = mixed_gram(X, kinds, X, kinds, kernel, LS3, SF2)
    assert np.array_equal(G, G.T)
    assert np.linalg.eigvalsh(G).min() > 0
    want = np.where(kinds < 0, SF2, dobs_ref.GRAD_PRIOR[kernel] * SF2 / LS3[np.maximum(kinds, 0)] ** 2)
    assert np.allclose(np.diag(G), want, rtol=1e-14, atol=0)


@pytest.mark.parametrize("kernel", ("rbf", "matern52"))
def test_without_derivative_rows_it_is_the_oracle(kernel):
    """(c)"""
    rng = np.random.default_rng(2)
    X, Xs = rng.uniform(size=(150, 3)), rng.uniform(size=(40, 3))
    y = np.sin(X @ np.array([3.0, 2.0, 4.0])) + 0.1 * rng.standard_normal(150)
    ls = (0.3, 0.25, 0.4)
    want = OracleGP(kernel, ls, 1.5, 1e-2, jitter=1e-10).fit(X, y)
    mr, vr = want.predict(Xs)
    ref = DobsGP(kernel, ls, 1.5, 1e-2, 5e-2, jitter=1e-10).fit(X, np.full(150, -1), y)
    m, v = ref.predict(Xs)
    assert np.max(np.abs(ref.alpha_ - want.alpha_)) <= 1e-9 * np.max(np.abs(want.alpha_))
    assert abs(ref.logdet - want.log_det_) <= 1e-10 * abs(want.log_det_)
    assert abs(ref.lml() - want.log_marginal_likelihood()) <= 1e-10 * abs(ref.lml())
    assert np.max(np.abs(m - mr)) <= 1e-10 * np.max(np.abs(mr)) and np.max(np.abs(v - vr)) <= 1e-10 * 1.5


def _quotient_gp(c, h):
    """The posterior at c["Xs"] (mean, var, dmean along dim 0 by the same quotient) of a GP built ONLY from kernel_matrix:
    f at the value points and at x -+ h e_j of every derivative point, conditioned on A f with A the identity on the value
    rows and (f(x + h e_j) - f(x - h e_j)) / 2h on the derivative rows."""
    X, Xd, dims = c["X"], c["Xd"], c["dims"]
    N, Nd, d = len(X), len(Xd), X.shape[1]
    E = np.zeros((Nd, d))
    E[np.arange(Nd), dims] = h
    P = np.concatenate([X, Xd + E, Xd - E])
    A = np.zeros((N + Nd, len(P)))
    A[np.arange(N), np.arange(N)] = 1.0
    A[N + np.arange(Nd), N + np.arange(Nd)] = 0.5 / h
    A[N + np.arange(Nd), N + Nd + np.arange(Nd)] = -0.5 / h
    K = A @ kernel_matrix(P, P, c["kernel"], c["ls"], c["sf2"]) @ A.T
    K[np.diag_indices_from(K)] += np.concatenate([np.full(N, c["sn2"]), np.full(Nd, c["sn2_deriv"])]) + c["jitter"]
    Y = np.concatenate([np.reshape(c["y"], (N, -1)), np.reshape(c["yd"], (Nd, -1))])
    Ks = kernel_matrix(c["Xs"], P, c["kernel"], c["ls"], c["sf2"]) @ A.T
    sol = np.linalg.solve(K, np.concatenate([Y, Ks.T], axis=1))
    mean = Ks @ sol[:, :Y.shape[1]]
    var = c["sf2"] - np.einsum("mn,nm->m", Ks, sol[:, Y.shape[1]:])
    return mean, var


@pytest.mark.parametrize("kernel,d", [("rbf", 1), ("matern52", 3), ("matern32", 3)])
def test_posterior_is_that_of_difference_quotients_as_linear_observations(kernel, d):
    """(d) an independent derivation.  The quotient's truncation error is O(h^2 / l^2) for RBF and Matern-5/2 (k is four
    times differentiable at 0) and O(h / l) for Matern-3/2 (its k has an r^3 term: the quotient's prior variance is off by
    (2/3) sqrt3 2h / l); with l >= 0.25: 1.6e-5 at h = 1e-3 resp. 1.4e-2 at h = 1e-3, and halving h must shrink the error."""
    c, ref = dobs_ref.case(f"{kernel}_d{d}_last")
    mr, vr = ref.predict(c["Xs"])
    mr = np.reshape(mr, (len(c["Xs"]), -1))
    errs = []
    for h in (2e-3, 1e-3):
        m, v = _quotient_gp(c, h)
        errs.append(max(np.max(np.abs(m - mr)) / np.max(np.abs(mr)), np.max(np.abs(v - vr)) / c["sf2"]))
    print(f"{kernel} d={d}: quotient GP vs closed form, h = 2e-3: {errs[0]:.2e}, h = 1e-3: {errs[1]:.2e}")
    assert errs[1] <= (1.4e-2 if kernel == "matern32" else 1e-4)
    assert errs[1] <= 0.7 * errs[0]


@pytest.mark.parametrize("name", list(dobs_ref.CASES))
def test_gpu_cases_are_well_conditioned(name):
    """(e) cond(K) 2.2e-16 <= 1e-8 for every case of the table: the 1e-6 bounds of tests/test_dobs_gpu.py keep at least a
    100 x margin over what conditioning alone explains"""
    c, ref = dobs_ref.case(name)
    ev = np.linalg.eigvalsh(ref.K)
    print(f"{name}: N = {len(ref.K)}, cond(K) eps = {ev[-1] / ev[0] * 2.2e-16:.2e}")
    assert ev[0] > 0 and ev[-1] / ev[0] * 2.2e-16 <= 1e-8
