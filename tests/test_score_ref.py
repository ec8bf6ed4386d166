"""CPU: the NumPy reference of gpx_score_blocks (tests/score_ref.py) against scipy.stats.multivariate_normal on three small
problems, and the bound on the blocks' condition numbers that the GPU tests' tolerances are written in."""
import os
import sys

import numpy as np
import pytest
from scipy.stats import multivariate_normal

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from score_ref import kappa_bound, kernel_matrix, problem, score_ref  # noqa: E402

CASES = [
    # kernel, lengthscale, d, k, N, G, Lg, sf2, sn2, diag_add
    ("rbf", 1.0, 1, 1, 40, 3, 5, 1.5, 1e-2, 1e-2),
    ("matern52", (1.0, 1.5, 2.0), 3, 2, 60, 2, 17, 1.5, 1e-2, 1e-2),
    ("matern12", 0.8, 1, 2, 50, 4, 8, 0.7, 5e-2, 0.0),
]


@pytest.mark.parametrize("kernel,ls,d,k,N,G,Lg,sf2,sn2,diag_add", CASES)
def test_reference_is_the_multivariate_normal_density(kernel, ls, d, k, N, G, Lg, sf2, sn2, diag_add):
    X, Y, Xq, Yq = problem(N, d, k, G, Lg, seed=N + Lg)
    ref = score_ref(X, Y, Xq, Yq, Lg, kernel, ls, sf2, sn2, diag_add)
    # an independent route to the joint posterior: dense solves with K, no Cholesky
    K = kernel_matrix(X, X, kernel, ls, sf2) + sn2 * np.eye(N)
    Ks = kernel_matrix(Xq, X, kernel, ls, sf2)
    mean = Ks @ np.linalg.solve(K, Y)
    cov = kernel_matrix(Xq, Xq, kernel, ls, sf2) - Ks @ np.linalg.solve(K, Ks.T)
    assert np.allclose(ref["mean"], mean, rtol=0, atol=1e-9)
    for g in range(G):
        sl = slice(g * Lg, (g + 1) * Lg)
        S = 0.5 * (cov[sl, sl] + cov[sl, sl].T) + diag_add * np.eye(Lg)
        for c in range(k):
            want = multivariate_normal.logpdf(Yq[sl, c], mean=mean[sl, c], cov=S)
            assert abs(ref["logp"][g, c] - want) <= 1e-8 * ref["kappa"][g] * (Lg + ref["maha"][g, c])
        sign, logdet = np.linalg.slogdet(S)
        assert sign > 0 and abs(ref["logdet"][g] - logdet) <= 1e-8 * ref["kappa"][g] * Lg
        assert np.allclose(ref["logp"][g], -0.5 * ref["maha"][g] - 0.5 * ref["logdet"][g] - 0.5 * Lg * np.log(2 * np.pi),
                           rtol=0, atol=1e-12)


@pytest.mark.parametrize("kernel,ls,d,k,N,G,Lg,sf2,sn2,diag_add", CASES[:2])
def test_block_condition_numbers_respect_the_trace_bound(kernel, ls, d, k, N, G, Lg, sf2, sn2, diag_add):
    X, Y, Xq, Yq = problem(N, d, k, G, Lg, seed=N + Lg)
    ref = score_ref(X, Y, Xq, Yq, Lg, kernel, ls, sf2, sn2, diag_add)
    assert np.all(ref["kappa"] >= 1.0)
    assert np.all(ref["kappa"] <= kappa_bound(Lg, sf2, diag_add))


def test_the_bound_of_the_gpu_settings():
    # sf2 = 1.5, diag_add = sn2 = 1e-2, Lg <= 64: kappa_g <= 9601
    assert kappa_bound(64, 1.5, 1e-2) == pytest.approx(9601.0)
