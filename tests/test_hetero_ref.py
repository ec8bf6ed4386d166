"""CPU: the reference of the per-observation-noise tests (tests/hetero_ref.py) is itself checked — against scikit-learn's
GaussianProcessRegressor(alpha=sn2 * w + jitter, optimizer=None) for the posterior and the log marginal likelihood, against
central differences of its own LML for the gradient (the noise entry 1/2 sn2 sum_i w_i (sum_c alpha_ic^2 - k (K^-1)_ii)
included) — and the standard inputs of the GPU tests are what those tests assume: well enough conditioned for their bars,
and with weights that change the answer by more than its own size."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hetero_ref as hr  # noqa: E402
from score_ref import score_ref  # noqa: E402

KERNELS = ("rbf", "matern52", "matern32", "matern12")
JITTER = 1e-10 * hr.SF2            # GP's default


def _sk_kernel(kernel, ls):
    from sklearn.gaussian_process.kernels import RBF, ConstantKernel, Matern
    ls = np.atleast_1d(ls) if np.ndim(ls) else ls
    base = RBF(ls) if kernel == "rbf" else Matern(ls, nu={"matern52": 2.5, "matern32": 1.5, "matern12": 0.5}[kernel])
    return ConstantKernel(hr.SF2) * base


@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("kernel", KERNELS)
def test_reference_agrees_with_scikit_learn(kernel, k):
    pytest.importorskip("sklearn")
    from sklearn.gaussian_process import GaussianProcessRegressor
    N, d, M = 300, 2, 200
    ls = hr.ard(d) if k == 3 else hr.LS
    X, y, Xs = hr.problem(N, d, M, k, seed=3)
    w = hr.weights(N, seed=4)
    ref = hr.HeteroGP(kernel, ls, hr.SF2, hr.SN2, JITTER).fit(X, y, w)
    sk = GaussianProcessRegressor(_sk_kernel(kernel, ls), alpha=hr.noise_diag(w, hr.SN2, JITTER), optimizer=None).fit(X, y)
    sm, ss = sk.predict(Xs, return_std=True)
    ss = ss if ss.ndim == 1 else ss[:, 0]            # one factor: the same for every target
    mean, var = ref.predict(Xs)
    fig = (np.max(np.abs(mean - sm)) / np.max(np.abs(sm)), np.max(np.abs(np.sqrt(var) - ss)) / np.max(ss),
           abs(ref.lml() - sk.log_marginal_likelihood()) / abs(sk.log_marginal_likelihood()))
    print(f"hetero_ref vs scikit-learn {kernel} k={k}: mean {fig[0]:.2e} std {fig[1]:.2e} lml {fig[2]:.2e}")
    assert max(fig) <= 1e-9


@pytest.mark.parametrize("kernel,N,d,k,is_ard", [
    ("rbf", 300, 2, 1, False), ("matern52", 300, 2, 3, True), ("matern32", 300, 2, 1, True), ("matern12", 300, 2, 3, False),
    ("rbf", 1153, 3, 3, True),
])
def test_reference_gradient_against_central_differences(kernel, N, d, k, is_ard):
    ls = np.atleast_1d(hr.ard(d) if is_ard else hr.LS).astype(np.float64)
    X, y, _ = hr.problem(N, d, 1, k, seed=N + d)
    w = hr.weights(N, seed=N)
    grad = hr.HeteroGP(kernel, ls, hr.SF2, hr.SN2, JITTER).fit(X, y, w).lml_gradient()
    v0 = np.log(np.concatenate([ls, [hr.SF2, hr.SN2]]))
    h = 1e-4                       # (1e-5 leaves the rounding of the LML, ~1e-13 |lml| / h, above 1e-6 of the small entries)
    fd = np.empty_like(v0)
    for i in range(len(v0)):
        f = []
        for sgn in (+1, -1):
            v = v0.copy()
            v[i] += sgn * h
            e = np.exp(v)
            f.append(hr.HeteroGP(kernel, e[:-2], e[-2], e[-1], JITTER).fit(X, y, w).lml())
        fd[i] = (f[0] - f[1]) / (2 * h)
    err = np.abs(fd - grad) / np.abs(grad)        # every log parameter on its own
    print(f"hetero_ref gradient vs central differences {kernel} N={N}: relative error per parameter "
          f"{' '.join(f'{e:.2e}' for e in err)}; noise entry {grad[-1]:.6g} vs {fd[-1]:.6g}")
    assert np.all(err <= 1e-6)


def test_ones_are_the_unweighted_reference():
    X, y, Xs = hr.problem(300, 2, 50, 2, seed=8)
    a = hr.HeteroGP("matern32", hr.LS, hr.SF2, hr.SN2, JITTER).fit(X, y, np.ones(300))
    b = hr.HeteroGP("matern32", hr.LS, hr.SF2, hr.SN2, JITTER).fit(X, y)
    assert np.array_equal(a.alpha, b.alpha) and a.lml() == b.lml()
    Xq, Yq = Xs[:48], np.sin(Xs[:48] @ np.ones((2, 2)))
    want = score_ref(X, y, Xq, Yq, 16, "matern32", hr.LS, hr.SF2, hr.SN2, hr.SN2, jitter=JITTER)
    got = a.score(Xq, Yq, 16, hr.SN2)
    for n in ("logp", "maha", "logdet"):
        assert np.max(np.abs(got[n] - want[n])) <= 1e-9 * np.max(np.abs(want[n])), n


def test_standard_inputs_are_well_conditioned_and_the_weights_matter():
    """what tests/test_hetero_gpu.py relies on: cond(K) <= 2.1e6 at N = 1153 for RBF (less for the Matern families), and
    weights that move alpha by more than its own size — a build that ignores them cannot pass a 1e-7 bar."""
    N, d = 1153, 3
    X, y, _ = hr.problem(N, d, 1, 1, seed=N)
    w = hr.weights(N, seed=N + 1)
    conds = {}
    for kernel in KERNELS:
        gp = hr.HeteroGP(kernel, hr.LS, hr.SF2, hr.SN2, JITTER)
        ev = np.linalg.eigvalsh(gp.gram(X, w))
        conds[kernel] = ev[-1] / ev[0]
    print("cond(K) at N = 1153:", {n: f"{v:.3g}" for n, v in conds.items()})
    assert conds["rbf"] <= 2.1e6 and all(conds[n] <= conds["rbf"] for n in KERNELS)
    a_w = hr.HeteroGP("rbf", hr.LS, hr.SF2, hr.SN2, JITTER).fit(X, y, w).alpha
    a_1 = hr.HeteroGP("rbf", hr.LS, hr.SF2, hr.SN2, JITTER).fit(X, y).alpha
    moved = np.max(np.abs(a_w - a_1)) / np.max(np.abs(a_1))
    print(f"weights move alpha by {moved:.3g} of its largest entry")
    assert moved > 1.0
