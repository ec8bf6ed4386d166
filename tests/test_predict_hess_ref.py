"""CPU: the reference of the posterior second derivatives (tests/hess_ref.py) held against central finite differences of
the references one derivative order below it."""
import os
import sys

import numpy as np
import pytest

from oracle.gp_oracle import synthetic_problem

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from deriv_ref import grad_ref, kernel_grad, lengthscales  # noqa: E402
from hess_ref import expand, hess_ref, kernel_hess, kernel_third, pairs, prior_hess_var  # noqa: E402

KERNELS = ("rbf", "matern52")
SHAPES = [(1, 0.3), (2, (0.3, 0.5)), (3, (0.2, 0.5, 0.35))]


def points(d, seed=0):
    rng = np.random.default_rng(seed + d)
    return rng.uniform(0, 1, (17, d)), rng.uniform(0, 1, (23, d))


def shifted(P, c, h):
    Q = P.copy()
    Q[:, c] += h
    return Q


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("d,ls", SHAPES)
def test_kernel_hess_is_the_derivative_of_kernel_grad(kernel, d, ls):
    A, B = points(d)
    l = lengthscales(ls, d)
    H = expand(np.moveaxis(kernel_hess(A, B, kernel, ls, 1.7), 0, 1), d)            # (na, d, d, nb)
    for j in range(d):
        h = 1e-5 * l[j]
        fd = (kernel_grad(shifted(A, j, h), B, kernel, ls, 1.7) - kernel_grad(shifted(A, j, -h), B, kernel, ls, 1.7)) / (2 * h)
        for i in range(d):
            err = np.max(np.abs(fd[i] - H[:, i, j, :])) / np.max(np.abs(H[:, i, j, :]))
            print(f"{kernel} d={d} H[{i}][{j}]: finite-difference err {err:.2e}")
            assert err <= 1e-4


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("d,ls", SHAPES)
def test_kernel_third_is_the_derivative_of_kernel_hess(kernel, d, ls):
    A, B = points(d, seed=5)
    l = lengthscales(ls, d)
    for c in range(d):
        h = 1e-5 * l[c]
        fd = (kernel_hess(A, shifted(B, c, h), kernel, ls, 1.7) - kernel_hess(A, shifted(B, c, -h), kernel, ls, 1.7)) / (2 * h)
        T = kernel_third(A, B, np.full(len(B), c), kernel, ls, 1.7)
        err = np.max(np.abs(fd - T)) / np.max(np.abs(T))
        print(f"{kernel} d={d} by x_{c}: finite-difference err {err:.2e}")
        assert err <= 1e-4


def prior_by_differences(kernel, ls, sf2, d, step):
    """Var[d_i d_j f] = d^2 / d b_i d b_j of H_ij(a, b) at b = a, by central differences of ``kernel_hess`` with steps
    ``step * l``"""
    l = lengthscales(ls, d)
    a = np.full((1, d), 0.4)
    out = []
    for b, (i, j) in enumerate(zip(*pairs(d))):
        def H(si, sj):
            return kernel_hess(a, shifted(shifted(a, i, si * step * l[i]), j, sj * step * l[j]), kernel, ls, sf2)[b, 0, 0]
        if i == j:   # both shifts along one axis: the second difference with the step 2 step l
            out.append((H(1, 1) - 2.0 * H(0, 0) + H(-1, -1)) / (2 * step * l[i]) ** 2)
        else:
            out.append((H(1, 1) - H(1, -1) - H(-1, 1) + H(-1, -1)) / (4 * step * l[i] * step * l[j]))
    return np.array(out)


@pytest.mark.parametrize("d,ls", SHAPES)
def test_rbf_prior_against_differences(d, ls):
    prior = prior_hess_var("rbf", ls, 1.3, d)
    fd = prior_by_differences("rbf", ls, 1.3, d, 5e-3)
    err = np.max(np.abs(fd - prior) / prior)
    print(f"rbf d={d}: prior {prior}, by differences {fd}, rel err {err:.2e}")
    assert err <= 1e-3


def test_matern52_prior_is_the_closed_form():
    """h(0) = 25 sf2 / 3 and three of it on the diagonal: 25 sf2 / l^4.  The fourth derivative of the Matern-5/2 kernel has a
    kink at r = 0 (H l^2 = -5/3 + 12.5 u^2 - (100 sqrt5 / 9) |u|^3 + ...), so a second difference with the step delta l is
    low by 2 (100 sqrt5 / 9) delta / 25 = 1.99 delta: 2 % at the step 0.01 l used here, inside the 5 % asked."""
    sf2, l = 1.3, 0.3
    prior = prior_hess_var("matern52", l, sf2, 1)
    assert prior.shape == (1,) and abs(prior[0] - 25.0 * sf2 / l ** 4) <= 1e-12 * prior[0]
    fd = prior_by_differences("matern52", l, sf2, 1, 5e-3)
    err = abs(fd[0] - prior[0]) / prior[0]
    print(f"matern52: prior {prior[0]:.6g}, by differences {fd[0]:.6g}, rel err {err:.2e}")
    assert err <= 0.05
    off = prior_hess_var("matern52", (0.3, 0.5), sf2, 2)
    assert np.allclose(off, [25 * sf2 / 0.3 ** 4, (25.0 / 3.0) * sf2 / (0.3 * 0.5) ** 2, 25 * sf2 / 0.5 ** 4], rtol=1e-14)


def test_posterior_reference_against_differences_of_the_gradient_reference():
    X, y, Xs = synthetic_problem(200, 2, 30, seed=2)
    y2 = np.stack([y, np.cos(2.0 * X.sum(axis=1))], axis=1)
    ls, sf2, sn2, jit = (0.3, 0.4), 1.5, 1e-2, 1.5e-10
    hm, hv = hess_ref(X, y2, Xs, "rbf", ls, sf2, sn2, jit)
    assert hm.shape == (30, 3, 2) and hv.shape == (30, 3)
    prior = prior_hess_var("rbf", ls, sf2, 2)
    assert np.all(hv <= prior[None, :] * (1 + 1e-12)) and np.all(hv > -1e-9 * prior[None, :])
    Hf = expand(hm, 2)                                                              # (M, d, d, k)
    l = lengthscales(ls, 2)
    for j in range(2):
        h = 1e-5 * l[j]
        fd = (grad_ref(X, y2, shifted(Xs, j, h), "rbf", ls, sf2, sn2, jit)[0] -
              grad_ref(X, y2, shifted(Xs, j, -h), "rbf", ls, sf2, sn2, jit)[0]) / (2 * h)    # (M, d, k): d dmean_i / d x_j
        err = np.max(np.abs(fd - Hf[:, :, j, :])) / np.max(np.abs(Hf[:, :, j, :]))
        print(f"posterior, by x_{j}: finite-difference err {err:.2e}")
        assert err <= 1e-4


class _StubGP:
    """stands in for a fitted GP on the host: fixed normalised gradients and second derivatives of a one-input model"""

    def __init__(self, dm, hm):
        self.dm, self.hm = dm, hm

    def predict_gradient(self, qn, return_var=True, **kw):
        return (self.dm, np.ones(self.dm.shape[:2])) if return_var else self.dm

    def predict_hessian(self, qn, return_var=True, **kw):
        return (self.hm, np.ones(self.hm.shape[:2])) if return_var else self.hm


def test_path_model_units_and_curvature_on_the_host():
    from gaussianprocesspathmodelling_amd import paths as gpaths
    # a circle of radius 2 run counter-clockwise, one run clockwise, a point at rest: (x', y'), (x'', y'') in raw units
    v = np.array([[0.0, 2.0], [0.0, -2.0], [0.0, 0.0]])
    a = np.array([[-2.0, 0.0], [-2.0, 0.0], [1.0, 1.0]])
    span, sd = np.array([4.0]), np.array([3.0, 5.0])
    gp = _StubGP((v * span[0] / sd)[:, None, :], (a * span[0] ** 2 / sd)[:, None, :])
    m = gpaths.PathModel(gp, ["p"], np.array([10.0]), span, np.zeros(2), sd, ("t",), ("x", "y"))
    q = np.array([10.0, 11.0, 12.0])
    acc, av = m.acceleration(q)
    assert np.allclose(acc, a, rtol=1e-15) and np.allclose(av, np.broadcast_to((sd / span[0] ** 2) ** 2, (3, 2)), rtol=1e-15)
    hm, hv = m.predict_hessian(q)
    assert hm.shape == hv.shape == (3, 1, 2) and np.array_equal(hm[:, 0, :], acc)
    kappa = m.curvature(q)
    assert np.allclose(kappa[:2], [0.5, -0.5], rtol=1e-14) and np.isnan(kappa[2])
    with pytest.raises(ValueError, match="'t'"):
        gpaths.PathModel(gp, ["p"], np.zeros(1), span, np.zeros(2), sd, ("x",), ("x", "y")).acceleration(q)
    with pytest.raises(ValueError, match="two targets"):
        gpaths.PathModel(gp, ["p"], np.zeros(1), span, np.zeros(1), sd[:1], ("t",), ("x",)).curvature(q)
