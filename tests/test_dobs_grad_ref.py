"""CPU: the reference of the LML gradient with derivative observations (tests/dobs_grad_ref.py) against what it does not
share code with — central differences of ``dobs_ref.mixed_gram`` for d K / d log l and of ``DobsGP.lml()`` for the
gradient — the agreement of its two analytic forms, and the conditioning of every case the GPU tests compare against it.

Bounds.  Central differences at step h carry h^2 f''' / 6 of truncation and eps |f| / h of rounding.  For the Gram entries
(h = 1e-5: 2e-11 f''' + 1e-11 |f|; the third log-lengthscale derivative of a derivative block is some hundred times its
first) 1e-7 of the largest entry.  For the LML (h = 1e-4, the step of tests/test_hetero_ref.py; the LML itself is rounded
at ~1e-13 |lml|, i.e. 1e-9 |lml| in the quotient, against gradients of 1e-3 .. 1 |lml|) 1e-5 of the largest entry, and
every figure is printed."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dobs_ref  # noqa: E402
import dobs_grad_ref as gr  # noqa: E402
from dobs_ref import DobsGP, mixed_gram  # noqa: E402

COND_MAX = 1e7   # the conditioning the GPU tolerances (1e-9 / 1e-8) assume: eps cond(K) = 1e-9
FD_CASES = ["rbf_d1_last", "matern52_d3_mixed", "matern32_d5_last", "matern32_d1_mixed", "rbf_d3_last", "matern52_d5_mixed",
            "waypoints", "weighted"]


@pytest.mark.parametrize("kernel", dobs_ref.KERNELS)
@pytest.mark.parametrize("d", [1, 3, 5])
def test_dl_table_against_central_differences_of_the_gram(kernel, d):
    """every kind pair among 70 x 50 rows of mixed kinds, coincident points of different kinds included"""
    A, ka, B, kb = gr.dl_problem(d)
    (na, nb), h = (len(A), len(B)), 1e-5
    ls = np.asarray(dobs_ref.LS[d], dtype=np.float64)
    got = gr.mixed_gram_dl(A, ka, B, kb, kernel, dobs_ref.LS[d], dobs_ref.SF2)
    assert got.shape == (ls.size if ls.ndim else 1, na, nb)
    l0 = np.atleast_1d(ls)
    worst = 0.0
    for c in range(l0.size):
        f = []
        for sgn in (+1, -1):
            l = l0.copy()
            l[c] *= np.exp(sgn * h)
            f.append(mixed_gram(A, ka, B, kb, kernel, l if ls.ndim else float(l[0]), dobs_ref.SF2))
        fd = (f[0] - f[1]) / (2 * h)
        worst = max(worst, float(np.max(np.abs(got[c] - fd)) / np.max(np.abs(got[c]))))
    print(f"{kernel} d={d}: worst |d gram / d log l - difference| / largest entry {worst:.2e}")
    assert worst <= 1e-7


def test_swapping_the_sides_transposes_the_derivative():
    rng = np.random.default_rng(3)
    A, B = rng.uniform(size=(30, 3)), rng.uniform(size=(20, 3))
    ka, kb = rng.integers(-1, 3, 30), rng.integers(-1, 3, 20)
    for kernel in dobs_ref.KERNELS:
        G = gr.mixed_gram_dl(A, ka, B, kb, kernel, dobs_ref.LS[3], 1.3)
        H = gr.mixed_gram_dl(B, kb, A, ka, kernel, dobs_ref.LS[3], 1.3)
        assert np.allclose(G, H.transpose(0, 2, 1), rtol=1e-13, atol=0)


def _theta(c):
    return np.log(np.concatenate([np.atleast_1d(np.asarray(c["ls"], dtype=np.float64)), [c["sf2"], c["sn2"]],
                                  [c["sn2_deriv"]] if c["sn2_deriv"] > 0 else []]))


def _lml_at(c, v, n_ls):
    e = np.exp(v)
    ls = e[:n_ls] if n_ls > 1 else float(e[0])
    sd = e[n_ls + 2] if c["sn2_deriv"] > 0 else 0.0
    return DobsGP(c["kernel"], ls, e[n_ls], e[n_ls + 1], sd, c["jitter"]).fit(c["Xall"], c["kinds"], c["yall"], c["w"]).lml()


@pytest.mark.parametrize("name", FD_CASES)
def test_gradient_against_central_differences_of_the_lml(name):
    c, ref, lml, grad = gr.case(name)
    n_ls = np.atleast_1d(np.asarray(c["ls"])).size
    assert grad.shape == (n_ls + 3,)
    v0, h = _theta(c), 1e-4
    fd = np.zeros(n_ls + 3)
    for i in range(len(v0)):
        f = []
        for sgn in (+1, -1):
            v = v0.copy()
            v[i] += sgn * h
            f.append(_lml_at(c, v, n_ls))
        fd[i] = (f[0] - f[1]) / (2 * h)
    err = float(np.max(np.abs(fd - grad)) / np.max(np.abs(grad)))
    print(f"{name}: lml {lml:.6f} gradient {np.array2string(grad, precision=5)} |gradient - difference| / largest {err:.2e}")
    assert err <= 1e-5
    if c["sn2_deriv"] == 0.0:
        assert grad[-1] == 0.0


@pytest.mark.parametrize("name", list(gr.GPU_CASES))
def test_two_analytic_forms_agree_and_the_case_is_well_conditioned(name):
    c, ref, lml, grad = gr.case(name)
    other = gr.lml_grad_inverse(ref, c["w"])
    err = float(np.max(np.abs(other - grad)) / np.max(np.abs(grad)))
    ev = np.linalg.eigvalsh(ref.K)
    cond = float(ev[-1] / ev[0])
    print(f"{name}: N {len(c['kinds'])} cond(K) {cond:.3g} inverse against solves {err:.2e}")
    assert err <= 1e-10
    assert cond <= COND_MAX
    assert np.isfinite(lml) and np.all(np.isfinite(grad))
