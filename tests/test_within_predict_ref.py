"""CPU: the reference of predicting an observed path itself (tests/within_predict_ref.py) against the references the project
already trusts — identities that pin what "query point x* with path id p*" means, without a GPU.

Problem: ``within_ref.problem(seed=0)``: 12 paths x 33 points, Matern-3/2, sf2 = 1.5, sg2 = 0.4, l = 0.25, l_path = 0.1,
noise = 1e-2; 13 query times."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import within_predict_ref as wpr  # noqa: E402
import within_ref as wr  # noqa: E402

HYP = dict(kernel="matern32", ls=0.25, sf2=1.5, ls_path=0.1, sg2=0.4, sn2=1e-2)
TQ = np.linspace(0.03, 0.97, 13).reshape(-1, 1)


def _fit(p, ids=None, rows=slice(None), kernel=None):
    ids = p["ids"] if ids is None else ids
    return wr.fit_ref(p["X"][rows], ids[rows], p["Y"][rows], kernel or HYP["kernel"], HYP["ls"], HYP["sf2"], HYP["sn2"],
                      HYP["ls_path"], HYP["sg2"])


def test_ids_minus_one_ask_for_the_cluster_mean():
    p = wr.problem(seed=0)
    fit = _fit(p)
    mean, cov = wpr.predict_path(fit, TQ, np.full(13, -1))
    mf, cf, _ = wr.predict_f(fit, TQ)
    assert np.array_equal(mean, mf) and np.array_equal(cov, cf)
    m1, c1 = wpr.predict_path(fit, TQ, -1)                      # an int is every point's id
    assert np.array_equal(m1, mf) and np.array_equal(c1, cf)


def test_a_fresh_id_is_a_path_nobody_has_seen():
    p = wr.problem(seed=0)
    fit = _fit(p)
    mean, cov = wpr.predict_path(fit, TQ, 99)
    mb, Sb = wr.block_cov(fit, TQ)
    e = max(float(np.max(np.abs(mean - mb))), float(np.max(np.abs(cov - Sb))))
    print(f"fresh id vs block_cov: {e:.2e}")
    assert e <= 1e-14 * (HYP["sf2"] + HYP["sg2"])               # (the two sum the same two matrices in another order)


def test_leaving_a_path_out_and_bringing_it_back():
    """Identity (c): fit without path 3's rows, condition a NEW path on exactly those rows (``forecast_schur``, their noise
    as diag_add) — the result is the full fit queried as path 3.  Two dense fp64 routes that share only the covariance
    function; bound 1e-10 kappa (mean: times max(1, max |yo - mean_o|); cov: times sf2 + sg2), the form of
    tests/test_within_ref.py's, kappa = cond(S_oo + diag_add I).  Measured: mean 2e-13, cov 4e-15, kappa 317."""
    p = wr.problem(seed=0)
    mine = p["ids"] == 3
    full = _fit(p)
    rest = _fit(p, rows=~mine)
    a = wr.forecast_schur(rest, p["X"][mine], p["Y"][mine], TQ, 1, HYP["sn2"])
    mean, cov = wpr.predict_path(full, TQ, 3)
    em, ec = float(np.max(np.abs(a["mean"] - mean))), float(np.max(np.abs(a["cov"][0] - cov)))
    kappa, resid = float(a["kappa"][0]), float(a["resid"][0])
    print(f"leave out / bring back: mean {em:.2e} cov {ec:.2e} kappa {kappa:.4g} resid {resid:.3g}")
    assert em <= 1e-10 * kappa * max(1.0, resid) and ec <= 1e-10 * kappa * (HYP["sf2"] + HYP["sg2"])
    # ... and the question is worth asking: path 3 is not the cluster mean, and it is known better than f near its points
    mf, cf, _ = wr.predict_f(full, TQ)
    vf, vp = np.diag(cf), np.diag(cov)
    print(f"var f {vf.min():.3g} .. {vf.max():.3g}, var path 3 {vp.min():.3g} .. {vp.max():.3g}, "
          f"mean moves up to {np.max(np.abs(mean - mf)):.3g}")
    assert np.max(np.abs(mean - mf)) > 0.5 and vp.min() < 0.5 * vf.min()


@pytest.mark.parametrize("kernel", ["rbf", "matern52"])
def test_gradient_against_central_differences(kernel):
    """Step and bound of tests/test_predict_grad_gpu.py: h = 1e-3 l, 1e-5 of the largest entry."""
    p = wr.problem(seed=0, kernel=kernel)
    fit = _fit(p, kernel=kernel)
    gq = np.array([3, -1, 3, 0, 99, 11, -1, 3, 5, 5, 0, 99, 3])
    dm, _ = wpr.predict_path_grad(fit, TQ, gq)
    h = 1e-3 * HYP["ls"]
    fd = (wpr.predict_path(fit, TQ + h, gq)[0] - wpr.predict_path(fit, TQ - h, gq)[0]) / (2 * h)
    e = float(np.max(np.abs(fd - dm[:, 0, :]))) / float(np.max(np.abs(dm)))
    print(f"{kernel}: gradient vs central differences {e:.2e} (of max)")
    assert e <= 1e-5


def test_gradient_against_central_differences_matern32():
    """Matern-3/2: k'' jumps at r = 0 (k = sf2 (1 + s) e^-s: k' = -3 sf2 r e^-s / l, whose slope changes sign through 0), so
    where a query time lies within h of a training time of its own path or of any path the central difference straddles the
    kink and errs by O(h k''') no longer but by O(|k''| h) per such training point.  The bound is therefore written from the
    reference itself: the difference between the central differences at h and at h / 2 — what the finite difference's own
    step dependence is at these points — plus the 1e-5 of the smooth families."""
    p = wr.problem(seed=0)
    fit = _fit(p)
    gq = np.array([3, -1, 3, 0, 99, 11, -1, 3, 5, 5, 0, 99, 3])
    dm, _ = wpr.predict_path_grad(fit, TQ, gq)
    h = 1e-3 * HYP["ls"]
    fd = lambda s: (wpr.predict_path(fit, TQ + s, gq)[0] - wpr.predict_path(fit, TQ - s, gq)[0]) / (2 * s)  # noqa: E731
    f1, f2 = fd(h), fd(h / 2)
    scale = float(np.max(np.abs(dm)))
    step = float(np.max(np.abs(f1 - f2))) / scale
    e = float(np.max(np.abs(f2 - dm[:, 0, :]))) / scale
    print(f"matern32: gradient vs central differences (h / 2) {e:.2e}, step dependence {step:.2e} (of max)")
    assert e <= 1e-5 + 2.0 * step


def test_gradient_variance_against_differences_of_the_covariance():
    """dvar = Var[d value / d x]: the second mixed difference of the reference's own joint covariance (the form of
    tests/test_predict_grad_gpu.py: h = 3e-3 l, 1e-4 of the prior), rbf."""
    p = wr.problem(seed=0, kernel="rbf")
    fit = _fit(p, kernel="rbf")
    gq = np.array([3, -1, 3, 0, 99, 11, -1, 3, 5, 5, 0, 99, 3])
    _, dv = wpr.predict_path_grad(fit, TQ, gq)
    h = 3e-3 * HYP["ls"]
    _, cov = wpr.predict_path(fit, np.concatenate([TQ + h, TQ - h]), np.concatenate([gq, gq]))
    M = len(TQ)
    fdv = (np.diag(cov)[:M] + np.diag(cov)[M:] - 2 * np.diag(cov[:M, M:])) / (4 * h * h)
    prior = wpr.grad_priors(fit, gq, 1)
    e = float(np.max(np.abs(fdv - dv[:, 0]) / prior[:, 0]))
    print(f"rbf: dvar vs differences of the covariance {e:.2e} (of the prior)")
    assert e <= 1e-4 and np.all(dv > 0) and np.all(dv <= prior)


def test_a_mixed_id_covariance_is_symmetric_positive_definite():
    p = wr.problem(seed=0)
    fit = _fit(p)
    gq = np.array([3, -1, 3, 0, 99, 11, -1, 3, 5, 5, 0, 99, 3])
    _, cov = wpr.predict_path(fit, TQ, gq)
    ev = np.linalg.eigvalsh(cov)
    print(f"mixed ids: smallest eigenvalue {ev[0]:.3g}, largest {ev[-1]:.3g}")
    assert np.array_equal(cov, cov.T) and ev[0] > 1e-3
