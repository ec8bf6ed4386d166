"""CPU: the NumPy reference of the pathwise sampler (tests/pathwise_ref.py) is itself right: its samples have the exact
posterior mean and the closed-form spread, with bounds derived from the sample size alone; its layout has the prefix
property; with zero normals in W and E it returns K* alpha."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pathwise_ref as pw  # noqa: E402

FAMILIES = ["rbf", "matern52", "matern32", "matern12"]
N, S, F, SEED = 150, 4096, 256, 7
LS, SF2, NOISE = 0.2, 1.5, 1e-2


def fixture_data():
    rng = np.random.default_rng(0)
    X = np.sort(rng.uniform(0.0, 1.0, N))[:, None]
    y = np.sin(6.0 * X[:, 0]) + 0.1 * rng.standard_normal(N)
    Xq = np.linspace(-0.2, 1.2, 40)[:, None]
    return X, y, Xq


@pytest.mark.parametrize("kernel", FAMILIES)
def test_samples_have_the_exact_mean_and_the_closed_form_spread(kernel):
    """S independent samples: |mean error| <= 5 standard errors, |variance error| <= 5 standard errors of a variance
    estimate of Gaussian samples (var sqrt(2 / (S - 1))) — bounds from S alone.  The reference with these inputs gives
    z-scores up to 3.05 (mean) and 2.47 (variance)."""
    X, y, Xq = fixture_data()
    z = pw.normals(SEED, kernel, F, 1, S, N)
    dr = pw.draw(kernel, X, y, LS, SF2, NOISE, z, S, F)
    f = pw.evaluate(dr, Xq)[:, :, 0]                                   # (S, M)
    mean, _ = pw.posterior(kernel, X, y, Xq, LS, SF2, NOISE)
    var = np.diag(pw.sampler_cov(kernel, X, Xq, LS, SF2, NOISE, dr["Omega"]))
    zm = np.abs(f.mean(axis=0) - mean[:, 0]) / np.sqrt(var / S)
    zv = np.abs(f.var(axis=0, ddof=1) - var) / (var * np.sqrt(2.0 / (S - 1)))
    print(f"{kernel}: largest z-score of the mean {zm.max():.2f}, of the variance {zv.max():.2f}")
    assert zm.max() <= 5.0
    assert zv.max() <= 5.0


@pytest.mark.parametrize("kernel", ["rbf", "matern32"])
def test_prefix_property_of_the_layout(kernel):
    """the first S' samples of a draw with S are the draw with S': the same numbers of the stream, the same functions"""
    X, y, Xq = fixture_data()
    Xm = np.stack([X[:, 0], X[::-1, 0] ** 2], axis=1)                  # d = 2, k = 2
    Y = np.stack([y, np.cos(3.0 * X[:, 0])], axis=1)
    Qm = np.stack([Xq[:, 0], Xq[:, 0] ** 2], axis=1)
    Fs, Sbig, Ssmall = 32, 5, 3
    zb = pw.normals(SEED, kernel, Fs, 2, Sbig * 2, N)
    zs = pw.normals(SEED, kernel, Fs, 2, Ssmall * 2, N)
    assert np.array_equal(zb[:zs.size], zs)                            # one stream, the smaller call a prefix of it
    big = pw.draw(kernel, Xm, Y, (0.2, 0.3), SF2, NOISE, zb, Sbig, Fs)
    small = pw.draw(kernel, Xm, Y, (0.2, 0.3), SF2, NOISE, zs, Ssmall, Fs)
    assert np.array_equal(big["Omega"], small["Omega"])
    assert np.array_equal(big["W"][:Ssmall * 2], small["W"])
    fb, fs = pw.evaluate(big, Qm), pw.evaluate(small, Qm)
    assert fb.shape == (Sbig, 40, 2) and fs.shape == (Ssmall, 40, 2)
    # (a dense solve with more right-hand sides may round differently: 1e-9 of the largest value, the project's bar for
    # the same quantity by another route)
    assert np.max(np.abs(fb[:Ssmall] - fs)) <= 1e-9 * np.max(np.abs(fs))


@pytest.mark.parametrize("kernel", FAMILIES)
def test_zero_normals_in_w_and_e_give_the_posterior_mean(kernel):
    X, y, Xq = fixture_data()
    Fs, Ss = 16, 2
    z = pw.normals(3, kernel, Fs, 1, Ss, N)
    z[Fs * (1 + pw.CHI_DOF[kernel]):] = 0.0                            # frequencies stay random; W = 0, E = 0
    f = pw.evaluate(pw.draw(kernel, X, y, LS, SF2, NOISE, z, Ss, Fs), Xq)
    mean, _ = pw.posterior(kernel, X, y, Xq, LS, SF2, NOISE)
    for s in range(Ss):
        assert np.max(np.abs(f[s] - mean)) <= 1e-9 * np.max(np.abs(mean))


def test_sampler_covariance_approaches_the_posterior_covariance():
    """more features, less bias (the O(1 / sqrt(F)) of the prior): the closed form at F = 4096 is closer to the true
    posterior variance than at F = 64"""
    X, y, Xq = fixture_data()
    _, cov = pw.posterior("rbf", X, y, Xq, LS, SF2, NOISE)
    err = []
    for Fs in (64, 4096):
        g, chin, _, _ = pw.split(pw.normals(SEED, "rbf", Fs, 1, 1, N), "rbf", Fs, 1, 1, N)
        c = pw.sampler_cov("rbf", X, Xq, LS, SF2, NOISE, pw.frequencies(g, chin))
        err.append(np.max(np.abs(np.diag(c) - np.diag(cov))))
    assert err[1] < err[0]
