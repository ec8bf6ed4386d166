"""Generate tests/golden/G8.npz: scikit-learn's posterior (mean, joint covariance) and log marginal likelihood with its
gradient for the Matern-3/2 and Matern-1/2 kernels, the fixture of tests/test_matern_ref.py and tests/test_matern_gpu.py.

Two cases, both with two target columns and M = 100 query points (not a multiple of 64):
  m32 — ConstantKernel * Matern(nu=1.5), scalar lengthscale, d = 1 (a time axis, as a path model has)
  m12 — ConstantKernel * Matern(nu=0.5), ARD lengthscales, d = 3; ten training inputs are repeated (r = 0 pairs)
``GaussianProcessRegressor(alpha=noise, optimizer=None)``: the hyper-parameters are fixed inputs, as in the library.
The LML and its gradient come from ``ConstantKernel * Matern + WhiteKernel(noise)`` with ``alpha=0``: the same
covariance, with the noise as a hyper-parameter.  scikit-learn orders theta as (log sf2, log l..., log sn2); stored
here in the library's order (log l..., log sf2, log sn2), as ``lml_grad``.
Stored per case (prefix ``m32_`` / ``m12_``): X, y, Xs, kernel, lengthscale, variance, noise, mean (M, 2), cov (M, M),
lml, lml_grad.  Needs scikit-learn (1.7.2 was used):

    python tools/make_golden_matern.py        # rewrites tests/golden/G8.npz
"""
from __future__ import annotations

import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "G8.npz")

CASES = {
    # prefix: (N, d, M, kernel, nu, lengthscale, sf2, sn2, seed)
    "m32": (300, 1, 100, "matern32", 1.5, 0.12, 1.3, 1e-2, 81),
    "m12": (297, 3, 100, "matern12", 0.5, (0.6, 0.45, 0.8), 0.8, 2e-2, 82),
}


def problem(N, d, M, seed, repeats):
    rng = np.random.default_rng(seed)
    X = rng.uniform(0.0, 1.0, (N, d))
    if repeats:
        X[N - repeats:] = X[:repeats]           # duplicate inputs: r = 0 off the diagonal
    Xs = rng.uniform(0.0, 1.0, (M, d))
    s = X.sum(axis=1)
    y = np.stack([np.sin(2.0 * np.pi * X[:, 0]) + 0.3 * np.cos(2.0 * s),
                  np.cos(3.0 * s) - 0.5 * X[:, -1]], axis=1) + 0.05 * rng.standard_normal((N, 2))
    return X, y, Xs


def sklearn_case(X, y, Xs, nu, ls, sf2, sn2):
    from sklearn.gaussian_process import GaussianProcessRegressor
    from sklearn.gaussian_process.kernels import ConstantKernel, Matern, WhiteKernel
    ls = np.atleast_1d(np.asarray(ls, float))
    lsk = float(ls[0]) if ls.size == 1 else ls
    gpr = GaussianProcessRegressor(kernel=ConstantKernel(sf2, "fixed") * Matern(lsk, "fixed", nu=nu), alpha=sn2,
                                   optimizer=None, normalize_y=False)
    gpr.fit(X, y)
    mean, cov = gpr.predict(Xs, return_cov=True)
    cov = cov[..., 0] if cov.ndim == 3 else cov       # (M, M, k): one matrix per target, all the same
    kern = ConstantKernel(sf2) * Matern(lsk, nu=nu) + WhiteKernel(sn2)
    lgp = GaussianProcessRegressor(kernel=kern, alpha=0.0, optimizer=None, normalize_y=False).fit(X, y)
    lml, grad = lgp.log_marginal_likelihood(lgp.kernel_.theta, eval_gradient=True)
    n_ls = ls.size
    grad = np.concatenate([grad[1:1 + n_ls], grad[:1], grad[1 + n_ls:]])    # -> (log l..., log sf2, log sn2)
    return mean, cov, float(lml), grad


def main():
    out = {}
    for name, (N, d, M, kernel, nu, ls, sf2, sn2, seed) in CASES.items():
        X, y, Xs = problem(N, d, M, seed, repeats=10 if kernel == "matern12" else 0)
        mean, cov, lml, grad = sklearn_case(X, y, Xs, nu, ls, sf2, sn2)
        out.update({f"{name}_X": X, f"{name}_y": y, f"{name}_Xs": Xs, f"{name}_kernel": np.array(kernel),
                    f"{name}_lengthscale": np.atleast_1d(np.asarray(ls, float)), f"{name}_variance": np.array(sf2),
                    f"{name}_noise": np.array(sn2), f"{name}_mean": mean, f"{name}_cov": cov,
                    f"{name}_lml": np.array(lml), f"{name}_lml_grad": grad})
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes)")


if __name__ == "__main__":
    main()
