"""Generate tests/golden/G7.npz: scikit-learn's joint posterior covariance (``predict(Xs, return_cov=True)``), the
fixture of the joint-posterior tests (tests/test_posterior_gpu.py).

Two cases, both with two target columns and M = 150 query points (not a multiple of 64):
  rbf  — ConstantKernel * RBF, scalar lengthscale, d = 1 (a time axis, as a path model has)
  mat  — ConstantKernel * Matern(nu=2.5), ARD lengthscales, d = 3
``GaussianProcessRegressor(alpha=noise, optimizer=None)``: the hyper-parameters are fixed inputs, as in the library.
Stored per case (prefix ``rbf_`` / ``mat_``): X, y, Xs, kernel, lengthscale, variance, noise, and sklearn's mean
(M, 2) and cov (M, M) — the covariance is the same for every target column.  Needs scikit-learn (1.7.2 was used):

    python tools/make_golden_cov.py        # rewrites tests/golden/G7.npz
"""
from __future__ import annotations

import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "G7.npz")

CASES = {
    # prefix: (N, d, M, kernel, lengthscale, sf2, sn2, seed)
    "rbf": (400, 1, 150, "rbf", 0.15, 1.3, 1e-2, 71),
    "mat": (397, 3, 150, "matern52", (0.4, 0.3, 0.5), 0.8, 2e-2, 72),
}


def problem(N, d, M, seed):
    rng = np.random.default_rng(seed)
    X = rng.uniform(0.0, 1.0, (N, d))
    Xs = rng.uniform(0.0, 1.0, (M, d))
    s = X.sum(axis=1)
    y = np.stack([np.sin(2.0 * np.pi * X[:, 0]) + 0.3 * np.cos(2.0 * s),
                  np.cos(3.0 * s) - 0.5 * X[:, -1]], axis=1) + 0.05 * rng.standard_normal((N, 2))
    return X, y, Xs


def sklearn_cov(X, y, Xs, kernel, ls, sf2, sn2):
    from sklearn.gaussian_process import GaussianProcessRegressor
    from sklearn.gaussian_process.kernels import RBF, ConstantKernel, Matern
    ls = np.atleast_1d(np.asarray(ls, float))
    ls = float(ls[0]) if ls.size == 1 else ls
    base = RBF(ls, "fixed") if kernel == "rbf" else Matern(ls, "fixed", nu=2.5)
    gpr = GaussianProcessRegressor(kernel=ConstantKernel(sf2, "fixed") * base, alpha=sn2, optimizer=None,
                                   normalize_y=False)
    gpr.fit(X, y)
    mean, cov = gpr.predict(Xs, return_cov=True)
    cov = cov[..., 0] if cov.ndim == 3 else cov       # (M, M, k): one matrix per target, all the same
    return mean, cov


def main():
    out = {}
    for name, (N, d, M, kernel, ls, sf2, sn2, seed) in CASES.items():
        X, y, Xs = problem(N, d, M, seed)
        mean, cov = sklearn_cov(X, y, Xs, kernel, ls, sf2, sn2)
        out.update({f"{name}_X": X, f"{name}_y": y, f"{name}_Xs": Xs, f"{name}_kernel": np.array(kernel),
                    f"{name}_lengthscale": np.atleast_1d(np.asarray(ls, float)), f"{name}_variance": np.array(sf2),
                    f"{name}_noise": np.array(sn2), f"{name}_mean": mean, f"{name}_cov": cov})
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes)")


if __name__ == "__main__":
    main()
