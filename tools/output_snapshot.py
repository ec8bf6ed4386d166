#!/usr/bin/env python
"""Every output of the public Python API on one fixed, seeded problem, written to one .npz.

For refactors of the host side of libgpx.so: run it in a checkout of the commit before and of the commit after
(public API only, so the same script runs in both) and compare the two files with ``--compare``: every array must
be equal bit for bit (``np.array_equal``).  Under ``rocprofv3 --kernel-trace --stats -- python
tools/output_snapshot.py OUT.npz`` the per-kernel call counts of the two runs must be equal as well.

    python tools/output_snapshot.py OUT.npz            # needs a GPU
    python tools/output_snapshot.py --compare A.npz B.npz

Sizes: N = 4096 and 8192 (k = 2 targets, d = 2), M = 3000 query points (padded to 3072) with GPX_PRED_BATCH=1024, so
padding and more than one batch of query points are exercised.
"""
from __future__ import annotations

import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

M, D, K = 3000, 2, 2
SIZES = (4096, 8192)
HYPER = dict(lengthscale=(0.3, 0.2), variance=1.5, noise=1e-2, jitter=0.0)


def problem(n, dtype):
    rng = np.random.default_rng(20240 + n)
    X = rng.uniform(0.0, 1.0, (n, D))
    W = rng.standard_normal((D, K))
    y = np.sin(4.0 * X @ W) + 0.1 * rng.standard_normal((n, K))
    Xs = rng.uniform(0.0, 1.0, (M, D))
    return X.astype(dtype), y.astype(dtype), Xs.astype(dtype)


def snapshot(out):
    from gaussianprocesspathmodelling_amd import GP

    def put(name, value):
        for i, a in enumerate(value if isinstance(value, tuple) else (value,)):
            out[f"{name}.{i}"] = np.asarray(a)

    for n in SIZES:
        for dtype in ("float64", "float32"):
            X, y, Xs = problem(n, dtype)
            tag = f"n{n}.{dtype}"
            with GP("matern52", dtype=dtype, device=0, **HYPER) as gp:
                gp.fit(X, y)
                put(f"{tag}.logdet", gp.log_det_)
                put(f"{tag}.predict_var", gp.predict(Xs))
                put(f"{tag}.predict_mean", gp.predict(Xs, return_var=False))
                put(f"{tag}.predict_cov", gp.predict(Xs[:1500], return_cov=True))
                put(f"{tag}.predict_after_cov", gp.predict(Xs))
                put(f"{tag}.sample_y", gp.sample_y(Xs[:1500], n_samples=3, random_state=7))
                put(f"{tag}.grad_mean", gp.predict_gradient(Xs, return_var=False))
                put(f"{tag}.grad_var", gp.predict_gradient(Xs))
                put(f"{tag}.grad_value", gp.predict_gradient(Xs, with_value=True))
                put(f"{tag}.alpha", gp.alpha_)
                if dtype == "float64":
                    put(f"{tag}.lml_gradient", gp.lml_gradient())
                put(f"{tag}.fit_predict", gp.fit_predict(X, y, Xs))
                gp.release_scratch()
                put(f"{tag}.predict_after_release", gp.predict(Xs))
        X, y, Xs = problem(n, "float64")
        with GP("matern52", dtype="mixed", device=0, **HYPER) as gp:
            gp.fit(X, y)
            put(f"n{n}.mixed.predict_var", gp.predict(Xs))
            put(f"n{n}.mixed.predict_mean", gp.predict(Xs, return_var=False))
            put(f"n{n}.mixed.alpha", gp.alpha_)
        # two ranks of a row-block shard on one card (local transport)
        with GP("matern52", devices=[0, 0], transport="local", **HYPER) as gp:
            gp.fit(X, y)
            put(f"n{n}.shard.logdet", gp.log_det_)
            put(f"n{n}.shard.predict_var", gp.predict(Xs))
            put(f"n{n}.shard.predict_mean", gp.predict(Xs, return_var=False))
            put(f"n{n}.shard.alpha", gp.alpha_)
            put(f"n{n}.shard.lml_gradient", gp.lml_gradient())
            put(f"n{n}.shard.fit_predict", gp.fit_predict(X, y, Xs))


def sha256(path):
    """of the CONTENT (names, dtypes, shapes, bytes in name order): the .npz container itself carries time stamps"""
    h, Z = hashlib.sha256(), np.load(path)
    for k in sorted(Z.files):
        a = np.ascontiguousarray(Z[k])
        h.update(f"{k}:{a.dtype.str}:{a.shape}".encode())
        h.update(a.tobytes())
    return h.hexdigest()


def compare(a, b):
    A, B = np.load(a), np.load(b)
    bad = sorted(set(A.files) ^ set(B.files))
    bad += [k for k in A.files if k in B.files and not np.array_equal(A[k], B[k])]
    print(f"{len(A.files)} arrays; sha256 {sha256(a)[:16]} {sha256(b)[:16]}; {'DIFFERENT: ' + ', '.join(bad) if bad else 'all equal'}")
    return 1 if bad else 0


def main(argv):
    if len(argv) == 3 and argv[0] == "--compare":
        return compare(argv[1], argv[2])
    if len(argv) != 1:
        print(__doc__)
        return 2
    os.environ["GPX_PRED_BATCH"] = "1024"
    out = {}
    snapshot(out)
    os.makedirs(os.path.dirname(os.path.abspath(argv[0])), exist_ok=True)
    np.savez(argv[0], **out)
    print(f"{len(out)} arrays -> {argv[0]}  sha256 {sha256(argv[0])}")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
