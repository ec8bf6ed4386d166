"""Tabulates the bias of the pathwise sampler's posterior variance (CPU, the NumPy reference of tests/pathwise_ref.py).

The data update of a pathwise sample is exact; its prior is a sum of F random Fourier features.  For a given set of
frequencies the sampler's covariance is known in closed form (pathwise_ref.sampler_cov), so the bias needs no sampling:
per family and F in {256, 1024, 4096}, max over the query points of |closed-form variance - true posterior variance| / sf2
on the fixture of tests/test_pathwise_ref.py (N = 150 sorted uniform points on [0, 1], 40 query points on [-0.2, 1.2],
l = 0.2, sf2 = 1.5, noise = 1e-2), for the frequencies of the seeds 7, 8 and 9 (each listed; the table quotes the largest).

    python tools/pathwise_bias.py [--out profiles/pathwise_bias.json]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import pathwise_ref as pw  # noqa: E402

N, LS, SF2, NOISE = 150, 0.2, 1.5, 1e-2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "pathwise_bias.json"))
    a = ap.parse_args()
    X = np.sort(np.random.default_rng(0).uniform(0.0, 1.0, N))[:, None]
    Xq = np.linspace(-0.2, 1.2, 40)[:, None]
    rows = []
    for kernel in ("rbf", "matern52", "matern32", "matern12"):
        true = np.diag(pw.posterior(kernel, X, np.zeros(N), Xq, LS, SF2, NOISE)[1])
        for F in (256, 1024, 4096):
            per_seed = []
            for seed in (7, 8, 9):
                g, chin, _, _ = pw.split(pw.normals(seed, kernel, F, 1, 1, N), kernel, F, 1, 1, N)
                var = np.diag(pw.sampler_cov(kernel, X, Xq, LS, SF2, NOISE, pw.frequencies(g, chin)))
                per_seed.append(float(np.max(np.abs(var - true)) / SF2))
            rows.append({"kernel": kernel, "F": F, "max_abs_variance_bias_over_sf2": max(per_seed), "per_seed": per_seed})
            print(f"{kernel:9s} F={F:5d}: {max(per_seed):.4f}  {['%.4f' % v for v in per_seed]}")
    out = {"tool": "tools/pathwise_bias.py", "fixture": {"N": N, "lengthscale": LS, "variance": SF2, "noise": NOISE,
                                                         "queries": "40 on [-0.2, 1.2]", "seeds": [7, 8, 9]},
           "quantity": "max over the queries of |closed-form sampler variance - true posterior variance| / variance",
           "rows": rows}
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
