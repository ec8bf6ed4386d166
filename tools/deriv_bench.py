"""Posterior-gradient timings: ``predict``, ``predict_gradient`` mean-only (matrix-free), ``predict_gradient`` with the
derivative variances, and the same with ``with_value=True`` (mean, var, dmean, dvar from one pass), at the C3 shape
(N = 65536, M = 4096, d = 3, fp64) and at a path-sized N, all on ONE handle per shape.  Prints one JSON line.  Queries are
device tensors (outputs stay on the device).  Times are the library's own hipEvent clocks (``timings_["predict_total"]``)
and the host wall time of the blocking call, medians over ``--iters`` calls after one warm-up call each.

    python tools/deriv_bench.py                               # N = 65536 and N = 4096, M = 4096, d = 3
    python tools/deriv_bench.py --shapes 4096,4096 --iters 3
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PHASES = ("kstar", "trsm", "mean", "var", "d2h")


def median_call(fn, gp, iters):
    fn()                                             # warm-up: buffers, code objects
    dev, wall = [], []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        wall.append((time.perf_counter() - t0) * 1e3)
        dev.append(gp.timings_["predict_total"])
    t = gp.timings_
    return {"ms": round(float(np.median(dev)), 3), "wall_ms": round(float(np.median(wall)), 3),
            "phases_ms": {k: round(t[k], 3) for k in PHASES}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="65536,4096;4096,4096")
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--d", type=int, default=3)
    args = ap.parse_args()
    import torch
    from gaussianprocesspathmodelling_amd import GP
    out = {"d": args.d, "dtype": "float64", "kernel": "rbf", "iters": args.iters, "shapes": []}
    for shape in args.shapes.split(";"):
        N, M = (int(v) for v in shape.split(","))
        rng = np.random.default_rng(N + M)
        X = rng.uniform(0.0, 1.0, (N, args.d))
        y = np.sin(2 * np.pi * X[:, 0]) + 0.1 * rng.standard_normal(N)
        Xs = torch.from_numpy(rng.uniform(0.0, 1.0, (M, args.d))).to("cuda:0")
        with GP("rbf", 0.25, 1.5, 1e-2) as gp:
            t0 = time.perf_counter()
            gp.fit(X, y)
            fit_s = time.perf_counter() - t0
            r = {"N": N, "M": M, "fit_s": round(fit_s, 3)}
            r["predict"] = median_call(lambda: gp.predict(Xs), gp, args.iters)
            r["grad_mean_only"] = median_call(lambda: gp.predict_gradient(Xs, return_var=False), gp, args.iters)
            r["grad_var"] = median_call(lambda: gp.predict_gradient(Xs), gp, args.iters)
            r["grad_var_with_value"] = median_call(lambda: gp.predict_gradient(Xs, with_value=True), gp, args.iters)
        r["mean_only_gexp_per_s"] = round(float(M) * N / (r["grad_mean_only"]["ms"] * 1e-3) / 1e9, 1)
        r["build_bytes_gb"] = round((args.d + 1) * M * (((N + 127) // 128) * 128) * 8 / 1e9, 2)
        out["shapes"].append(r)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
