"""Posterior second-derivative timings: ``predict_hessian`` mean-only (matrix-free) and with the variances, beside
``predict`` and ``predict_gradient`` (mean-only, with variances) on the SAME handle, fp64 RBF, for d = 1 and d = 3 at
M = 4096 query points and N = 4096 and 65536.  Prints one JSON line per d.  Queries are device tensors (outputs stay on the
device).  Times are the library's own hipEvent clocks (``timings_["predict_total"]``) and the host wall time of the blocking
call, medians over ``--iters`` calls after one warm-up call each.

    python tools/hess_bench.py > profiles/hess_bench.jsonl
    python tools/hess_bench.py --shapes 4096,4096 --dims 3 --iters 3
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
    ap.add_argument("--dims", default="1,3")
    ap.add_argument("--iters", type=int, default=5)
    args = ap.parse_args()
    import torch
    from gaussianprocesspathmodelling_amd import GP
    for d in (int(v) for v in args.dims.split(",")):
        d2 = d * (d + 1) // 2
        out = {"d": d, "pairs": d2, "dtype": "float64", "kernel": "rbf", "iters": args.iters, "shapes": []}
        for shape in args.shapes.split(";"):
            N, M = (int(v) for v in shape.split(","))
            rng = np.random.default_rng(N + M + d)
            X = rng.uniform(0.0, 1.0, (N, d))
            y = np.sin(2 * np.pi * X[:, 0]) + 0.1 * rng.standard_normal(N)
            Xs = torch.from_numpy(rng.uniform(0.0, 1.0, (M, d))).to("cuda:0")
            with GP("rbf", 0.25, 1.5, 1e-2) as gp:
                t0 = time.perf_counter()
                gp.fit(X, y)
                r = {"N": N, "M": M, "fit_s": round(time.perf_counter() - t0, 3)}
                r["predict"] = median_call(lambda: gp.predict(Xs), gp, args.iters)
                r["grad_mean_only"] = median_call(lambda: gp.predict_gradient(Xs, return_var=False), gp, args.iters)
                r["grad_var"] = median_call(lambda: gp.predict_gradient(Xs), gp, args.iters)
                r["hess_mean_only"] = median_call(lambda: gp.predict_hessian(Xs, return_var=False), gp, args.iters)
                r["hess_var"] = median_call(lambda: gp.predict_hessian(Xs), gp, args.iters)
            r["hess_var_trsm_over_predict_trsm"] = round(r["hess_var"]["phases_ms"]["trsm"] / r["predict"]["phases_ms"]["trsm"], 2)
            r["hess_mean_only_over_grad_mean_only"] = round(r["hess_mean_only"]["ms"] / r["grad_mean_only"]["ms"], 2)
            r["build_bytes_gb"] = round(d2 * M * (((N + 127) // 128) * 128) * 8 / 1e9, 2)
            out["shapes"].append(r)
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
