"""Joint-posterior timings: ``predict``, ``predict(return_cov=True)`` and ``sample_y`` at (N, M, S) shapes, one JSON
line per shape.  Queries are device tensors (outputs stay on the device: no copy of the M x M covariance to the host
inside the timed window).  Times are the library's own hipEvent clocks (``timings_["predict_total"]``: the call's work
on its stream) and the host wall time of the blocking call, medians over ``--iters`` calls after one warm-up call each.
``sigma_tflops`` = the SYRK's M^2 N flops over the ``var`` phase of ``predict(return_cov=True)`` (symmetric kernel
build + SYRK + mirror: a lower bound on the SYRK's own rate).

    python tools/posterior_bench.py                       # (8192, 4096, 64) and (65536, 4096, 64)
    python tools/posterior_bench.py --shapes 8192,4096,64 --iters 3
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def median_call(fn, gp, iters):
    fn()                                             # warm-up: buffers, code objects
    dev, wall = [], []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        wall.append((time.perf_counter() - t0) * 1e3)
        dev.append(gp.timings_["predict_total"])
    return float(np.median(dev)), float(np.median(wall)), gp.timings_


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="8192,4096,64;65536,4096,64")
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--d", type=int, default=3)
    args = ap.parse_args()
    import torch
    from gaussianprocesspathmodelling_amd import GP
    for shape in args.shapes.split(";"):
        N, M, S = (int(v) for v in shape.split(","))
        rng = np.random.default_rng(N + M)
        X = rng.uniform(0.0, 1.0, (N, args.d))
        y = np.sin(2 * np.pi * X[:, 0]) + 0.1 * rng.standard_normal(N)
        Xs = torch.from_numpy(rng.uniform(0.0, 1.0, (M, args.d))).to("cuda:0")
        with GP("rbf", 0.25, 1.5, 1e-2) as gp:
            t0 = time.perf_counter()
            gp.fit(X, y)
            fit_s = time.perf_counter() - t0
            p_dev, p_wall, _ = median_call(lambda: gp.predict(Xs), gp, args.iters)
            c_dev, c_wall, tc = median_call(lambda: gp.predict(Xs, return_cov=True), gp, args.iters)
            s_dev, s_wall, ts = median_call(lambda: gp.sample_y(Xs, S, random_state=1), gp, args.iters)
        flops = float(M) * M * (((N + 127) // 128) * 128)
        print(json.dumps({
            "N": N, "M": M, "S": S, "fit_s": round(fit_s, 3),
            "predict_ms": round(p_dev, 3), "predict_cov_ms": round(c_dev, 3), "sample_ms": round(s_dev, 3),
            "predict_wall_ms": round(p_wall, 3), "predict_cov_wall_ms": round(c_wall, 3),
            "sample_wall_ms": round(s_wall, 3),
            "cov_extra_ms": round(c_dev - p_dev, 3), "sample_extra_ms": round(s_dev - c_dev, 3),
            "cov_phases_ms": {k: round(tc[k], 3) for k in ("kstar", "trsm", "mean", "var", "d2h")},
            "sample_phases_ms": {k: round(ts[k], 3) for k in ("kstar", "trsm", "mean", "var", "d2h")},
            "sigma_tflops": round(flops / (tc["var"] * 1e-3) / 1e12, 2),
            "sample_jitter": gp.sample_jitter_,
        }), flush=True)


if __name__ == "__main__":
    main()
