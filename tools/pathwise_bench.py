"""Times pathwise posterior function samples beside gpx_sample_posterior.

One fp64 handle, the C3 shape: N = 65536, d = 3, k = 2, rbf; S = 32 functions (C = 64 columns), F = 4096 frequencies.
Measured, each after `--warmup` untimed calls, `--runs` times, medians reported with min / max and every run:
  draw           GP.sample_functions: wall, and the handle's clocks kstar (normals, features at the training points,
                 residual rows) and trsm (the two triangular solves)
  eval           the functions at M = 4096 and M = 262144 device-resident query points: wall and the `mean` clock (the
                 evaluation kernel with its finish and unpack); from the latter the kernel evaluations per second
                 (M N + 2 F M per 64 columns) and the achieved MFMA rate (2 C (N + 2 F) M flops)
  sample_y       GP.sample_y with the same S at M = 4096, for comparison
A device synchronise before and after every call, wall-clock around it.

    python tools/pathwise_bench.py [--out profiles/pathwise_bench.json] [--n 65536] [--runs 5] [--warmup 2]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gaussianprocesspathmodelling_amd import GP  # noqa: E402


def summary(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "all": list(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "pathwise_bench.json"))
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--samples", type=int, default=32)
    ap.add_argument("--features", type=int, default=4096)
    ap.add_argument("--queries", default="4096,262144")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("pathwise_bench needs a GPU: nothing is measured without one")

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, r

    N, d, k, S, F = a.n, 3, 2, a.samples, a.features
    C = S * k
    rng = np.random.default_rng(1)
    X = rng.uniform(0.0, 1.0, (N, d))
    y = np.stack([np.sin(2.0 * np.pi * X[:, 0]) + 0.5 * np.cos(3.0 * X[:, 1:].sum(axis=1)), np.cos(2.0 * X.sum(axis=1))], axis=1)
    y += 0.1 * rng.standard_normal(y.shape)
    out = {"tool": "tools/pathwise_bench.py", "dtype": "float64", "kernel": "rbf", "N": N, "d": d, "k": k, "S": S, "F": F,
           "columns": C, "runs": a.runs, "warmup": a.warmup}
    with GP("rbf", 0.25, 1.5, 1e-2, jitter=0.0) as gp:
        gp.fit(X, y)
        out["fit_total_ms"] = gp.timings_["fit_total"]
        wall, feat, solve = [], [], []
        for run in range(a.warmup + a.runs):
            w, fs = timed(lambda: gp.sample_functions(S, n_features=F, random_state=run))
            tm = gp.timings_
            if run >= a.warmup:
                wall.append(w), feat.append(tm["kstar"]), solve.append(tm["trsm"])
        out["draw"] = {"wall_ms": summary(wall), "features_ms": summary(feat), "solve_ms": summary(solve)}
        print(f"draw: {out['draw']['wall_ms']['median']:.1f} ms wall (features {out['draw']['features_ms']['median']:.1f}, "
              f"solve {out['draw']['solve_ms']['median']:.1f})", flush=True)
        out["eval"] = []
        for M in (int(s) for s in a.queries.split(",")):
            Xs = torch.as_tensor(rng.uniform(0.0, 1.0, (M, d)), device=f"cuda:{gp.device}")
            wall, kern = [], []
            for run in range(a.warmup + a.runs):
                w, _ = timed(lambda: fs(Xs))
                if run >= a.warmup:
                    wall.append(w), kern.append(gp.timings_["mean"])
            r = {"M": M, "wall_ms": summary(wall), "kernel_ms": summary(kern)}
            s = r["kernel_ms"]["median"] * 1e-3
            blocks = (C + 63) // 64
            r["kernel_evaluations_per_s"] = blocks * (float(M) * N + 2.0 * F * M) / s
            r["mfma_tflops"] = 2.0 * blocks * 64 * (N + 2.0 * F) * M / s / 1e12
            out["eval"].append(r)
            print(f"eval M={M}: {r['wall_ms']['median']:.2f} ms wall, kernel {r['kernel_ms']['median']:.2f} ms, "
                  f"{r['kernel_evaluations_per_s'] / 1e12:.2f} T evaluations/s, {r['mfma_tflops']:.1f} TF on the MFMA units",
                  flush=True)
        M = int(a.queries.split(",")[0])
        Xs = torch.as_tensor(rng.uniform(0.0, 1.0, (M, d)), device=f"cuda:{gp.device}")
        wall = []
        for run in range(a.warmup + a.runs):
            w, _ = timed(lambda: gp.sample_y(Xs, S, random_state=run))
            if run >= a.warmup:
                wall.append(w)
        out["sample_y"] = {"M": M, "wall_ms": summary(wall)}
        ratio = out["sample_y"]["wall_ms"]["median"] / out["eval"][0]["wall_ms"]["median"]
        out["sample_y_over_eval"] = ratio
        print(f"sample_y M={M}: {out['sample_y']['wall_ms']['median']:.1f} ms wall = {ratio:.0f} x the evaluation", flush=True)
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
