"""Times gpx_remove_rows against the refit it replaces.

On one handle per size (N = 16896 and N = 65536, d = 3, fp64): fit N points, then remove (a) the first 128 rows — the
worst place: every remaining row is below them — and (b) the 33 rows of a path in the middle; beside them gpx_fit of the
remaining rows on the same handle, same build — what a model without the call has to do.  Every removal starts from a
fresh fit of the N points (not timed).  One warm-up, then `--runs` timed runs (default 5): the median, every single run
and min / max are reported, wall-clock around the C call and the library's own stream clock (timings_["fit_total"]).
The flop count is the header's n3^2 (w + 2 m + m^2 / w) per pass (w = 64, m <= 64 columns per pass).

    python tools/remove_bench.py [--out profiles/remove_bench.json] [--sizes 16896,65536] [--runs 5]
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

W = 64


def data(n, seed=1):
    rng = np.random.default_rng(seed)
    X = rng.uniform(0.0, 1.0, (n, 3))
    y = np.sin(2.0 * np.pi * X[:, 0]) + 0.5 * np.cos(3.0 * X[:, 1:].sum(axis=1)) + 0.1 * rng.standard_normal(n)
    return X, y


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def remove_flops(N, start, count):
    total, hi = 0.0, start + count
    while hi > start:
        lo = max(start, hi - W)
        m, n3 = hi - lo, N - hi
        total += float(n3) ** 2 * (W + 2 * m + m * m / W)
        N, hi = N - m, lo
    return total


def summary(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "all": list(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "remove_bench.json"))
    ap.add_argument("--sizes", default="16896,65536")
    ap.add_argument("--runs", type=int, default=5)
    a = ap.parse_args()
    results = []
    for N in (int(s) for s in a.sizes.split(",")):
        X, y = data(N)
        mid = (N // 66) * 33
        with GP("rbf", 0.25, 1.5, 1e-2, jitter=0.0) as gp:
            for name, start, count in (("first_128", 0, 128), ("middle_path_33", mid, 33)):
                keep = np.r_[0:start, start + count:N]
                Xk, yk = np.ascontiguousarray(X[keep]), np.ascontiguousarray(y[keep])
                rem_wall, rem_dev, fit_wall, fit_dev = [], [], [], []
                for run in range(a.runs + 1):
                    gp.fit(X, y)
                    w = timed(lambda: gp.remove(start, start + count))
                    dv = gp.timings_["fit_total"]
                    wf = timed(lambda: gp.fit(Xk, yk))
                    df = gp.timings_["fit_total"]
                    if run:  # run 0 warms up
                        rem_wall.append(w), rem_dev.append(dv), fit_wall.append(wf), fit_dev.append(df)
                flops = remove_flops(N, start, count)
                r = {"N": N, "case": name, "start": start, "count": count, "passes": -(-count // W),
                     "panels_per_pass": -(-(N - start - count) // W), "remove_flops": flops, "fit_flops": (N - count) ** 3 / 3,
                     "remove_wall_ms": summary(rem_wall), "remove_dev_ms": summary(rem_dev),
                     "refit_wall_ms": summary(fit_wall), "refit_dev_ms": summary(fit_dev)}
                r["remove_tflops"] = flops / (r["remove_dev_ms"]["median"] * 1e-3) / 1e12
                r["speedup_wall"] = r["refit_wall_ms"]["median"] / r["remove_wall_ms"]["median"]
                results.append(r)
                print(f"N={N} {name}: remove {r['remove_wall_ms']['median']:.2f} ms wall ({r['remove_dev_ms']['median']:.2f} "
                      f"device, {r['remove_tflops']:.2f} TFLOP/s by count), refit {r['refit_wall_ms']['median']:.2f} ms: "
                      f"{r['speedup_wall']:.1f}x", flush=True)
    out = {"tool": "tools/remove_bench.py", "runs": a.runs, "dtype": "float64", "kernel": "rbf", "d": 3, "results": results}
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
