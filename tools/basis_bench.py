#!/usr/bin/env python3
"""Cost of explicit basis functions (GP.fit(basis=)): fit_total and predict_total (M = 4096) of a fit with
basis="quadratic" beside the plain fit of the same data on the same handle, alternating, at N = 8192 and N = 65536, d = 3,
k = 1, RBF fp64.  One warm-up round and --repeats timed rounds per size; medians and every repeat are reported, and the
solve entry of the basis fit (the Gram of the bordered rows, the coefficient solve and the projection are booked there).
    python tools/basis_bench.py [--sizes 8192,65536] [--repeats 5] [--plain-only]
--plain-only times the plain fit alone: the form that also runs on a checkout without basis functions, for the
no-regression comparison (run both checkouts in one session, alternating)."""
import argparse, json, os, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench import synthetic
from gaussianprocesspathmodelling_amd import GP

ap = argparse.ArgumentParser()
ap.add_argument("--sizes", default="8192,65536")
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--queries", type=int, default=4096)
ap.add_argument("--plain-only", action="store_true")
a = ap.parse_args()
keys = ("fit_total", "chol", "solve", "predict_total", "mean", "var")
variants = [None] if a.plain_only else [None, "quadratic"]
out = {"config": f"d=3 k=1 RBF ARD fp64, M={a.queries}, 1 warm-up + {a.repeats} repeats alternating, medians (ms)"}
for N in (int(v) for v in a.sizes.split(",")):
    X, y, Xs = synthetic(N, 3, a.queries, 12345)
    rows = {str(b): [] for b in variants}
    with GP("rbf", np.array([0.3, 0.2, 0.25]), 1.5, 1e-2, jitter=0.0) as gp:
        for rep in range(1 + a.repeats):                       # the first round is the warm-up (allocations)
            for b in variants:
                gp.fit(X, y, **({} if b is None else {"basis": b}))
                fit_tm = gp.timings_
                gp.predict(Xs)
                tm = gp.timings_
                if rep:
                    rows[str(b)].append({k: (fit_tm if k in ("fit_total", "chol", "solve") else tm)[k] for k in keys})
    res = {b: {k + "_ms": float(np.median([r[k] for r in rs])) for k in keys} | {"repeats": rs} for b, rs in rows.items()}
    if not a.plain_only:
        for k in ("fit_total", "predict_total"):
            res[k + "_ratio"] = res["quadratic"][k + "_ms"] / res["None"][k + "_ms"]
            res[k + "_plain_spread"] = (max(r[k] for r in rows["None"]) - min(r[k] for r in rows["None"])) / res["None"][k + "_ms"]
    out[f"N{N}"] = res
print(json.dumps(out))
