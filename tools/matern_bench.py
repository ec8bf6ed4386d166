#!/usr/bin/env python3
"""Cost of the four kernel families at the bench size (N = 65536, M = 4096, d = 3, fp64, the bench's scalar
lengthscale 0.25, sf2 1.5, sn2 1e-2): fit + predict (mean and variance) wall time, the kernel-build phase
(``timings_["kbuild"]``) and the LML-gradient wall time.  The kernels are visited in turn, ``--reps`` times, on
one handle each (warmed up once), so a drift of the card shows up in every family alike; the best of the reps is
reported with all of them.  One JSON line per kernel, appended to profiles/matern_bench.jsonl and printed.

    python tools/matern_bench.py [--ntrain 65536] [--m 4096] [--reps 3] [--no-grad] [--kernels rbf,matern52] [--tag T]

``--kernels`` / ``--tag`` serve an A/B of the existing families against an older build: run a copy of this file from
that build's tree with ``--kernels rbf,matern52``, alternating with this tree, and compare the tagged lines.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench import LENGTHSCALE, SF2, SN2, synthetic  # noqa: E402
from gaussianprocesspathmodelling_amd import GP  # noqa: E402

KERNELS = ("rbf", "matern52", "matern32", "matern12")

ap = argparse.ArgumentParser()
ap.add_argument("--ntrain", type=int, default=65536)
ap.add_argument("--m", type=int, default=4096)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--no-grad", action="store_true")
ap.add_argument("--kernels", default=",".join(KERNELS), help="comma-separated subset (A/B against an older build)")
ap.add_argument("--tag", default=None, help="label stored with every line, e.g. which build ran")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "matern_bench.jsonl"))
a = ap.parse_args()
KERNELS = tuple(a.kernels.split(","))
N, M, d = a.ntrain, a.m, 3
X, y, Xs = synthetic(N, d, M, 12345)

res = {k: {"fit_predict_ms": [], "fit_ms": [], "kbuild_ms": [], "grad_ms": []} for k in KERNELS}
check = {}
for rep in range(a.reps):
    for kernel in KERNELS:
        with GP(kernel, LENGTHSCALE, SF2, SN2, jitter=0.0) as gp:
            if rep == 0:
                gp.fit(X, y).predict(Xs)                        # warm-up: allocations, code objects
                if not a.no_grad:
                    gp.lml_gradient()
            t0 = time.perf_counter()
            mean, var = gp.fit(X, y).predict(Xs)
            dt = time.perf_counter() - t0
            tm = gp.timings_
            r = res[kernel]
            r["fit_predict_ms"].append(dt * 1e3)
            r["fit_ms"].append(tm["fit_total"])
            r["kbuild_ms"].append(tm["kbuild"])
            if not a.no_grad:
                t0 = time.perf_counter()
                lml, grad = gp.lml_gradient()
                r["grad_ms"].append((time.perf_counter() - t0) * 1e3)
            check[kernel] = {"mean0": float(mean[0]), "var0": float(var[0]), "finite": bool(np.all(np.isfinite(mean)))}

os.makedirs(os.path.dirname(a.out), exist_ok=True)
base = min(res["rbf"]["fit_ms"]) if "rbf" in res else float("nan")
with open(a.out, "a") as f:
    for kernel in KERNELS:
        r = res[kernel]
        line = {"config": f"N={N} M={M} d={d} fp64 scalar lengthscale {LENGTHSCALE}", "kernel": kernel,
                "fit_predict_ms": min(r["fit_predict_ms"]), "fit_ms": min(r["fit_ms"]),
                "kbuild_ms": min(r["kbuild_ms"]),
                "kbuild_tbs": 8.0 * N * (N + 1) / 2 / (min(r["kbuild_ms"]) * 1e-3) / 1e12,
                "grad_ms": min(r["grad_ms"]) if r["grad_ms"] else None,
                "fit_vs_rbf": min(r["fit_ms"]) / base, "reps": r, "check": check[kernel]}
        if a.tag:
            line["build"] = a.tag
        print(json.dumps(line), flush=True)
        f.write(json.dumps(line) + "\n")
