"""What the KINDS kernel build costs: hipEvent phase clocks ``timings_["kbuild"]``, ``["chol"]`` (fit) and
``["kstar"]`` (predict, M = 2048) at N = 16384 observation rows, d = 3, for

  plain      fit(X, y)                                   the kernels every handle launched before
  all_values the same rows with kinds all -1             KINDS build, every tile on its value-only path
  deriv10    10 % of the rows derivative observations    KINDS build, the tiles that touch the last 10 % of the rows mixed

The three are measured round-robin in one process (median of --iters rounds after one warm-up round), so drift hits them
alike.  On a checkout without ``GP.fit(derivatives=)`` — the parent commit — only ``plain`` runs: run this file there with
``--out <file>`` and pass that file as ``--parent`` here; the result then carries the parent's plain fit beside this
commit's, and the ratios against it.  Writes profiles/dobs_build.json."""
import argparse
import inspect
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PHASES = ("kbuild", "chol", "kstar")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=16384)
    ap.add_argument("--m", type=int, default=2048)
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--kernel", default="matern52")
    ap.add_argument("--parent", default=None, help="result file of a run of this tool on the parent commit")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dobs_build.json"))
    a = ap.parse_args()
    from gaussianprocesspathmodelling_amd import GP
    has_feature = "derivatives" in inspect.signature(GP.fit).parameters
    rng = np.random.default_rng(0)
    N, d, Nd = a.n, 3, a.n // 10
    X = rng.uniform(0.0, 1.0, (N, d))
    w = np.array([3.0, 2.0, 4.0])
    y = np.sin(X @ w) + 0.1 * rng.standard_normal(N)
    Xs = rng.uniform(0.0, 1.0, (a.m, d))
    Xv, yv, Xd = X[:N - Nd], y[:N - Nd], X[N - Nd:]
    dims = rng.integers(0, d, Nd)
    yd = np.cos(Xd @ w) * w[dims] + 0.2 * rng.standard_normal(Nd)
    empty = (np.empty((0, d)), np.empty((0,), dtype=np.int64), np.empty((0,)))
    configs = {"plain": lambda gp: gp.fit(X, y)}
    if has_feature:
        configs["all_values"] = lambda gp: gp.fit(X, y, derivatives=empty)
        configs["deriv10"] = lambda gp: gp.fit(Xv, yv, derivatives=(Xd, dims, yd), derivative_noise=5e-2)
    samples = {c: {p: [] for p in PHASES} for c in configs}
    with GP(a.kernel, (0.3, 0.25, 0.4), 1.5, 1e-2) as gp:
        for it in range(a.iters + 1):
            for name, fit in configs.items():
                fit(gp)
                t = gp.timings_
                gp.predict(Xs)
                t["kstar"] = gp.timings_["kstar"]
                if it:
                    for p in PHASES:
                        samples[name][p].append(t[p])
    res = {"n": N, "d": d, "m": a.m, "kernel": a.kernel, "iters": a.iters, "unit": "ms",
           "median": {c: {p: round(float(np.median(v)), 4) for p, v in ph.items()} for c, ph in samples.items()},
           "min_max": {c: {p: [round(float(np.min(v)), 4), round(float(np.max(v)), 4)] for p, v in ph.items()}
                       for c, ph in samples.items()}}
    if a.parent:
        par = json.load(open(a.parent))
        res["parent_plain"] = {"median": par["median"]["plain"], "min_max": par["min_max"]["plain"]}
        res["ratio_to_parent_plain"] = {c: {p: round(res["median"][c][p] / par["median"]["plain"][p], 3) for p in PHASES}
                                        for c in res["median"]}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
