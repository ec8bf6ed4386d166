"""Measurements of predicting observed paths themselves (profiles/within_predict.json) on one GPU: on ONE
grouped fit (N = 8192 = 256 paths of 32 points, Matern-3/2, d = 1) and M = 4096 query points, ``predict`` against
``predict(path_ids=...)`` and ``predict_gradient`` against ``predict_gradient(path_ids=...)`` — the two sides of each
comparison alternated in one process after a warm-up, five runs each.  The query ids are those of the nearest training
point's path, so every 64 x 64 tile of K* whose id ranges overlap evaluates the second term.  Reported per side: the
median, lowest and highest of the host clock around the blocking call and of the library's phase clocks (``kstar``: the
builders, ``var``: the row norms, ``trsm``: the forward solve, ``predict_total``).  Prints one JSON line and writes it to
profiles/within_predict.json (``--out FILE``: there instead)."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gaussianprocesspathmodelling_amd import GP  # noqa: E402

rng = np.random.default_rng(0)
P, L, M = 256, 32, 4096
N = P * L
t = np.sort(rng.uniform(0, 1, (P, L)), axis=1).reshape(N, 1)
ids = np.repeat(np.arange(P), L).astype(np.int32)
Y = np.sin(6 * t) + 0.3 * np.repeat(rng.standard_normal((P, 1)), L, axis=0) + 0.1 * rng.standard_normal((N, 1))
Y = np.concatenate([Y, np.cos(5 * t) + 0.1 * rng.standard_normal((N, 1))], axis=1)
pick = rng.choice(N, M, replace=False)
Xq = np.ascontiguousarray(t[pick] + 0.002 * rng.standard_normal((M, 1)))
gq = np.ascontiguousarray(ids[pick])
NAMES = ("wall_ms", "predict_total_ms", "kstar_ms", "trsm_ms", "mean_ms", "var_ms")
res = {"N": N, "paths": P, "points_per_path": L, "M": M, "kernel": "matern32", "d": 1, "runs": 5}


def timed(gp, call):
    t0 = time.perf_counter()
    call()
    w = (time.perf_counter() - t0) * 1e3
    a = gp.timings_
    return (w, a["predict_total"], a["kstar"], a["trsm"], a["mean"], a["var"])


def spread(rows):
    return {n: {"median": float(np.median([r[i] for r in rows])), "min": float(min(r[i] for r in rows)),
                "max": float(max(r[i] for r in rows))} for i, n in enumerate(NAMES)}


with GP("matern32", 0.25, 1.5, 1e-2) as gp:
    gp.fit(t, Y, path_ids=ids, path_variance=0.4, path_lengthscale=0.1)
    pairs = {"predict": (lambda: gp.predict(Xq), lambda: gp.predict(Xq, path_ids=gq)),
             "predict_gradient": (lambda: gp.predict_gradient(Xq), lambda: gp.predict_gradient(Xq, path_ids=gq))}
    for name, (plain, paths) in pairs.items():
        for _ in range(2):
            plain()
            paths()
        a, b = [], []
        for _ in range(5):
            a.append(timed(gp, plain))
            b.append(timed(gp, paths))
        res[name] = spread(a)
        res[name + "_path_ids"] = spread(b)
out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "within_predict.json")
with open(out, "w") as f:
    json.dump(res, f, indent=1)
print(json.dumps(res))
