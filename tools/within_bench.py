"""Measurements of the within-path model (profiles/within_paths.json) on one GPU, the two sides of each
comparison alternated in one process after a warm-up, five runs each: the fit at N = 8192 with sorted path ids (256 paths of
32 points) against the plain fit of the same data (``timings_["kbuild"]``, ``fit_total``), and ``forecast_blocks`` with
G = 2048, (Lo, Lp) = (20, 13) against ``score_blocks`` of the same 33-row blocks (host clock around the blocking call and the
library's phase clocks).  Prints one JSON line; ``--out FILE`` also writes it there.  The step times of ``bench.py`` for the
parent commit and this one come from running ``bench.py --workload C2 | C3`` of both trees alternately."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gaussianprocesspathmodelling_amd import GP  # noqa: E402

rng = np.random.default_rng(0)
P, L = 256, 32
N = P * L
t = np.sort(rng.uniform(0, 1, (P, L)), axis=1).reshape(N, 1)
ids = np.repeat(np.arange(P), L).astype(np.int32)
Y = np.sin(6 * t) + 0.3 * np.repeat(rng.standard_normal((P, 1)), L, axis=0) + 0.1 * rng.standard_normal((N, 1))
Y = np.concatenate([Y, np.cos(5 * t) + 0.1 * rng.standard_normal((N, 1))], axis=1)
res = {"N": N, "paths": P, "points_per_path": L}
kw = dict(path_ids=ids, path_variance=0.4, path_lengthscale=0.1)

with GP("matern32", 0.25, 1.5, 1e-2) as gp:
    for _ in range(2):
        gp.fit(t, Y)
        gp.fit(t, Y, **kw)
    plain, grouped = [], []
    for _ in range(5):
        gp.fit(t, Y)
        a = gp.timings_
        plain.append((a["kbuild"], a["fit_total"]))
        gp.fit(t, Y, **kw)
        a = gp.timings_
        grouped.append((a["kbuild"], a["fit_total"]))
    res["fit_plain_kbuild_ms"] = sorted(v[0] for v in plain)
    res["fit_grouped_kbuild_ms"] = sorted(v[0] for v in grouped)
    res["fit_plain_total_ms"] = sorted(v[1] for v in plain)
    res["fit_grouped_total_ms"] = sorted(v[1] for v in grouped)

    G, Lo, Lp = 2048, 20, 13
    tb = np.sort(rng.uniform(0, 1, (G, Lo + Lp)), axis=1)
    yb = np.stack([np.sin(6 * tb), np.cos(5 * tb)], axis=-1) + 0.2 * rng.standard_normal((G, Lo + Lp, 2))
    Xq, Yq = tb.reshape(-1, 1).copy(), yb.reshape(-1, 2).copy()
    Xo, Yo, Xp = tb[:, :Lo].reshape(-1, 1).copy(), yb[:, :Lo].reshape(-1, 2).copy(), tb[:, Lo:].reshape(-1, 1).copy()
    for _ in range(2):
        gp.score_blocks(Xq, Yq, Lo + Lp)
        gp.forecast_blocks(Xo, Yo, Xp, blocks=G)
    sc, fc = [], []
    for _ in range(5):
        t0 = time.perf_counter()
        gp.score_blocks(Xq, Yq, Lo + Lp)
        w = (time.perf_counter() - t0) * 1e3
        a = gp.timings_
        sc.append((w, a["predict_total"], a["var"], a["trsm"], a["kstar"], a["mean"]))
        t0 = time.perf_counter()
        gp.forecast_blocks(Xo, Yo, Xp, blocks=G)
        w = (time.perf_counter() - t0) * 1e3
        a = gp.timings_
        fc.append((w, a["predict_total"], a["var"], a["trsm"], a["kstar"], a["mean"]))
    names = ("wall_ms", "predict_total_ms", "var_ms", "trsm_ms", "kstar_ms", "mean_ms")
    med = lambda rows: {n: float(np.median([r[i] for r in rows])) for i, n in enumerate(names)}  # noqa: E731
    res["score_blocks_G2048_L33"] = med(sc)
    res["forecast_blocks_G2048_20_13"] = med(fc)
if "--out" in sys.argv:
    with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
        json.dump(res, f, indent=1)
print(json.dumps(res))
