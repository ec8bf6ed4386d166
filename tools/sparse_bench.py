"""Performance record of the inducing-point GP (SparseGP): writes profiles/sparse_bench.json.

    python tools/sparse_bench.py [--out profiles/sparse_bench.json] [--repeats 5] [--quick]

* the contraction alone at (n = 4096, rows = 16384) and at (n = 256, rows = 65536): the TN kernel as the fit launches it,
  a transpose of the chunk followed by the NT tile engine, and that NT launch alone (gpx_debug_syrk_tn_bench, device
  events, operands resident).  The routes are interleaved, `repeats` times; the record keeps the median and the spread.
* fit and predict (M = 4096) of 32768 paths x 33 steps (N = 1 081 344, d = 1, m = 128, two targets) and of N = 1 048 576,
  d = 3, m = 4096: wall time around the call (it ends in a device synchronise; NumPy inputs, so the chunks' host-to-device
  copies are inside) and the library's own phase clocks.
* the same 65 536 rows of path data through the dense GP and through SparseGP with m = 128: times and the largest
  difference of mean and variance.

Rates count rows * n^2 flops for a contraction (the lower triangle of 2 rows n^2)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gaussianprocesspathmodelling_amd import GP, SparseGP, _abi  # noqa: E402
from gaussianprocesspathmodelling_amd.sparse import choose_inducing  # noqa: E402


def spread(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4), "n": len(xs)}


def contraction(lib, n, rows, repeats):
    names = {0: "tn_kernel", 1: "transpose_then_nt", 2: "nt_engine_alone"}
    ms = {r: [] for r in names}
    out = C.c_double(0.0)
    for _ in range(repeats):
        for route in names:                                  # interleaved
            rc = lib.gpx_debug_syrk_tn_bench(n, rows, route, 5, C.byref(out))
            if rc != 0:
                raise RuntimeError(f"gpx_debug_syrk_tn_bench failed: {rc} {lib.gpx_last_error(None)}")
            ms[route].append(out.value)
    rec = {"n": n, "rows": rows, "flops_counted": float(rows) * n * n}
    for route, name in names.items():
        rec[name] = {"ms": spread(ms[route]), "tflops": round(rows * n * n / (statistics.median(ms[route]) * 1e-3) / 1e12, 2)}
    rec["tn_over_nt_engine_rate"] = round(rec["tn_kernel"]["tflops"] / rec["nt_engine_alone"]["tflops"], 3)
    rec["tn_over_transpose_then_nt_time"] = round(rec["tn_kernel"]["ms"]["median"] / rec["transpose_then_nt"]["ms"]["median"], 3)
    return rec


def path_data(n_paths, steps, seed):
    rng = np.random.default_rng(seed)
    t = np.linspace(0.0, 1.0, steps)
    X = np.tile(t, n_paths).reshape(-1, 1)
    base = np.stack([np.sin(2.0 * np.pi * t), np.cos(1.5 * np.pi * t) * t], axis=1)
    off = 0.3 * rng.standard_normal((n_paths, 1, 2))
    y = (base[None] + off * t[None, :, None] + 0.05 * rng.standard_normal((n_paths, steps, 2))).reshape(-1, 2)
    return X, np.ascontiguousarray(y)


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def sparse_case(name, X, y, m, kernel, ls, repeats, M=4096):
    rng = np.random.default_rng(5)
    Xs = np.ascontiguousarray(rng.uniform(0.0, 1.0, (M, X.shape[1])))
    fit_ms, pred_ms, phases = [], [], None
    m = choose_inducing(X, m)                                # (chosen once, outside the clock: a sort of the rows for d > 1)
    with SparseGP(kernel, ls, 1.0, 0.05 ** 2) as gp:
        gp.fit(X, y, inducing=m)                             # warm-up: allocations, code objects
        gp.predict(Xs)
        for _ in range(repeats):
            fit_ms.append(timed(lambda: gp.fit(X, y, inducing=m))[0])
            tm = gp.timings_
            phases = {k: round(tm[k], 3) for k in ("h2d", "kbuild", "chol", "solve", "logdet", "fit_total")}
            pred_ms.append(timed(lambda: gp.predict(Xs))[0])
        tm = gp.timings_
        phases.update({k: round(tm[k], 3) for k in ("kstar", "trsm", "mean", "var", "d2h", "predict_total")})
        rec = {"case": name, "N": len(X), "d": X.shape[1], "m": int(gp.inducing_.shape[0]), "k": 1 if y.ndim == 1 else y.shape[1],
               "M": M, "kernel": kernel, "chunk": gp.chunk_, "fit_wall_ms": spread(fit_ms), "predict_wall_ms": spread(pred_ms),
               "phase_ms_last_repeat": phases, "elbo_sum": float(gp.elbo().sum())}
    print(rec, flush=True)
    return rec


def equal_data(repeats, N=65536, m=128, M=4096):
    X, y = path_data(N // 33 + 1, 33, 11)
    X, y = np.ascontiguousarray(X[:N]), np.ascontiguousarray(y[:N])
    Xs = np.linspace(0.0, 1.0, M).reshape(-1, 1)
    kw = dict(kernel="matern52", lengthscale=0.3, variance=1.0, noise=0.05 ** 2)
    dense_fit, dense_pred, sp_fit, sp_pred = [], [], [], []
    with GP(**kw) as gp, SparseGP(**kw) as sp:
        gp.fit(X, y), sp.fit(X, y, inducing=m)               # warm-up
        gp.predict(Xs), sp.predict(Xs)
        for _ in range(repeats):                             # interleaved
            dense_fit.append(timed(lambda: gp.fit(X, y))[0])
            dt, (md, vd) = timed(lambda: gp.predict(Xs))
            dense_pred.append(dt)
            sp_fit.append(timed(lambda: sp.fit(X, y, inducing=m))[0])
            dt, (ms, vs) = timed(lambda: sp.predict(Xs))
            sp_pred.append(dt)
    rec = {"N": N, "d": 1, "m": m, "M": M, "dense_fit_wall_ms": spread(dense_fit), "dense_predict_wall_ms": spread(dense_pred),
           "sparse_fit_wall_ms": spread(sp_fit), "sparse_predict_wall_ms": spread(sp_pred),
           "largest_mean_difference": float(np.max(np.abs(ms - md))),
           "largest_variance_difference_relative": float(np.max(np.abs(vs - vd) / np.abs(vd))),
           "largest_variance_difference": float(np.max(np.abs(vs - vd)))}
    print(rec, flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sparse_bench.json"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="small shapes: a rehearsal of the script, not a record")
    args = ap.parse_args()
    lib = _abi.load()
    q = args.quick
    rec = {"what": "SparseGP on one MI355X: tools/sparse_bench.py (medians over interleaved repeats, with the spread)",
           "quick": q, "contraction": [], "fits": []}
    for n, rows in ((256, 1024),) if q else ((4096, 16384), (256, 65536)):
        rec["contraction"].append(contraction(lib, n, rows, args.repeats))
        print(rec["contraction"][-1], flush=True)
    Xp, yp = path_data(64 if q else 32768, 33, 7)
    rec["fits"].append(sparse_case("paths_32768x33", Xp, yp, 128, "matern52", 0.3, args.repeats, 256 if q else 4096))
    rng = np.random.default_rng(9)
    N3 = 4096 if q else 1048576
    X3 = rng.uniform(0.0, 1.0, (N3, 3))
    y3 = np.sin(2.0 * np.pi * X3[:, 0]) + 0.5 * np.cos(3.0 * X3[:, 1:].sum(axis=1)) + 0.1 * rng.standard_normal(N3)
    rec["fits"].append(sparse_case("d3_m4096", X3, y3, 256 if q else 4096, "matern52", 0.5, max(1, args.repeats // 2),
                                   256 if q else 4096))
    rec["equal_data"] = equal_data(max(1, args.repeats // 2), 2048 if q else 65536, 128, 256 if q else 4096)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
