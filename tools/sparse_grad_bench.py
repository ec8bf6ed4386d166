"""Cost of the gradient of the inducing-point bound beside a fit: writes profiles/sparse_grad_bench.json.

    python tools/sparse_grad_bench.py [--out profiles/sparse_grad_bench.json] [--repeats 5] [--quick]

* fit against fit + elbo_gradient at the two shapes of profiles/sparse_bench.json — 32768 paths x 33 steps (N = 1 081 344,
  d = 1, m = 128, two targets) and N = 1 048 576, d = 3, m = 4096: wall time around the calls (each ends in a device
  synchronise; NumPy inputs, so the chunks' host-to-device copies are inside), interleaved, `repeats` times; the record
  keeps the medians with the spread, their ratio, and the library's own clocks of the gradient call.
* the contraction kernel alone (gpx_debug_cross_dtheta_bench, device events, operands resident) at one chunk of each
  shape, as GB/s of the weight matrix W it reads (rows x cols doubles)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from gaussianprocesspathmodelling_amd import SparseGP, _abi  # noqa: E402
from gaussianprocesspathmodelling_amd.sparse import choose_inducing  # noqa: E402
from sparse_bench import path_data, spread, timed  # noqa: E402


def kernel_alone(lib, kernel, rows, cols, d, n_ls, repeats):
    out = C.c_double(0.0)
    ms = []
    for _ in range(repeats):
        rc = lib.gpx_debug_cross_dtheta_bench(_abi.KERNEL_IDS[kernel], rows, cols, d, n_ls, 5, C.byref(out))
        if rc != 0:
            raise RuntimeError(f"gpx_debug_cross_dtheta_bench failed: {rc} {lib.gpx_last_error(None)}")
        ms.append(out.value)
    rec = {"kernel": kernel, "rows": rows, "cols": cols, "d": d, "n_ls": n_ls, "ms": spread(ms),
           "gb_per_s_of_w": round(8.0 * rows * cols / (statistics.median(ms) * 1e-3) / 1e9, 1)}
    print(rec, flush=True)
    return rec


def grad_case(name, X, y, m, kernel, ls, repeats):
    Z = choose_inducing(X, m)
    fit_ms, both_ms = [], []
    with SparseGP(kernel, ls, 1.0, 0.05 ** 2) as gp:
        gp.fit(X, y, inducing=Z).elbo_gradient()             # warm-up: allocations, code objects
        for _ in range(repeats):                             # interleaved
            fit_ms.append(timed(lambda: gp.fit(X, y, inducing=Z))[0])
            both_ms.append(timed(lambda: gp.fit(X, y, inducing=Z).elbo_gradient())[0])
        tm = gp.timings_
        F, g = gp.elbo_gradient()
        rec = {"case": name, "N": len(X), "d": X.shape[1], "m": int(Z.shape[0]), "k": 1 if y.ndim == 1 else y.shape[1],
               "kernel": kernel, "chunk": gp.chunk_, "fit_wall_ms": spread(fit_ms), "fit_and_gradient_wall_ms": spread(both_ms),
               "fit_and_gradient_over_fit": round(statistics.median(both_ms) / statistics.median(fit_ms), 3),
               "gradient_phase_ms_last_repeat": {k: round(tm[k], 3) for k in ("grad_trtri", "grad_trace", "grad_total")},
               "elbo_sum": F, "gradient": [float(v) for v in g]}
    print(rec, flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sparse_grad_bench.json"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="small shapes: a rehearsal of the script, not a record")
    args = ap.parse_args()
    lib = _abi.load()
    q = args.quick
    rec = {"what": "the gradient of SparseGP's bound beside a fit on one MI355X: tools/sparse_grad_bench.py (medians over "
                   "interleaved repeats, with the spread)", "quick": q, "kernel_alone": [], "fits": []}
    for rows, cols, d in ((1024, 128, 1), (1024, 256, 3)) if q else ((65536, 128, 1), (8064, 4096, 3)):
        rec["kernel_alone"].append(kernel_alone(lib, "matern52", rows, cols, d, 1, args.repeats))
    Xp, yp = path_data(64 if q else 32768, 33, 7)
    rec["fits"].append(grad_case("paths_32768x33", Xp, yp, 128, "matern52", 0.3, args.repeats))
    rng = np.random.default_rng(9)
    N3 = 4096 if q else 1048576
    X3 = rng.uniform(0.0, 1.0, (N3, 3))
    y3 = np.sin(2.0 * np.pi * X3[:, 0]) + 0.5 * np.cos(3.0 * X3[:, 1:].sum(axis=1)) + 0.1 * rng.standard_normal(N3)
    rec["fits"].append(grad_case("d3_m4096", X3, y3, 256 if q else 4096, "matern52", 0.5, max(1, args.repeats // 2)))
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
