"""Times gpx_append against the refit it replaces.

On one handle per configuration: fit N points, append m in {1, 128, 1024}, with and without gpx_reserve, at N = 8192
and N = 65536; beside it gpx_fit of the N + m points on the same card — what a model without append has to do.  Medians
of `--runs` runs (default 5) after one warm-up each; every append starts from a fresh fit of the N points (not timed).
Wall-clock around the C call and the library's own stream clock (timings_["fit_total"]).  Also samples the device memory
in use while an unreserved append moves the factor (old and new buffer side by side).

    python tools/append_bench.py [--out profiles/append_bench.json] [--sizes 8192,65536] [--runs 5]
"""
import argparse
import json
import os
import statistics
import sys
import threading
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gaussianprocesspathmodelling_amd import GP  # noqa: E402


def data(n, seed=1):
    rng = np.random.default_rng(seed)
    X = rng.uniform(0.0, 1.0, (n, 3))
    y = np.sin(2.0 * np.pi * X[:, 0]) + 0.5 * np.cos(3.0 * X[:, 1:].sum(axis=1)) + 0.1 * rng.standard_normal(n)
    return X, y


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def flop_model(N, m, nb):
    R0, R1, npad = N // nb * nb, N // 128 * 128, -(-(N + m) // 128) * 128
    mp, n1 = npad - R1, npad - R0
    return {"R0": R0, "rows_solved": mp, "trailing": n1, "append_flops": mp * R0 ** 2 + n1 ** 2 * R0 + n1 ** 3 / 3,
            "fit_flops": (N + m) ** 3 / 3}


def peak_memory_of_unreserved_append(gp, X, y, N, m):
    import torch
    used = lambda: (lambda f, t: t - f)(*torch.cuda.mem_get_info())  # noqa: E731
    gp.fit(X[:N], y[:N])
    gp.release_scratch()
    before, peak, stop = used(), [0], threading.Event()

    def poll():
        while not stop.is_set():
            peak[0] = max(peak[0], used())

    th = threading.Thread(target=poll)
    th.start()
    try:
        gp.update(X[N:N + m], y[N:N + m])
    finally:
        stop.set()
        th.join()
    return {"N": N, "m": m, "used_before_bytes": before, "peak_bytes": max(peak[0], before), "used_after_bytes": used()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "append_bench.json"))
    ap.add_argument("--sizes", default="8192,65536")
    ap.add_argument("--ms", default="1,128,1024")
    ap.add_argument("--runs", type=int, default=5)
    a = ap.parse_args()
    sizes, ms = [int(v) for v in a.sizes.split(",")], [int(v) for v in a.ms.split(",")]
    rows, mem = [], []
    for N in sizes:
        X, y = data(N + max(ms))
        nb = 2048 if -(-N // 128) * 128 >= 40960 else 1024
        for m in ms:
            row = {"N": N, "m": m, "nb": nb, **flop_model(N, m, nb)}
            with GP("rbf", 0.25, 1.5, 1e-2, jitter=0.0) as gp:
                wall, dev = [], []
                for r in range(a.runs + 1):
                    w = timed(lambda: gp.fit(X[:N + m], y[:N + m]))
                    if r:
                        wall.append(w)
                        dev.append(gp.timings_["fit_total"])
                row["fit_wall_ms"], row["fit_dev_ms"] = statistics.median(wall), statistics.median(dev)
            for reserve in (0, N + 2048):
                with GP("rbf", 0.25, 1.5, 1e-2, jitter=0.0) as gp:
                    gp.reserve(reserve)
                    wall, dev = [], []
                    for r in range(a.runs + 1):
                        gp.fit(X[:N], y[:N])
                        w = timed(lambda: gp.update(X[N:N + m], y[N:N + m]))
                        if r:
                            wall.append(w)
                            dev.append(gp.timings_["fit_total"])
                    tag = "reserved" if reserve else "unreserved"
                    row[f"append_{tag}_wall_ms"], row[f"append_{tag}_dev_ms"] = statistics.median(wall), statistics.median(dev)
                    row[f"append_{tag}_wall_all_ms"] = wall
                    t = gp.timings_
                    row[f"append_{tag}_phases_ms"] = {k: t[k] for k in ("h2d", "kbuild", "chol", "logdet")}
            row["speedup_reserved_wall"] = row["fit_wall_ms"] / row["append_reserved_wall_ms"]
            row["speedup_unreserved_wall"] = row["fit_wall_ms"] / row["append_unreserved_wall_ms"]
            print(json.dumps(row), flush=True)
            rows.append(row)
        with GP("rbf", 0.25, 1.5, 1e-2, jitter=0.0) as gp:
            mem.append(peak_memory_of_unreserved_append(gp, X, y, N, 128))
            print(json.dumps(mem[-1]), flush=True)
    out = {"tool": "tools/append_bench.py", "runs": a.runs, "dtype": "float64", "kernel": "rbf", "d": 3, "results": rows,
           "unreserved_reallocation_memory": mem}
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
