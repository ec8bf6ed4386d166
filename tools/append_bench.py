"""Times gpx_append against the refit it replaces.

On one handle per configuration: fit N points, append m in {1, 128, 1024}, with and without gpx_reserve, at N = 8192
and N = 65536; beside it gpx_fit of the N + m points on the same card — what a model without append has to do.  Medians
of `--runs` runs (default 5) after one warm-up each; every append starts from a fresh fit of the N points (not timed).
Wall-clock around the C call and the library's own stream clock (timings_["fit_total"]).  Also samples the device memory
in use while an unreserved append moves the factor (old and new buffer side by side).

    python tools/append_bench.py [--out profiles/append_bench.json] [--sizes 8192,65536] [--runs 5]

``--model paths | velocities`` times gpx_append_rows instead (GP.update with path_ids= / derivatives=) at one shape, d = 3:
N = 16896 rows — 512 paths of 33 points with path ids, or 256 paths of 33 values and 33 velocities along the first input —
and m = 132 more (4 paths, or 2 paths with their velocities), reserved and unreserved, against the fresh fit of the
concatenated rows in the same order and against the plain model (no ids, every row a value) at the same shape; writes
profiles/append_rows_bench.json.  ``--model plain`` (the default) is the run described above.
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


ROWS_N, ROWS_M, ROWS_L, ROWS_NB = 16896, 132, 33, 1024
PHASES = ("h2d", "kbuild", "chol", "logdet")


def rows_data(model, seed=1):
    """(X, y, side) of N + m rows in the order the model holds them after the append: side = the path ids ('paths'), the
    kinds ('velocities': values of the fitted paths, their velocities, values of the new paths, their velocities)"""
    rng = np.random.default_rng(seed)
    T = ROWS_N + ROWS_M
    if model == "paths":
        P = T // ROWS_L
        t = np.sort(rng.uniform(0.0, 1.0, (P, ROWS_L)), axis=1)
        off = 0.3 * rng.standard_normal((P, 1))
        X = np.stack([t, np.sin(2.0 * t) + 0.02 * rng.standard_normal(t.shape), np.cos(3.0 * t) + 0.02 * rng.standard_normal(t.shape)],
                     axis=-1).reshape(T, 3)
        y = (np.sin(2.0 * np.pi * t) + off + 0.1 * rng.standard_normal(t.shape)).reshape(T)
        return X, y, np.repeat(np.arange(P), ROWS_L).astype(np.int32)
    X = rng.uniform(0.0, 1.0, (T, 3))
    f = np.sin(2.0 * np.pi * X[:, 0]) + 0.5 * np.cos(3.0 * X[:, 1:].sum(axis=1))
    if model == "plain":
        return X, f + 0.1 * rng.standard_normal(T), None
    half0, half1 = ROWS_N // 2, ROWS_M // 2
    kinds = np.concatenate([np.full(half0, -1), np.zeros(half0), np.full(half1, -1), np.zeros(half1)]).astype(np.int32)
    X[half0:ROWS_N] = X[:half0]                            # the velocities are observed where the values are
    X[ROWS_N + half1:] = X[ROWS_N:ROWS_N + half1]
    df = 2.0 * np.pi * np.cos(2.0 * np.pi * X[:, 0])
    return X, np.where(kinds < 0, f + 0.1 * rng.standard_normal(T), df + 0.2 * rng.standard_normal(T)), kinds


def rows_calls(model, X, y, side):
    """fit(gp, n) of the first n rows and append(gp) of the last m, through the public calls of the model"""
    N, T = ROWS_N, ROWS_N + ROWS_M
    if model == "paths":
        return (lambda gp, n: gp.fit(X[:n], y[:n], path_ids=side[:n], path_variance=0.4, path_lengthscale=0.1),
                lambda gp: gp.update(X[N:], y[N:], path_ids=side[N:]))
    if model == "velocities":
        nv = N + ROWS_M // 2
        return (lambda gp, n: gp._fit_rows(X[:n], y[:n], None, np.ascontiguousarray(side[:n]), 0.05),
                lambda gp: gp.update(X[N:nv], y[N:nv], derivatives=(X[nv:T], 0, y[nv:T])))
    return lambda gp, n: gp.fit(X[:n], y[:n]), lambda gp: gp.update(X[N:], y[N:])


def bench_rows(model, runs):
    X, y, side = rows_data(model)
    fit, append = rows_calls(model, X, y, side)
    N, m = ROWS_N, ROWS_M
    row = {"model": model, "N": N, "m": m, "nb": ROWS_NB, **flop_model(N, m, ROWS_NB)}
    with GP("matern52", 0.25, 1.5, 1e-2, block=ROWS_NB) as gp:
        wall, dev = [], []
        for r in range(runs + 1):
            w = timed(lambda: fit(gp, N + m))
            if r:
                wall.append(w)
                dev.append(gp.timings_["fit_total"])
        t = gp.timings_
        row["fit_wall_ms"], row["fit_dev_ms"] = statistics.median(wall), statistics.median(dev)
        row["fit_phases_ms"] = {k: t[k] for k in PHASES}
    for reserve in (0, N + 2048):
        with GP("matern52", 0.25, 1.5, 1e-2, block=ROWS_NB) as gp:
            gp.reserve(reserve)
            wall, dev = [], []
            for r in range(runs + 1):
                fit(gp, N)
                w = timed(lambda: append(gp))
                if r:
                    wall.append(w)
                    dev.append(gp.timings_["fit_total"])
            tag = "reserved" if reserve else "unreserved"
            row[f"append_{tag}_wall_ms"], row[f"append_{tag}_dev_ms"] = statistics.median(wall), statistics.median(dev)
            row[f"append_{tag}_wall_all_ms"] = wall
            t = gp.timings_
            row[f"append_{tag}_phases_ms"] = {k: t[k] for k in PHASES}
    row["speedup_reserved_wall"] = row["fit_wall_ms"] / row["append_reserved_wall_ms"]
    row["speedup_unreserved_wall"] = row["fit_wall_ms"] / row["append_unreserved_wall_ms"]
    print(json.dumps(row), flush=True)
    return row


def main_rows(model, out, runs):
    rows = [bench_rows(model, runs), bench_rows("plain", runs)]          # the plain model at the same shape beside it
    doc = {}
    if os.path.exists(out):                          # one file for both models: keep the other's rows and any further record
        with open(out) as f:
            doc = json.load(f)
    doc.update({"tool": "tools/append_bench.py", "runs": runs, "dtype": "float64", "kernel": "matern52", "d": 3,
                "results": [r for r in doc.get("results", []) if r.get("compared_with") != model]})
    for r in rows:
        r["compared_with"] = model
    doc["results"] += rows
    os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)
    print("wrote", out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", choices=("plain", "paths", "velocities"), default="plain")
    ap.add_argument("--out", default=None)
    ap.add_argument("--sizes", default="8192,65536")
    ap.add_argument("--ms", default="1,128,1024")
    ap.add_argument("--runs", type=int, default=5)
    a = ap.parse_args()
    if a.model != "plain":
        return main_rows(a.model, a.out or os.path.join("profiles", "append_rows_bench.json"), a.runs)
    a.out = a.out or os.path.join("profiles", "append_bench.json")
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
