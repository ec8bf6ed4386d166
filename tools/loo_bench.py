"""Times gpx_loo beside the gradient whose L^-T stage it shares.

One fp64 handle per size (N = 8192 and N = 65536, rbf, d = 3, k = 1): fit, then gpx_loo and gpx_lml_grad in turn — one
warm-up of each, then `--runs` rounds (default 5), a device synchronise before and after every call, wall-clock around the
call.  Reported per size: the medians, every single run and min / max of the LOO wall time, of the gradient's wall time
and of its own `grad_trtri` / `grad_trace` stream clocks, the fit's `fit_total`, and what LOO costs beyond the L^-T build
(LOO wall minus `grad_trtri`, as a share of `grad_trtri`).

`--kernel-ms ROWS,FINISH` measures nothing: it takes the kernel times of loo_rows_kernel and loo_finish_kernel at the LAST
size, in ms per call, from a separate `rocprofv3 --kernel-trace --stats -- python tools/loo_bench.py --sizes N --runs 1
--loo-only --out /dev/null` run, and adds them to the file of the timed run (`--out`) with the row pass's bytes,
8 N (N + 1) / 2, over its kernel time and that as a share of the 8.0 TB/s HBM peak.

    python tools/loo_bench.py [--out profiles/loo_bench.json] [--sizes 8192,65536] [--runs 5]
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

HBM_PEAK = 8.0e12   # bytes / s


def data(n, seed=1):
    rng = np.random.default_rng(seed)
    X = rng.uniform(0.0, 1.0, (n, 3))
    y = np.sin(2.0 * np.pi * X[:, 0]) + 0.5 * np.cos(3.0 * X[:, 1:].sum(axis=1)) + 0.1 * rng.standard_normal(n)
    return X, y


def summary(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "all": list(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "loo_bench.json"))
    ap.add_argument("--sizes", default="8192,65536")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--loo-only", action="store_true", help="no gradient calls (the run under the kernel trace)")
    ap.add_argument("--kernel-ms", default=None, help="ROWS,FINISH kernel times of the last size, from the kernel trace")
    a = ap.parse_args()
    if a.kernel_ms:  # no measurement: the kernel times of the trace go into the file of the timed run
        with open(a.out) as f:
            out = json.load(f)
        rows_ms, finish_ms = (float(v) for v in a.kernel_ms.split(","))
        r = out["results"][-1]
        rate = r["row_pass_bytes"] / (rows_ms * 1e-3)
        r.update(loo_rows_kernel_ms=rows_ms, loo_finish_kernel_ms=finish_ms, row_pass_bytes_per_s=rate,
                 row_pass_share_of_hbm_peak=rate / HBM_PEAK)
        print(f"N={r['N']}: loo_rows_kernel {rows_ms:.3f} ms = {rate / 1e12:.2f} TB/s ({100 * rate / HBM_PEAK:.0f} % of the HBM peak)")
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
        return
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("loo_bench needs a GPU: nothing is measured without one")

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    results = []
    for N in (int(s) for s in a.sizes.split(",")):
        X, y = data(N)
        with GP("rbf", 0.25, 1.5, 1e-2, jitter=0.0) as gp:
            gp.fit(X, y)
            fit_ms = gp.timings_["fit_total"]
            loo, grad, trtri, trace = [], [], [], []
            for run in range(a.runs + 1):
                w = timed(lambda: gp.loo(return_logp=True))
                if not a.loo_only:
                    g = timed(gp.lml_gradient)
                    tm = gp.timings_
                if run:  # run 0 warms up
                    loo.append(w)
                    if not a.loo_only:
                        grad.append(g), trtri.append(tm["grad_trtri"]), trace.append(tm["grad_trace"])
            r = {"N": N, "fit_total_ms": fit_ms, "loo_wall_ms": summary(loo), "row_pass_bytes": 8.0 * N * (N + 1) / 2,
                 "loo_log_likelihood": float(gp.loo_log_likelihood())}
            if not a.loo_only:
                r.update(grad_wall_ms=summary(grad), grad_trtri_ms=summary(trtri), grad_trace_ms=summary(trace))
                extra = r["loo_wall_ms"]["median"] - r["grad_trtri_ms"]["median"]
                r.update(loo_minus_trtri_ms=extra, loo_minus_trtri_share=extra / r["grad_trtri_ms"]["median"])
            results.append(r)
            print(f"N={N}: fit {fit_ms:.2f} ms, loo {r['loo_wall_ms']['median']:.2f} ms wall "
                  f"[{r['loo_wall_ms']['min']:.2f}, {r['loo_wall_ms']['max']:.2f}]"
                  + ("" if a.loo_only else f", gradient {r['grad_wall_ms']['median']:.2f} ms wall, grad_trtri "
                     f"{r['grad_trtri_ms']['median']:.2f} ms, loo - grad_trtri {r['loo_minus_trtri_ms']:.2f} ms "
                     f"({100 * r['loo_minus_trtri_share']:.1f} %)"), flush=True)
    out = {"tool": "tools/loo_bench.py", "runs": a.runs, "dtype": "float64", "kernel": "rbf", "d": 3, "k": 1, "results": results}
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
