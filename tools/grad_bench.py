#!/usr/bin/env python3
"""Cost of the analytic LML gradient (gpx_lml_grad) at the bench size: one fit, then the gradient
(L^-T by structured forward substitution + fused K^-1 trace pass), against central differences of
the GPU's own LML for two parameters.   python tools/grad_bench.py [--ntrain 65536]
With --devices n: the same gradient on a device group of n ranks (one GPU box: the ranks share the
card, so this checks the sharded gradient at scale against the single-GPU one, it is not a speed-up).
With --derivatives: a quarter of the ntrain rows are derivative observations (gpx_lml_grad_full, the KINDS instantiations
of the trace kernels), beside the value-only gradient at the same N in the same run, and the wall time of
GP.optimize(maxiter=3) on the same data with the analytic gradient and with central differences.
With --paths: the gradient of a fit with path ids (gpx_lml_grad_paths, the GROUPS instantiations of the trace kernels) at
N = 16896 = 512 paths x 33, Matern-3/2, for d = 1 and for d = 3 ARD: grad_total / grad_trace on the grouped fit beside
gpx_lml_grad on the plain fit of the same data on the same handle, alternating, one warm-up and five repeats each (medians
and every repeat are reported); the same with the rows shuffled (every tile then takes the path passes); and the wall time
of GP.optimize(maxiter=3) over all five (d = 1) or nine (d = 3) parameters with the analytic gradient and with
jac="3-point".  --ntrain sets N (rounded down to whole paths)."""
import argparse, json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench import synthetic
from gaussianprocesspathmodelling_amd import GP

ap = argparse.ArgumentParser()
ap.add_argument("--ntrain", type=int, default=65536)
ap.add_argument("--devices", type=int, default=0)
ap.add_argument("--derivatives", action="store_true")
ap.add_argument("--paths", action="store_true")
a = ap.parse_args()
N = a.ntrain
if a.paths:
    L, REPS = 33, 5
    P = (16896 if a.ntrain == 65536 else a.ntrain) // L          # (the default size of this mode is 512 paths)
    N = P * L
    keys = ("grad_total", "grad_trtri", "grad_trace")
    out = {"config": f"N={N} ({P} paths x {L}) Matern-3/2 fp64, sf2 1.5 sg2 0.4 sn2 1e-2, 1 warm-up + {REPS} repeats, medians"}

    def data(d, rng):
        # one cluster mean for all, a smooth deviation per path, noise: what fit_path_models sees (sorted ids)
        t = np.sort(rng.uniform(0.0, 1.0, (P, L)), axis=1)
        cols = [t] + [np.sin((c + 1.0) * t) + 0.02 * rng.standard_normal(t.shape) for c in range(1, d)]
        X = np.stack(cols, axis=-1).reshape(N, d)
        ph, am = rng.uniform(0.0, 6.28, (P, 1)), 0.6 * rng.standard_normal((P, 1))
        y = (np.sin(5.0 * t) + 0.5 * np.cos(11.0 * t) + am * np.sin(9.0 * t + ph) + 0.1 * rng.standard_normal(t.shape)).reshape(N)
        return np.ascontiguousarray(X), np.ascontiguousarray(y), np.repeat(np.arange(P), L).astype(np.int32)

    def med(rows):
        return {k + "_ms": float(np.median([r[k] for r in rows])) for k in keys} | {"repeats": rows}

    for d in (1, 3):
        rng = np.random.default_rng(12345 + d)
        X, y, ids = data(d, rng)
        ls = np.array([0.25]) if d == 1 else np.linspace(0.25, 0.4, d)
        lsp = np.array([0.1]) if d == 1 else np.linspace(0.1, 0.15, d)
        res = {}
        with GP("matern32", ls, 1.5, 1e-2) as gp:
            for order in ("sorted", "shuffled"):
                if order == "shuffled":
                    perm = rng.permutation(N)
                    X, y, ids = np.ascontiguousarray(X[perm]), np.ascontiguousarray(y[perm]), np.ascontiguousarray(ids[perm])
                kw = dict(path_ids=ids, path_variance=0.4, path_lengthscale=lsp)
                rows = {"plain": [], "paths": []}
                for rep in range(1 + REPS):                        # alternating; the first round is the warm-up
                    gp.fit(X, y); gp.lml_gradient()
                    if rep:
                        rows["plain"].append({k: gp.timings_[k] for k in keys})
                    gp.fit(X, y, **kw); lml, grad = gp.lml_gradient(path=True)
                    if rep:
                        rows["paths"].append({k: gp.timings_[k] for k in keys})
                r = {"plain_gpx_lml_grad": med(rows["plain"]), "gpx_lml_grad_paths": med(rows["paths"]), "lml": lml,
                     "grad": grad.tolist()}
                r["grad_total_ratio"] = r["gpx_lml_grad_paths"]["grad_total_ms"] / r["plain_gpx_lml_grad"]["grad_total_ms"]
                r["trace_ratio"] = r["gpx_lml_grad_paths"]["grad_trace_ms"] / r["plain_gpx_lml_grad"]["grad_trace_ms"]
                res[order] = r
            X, y, ids = data(d, np.random.default_rng(12345 + d))   # the sorted rows again
            params = ("lengthscale", "variance", "noise", "path_variance", "path_lengthscale")
            for jac in ("analytic", "3-point"):
                walls = []
                for rep in range(2):                               # (the first run imports the optimiser)
                    gp.lengthscale, gp.variance, gp.noise = ls.copy(), 1.5, 1e-2
                    t0 = time.perf_counter()
                    o = gp.optimize(X, y, params=params, maxiter=3, jac=jac, path_ids=ids, path_variance=0.4,
                                    path_lengthscale=lsp)
                    walls.append(time.perf_counter() - t0)
                res[f"optimize_maxiter3_{jac}"] = {"wall_s": walls[1], "first_wall_s": walls[0], "nfev": int(o.nfev),
                                                   "lml": -float(o.fun), "parameters": int(o.x.size)}
        out[f"d{d}"] = res
    print(json.dumps(out))
    sys.exit(0)
if a.derivatives:
    rng = np.random.default_rng(12345)
    Nd = N // 4
    Nv, d = N - Nd, 3
    w = rng.uniform(2.0, 5.0, d)
    f = lambda A: np.sin(A @ w) + 0.3 * np.cos(2.0 * A.sum(axis=1))  # noqa: E731
    df = lambda A, j: np.cos(A @ w) * w[j] - 0.6 * np.sin(2.0 * A.sum(axis=1))  # noqa: E731
    X, Xd, dims = rng.uniform(0, 1, (Nv, d)), rng.uniform(0, 1, (Nd, d)), rng.integers(0, d, Nd)
    y, yd = f(X) + 0.1 * rng.standard_normal(Nv), df(Xd, dims) + 0.2 * rng.standard_normal(Nd)
    der = (Xd, dims, yd)
    ls, sf2, sn2, snd = np.array([0.3, 0.25, 0.4]), 1.5, 1e-2, 5e-2
    keys = ("fit_total", "grad_total", "grad_trtri", "grad_trace")
    out = {"config": f"N={N} ({Nv} values + {Nd} derivative rows) d=3 Matern-5/2 ARD fp64"}
    with GP("matern52", ls, sf2, sn2) as gp:
        Xall = np.concatenate([X, Xd])
        yall = f(Xall) + 0.1 * rng.standard_normal(N)
        gp.fit(Xall, yall); gp.lml_gradient()                 # warm-up (allocations)
        gp.fit(Xall, yall)
        t0 = time.perf_counter(); gp.lml_gradient(); dt = time.perf_counter() - t0
        tm = gp.timings_
        out["values_only_same_N"] = dict({k + "_ms": tm[k] for k in keys}, grad_wall_ms=dt * 1e3)
        gp.fit(X, y, derivatives=der, derivative_noise=snd); gp.lml_gradient(derivative_noise=True)
        gp.fit(X, y, derivatives=der, derivative_noise=snd)
        t0 = time.perf_counter(); lml, grad = gp.lml_gradient(derivative_noise=True); dt = time.perf_counter() - t0
        tm = gp.timings_
        out["with_derivatives"] = dict({k + "_ms": tm[k] for k in keys}, grad_wall_ms=dt * 1e3, lml=lml, grad=grad.tolist())
        out["grad_total_ratio"] = out["with_derivatives"]["grad_total_ms"] / out["values_only_same_N"]["grad_total_ms"]
        out["trace_ratio"] = out["with_derivatives"]["grad_trace_ms"] / out["values_only_same_N"]["grad_trace_ms"]
        for jac in ("analytic", "3-point"):
            walls = []
            for rep in range(2):                               # (the first run imports the optimiser)
                gp.lengthscale, gp.variance, gp.noise = ls.copy(), sf2, sn2
                t0 = time.perf_counter()
                res = gp.optimize(X, y, maxiter=3, jac=jac, derivatives=der, derivative_noise=snd)
                walls.append(time.perf_counter() - t0)
            out[f"optimize_maxiter3_{jac}"] = {"wall_s": walls[1], "first_wall_s": walls[0], "nfev": int(res.nfev),
                                               "lml": -float(res.fun)}
    print(json.dumps(out))
    sys.exit(0)
X, y, _ = synthetic(N, 3, 16, 12345)
ls, sf2, sn2 = np.array([0.3, 0.2, 0.25]), 1.5, 1e-2
if a.devices > 1:
    with GP("rbf", ls, sf2, sn2, jitter=0.0) as g1:
        lml1, grad1 = g1.fit(X, y).lml_gradient()
        t1 = g1.timings_
    with GP("rbf", ls, sf2, sn2, jitter=0.0, devices=a.devices, oversubscribe=True) as gp:
        gp.fit(X, y); gp.lml_gradient()
        t0 = time.perf_counter(); lml, grad = gp.lml_gradient(); dt = time.perf_counter() - t0
        tm = gp.timings_
    print(json.dumps({"config": f"N={N} d=3 RBF ARD fp64, {a.devices} ranks sharing one GPU (in-process transport)",
                      "single_gpu": {"grad_ms": t1["grad_total"], "trtri_ms": t1["grad_trtri"], "trace_ms": t1["grad_trace"]},
                      "group_rank0": {"grad_ms": tm["grad_total"], "grad_wall_ms": dt * 1e3,
                                      "trtri_plus_allgather_ms": tm["grad_trtri"], "trace_ms": tm["grad_trace"]},
                      "lml_rel_diff": abs(lml - lml1) / abs(lml1),
                      "grad_rel_diff": float(np.max(np.abs(grad - grad1)) / np.max(np.abs(grad1))),
                      "grad": grad.tolist(), "grad_single": grad1.tolist()}))
    sys.exit(0)
with GP("rbf", ls, sf2, sn2, jitter=0.0) as gp:
    gp.fit(X, y); gp.lml_gradient()                       # warm-up (allocations)
    gp.fit(X, y)
    t0 = time.perf_counter(); lml, grad = gp.lml_gradient(); dt = time.perf_counter() - t0
    tm = gp.timings_
    fd = {}
    h = 1e-4
    v0 = np.log(np.concatenate([ls, [sf2, sn2]]))
    for i in (0, 4):
        f = []
        for sgn in (+1, -1):
            v = v0.copy(); v[i] += sgn * h
            gp.lengthscale, gp.variance, gp.noise = np.exp(v[:3]), float(np.exp(v[3])), float(np.exp(v[4]))
            f.append(gp.fit(X, y).log_marginal_likelihood(y))
        fd[i] = (f[0] - f[1]) / (2 * h)
print(json.dumps({"config": f"N={N} d=3 RBF ARD fp64", "fit_ms": tm["fit_total"], "grad_ms": tm["grad_total"],
                  "grad_wall_ms": dt * 1e3, "trtri_ms": tm["grad_trtri"], "trace_ms": tm["grad_trace"],
                  "trtri_tflops": N ** 3 / 3 / (tm["grad_trtri"] * 1e-3) / 1e12,
                  "trace_tflops": N ** 3 / 3 / (tm["grad_trace"] * 1e-3) / 1e12,
                  "grad_over_fit": tm["grad_total"] / tm["fit_total"], "lml": lml, "grad": grad.tolist(),
                  "central_difference": {str(k): v for k, v in fd.items()},
                  "fd_rel_err": {str(k): abs(v - grad[k]) / np.abs(grad).max() for k, v in fd.items()}}))
