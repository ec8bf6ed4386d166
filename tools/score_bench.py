"""Whole-path scoring timings (``GP.score_blocks``) -> profiles/score_bench.json.

Two comparisons, inputs resident in HBM (device tensors), medians of ``--iters`` (>= 5) calls after one warm-up call each:

* against the only route there was before: ``predict(return_cov=True)`` over all P * 33 query points, then the P diagonal
  33 x 33 blocks of the joint covariance to the host and their Cholesky factorisations and solves there (``route_cov``);
  N = 8250 (250 paths of 33 points), P = 1024 paths, fp64.  Both are host wall times of blocking calls (the old route has
  a host part), and ``logp`` of the two routes is compared.
* against ``predict`` with variances at the same N and M: the two calls share the K* build, the solve and the mean
  product, so the comparison is their ``timings_["var"]`` (hipEvent clocks): the Gram pass plus the block factorisations
  against ``var_rows_kernel``, over the same M * Npad elements of V^T.  ``gram_pass_gbs`` = those bytes over the scoring
  call's whole ``var`` phase (a lower bound on the Gram kernel's own rate), beside ``copy_gbs`` of ``gpx_microbench``.
  Shapes: the one above and N = 65536, P = 124 (long rows of V^T).

    python tools/score_bench.py [--iters 5] [--skip-large]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
L = 33


def median_wall(fn, iters):
    fn()
    ts = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def median_phase(fn, gp, phase, iters):
    fn()
    vals = []
    for _ in range(iters):
        fn()
        vals.append(gp.timings_[phase])
    return float(np.median(vals))


def problem(N, P, seed):
    rng = np.random.default_rng(seed)
    X = rng.uniform(0.0, 1.0, (N, 1))
    f = lambda a: np.stack([np.sin(6 * a[:, 0]), np.cos(4 * a[:, 0])], axis=1)  # noqa: E731
    Y = f(X) + 0.2 * rng.standard_normal((N, 2))
    Xq = np.tile(np.linspace(0.0, 1.0, L), P)[:, None] + 0.002 * rng.standard_normal((P * L, 1))
    Yq = f(Xq) + 0.2 * rng.standard_normal((P * L, 2))
    return X, Y, Xq, Yq


def route_cov(gp, Xq, Yq, P):
    """the parent's only route to a path's joint density: the full joint covariance, its diagonal blocks on the host"""
    import torch
    mean, cov = gp.predict(Xq, return_cov=True, include_noise=True)
    idx = torch.arange(P * L, device=cov.device).reshape(P, L)
    blocks = cov[idx[:, :, None], idx[:, None, :]].cpu().numpy()          # (P, L, L)
    r = (Yq - mean).reshape(P, L, -1).cpu().numpy()
    Ls = np.linalg.cholesky(blocks)
    w = np.linalg.solve(Ls, r)
    logdet = 2.0 * np.log(np.diagonal(Ls, axis1=1, axis2=2)).sum(axis=1)
    return -0.5 * (w * w).sum(axis=1) - 0.5 * logdet[:, None] - 0.5 * L * np.log(2 * np.pi)


def var_comparison(gp, Xq, Yq, P, Npad, iters, copy_gbs):
    v_pred = median_phase(lambda: gp.predict(Xq), gp, "var", iters)
    v_score = median_phase(lambda: gp.score_blocks(Xq, Yq, L), gp, "var", iters)
    byts = float(P * L) * Npad * 8
    return {"predict_var_ms": round(v_pred, 4), "score_var_ms": round(v_score, 4), "ratio": round(v_score / v_pred, 3),
            "vt_bytes": byts, "var_rows_gbs": round(byts / (v_pred * 1e-3) / 1e9, 1),
            "gram_pass_gbs": round(byts / (v_score * 1e-3) / 1e9, 1), "copy_gbs": round(copy_gbs, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--skip-large", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "score_bench.json"))
    a = ap.parse_args()
    iters = max(5, a.iters)
    import torch
    from gaussianprocesspathmodelling_amd import GP, _abi
    lib = _abi.load()
    tf, gbs = C.c_double(0), C.c_double(0)
    if lib.gpx_microbench(C.byref(tf), C.byref(gbs)) != 0:
        raise RuntimeError("gpx_microbench failed")
    dev = torch.device("cuda", 0)
    res = {"iters": iters, "copy_gbs": round(gbs.value, 1), "mfma_f64_tflops": round(tf.value, 2)}

    N, P = 250 * L, 1024
    X, Y, Xq, Yq = problem(N, P, 1)
    Xd, Yd = torch.as_tensor(Xq, device=dev), torch.as_tensor(Yq, device=dev)
    with GP("matern32", 0.3, 1.0, 0.05) as gp:
        gp.fit(X, Y)
        new = gp.score_blocks(Xd, Yd, L)
        old = route_cov(gp, Xd, Yd, P)
        diff = float(np.max(np.abs(new.cpu().numpy() - old)))
        t_new = median_wall(lambda: (gp.score_blocks(Xd, Yd, L), torch.cuda.synchronize()), iters)
        new_phases = {k: round(gp.timings_[k], 4) for k in ("kstar", "trsm", "mean", "var", "d2h", "predict_total")}
        gp.release_scratch()
        t_old = median_wall(lambda: route_cov(gp, Xd, Yd, P), iters)
        gp.release_scratch()
        res["against_joint_covariance"] = {
            "N": N, "paths": P, "M": P * L, "score_blocks_ms": round(t_new, 3), "predict_cov_route_ms": round(t_old, 3),
            "ratio": round(t_old / t_new, 2), "max_abs_logp_difference": diff, "score_phases_ms": new_phases}
        res["against_predict_var"] = [dict(N=N, paths=P, **var_comparison(gp, Xd, Yd, P, (N + 127) // 128 * 128, iters, gbs.value))]
    print(json.dumps(res), flush=True)

    if not a.skip_large:
        N, P = 65536, 124
        X, Y, Xq, Yq = problem(N, P, 2)
        Xd, Yd = torch.as_tensor(Xq, device=dev), torch.as_tensor(Yq, device=dev)
        with GP("matern32", 0.3, 1.0, 0.05) as gp:
            gp.fit(X, Y)
            res["against_predict_var"].append(dict(N=N, paths=P, **var_comparison(gp, Xd, Yd, P, N, iters, gbs.value)))
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
