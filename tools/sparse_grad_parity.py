"""Writes profiles/sparse_grad_parity.json: the error of SparseGP.elbo_gradient against tests/sparse_grad_ref.py for every
parity case of tests/test_sparse_grad_gpu.py, on the GPU this runs on — the metric max_i |g_i - f_i| / (|f_i| + 1e-3 max_j
|f_j|) — with the identity against the dense GP's LML gradient and the largest error of the contraction kernel alone
against its bound.  The test's tight bar is one decade above the largest gradient figure recorded here.

    python tools/sparse_grad_parity.py [--out profiles/sparse_grad_parity.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sparse_grad_parity.json"))
    args = ap.parse_args()
    import sparse_ref
    import test_sparse_grad_gpu as t
    from gaussianprocesspathmodelling_amd import _abi
    fits = []
    for case in sparse_ref.CASES:
        fig = t.parity_figures(case)
        fits.append({"case": case["id"], **{k: case[k] for k in ("N", "m", "d", "k", "chunk", "jitter")},
                     **{k: float(f"{v:.3g}") for k, v in fig.items()}})
        print(fits[-1], flush=True)
    dense = {}
    for kernel in ("matern32", "matern12"):
        g, f = t.dense_identity_figure(kernel)
        dense[kernel] = {"grad": float(f"{g:.3g}"), "elbo_vs_lml": float(f"{f:.3g}")}
    print(dense, flush=True)
    rec = {"what": "SparseGP.elbo_gradient against tests/sparse_grad_ref.py for every parity case of "
                   "tests/test_sparse_grad_gpu.py on one MI355X: grad = max_i |g_i - f_i| / (|f_i| + 1e-3 max_j |f_j|), elbo with "
                   "floor 1; the test's tight bar is one decade above `largest` (grad).  dense_identity: the same metric against "
                   "GP.lml_gradient with Z = the shared grid and jitter = 0.  kernel_largest: gpx_cross_dtheta_contract, the "
                   "largest |out - ref| / sum |W| |dK| over the unit test's shapes",
           "fits": fits, "largest": max(f["grad"] for f in fits), "dense_identity": dense,
           "kernel_largest": float(f"{t.largest_kernel_ratio(_abi.load()):.3g}")}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print("largest", rec["largest"], "kernel_largest", rec["kernel_largest"])


if __name__ == "__main__":
    main()
