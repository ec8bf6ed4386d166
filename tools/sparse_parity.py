"""Writes profiles/sparse_parity.json: the largest elementwise error of SparseGP against tests/sparse_ref.py for every
parity case of tests/test_sparse_gpu.py, on the GPU this runs on.  The test's tight bar is one decade above the largest of
the mean / variance / bound figures recorded here.

    python tools/sparse_parity.py [--out profiles/sparse_parity.json]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sparse_parity.json"))
    args = ap.parse_args()
    import sparse_ref
    import test_sparse_gpu as t
    fits = []
    for case in sparse_ref.CASES:
        fig = t.parity_figures(case)
        fits.append({"case": case["id"], **{k: case[k] for k in ("N", "m", "d", "k", "chunk", "jitter")},
                     **{k: float(f"{v:.3g}") for k, v in fig.items()}})
        print(fits[-1], flush=True)
    rec = {"what": "largest elementwise error of SparseGP against tests/sparse_ref.py for every parity case of "
                   "tests/test_sparse_gpu.py on one MI355X: mean with floor 1e-6, var relative, elbo with floor 1, cov over "
                   "the signal variance; the test's tight bar is one decade above `largest` (mean, var, elbo)",
           "fits": fits, "largest": max(max(f["mean"], f["var"], f["elbo"]) for f in fits)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print("largest", rec["largest"])


if __name__ == "__main__":
    main()
