#!/usr/bin/env python3
"""The tile engine alone through no, one and two Strassen levels (gpx_debug_gemm_bench, fp64, zero-filled operands
resident in HBM): modes 0 / 2 / 3 alternating at the shapes of the two-level fit's two deep products (16384 x 16384 x
32768, 16384^3), modes 0 / 2 at the shapes of their first-level products.  Writes profiles/strassen_l2_engine_alone.json.
    python tools/strassen_l2_engine_alone.py [--repeats 3] [--out profiles/strassen_l2_engine_alone.json]"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gaussianprocesspathmodelling_amd import _abi  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--iters", type=int, default=3)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "strassen_l2_engine_alone.json"))
args = ap.parse_args()
lib = _abi.load()
f64 = _abi.DTYPE_IDS["float64"]
rows = []
for n, k, modes in ((16384, 32768, (0, 2, 3)), (16384, 16384, (0, 2, 3)), (8192, 16384, (0, 2)), (8192, 8192, (0, 2))):
    for rep in range(args.repeats):
        for mode in modes:
            ms = C.c_double(0)
            rc = lib.gpx_debug_gemm_bench(f64, n, k, 0, mode, args.iters, C.byref(ms))
            assert rc == 0, rc
            rows.append({"dtype": "f64", "n": n, "k": k, "lower": 0, "mode": mode, "repeat": rep, "rc": rc, "ms": ms.value,
                         "tflops_classical_count": 2.0 * n * n * k / (ms.value * 1e-3) / 1e12})
            print(rows[-1], file=sys.stderr, flush=True)
res = {"what": "gpx_debug_gemm_bench, fp64, zero-filled operands: mode 0 classical C -= A B^T, mode 2 through strassen_nt "
               "with one level, mode 3 with two",
       "rows": rows}
json.dump(res, open(args.out, "w"), indent=1)
