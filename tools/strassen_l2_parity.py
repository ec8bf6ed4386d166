#!/usr/bin/env python3
"""Errors of one and of two Strassen levels on the inputs of tests/test_strassen_levels_gpu.py (the inputs, the switches
and the error definitions are that file's own): gpx_gemm_nt against NumPy, the fits against OracleGP.  Writes
profiles/strassen_l2_parity.json, from which that file's BARS and GEMM_BAR are taken.
    python tools/strassen_l2_parity.py [--out profiles/strassen_l2_parity.json]"""
import argparse
import importlib.util
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
spec = importlib.util.spec_from_file_location("strassen_levels_tests", os.path.join(ROOT, "tests", "test_strassen_levels_gpu.py"))
t = importlib.util.module_from_spec(spec)
spec.loader.exec_module(t)
from gaussianprocesspathmodelling_amd import _abi  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "strassen_l2_parity.json"))
args = ap.parse_args()
lib = _abi.load()
names = ("mean", "var", "alpha", "logdet")
LEVELS = (("classical", {"GPX_STRASSEN_MIN": "0"}), ("one", {"GPX_STRASSEN_MIN": "128", "GPX_STRASSEN_MIN_TWO": "0"}),
          ("two", {"GPX_STRASSEN_MIN": "128", "GPX_STRASSEN_MIN_TWO": "128"}))
gemm = []
for m, n, k in t.GEMM_SHAPES:
    row = {"m": m, "n": n, "k": k}
    for level, env in LEVELS:
        row[level] = t.gemm_run(lib, m, n, k, env)[1]
    gemm.append(row)
    print(row, file=sys.stderr, flush=True)
fits = []
for case in t.CASES:
    for level, env in (("one", t.ONE0), ("two", t.TWO)):
        e = t.fit_run(case, env)["errors"]
        fits.append({"case": case, "levels": level, **dict(zip(names, e))})
        print(fits[-1], file=sys.stderr, flush=True)
worst = {lv: {q: max(r[q] for r in fits if r["levels"] == lv) for q in names} for lv in ("one", "two")}
res = {"what": "tools/strassen_l2_parity.py: gpx_gemm_nt's largest difference from NumPy over max|A| max|B| k eps, and the "
               "errors against OracleGP (fp64) of the fits of tests/test_strassen_levels_gpu.py, with one and two Strassen levels",
       "bars_at_full_size": {"mean": 1e-6, "var": 1e-6, "alpha": 1e-8, "logdet": 1e-12},
       "gemm_nt": gemm, "largest_gemm_nt": {lv: max(r[lv] for r in gemm) for lv, _ in LEVELS},
       "largest_fit": worst, "fits": fits}
json.dump(res, open(args.out, "w"), indent=1)
print(json.dumps({"gemm_nt": res["largest_gemm_nt"], "fit": worst}))
