#!/usr/bin/env python3
"""Errors against OracleGP of the fits of tests/test_deferred_left_gpu.py, with GPX_DEFER_LEFT 0 and 1 (the inputs, the
switches and the error definitions are that file's own).  Writes profiles/deferred_left_parity.json, from which the
file's BARS are taken.
    python tools/deferred_left_parity.py [--out profiles/deferred_left_parity.json]"""
import argparse
import importlib.util
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
spec = importlib.util.spec_from_file_location("deferred_left_tests", os.path.join(ROOT, "tests", "test_deferred_left_gpu.py"))
t = importlib.util.module_from_spec(spec)
spec.loader.exec_module(t)

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "deferred_left_parity.json"))
args = ap.parse_args()
names = ("mean", "var", "alpha", "logdet")
rows = []
for case in ("n4500", "n2900_b512", "n4500_wide"):
    for level, env in (("strassen", t.STRASSEN), ("classical", t.SPLIT)):
        for defer, sw in (("off", t.OFF), ("on", t.ON)):
            e = t.fit_run(case, {**env, **sw})["errors"]
            rows.append({"case": case, "products": level, "GPX_DEFER_LEFT": defer, **dict(zip(names, e))})
            print(rows[-1], file=sys.stderr, flush=True)
# the cases in which a product is deferred (n4500_wide: a single panel, bit-identical off and on)
worst = {d: {q: max(r[q] for r in rows if r["products"] == "strassen" and r["GPX_DEFER_LEFT"] == d and r["case"] != "n4500_wide")
             for q in names} for d in ("off", "on")}
res = {"what": "tools/deferred_left_parity.py: errors against OracleGP (fp64) of the fits of tests/test_deferred_left_gpu.py",
       "bars_at_full_size": {"mean": 1e-6, "var": 1e-6, "alpha": 1e-8, "logdet": 1e-12},
       "largest_strassen": worst, "rows": rows}
json.dump(res, open(args.out, "w"), indent=1)
print(json.dumps(worst))
