"""Writes profiles/bad_pivot_parity.json: for every case of tests/test_bad_pivot_gpu.py, on the GPU this runs on, the pivot
index the library reports beside LAPACK's, and per schedule the largest error of the factor's prefix — rows [0, p0) against
the reference matrix (|L L^T - K| / |K| over p0 eps: the test's bar is 8) and against LAPACK's factor (max |L - ref| /
max |ref|: the bar is 1e-9) — and the info of the one case that is not an equality, a NaN row right of c under a Strassen
level.

    python tools/bad_pivot_parity.py [--out profiles/bad_pivot_parity.json]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bad_pivot_parity.json"))
    args = ap.parse_args()
    import bad_pivot_ref as bp
    import test_bad_pivot_gpu as t
    schedules = {}

    def book(schedule, p0, info, want, prefix, eps):
        # (the prefix figures stay null where no factor can be read back: GPX_MIXED handles, device groups)
        s = schedules.setdefault(schedule, {"cases": 0, "info_equal": 0, "backward_over_p0_eps": None, "factor": None})
        s["cases"] += 1
        s["info_equal"] += int(info == want)
        if prefix:
            s["backward_over_p0_eps"] = max(s["backward_over_p0_eps"] or 0.0, float(f"{prefix[0] / (p0 * eps):.3g}"))
            s["factor"] = max(s["factor"] or 0.0, float(f"{prefix[1]:.3g}"))

    for name, env, n, block, bad in bp.potrf_cases():
        rc, info, prefix = t.potrf_figures(env, n, block, bad)
        assert rc == 0, (name, rc)
        book("potrf " + name.rsplit("-", len(bad))[0], bp.first_bad(bad), info, t.info_ref(n, bad), prefix, bp.EPS)
        print(name, info, prefix, flush=True)
    for name, case in bp.FIT_CASES.items():
        info, grew, prefix, eps = t.fit_figures(name)
        assert grew == 0, name
        book("fit " + name.rsplit("-", 1)[0], case["p0"], info, case["p0"] + 1, prefix, eps)
        print(name, info, prefix, flush=True)
    info, grew, prefix = t.strassen_nan_row_figures()
    c = bp.STRASSEN_NAN_ROW
    rec = {"what": "tests/test_bad_pivot_gpu.py on one MI355X.  Per schedule: cases run, cases whose info equals LAPACK's, and "
                   "the largest prefix errors (rows [0, p0) of the factor): backward_over_p0_eps = |L L^T - K| / |K| / (p0 eps), "
                   "eps of the factor's element type, bar 8; factor = max |L - ref| / max |ref| against LAPACK's factor, bar "
                   "1e-9 in fp64 (none in fp32).  strassen_nan_row: the fit that is not held to info = p0 + 1",
           "schedules": schedules,
           "strassen_nan_row": {"N": c["N"], "block": c["block"], "c": c["c"], "p0": c["p0"], "info": info,
                                "rows_reached": sorted(bp.strassen_partner_rows(c["p0"], c["c"], c["npad"] - c["c"])),
                                "backward_over_rows_eps": float(f"{prefix[0] / ((info - 1) * bp.EPS):.3g}"),
                                "factor": float(f"{prefix[1]:.3g}")}}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print("schedules", len(schedules), "all equal", all(s["info_equal"] == s["cases"] for s in schedules.values()),
          "strassen_nan_row info", info)


if __name__ == "__main__":
    main()
