"""CPU: the reference of the hierarchical path model (tests/within_ref.py) against itself — the Schur-form forecast, which
is what the library computes, against the refit-form forecast, which shares no step with it beyond the covariance function.

Problem: P = 12 paths x L = 33 points, Matern-3/2, sf2 = 1.5, sg2 = 0.4, l = 0.25, l_path = 0.1, noise = 1e-2, G = 5 new paths
of (Lo, Lp) = (20, 13), k = 2, seed fixed.  Both routes are fp64 dense algebra on matrices of condition number <= 3801 (the
conditioning matrix) and ~ N (sf2 + sg2) / noise ~ 1e5 (the refit), so they agree to about 1e5 x 1e-16 x O(10) ~ 1e-10 at
worst; measured 4e-13 with this seed (0) and G = 5, where the largest condition number is 366 against the bound 3801."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import within_ref as wr  # noqa: E402
from score_ref import score_ref  # noqa: E402

HYP = dict(kernel="matern32", ls=0.25, sf2=1.5, ls_path=0.1, sg2=0.4, sn2=1e-2)


def _fit(p, ids):
    return wr.fit_ref(p["X"], ids, p["Y"], HYP["kernel"], HYP["ls"], HYP["sf2"], HYP["sn2"], HYP["ls_path"], HYP["sg2"])


def test_schur_forecast_is_the_refit_forecast():
    p = wr.problem(seed=0)
    G = 5
    a = wr.forecast_schur(_fit(p, p["ids"]), p["Xo"], p["Yo"], p["Xp"], G, HYP["sn2"])
    b = wr.forecast_refit(dict(X=p["X"], ids=p["ids"], Y=p["Y"], **HYP), p["Xo"], p["Yo"], p["Xp"], G, HYP["sn2"])
    em, ec, el = (float(np.max(np.abs(a[n] - b[n]))) for n in ("mean", "cov", "logp"))
    bound = wr.kappa_bound(20, HYP["sf2"], HYP["sg2"], HYP["sn2"])
    print(f"schur vs refit: mean {em:.2e} cov {ec:.2e} logp {el:.2e}; kappa max {a['kappa'].max():.4g} (bound {bound:.5g})")
    assert em <= 1e-10 and ec <= 1e-10 and el <= 1e-10
    assert np.all(a["kappa"] <= bound)
    # the forecast says something: it leaves the cluster mean, and it is surer than the prior of a new path
    fmean = wr.predict_f(_fit(p, p["ids"]), p["Xp"])[0]
    var = np.concatenate([np.diag(c) for c in a["cov"]])
    print(f"forecast moves up to {np.max(np.abs(a['mean'] - fmean)):.3g} off the cluster mean, variances "
          f"{var.min():.3g} .. {var.max():.3g}")
    assert np.max(np.abs(a["mean"] - fmean)) > 0.1 and var.max() < HYP["sg2"] + 0.1 and var.min() > 0


def test_plain_fit_forecast_is_the_refit_forecast_too():
    p = wr.problem(seed=1)
    a = wr.forecast_schur(_fit(p, None), p["Xo"], p["Yo"], p["Xp"], 5, HYP["sn2"])
    b = wr.forecast_refit(dict(X=p["X"], ids=None, Y=p["Y"], **HYP), p["Xo"], p["Yo"], p["Xp"], 5, HYP["sn2"])
    e = max(float(np.max(np.abs(a[n] - b[n]))) for n in ("mean", "cov"))
    # the data come from the hierarchical model, so under the plain one the prefixes are far out (maha ~ 1e3) and the
    # refit's logp is the difference of two LMLs of ~ 1e4: its error scales with them — the score bound's (Lo + maha)
    el = float(np.max(np.abs(a["logp"] - b["logp"]) / (20 + a["maha"])))
    print(f"plain fit, schur vs refit: mean / cov {e:.2e}, logp / (Lo + maha) {el:.2e} (maha max {a['maha'].max():.4g})")
    assert e <= 1e-10 and el <= 1e-10


def test_all_ids_minus_one_is_score_ref_exactly():
    p = wr.problem(seed=2)
    Xq = np.concatenate([p["Xo"].reshape(5, 20, 1), p["Xp"].reshape(5, 13, 1)], axis=1).reshape(-1, 1)
    Yq = np.concatenate([p["Yo"].reshape(5, 20, 2), p["Yp"].reshape(5, 13, 2)], axis=1).reshape(-1, 2)
    none = np.full(len(p["X"]), -1)
    got = wr.score_ref_within(_fit(p, none), Xq, Yq, 33, HYP["sn2"])
    ref = score_ref(p["X"], p["Y"], Xq, Yq, 33, HYP["kernel"], HYP["ls"], HYP["sf2"], HYP["sn2"], HYP["sn2"])
    for n in ("logp", "maha", "logdet", "kappa"):
        assert np.array_equal(got[n], ref[n]), n
    K = wr.path_cov(p["X"], none, p["X"], none, HYP["kernel"], HYP["ls"], HYP["sf2"], HYP["ls_path"], HYP["sg2"])
    assert np.array_equal(K, wr.path_cov(p["X"], None, p["X"], None, HYP["kernel"], HYP["ls"], HYP["sf2"], 1.0, 0.0))
