"""GPU: GP.loo / GP.loo_log_likelihood / gpx_loo — the leave-one-out predictions of a fitted model (include/gpx.h;
DESIGN.md §3.4o) against the dense closed form of tests/loo_ref.py (which tests/test_loo_ref.py holds to the refit), for every
kind of fit one fp64 handle can hold.  ``jitter=0.0``, SF2 = 1.5, SN2 = 1e-2 as in tests/test_append_gpu.py.

Bars: the project's own 1e-6 elementwise against the dense reference — mean with floor 1e-6, var purely relative (it is at
least the row's noise), logp with floor 1 — and 1e-9 against the library's own fresh fit of the same rows (after update /
remove).  ``total`` (the sum of logp over the rows) has no precedent: TOTAL_BAR is one decade above the largest figure
measured over the cases of this file on one MI355X (profiles/loo_parity.json).  Every test prints its figures before it
asserts."""
import contextlib
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

from gaussianprocesspathmodelling_amd import GP, _abi
from gaussianprocesspathmodelling_amd._abi import GpxError
from oracle.gp_oracle import synthetic_problem

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import basis_ref  # noqa: E402
import dobs_ref  # noqa: E402
import loo_ref  # noqa: E402
import within_ref  # noqa: E402

pytestmark = pytest.mark.gpu

SF2, SN2 = 1.5, 1e-2
BAR, FRESH_BAR = 1e-6, 1e-9
TOTAL_BAR = 4e-13         # measured at most 3.81e-14 (the case "derivatives"; profiles/loo_parity.json)
ARD = (0.3, 0.2, 0.25)
SWITCHES = ("GPX_NB_GRAD", "GPX_NB_WIDE_FROM", "GPX_NB_PRED", "GPX_FEW_SOLVE")

# name -> what is fitted.  kind "plain": synthetic_problem(N, 3), k targets, optional noise weights; the others take the
# problems of their own reference modules.
CASES = {
    "n150_rbf": dict(kind="plain", N=150, kernel="rbf", ls=0.25, k=1),                        # Npad = 192: less than one block
    "n333_matern52_ard_k3": dict(kind="plain", N=333, kernel="matern52", ls=ARD, k=3),        # several targets, 64-boundaries
    "n700_nb_grad_128": dict(kind="plain", N=700, kernel="rbf", ls=0.25, k=1, env={"GPX_NB_GRAD": "128"}),  # six trtri blocks
    "n1100_matern12_block1024": dict(kind="plain", N=1100, kernel="matern12", ls=ARD, k=1, block=1024),     # crosses 1024 once
    "n4500_wide": dict(kind="plain", N=4500, kernel="rbf", ls=0.25, k=1, env={"GPX_NB_WIDE_FROM": "2048"}),  # wide-panel fit
    "n333_weights": dict(kind="plain", N=333, kernel="rbf", ls=0.25, k=1, weights=True),
    "derivatives": dict(kind="dobs"),
    "paths": dict(kind="within"),
    "basis_constant": dict(kind="basis", basis="constant", N=300, k=2),                       # p = 1
    "basis_quadratic": dict(kind="basis", basis="quadratic", N=300, k=2),                     # p = 7
    # p > 8: the row pass's other instantiation (one row per wave, up to 63 accumulators per lane); p = 9, and the limit p = 63
    "basis_quadratic_d4": dict(kind="basis", basis="quadratic", N=300, k=2, d=4, ls=0.3),
    "basis_quadratic_d31": dict(kind="basis", basis="quadratic", N=300, k=1, d=31, ls=2.0),
}


@contextlib.contextmanager
def switches(env):
    with pytest.MonkeyPatch.context() as mp:
        for name in SWITCHES:
            mp.delenv(name, raising=False)
        for name, value in (env or {}).items():
            mp.setenv(name, value)
        yield


def plain_data(N, k, seed=None):
    X, y, _ = synthetic_problem(N, 3, 1, seed=N if seed is None else seed)
    if k > 1:
        rng = np.random.default_rng(5)
        y = np.stack([y] + [np.sin((c + 2) * X[:, 0]) + 0.1 * rng.standard_normal(N) for c in range(k - 1)], axis=1)
    return X, y


def plain_weights(N):
    return np.random.default_rng(7).uniform(0.25, 4.0, N)


@functools.lru_cache(maxsize=None)
def setup(name):
    """(make_gp, fit, K, Y, H) of a case: the handle, the call that fits it, and the dense inputs of the reference"""
    c = CASES[name]
    if c["kind"] == "plain":
        X, y = plain_data(c["N"], c["k"])
        w = plain_weights(c["N"]) if c.get("weights") else None
        make = lambda: GP(c["kernel"], c["ls"], SF2, SN2, jitter=0.0, block=c.get("block", 0))       # noqa: E731
        return make, (lambda gp: gp.fit(X, y, noise_weights=w)), loo_ref.plain_gram(X, c["kernel"], c["ls"], SF2, SN2, w), y, None
    if c["kind"] == "dobs":
        p = dict(dobs_ref.problem("matern52", 3, "last", 1003), jitter=0.0)
        make = lambda: GP(p["kernel"], p["ls"], p["sf2"], p["sn2"], jitter=0.0)                        # noqa: E731
        fit = lambda gp: gp.fit(p["X"], p["y"], derivatives=(p["Xd"], p["dims"], p["yd"]),             # noqa: E731
                                derivative_noise=p["sn2_deriv"])
        return make, fit, loo_ref.dobs_gram(p), p["yall"], None
    if c["kind"] == "within":
        p = within_ref.problem()                                      # 12 paths of 33 points, matern32, two targets
        make = lambda: GP("matern32", 0.25, SF2, SN2, jitter=0.0)                                      # noqa: E731
        fit = lambda gp: gp.fit(p["X"], p["Y"], path_ids=p["ids"], path_variance=0.4, path_lengthscale=0.1)  # noqa: E731
        return make, fit, loo_ref.within_gram(p["X"], p["ids"], "matern32", 0.25, SF2, SN2, 0.1, 0.4), p["Y"], None
    d, ls = c.get("d", 3), c.get("ls", ARD)
    X, Y, _ = basis_ref.trend_problem(c["N"], d, c["k"], 1, seed=c["N"] + d)
    make = lambda: GP("rbf", ls, SF2, SN2, jitter=0.0)                                                 # noqa: E731
    return (make, (lambda gp: gp.fit(X, Y, basis=c["basis"])), loo_ref.plain_gram(X, "rbf", ls, SF2, SN2), Y,
            basis_ref.basis_matrix(X, c["basis"]))


@functools.lru_cache(maxsize=None)
def reference(name):
    _, _, K, Y, H = setup(name)
    return loo_ref.loo_closed(K, Y, H)


def loo_all(gp):
    mean, var, logp = gp.loo(return_logp=True)
    return {"mean": mean, "var": var, "logp": logp, "total": gp.loo_log_likelihood()}


def same_bits(a, b):
    return all(np.array_equal(np.asarray(a[key]), np.asarray(b[key]), equal_nan=True) for key in a)


def measure(name):
    """the figures of one case (also what profiles/loo_parity.json records)"""
    make, fit, K, _, _ = setup(name)
    with switches(CASES[name].get("env")), make() as gp:
        fit(gp)
        got = loo_all(gp)
    fig = loo_ref.errors(got, reference(name))
    fig["N"] = len(K)
    return got, fig


@pytest.mark.parametrize("name", sorted(CASES))
def test_parity_with_the_dense_closed_form(name):
    got, fig = measure(name)
    ref = reference(name)
    print(f"{name}: N = {fig['N']}: {fig}")
    assert np.asarray(got["mean"]).shape == np.squeeze(ref["mean"]).shape and got["var"].shape == ref["var"].shape
    assert np.asarray(got["logp"]).shape == np.squeeze(ref["logp"]).shape
    assert np.all(got["var"] > 0)
    assert fig["mean"] < BAR and fig["var"] < BAR and fig["logp"] < BAR, fig
    assert fig["total"] < TOTAL_BAR, fig


def test_rows_that_the_basis_alone_determines():
    """N = p = 3 (linear basis, d = 2): var +inf, mean NaN, logp -inf in every row, total -inf"""
    X = np.random.default_rng(0).uniform(0.0, 1.0, (3, 2))
    y = np.array([0.3, -1.0, 2.0])
    with GP("rbf", 0.5, SF2, SN2, jitter=0.0) as gp:
        got = loo_all(gp.fit(X, y, basis="linear"))
        ok = gp.predict(X)
    print(f"N = p = 3: mean {got['mean']} var {got['var']} logp {got['logp']} total {got['total']}")
    assert np.all(got["var"] == np.inf) and np.all(np.isnan(got["mean"])) and np.all(got["logp"] == -np.inf)
    assert got["total"] == -np.inf and np.all(np.isfinite(ok[0]))


@pytest.mark.parametrize("how", ["update", "remove"])
def test_after_update_and_remove_loo_is_that_of_a_fresh_fit(how):
    X, y = plain_data(1050, 1, seed=1000)
    gone = np.arange(100, 150)
    with GP("rbf", 0.25, SF2, SN2, jitter=0.0) as gp, GP("rbf", 0.25, SF2, SN2, jitter=0.0) as fresh:
        if how == "update":
            gp.fit(X[:800], y[:800])
            gp.update(X[800:1000], y[800:1000])
            keep = np.arange(1000)
        else:
            gp.fit(X, y)
            gp.remove(gone)
            keep = np.setdiff1d(np.arange(1050), gone)
        got = loo_all(gp)
        want = loo_all(fresh.fit(X[keep], y[keep]))
    want = {key: np.asarray(v).reshape(len(keep), -1) if key in ("mean", "logp") else np.asarray(v) for key, v in want.items()}
    want["total"] = want["total"].reshape(-1)
    fig = loo_ref.errors(got, want)
    print(f"after {how}: N = {len(keep)}, against a fresh fit of the same rows: {fig}")
    assert len(got["var"]) == len(keep)
    assert max(fig.values()) < FRESH_BAR, fig


def test_two_calls_and_a_call_after_release_scratch_return_the_same_bits():
    for case in ("n333_matern52_ard_k3", "basis_quadratic"):
        make, fit, _, _, _ = setup(case)
        with make() as gp:
            fit(gp)
            first = loo_all(gp)
            second = loo_all(gp)
            gp.release_scratch()
            third = loo_all(gp)
        print(f"{case}: second call {same_bits(first, second)}, after release_scratch {same_bits(first, third)}")
        assert same_bits(first, second) and same_bits(first, third)


def test_loo_and_the_gradient_do_not_see_each_other():
    """both build L^-T in the same scratch: the gradient before and after a loo(), and loo() before and after a gradient"""
    make, fit, _, _, _ = setup("n700_nb_grad_128")
    for env in (None, {"GPX_NB_GRAD": "128"}):
        with switches(env), make() as gp:
            fit(gp)
            g0 = gp.lml_gradient()
            l0 = loo_all(gp)
            g1 = gp.lml_gradient()
            l1 = loo_all(gp)
        grads = g0[0] == g1[0] and np.array_equal(g0[1], g1[1])
        print(f"GPX_NB_GRAD {env}: gradient before / after loo() {grads}, loo() before / after the gradient {same_bits(l0, l1)}")
        assert grads and same_bits(l0, l1)
        with switches(env), make() as gp:                                # loo() on a handle that never ran a gradient
            assert same_bits(loo_all(fit(gp)), l0)


def test_the_fit_is_untouched_by_loo():
    make, fit, _, _, _ = setup("n333_matern52_ard_k3")
    Xs = synthetic_problem(10, 3, 70, seed=3)[2]
    with make() as gp:
        fit(gp)
        before = (*gp.predict(Xs), gp.alpha_.copy(), gp.log_det_)
        gp.loo()
        gp._alpha = None                                                 # (read alpha from the handle again)
        after = (*gp.predict(Xs), gp.alpha_.copy(), gp.log_det_)
    same = [np.array_equal(a, b) for a, b in zip(before, after)]
    print(f"predict mean / var, alpha_, log_det_ bit-identical before and after loo(): {same}")
    assert all(same)


@pytest.mark.parametrize("dtype", ["float32", "mixed"])
def test_handles_that_are_not_fp64_are_refused_and_keep_their_fit(dtype):
    X, y = plain_data(150, 1)
    X, y = (X.astype(np.float32), y.astype(np.float32)) if dtype == "float32" else (X, y)
    with GP("rbf", 0.25, SF2, SN2, dtype=dtype) as gp:
        before = gp.fit(X, y).predict(X[:20])
        for call in (gp.loo, gp.loo_log_likelihood):
            with pytest.raises(GpxError, match="gpx_loo: fp64 handles only") as e:
                call()
            assert e.value.code == _abi.E_UNSUPPORTED
        after = gp.predict(X[:20])
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])


def test_argument_refusals_of_the_c_call():
    X, y = plain_data(150, 1)
    with GP("rbf", 0.25, SF2, SN2) as gp:
        with pytest.raises(RuntimeError):
            gp.loo()                                                     # no fit yet (the Python host)
        var = np.zeros(150)
        assert gp._lib.gpx_loo(gp._h, None, _abi.dptr(var), None, None) == _abi.E_ARG    # ... and the library
        assert b"gpx_loo" in gp._lib.gpx_last_error(gp._h) and not var.any()
        gp.fit(X, y)
        assert gp._lib.gpx_loo(gp._h, None, None, None, None) == _abi.E_ARG
        assert b"gpx_loo" in gp._lib.gpx_last_error(gp._h)
        assert gp._lib.gpx_loo(gp._h, None, _abi.dptr(var), None, None) == 0             # any subset of the outputs
        total = C.c_double(0.0)
        assert gp._lib.gpx_loo(gp._h, None, None, None, C.byref(total)) == 0
        mean, v2, logp = gp.loo(return_logp=True)
        in_row_order = 0.0
        for v in logp:
            in_row_order += float(v)
        assert np.array_equal(var, v2) and total.value == gp.loo_log_likelihood() == in_row_order
        assert gp.loo(return_var=False).shape == (150,)
