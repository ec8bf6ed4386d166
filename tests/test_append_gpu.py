"""GPU: GP.update / gpx_append — observations appended to a fitted model without factorising the old ones again
(include/gpx.h), GP.reserve / gpx_reserve, PathModel.add_paths.

Bars (the project's own): against the dense fp64 reference fitted on the concatenated data 1e-6 elementwise with the
floors of tests/test_fit_predict_gpu.py (alpha 1e-7 of its largest entry, tests/test_gp_parity_gpu.py), against a fresh
fit of the same library on the concatenated data 1e-9 (the same arithmetic in another summation order), float32 handles
the bars of tests/test_fp32_gpu.py.  The reference is OracleGP for "rbf" and "matern52"; the oracle does not know
Matern-3/2 and Matern-1/2, whose reference is tests/matern_ref.py's DenseGP (as in tests/test_matern_gpu.py).
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest
from scipy.linalg import solve_triangular

from gaussianprocesspathmodelling_amd import GP, _abi
from gaussianprocesspathmodelling_amd import paths as gpaths
from oracle.gp_oracle import OracleGP, kernel_matrix, synthetic_problem

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import matern_ref  # noqa: E402
from deriv_ref import grad_ref, prior_grad_var  # noqa: E402

pytestmark = pytest.mark.gpu

SF2, SN2 = 1.5, 1e-2


def rel(a, b, floor):
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), floor)))


def problem(N, d, M, k, seed):
    X, y, Xs = synthetic_problem(N, d, M, seed=seed)
    if k > 1:
        rng = np.random.default_rng(5)
        y = np.stack([y] + [np.sin((c + 2) * X[:, 0]) + 0.1 * rng.standard_normal(N) for c in range(k - 1)], axis=1)
    return X, y, Xs


def reference(kernel, ls, X, y, Xs, want_grad, want_lml):
    """mean, var, alpha, logdet, joint covariance (+ LML and its gradient, + posterior gradient) of the dense fp64 GP"""
    r = {}
    if kernel in ("rbf", "matern52"):
        og = OracleGP(kernel, ls, SF2, SN2, jitter=0.0).fit(X, y)
        r["mean"], r["var"] = og.predict(Xs)
        r["alpha"], r["logdet"] = og.alpha_, og.log_det_
        V = solve_triangular(og.L_, kernel_matrix(Xs, X, kernel, ls, SF2).T, lower=True)
        r["cov"] = kernel_matrix(Xs, Xs, kernel, ls, SF2) - V.T @ V
        if want_lml:
            r["lml"], r["grad"] = og.log_marginal_likelihood(), og.lml_gradient()
        if want_grad:
            r["dmean"], r["dvar"] = grad_ref(X, y, Xs, kernel, ls, SF2, SN2, 0.0)
            r["prior"] = prior_grad_var(kernel, ls, SF2, X.shape[1])
    else:
        dg = matern_ref.DenseGP(kernel, ls, SF2, SN2, 0.0).fit(X, y)
        mean, r["var"] = dg.predict(Xs)
        r["mean"] = mean[:, 0] if np.ndim(y) == 1 else mean
        r["alpha"] = dg.alpha[:, 0] if np.ndim(y) == 1 else dg.alpha
        r["logdet"] = 2.0 * float(np.sum(np.log(np.diag(dg.L))))
        r["cov"] = dg.predict_cov(Xs)[1]
        if want_lml:
            r["lml"], r["grad"] = dg.lml(), dg.lml_grad()
        if want_grad and kernel == "matern32":
            r["dmean"], r["dvar"] = dg.predict_grad(Xs)
            r["prior"] = matern_ref.prior_grad_var(ls, SF2, X.shape[1])
    return r


def outputs(gp, Xs, want_grad, want_lml):
    o = {}
    o["mean"], o["var"] = gp.predict(Xs)
    o["alpha"], o["logdet"] = gp.alpha_.copy(), gp.log_det_
    o["cov"] = gp.predict(Xs, return_cov=True)[1]
    if want_lml:
        o["lml"], o["grad"] = gp.lml_gradient()
    if want_grad:
        o["dmean"], o["dvar"] = gp.predict_gradient(Xs)
    return o


def check(o, ref, fresh, tag):
    """the appended model `o` against the dense reference (1e-6) and a fresh fit of the library (1e-9).  Elementwise with
    the floors of tests/test_fit_predict_gpu.py; alpha, the gradients and — against the fresh fit — the joint covariance
    relative to their largest entry, as tests/test_posterior_gpu.py and tests/test_predict_grad_gpu.py compare two routes
    of the library: off-diagonal covariances cancel to zero, where 1e-9 of a 1e-6 sf2 floor is below fp64 rounding."""
    M = len(o["var"])
    fig = {
        "mean/ref": rel(o["mean"], ref["mean"], 1e-6), "var/ref": rel(o["var"], ref["var"], 1e-6 * SF2),
        "alpha/ref": float(np.max(np.abs(o["alpha"] - ref["alpha"])) / np.max(np.abs(ref["alpha"]))),
        "logdet/ref": abs(o["logdet"] - ref["logdet"]) / abs(ref["logdet"]),
        "cov/ref": rel(o["cov"], ref["cov"], 1e-6 * SF2),
        "mean/fresh": rel(o["mean"], fresh["mean"], 1e-6), "var/fresh": rel(o["var"], fresh["var"], 1e-6 * SF2),
        "alpha/fresh": float(np.max(np.abs(o["alpha"] - fresh["alpha"])) / np.max(np.abs(fresh["alpha"]))),
        "logdet/fresh": abs(o["logdet"] - fresh["logdet"]) / abs(fresh["logdet"]),
        "cov/fresh": float(np.max(np.abs(o["cov"] - fresh["cov"])) / np.max(np.abs(fresh["cov"]))),
    }
    if "lml" in o:
        fig["lml/ref"] = abs(o["lml"] - ref["lml"]) / abs(o["lml"])
        fig["grad/ref"] = float(np.max(np.abs(o["grad"] - ref["grad"])) / np.max(np.abs(o["grad"])))
        fig["lml/fresh"] = abs(o["lml"] - fresh["lml"]) / abs(fresh["lml"])
        fig["grad/fresh"] = float(np.max(np.abs(o["grad"] - fresh["grad"])) / np.max(np.abs(fresh["grad"])))
    if "dmean" in o:
        dmr = np.asarray(ref["dmean"]).reshape(M, o["dvar"].shape[1], -1)
        dm, dmf = (np.asarray(v["dmean"]).reshape(dmr.shape) for v in (o, fresh))
        fig["dmean/ref"] = float(np.max(np.abs(dm - dmr)) / np.max(np.abs(dmr)))
        fig["dvar/ref"] = rel(o["dvar"], ref["dvar"], 1e-6 * ref["prior"][None, :])
        fig["dmean/fresh"] = float(np.max(np.abs(dm - dmf)) / np.max(np.abs(dmf)))
        fig["dvar/fresh"] = rel(o["dvar"], fresh["dvar"], 1e-6 * ref["prior"][None, :])
    print(tag, " ".join(f"{n} {v:.2e}" for n, v in fig.items()))
    for n, v in fig.items():
        bar = 1e-9 if n.endswith("/fresh") or n in ("logdet/ref", "lml/ref") else 1e-7 if n == "alpha/ref" else 1e-6
        assert v <= bar, (tag, n, v, bar)


@pytest.mark.parametrize("N,m,d,k,kernel,ard,block", [
    (1000, 20, 3, 1, "rbf", False, 0),            # the new points fit into the padding of Npad = 1024: nothing moves
    (1000, 200, 3, 3, "matern52", True, 256),     # crosses 128-boundaries; R0 = 768: left part, Schur term, three targets
    (900, 150, 2, 1, "matern32", False, 256),
    (900, 150, 3, 1, "matern12", False, 512),
    (2048, 100, 3, 1, "rbf", False, 1024),        # N an exact multiple of nb: R0 = N, only new rows are factorised
    (1500, 2500, 3, 1, "rbf", False, 1024),       # m > nb: several panels of the restart, the look-ahead schedule
    (8192 + 512, 200, 3, 1, "rbf", False, 0),     # the library's width, R0 = 8192
    (4000, 450, 3, 1, "rbf", False, 2048),        # a wide factor: R0 = 2048, the new points cross 4096 and open a third panel
    (4300, 200, 3, 1, "rbf", False, 2048),        # R0 = 4096: only the ragged third panel is redone
])
def test_single_append(N, m, d, k, kernel, ard, block):
    X, y, Xs = problem(N + m, d, 90, k, seed=N + m)
    ls = tuple(0.2 + 0.05 * i for i in range(d)) if ard else 0.25
    small = N + m <= 4000
    want_grad = kernel != "matern12" and small
    ref = reference(kernel, ls, X, y, Xs, want_grad, small)
    with GP(kernel, ls, SF2, SN2, jitter=0.0, block=block) as gp:
        fresh = outputs(gp.fit(X, y), Xs, want_grad, small)
        assert gp.fit(X[:N], y[:N]).update(X[N:], y[N:]) is gp
        assert gp.get_state()["fitted"]["N"] == N + m and gp.alpha_.shape[0] == N + m
        check(outputs(gp, Xs, want_grad, small), ref, fresh, f"N={N} m={m} {kernel} block={block}:")
        t = gp.timings_
        assert t["fit_total"] > 0 and t["chol"] > 0


def test_single_append_float32():
    N, m = 1000, 200
    X, y, Xs = synthetic_problem(N + m, 3, 90, seed=11)
    ls, noise = (0.3, 0.2, 0.25), 1e-1
    og = OracleGP("rbf", ls, 1.5, noise, jitter=0.0).fit(X, y)
    mr, vr = og.predict(Xs)
    with GP("rbf", ls, 1.5, noise, jitter=0.0, dtype="float32", block=256) as gp:
        m1, v1 = gp.fit(X, y).predict(Xs)
        a1, ld1 = gp.alpha_.copy(), gp.log_det_
        mean, var = gp.fit(X[:N], y[:N]).update(X[N:], y[N:]).predict(Xs)
        assert mean.dtype == np.float32 and gp.alpha_.shape == (N + m,)
        em, ev = np.max(np.abs(mean - mr)) / np.max(np.abs(mr)), np.max(np.abs(var - vr)) / 1.5
        el = abs(gp.log_det_ - og.log_det_) / abs(og.log_det_)
        print(f"fp32 append: mean {em:.2e} var {ev:.2e} logdet {el:.2e}")
        assert em <= 2e-3 and ev <= 2e-3 and el <= 1e-3
        assert np.max(np.abs(mean - m1)) <= 1e-3 * np.max(np.abs(m1)) and np.max(np.abs(var - v1)) <= 1e-3 * 1.5
        assert np.max(np.abs(gp.alpha_ - a1)) <= 2e-3 * np.max(np.abs(a1)) and abs(gp.log_det_ - ld1) <= 1e-4 * abs(ld1)


def factor_ptr(gp):
    ptr, ld, cap = C.c_void_p(0), C.c_int64(0), C.c_int64(0)
    gp._check(gp._lib.gpx_factor_info(gp._h, C.byref(ptr), C.byref(ld), C.byref(cap)))
    return ptr.value, ld.value, cap.value


def test_chain_of_appends_with_and_without_reserve():
    N0, m, steps = 700, 37, 40
    N = N0 + m * steps
    X, y, Xs = problem(N, 3, 90, 1, seed=77)
    ref = reference("rbf", 0.25, X, y, Xs, True, True)
    with GP("rbf", 0.25, SF2, SN2, jitter=0.0, block=1024) as gp:
        fresh = outputs(gp.fit(X, y), Xs, True, True)

    def chain(reserve):
        with GP("rbf", 0.25, SF2, SN2, jitter=0.0, block=1024) as gp:
            if reserve:
                gp.reserve(reserve)
            gp.fit(X[:N0], y[:N0])
            ptrs = [factor_ptr(gp)[0]]
            for s in range(steps):
                a = N0 + s * m
                gp.update(X[a:a + m], y[a:a + m])
                ptrs.append(factor_ptr(gp)[0])
            assert gp.get_state()["fitted"]["N"] == N
            return outputs(gp, Xs, True, True), ptrs, factor_ptr(gp)

    plain, ptrs, (_, ld, cap) = chain(0)
    check(plain, ref, fresh, "chain:")
    moves = sum(a != b for a, b in zip(ptrs, ptrs[1:]))
    assert 1 <= moves <= 3 and cap >= N and ld == cap + 16        # at most one move per panel width of points
    res, ptrs, (_, ld, cap) = chain(4096)
    assert len(set(ptrs)) == 1 and cap == 4096 and ld == 4096 + 16     # in place: the factor never moved
    check(res, ref, fresh, "reserved chain:")
    check(res, ref, plain, "reserved against unreserved chain:")


def test_append_in_place_on_the_wide_panel_width(monkeypatch):
    """the first wide row of test_single_append under the library's own choice of 2048-wide panels (GPX_NB_WIDE_FROM=2048:
    nb_pred = 2048, so the forward solve of the new rows takes the dense block solves) on a reserved factor: it does not move"""
    N, m = 4000, 450
    X, y, Xs = problem(N + m, 3, 90, 1, seed=N + m)
    ref = reference("rbf", 0.25, X, y, Xs, False, False)
    monkeypatch.setenv("GPX_NB_WIDE_FROM", "2048")
    monkeypatch.delenv("GPX_NB_PRED", raising=False)
    with GP("rbf", 0.25, SF2, SN2, jitter=0.0) as gp:
        fresh = outputs(gp.fit(X, y), Xs, False, False)
    with GP("rbf", 0.25, SF2, SN2, jitter=0.0) as gp:
        gp.reserve(6144)
        gp.fit(X[:N], y[:N])
        before = factor_ptr(gp)
        gp.update(X[N:], y[N:])
        assert factor_ptr(gp) == before and before[1:] == (6144 + 16, 6144)       # in place: the factor never moved
        assert gp.get_state()["fitted"]["N"] == N + m
        check(outputs(gp, Xs, False, False), ref, fresh, "wide-auto, reserved, N=4000 m=450:")
    monkeypatch.delenv("GPX_NB_WIDE_FROM")
    with GP("rbf", 0.25, SF2, SN2, jitter=0.0) as gp:                          # the 1024 fit: other bits, so the width took
        assert not np.array_equal(gp.fit(X, y).alpha_, fresh["alpha"])


def test_untouched_handles_keep_their_bits_and_appends_do_not_depend_on_stream_timing():
    N, m = 3000, 700
    X, y, Xs = synthetic_problem(N + m, 3, 200, seed=21)
    lib = _abi.load()

    def plain():
        with GP("matern52", (0.3, 0.2, 0.25), SF2, SN2, jitter=0.0, block=256) as gp:
            mean, var = gp.fit(X[:N], y[:N]).predict(Xs)
            return mean, var, gp.alpha_.copy(), gp.log_det_, factor_ptr(gp)[1:]

    def appended(reserve):
        with GP("matern52", (0.3, 0.2, 0.25), SF2, SN2, jitter=0.0, block=256) as gp:
            if reserve:
                gp.reserve(reserve)
            mean, var = gp.fit(X[:N], y[:N]).update(X[N:], y[N:]).predict(Xs)
            return mean, var, gp.alpha_.copy(), gp.log_det_

    before = plain()
    assert before[4] == (3072 + 16, 3072)          # the layout of a handle that never reserves: ld = Npad + one line
    base = [appended(0), appended(5000)]
    after = plain()                                # constructed after other handles reserved and appended
    assert all(np.array_equal(a, b) for a, b in zip(before[:3], after[:3])) and before[3:] == after[3:]
    try:
        for seed in (1, 2, 3):
            lib.gpx_debug_set_delay(seed)
            for got, want in zip((appended(0), appended(5000)), base):
                assert all(np.array_equal(a, b) for a, b in zip(got[:3], want[:3])) and got[3] == want[3], seed
    finally:
        lib.gpx_debug_set_delay(0)


def test_failed_append_keeps_the_model():
    """K of the 300 fitted points is exactly the identity (every off-diagonal exp underflows); the point -100 twice gives
    the Schur block [[1, 1], [1, 1]]: the second pivot is exactly 0 (LAPACK dpotrf on the 302 x 302 matrix: info = 302)."""
    X = 100.0 * np.arange(300, dtype=np.float64)[:, None]
    y = np.sin(np.arange(300, dtype=np.float64))
    Xs = X[:50] + 0.3
    twice = np.array([[-100.0], [-100.0]])
    apart = np.array([[-100.0], [-200.0]])
    ynew = np.array([0.5, -0.25])
    with GP("rbf", 1.0, 1.0, noise=0.0, jitter=0.0) as gp:
        m0, v0 = gp.fit(X, y).predict(Xs)
        a0, ld0 = gp.alpha_.copy(), gp.log_det_
        info = C.c_int64(-1)
        rc = gp._lib.gpx_append(gp._h, twice.ctypes.data_as(C.c_void_p), ynew.ctypes.data_as(C.c_void_p), 2,
                                _abi.MEM_HOST, C.byref(info))
        assert rc == 0 and info.value == 302
        with pytest.raises(np.linalg.LinAlgError, match="unchanged"):
            gp.update(twice, ynew)
        assert gp.get_state()["fitted"]["N"] == 300
        m1, v1 = gp.predict(Xs)
        assert rel(m1, m0, 1e-6) <= 1e-9 and rel(v1, v0, 1e-6) <= 1e-9
        assert np.max(np.abs(gp.alpha_ - a0)) <= 1e-9 * np.max(np.abs(a0)) and abs(gp.log_det_ - ld0) <= 1e-9
        gp.update(apart, ynew)                                 # two distinct far points: positive definite
        assert gp.get_state()["fitted"]["N"] == 302
        m2, v2 = gp.predict(np.concatenate([Xs, apart + 0.3]))
        with GP("rbf", 1.0, 1.0, noise=0.0, jitter=0.0) as gf:
            mf, vf = gf.fit(np.concatenate([X, apart]), np.concatenate([y, ynew])).predict(np.concatenate([Xs, apart + 0.3]))
        assert rel(m2, mf, 1e-6) <= 1e-9 and rel(v2, vf, 1e-6) <= 1e-9


@pytest.mark.parametrize("kw", [{"dtype": "mixed"}, {"devices": [0], "transport": "local"}])
def test_append_and_reserve_are_refused_beyond_single_device_fp64_fp32(kw):
    X, y, Xs = synthetic_problem(1200, 3, 60, seed=31)
    with GP("rbf", 0.25, SF2, SN2, jitter=0.0, **kw) as gp:
        m0, v0 = gp.fit(X[:1000], y[:1000]).predict(Xs)
        with pytest.raises(_abi.GpxError) as e:
            gp.update(X[1000:], y[1000:])
        assert e.value.code == _abi.E_UNSUPPORTED
        with pytest.raises(_abi.GpxError) as e:
            gp.reserve(4096)
        assert e.value.code == _abi.E_UNSUPPORTED
        assert gp.get_state()["fitted"]["N"] == 1000
        m1, v1 = gp.predict(Xs)
        assert np.array_equal(m1, m0) and np.array_equal(v1, v0)


def test_update_argument_rules():
    X, y, Xs = synthetic_problem(600, 3, 10, seed=41)
    with GP("rbf", 0.25, SF2, SN2, jitter=0.0) as gp:
        with pytest.raises(RuntimeError):
            gp.update(X[:5], y[:5])                            # before a fit
        gp.fit(X[:500], y[:500])
        with pytest.raises(ValueError):
            gp.update(X[500:, :2], y[500:])
        with pytest.raises(ValueError):
            gp.update(X[500:], np.stack([y[500:], y[500:]], 1))
        with pytest.raises(_abi.GpxError) as e:
            gp.reserve(100)                                    # below what the handle holds
        assert e.value.code == _abi.E_ARG
        assert gp.update(X[500:500], y[500:500]) is gp and gp.get_state()["fitted"]["N"] == 500


def test_update_with_device_tensors():
    torch = pytest.importorskip("torch")
    N, m = 1500, 300
    X, y, Xs = synthetic_problem(N + m, 3, 100, seed=51)
    dev = torch.device("cuda", 0)
    Xd, yd, Xsd = (torch.from_numpy(v).to(dev) for v in (X, y, Xs))
    with GP("rbf", 0.25, SF2, SN2, jitter=0.0, block=512) as gp:
        mh, vh = gp.fit(X[:N], y[:N]).update(X[N:], y[N:]).predict(Xs)
        md, vd = gp.fit(Xd[:N], yd[:N]).update(Xd[N:], yd[N:]).predict(Xsd)
        assert md.is_cuda and vd.is_cuda
        assert rel(md.cpu().numpy(), mh, 1e-6) <= 1e-9 and rel(vd.cpu().numpy(), vh, 1e-6 * SF2) <= 1e-9
        with pytest.raises(ValueError):
            gp.update(Xd[:3], y[:3])                           # one on the device, one on the host


def test_add_paths_matches_the_oracle_on_all_paths():
    from test_paths_gpu import _synthetic_groups
    t, truth = _synthetic_groups(n_groups=1, per_group=9, seed=6)
    keys = truth[0]
    first, later = keys[:5], keys[5:]
    models = gpaths.fit_path_models(t, {0: first}, kernel="matern52", lengthscale=0.3, variance=1.0, noise=0.02)
    pm = models[0]
    try:
        assert pm.add_paths(t, later[:2]).add_paths(t, later[2:]) is pm and pm.keys == keys
        X1, Y1, (lo, span) = gpaths.to_gp_inputs(t, first)
        mu, sd = Y1.mean(0), Y1.std(0)
        Xa, Ya, _ = gpaths.to_gp_inputs(t, keys, normalise=False)
        o = OracleGP("matern52", 0.3, 1.0, 0.02, jitter=1e-10).fit((Xa - lo) / span, (Ya - mu) / sd)
        q = np.linspace(-50.0, 1400.0, 57)
        om, ov = o.predict((q.reshape(-1, 1) - lo) / span)
        om, ov = om * sd + mu, ov[:, None] * sd ** 2
        mean, var = pm.predict(q)
        assert np.max(np.abs(mean - om)) <= 1e-6 * np.max(np.abs(om))
        assert np.max(np.abs(var - ov)) <= 1e-6 * np.max(np.abs(ov))
    finally:
        pm.close()
