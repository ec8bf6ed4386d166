"""GPU: a GP conditioned on derivative (velocity) observations — ``GP.fit(derivatives=)`` / gpx_set_observation_kinds —
against the dense fp64 reference of tests/dobs_ref.py, whose table holds the cases (conditioned by tests/test_dobs_ref.py):
200 values + 70 derivative rows (270: no multiple of 64 or 128, the kind boundary inside the tile [192, 256)), block=128
(three panels at the padded 384), 130 queries, d = 1 (scalar lengthscale), 3 (ARD, the D = 3 kernels) and 5 (ARD, the
generic-D kernels), the derivative rows last (through ``derivatives=``) or interleaved at random (kinds through the C call).

Bounds: those of tests/test_predict_grad_gpu.py (1e-6 of the largest entry for means and alpha; variances relative to
max(|ref|, 1e-6 prior)) and of tests/test_score_gpu.py (eps kappa_g (Lg + maha_g), eps = 1e-10 / 1e-4) for the same
quantities; on a float32 handle the levels of tests/test_fp32_gpu.py (mean 2e-3 of its largest entry, variance 2e-3 sf2,
log-determinant 1e-3) and of test_predict_grad_gpu.py's fp32 test (5e-3).  Every figure is printed before it is asserted."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from gaussianprocesspathmodelling_amd import GP, GpxError, _abi

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dobs_ref  # noqa: E402
from dobs_ref import BLOCK, SCORE_LG, case  # noqa: E402

pytestmark = pytest.mark.gpu

PARITY = [n for n in dobs_ref.CASES if n != "waypoints"]


def make_gp(c, **kw):
    return GP(c["kernel"], c["ls"], c["sf2"], c["sn2"], jitter=c["jitter"], block=BLOCK, **kw)


def fit_case(gp, c, name, dt=np.float64):
    """derivative rows last: through ``derivatives=``; interleaved: the kinds through the C call, the rows as they are (a
    model that never had kinds set through Python makes no call of its own that would clear them)"""
    a = lambda v: np.asarray(v, dtype=dt)  # noqa: E731
    if name.endswith("_mixed"):
        kinds = np.ascontiguousarray(c["kinds"], dtype=np.int32)
        rc = gp._lib.gpx_set_observation_kinds(gp._h, C.c_void_p(kinds.ctypes.data), kinds.size, c["sn2_deriv"], _abi.MEM_HOST)
        assert rc == 0
        return gp.fit(a(c["Xall"]), a(c["yall"]))
    return gp.fit(a(c["X"]), a(c["y"]), derivatives=(a(c["Xd"]), c["dims"], a(c["yd"])), derivative_noise=c["sn2_deriv"],
                  noise_weights=None if c.get("w_values") is None else a(c["w_values"]))


def rel_max(got, ref):
    return float(np.max(np.abs(np.asarray(got, dtype=np.float64) - ref)) / np.max(np.abs(ref)))


def rel_var(got, ref, floor):
    return float(np.max(np.abs(np.asarray(got, dtype=np.float64) - ref) / np.maximum(np.abs(ref), floor)))


def score_ratio(got, ref, eps):
    logp, maha, logdet = (np.asarray(a, dtype=np.float64) for a in got)
    G = len(ref["kappa"])
    bound = eps * ref["kappa"][:, None] * (SCORE_LG + ref["maha"])
    return max(float(np.max(np.abs(logp.reshape(G, -1) - ref["logp"]) / bound)),
               float(np.max(np.abs(maha.reshape(G, -1) - ref["maha"]) / bound)),
               float(np.max(np.abs(logdet - ref["logdet"]) / bound.min(axis=1))))


@pytest.mark.parametrize("name", PARITY)
def test_parity_fp64(name):
    c, ref = case(name)
    Xs, M, d = c["Xs"], len(c["Xs"]), c["Xs"].shape[1]
    with make_gp(c) as gp:
        fit_case(gp, c, name)
        assert np.array_equal(gp.observation_kinds_, c["kinds"])
        alpha, logdet, lml = gp.alpha_, gp.log_det_, gp.log_marginal_likelihood(c["yall"])
        mean, var = gp.predict(Xs)
        mean_c, cov = gp.predict(Xs, return_cov=True)
        dm, dv = gp.predict_gradient(Xs)
        dm_only = gp.predict_gradient(Xs, return_var=False)
        got_score = gp.score_blocks(c["Xq"], c["Yq"], SCORE_LG, return_parts=True)
    mr, vr = ref.predict(Xs)
    _, cr = ref.predict_cov(Xs)
    dmr, dvr = ref.predict_grad(Xs)
    prior = ref.prior_grad_var()
    sr = ref.score(c["Xq"], c["Yq"], SCORE_LG, c["sn2"])
    e = {"alpha": rel_max(alpha, ref.alpha_), "logdet": abs(logdet - ref.logdet) / max(abs(ref.logdet), 1.0),
         "lml": abs(lml - ref.lml()) / max(abs(ref.lml()), 1.0),
         "mean": rel_max(mean, mr), "var": rel_var(var, vr, 1e-6 * c["sf2"]), "mean_cov": rel_max(mean_c, mr),
         "cov": float(np.max(np.abs(cov - cr))) / c["sf2"],
         "dmean": rel_max(np.reshape(dm, (M, d, -1)), dmr), "dmean_only": rel_max(np.reshape(dm_only, (M, d, -1)), dmr),
         "dvar": rel_var(dv, dvr, 1e-6 * prior[None, :])}
    r = score_ratio(got_score, sr, 1e-10)
    print(f"{name}: " + " ".join(f"{k} {v:.2e}" for k, v in e.items()) + f" score error / bound {r:.3g}")
    assert all(v <= 1e-6 for v in e.values()), e
    assert r <= 1.0


@pytest.mark.parametrize("name", [n for n in PARITY if n.endswith("_last")])
def test_parity_fp32(name):
    c, ref = case(name)
    Xs, M, d = c["Xs"], len(c["Xs"]), c["Xs"].shape[1]
    f32 = lambda v: np.asarray(v, dtype=np.float32)  # noqa: E731
    with make_gp(c, dtype="float32") as gp:
        fit_case(gp, c, name, np.float32)
        logdet = gp.log_det_
        mean, var = gp.predict(f32(Xs))
        dm, dv = gp.predict_gradient(f32(Xs))
        dm_only = gp.predict_gradient(f32(Xs), return_var=False)
        got_score = gp.score_blocks(f32(c["Xq"]), f32(c["Yq"]), SCORE_LG, return_parts=True)
    assert mean.dtype == np.float32 and dv.dtype == np.float32
    mr, vr = ref.predict(Xs)
    dmr, dvr = ref.predict_grad(Xs)
    prior = ref.prior_grad_var()
    e = {"mean": rel_max(mean, mr), "var": float(np.max(np.abs(var - vr))) / c["sf2"],
         "logdet": abs(logdet - ref.logdet) / abs(ref.logdet),
         "dmean": rel_max(np.reshape(dm, (M, d, -1)), dmr), "dmean_only": rel_max(np.reshape(dm_only, (M, d, -1)), dmr),
         "dvar": float(np.max(np.abs(dv - dvr) / prior[None, :]))}
    r = score_ratio(got_score, ref.score(c["Xq"], c["Yq"], SCORE_LG, c["sn2"]), 1e-4)
    print(f"fp32 {name}: " + " ".join(f"{k} {v:.2e}" for k, v in e.items()) + f" score error / bound {r:.3g}")
    assert e["mean"] <= 2e-3 and e["var"] <= 2e-3 and e["logdet"] <= 1e-3
    assert e["dmean"] <= 5e-3 and e["dmean_only"] <= 5e-3 and e["dvar"] <= 5e-3
    assert r <= 1.0


def test_waypoints_with_exact_velocities():
    """five waypoints (w = 0) with exact velocities (derivative_noise = 0) at the same five times, d = 1"""
    c, ref = case("waypoints")
    Xs = c["Xs"]
    with make_gp(c) as gp:
        fit_case(gp, c, "waypoints")
        assert np.array_equal(gp.observation_kinds_, c["kinds"]) and np.array_equal(gp.noise_weights_, c["w"])
        mean, var, dm, dv = gp.predict_gradient(Xs, with_value=True)
        m0, v0 = gp.predict(Xs)
    mr, vr = ref.predict(Xs)
    dmr, dvr = ref.predict_grad(Xs)
    prior = ref.prior_grad_var()
    e = {"mean": rel_max(mean, mr), "predict": rel_max(m0, mr), "var": rel_var(var, vr, 1e-6 * c["sf2"]),
         "predict_var": rel_var(v0, vr, 1e-6 * c["sf2"]), "dmean": rel_max(dm[:, 0], dmr[:, 0, 0]),
         "dvar": rel_var(dv, dvr, 1e-6 * prior[None, :])}
    # what the constraints say: the curve passes through the waypoints (the first five queries) with the given velocities,
    # up to the jitter's share jitter |alpha_i| of an exact row's residual
    slack = c["jitter"] * np.max(np.abs(ref.alpha_))
    through = float(np.max(np.abs(mean[:5] - c["y"][30:])))
    speed = float(np.max(np.abs(dm[:5, 0] - c["yd"])))
    print("waypoints: " + " ".join(f"{k} {v:.2e}" for k, v in e.items()) +
          f" |mean - waypoint| {through:.2e} |velocity - given| {speed:.2e} (jitter |alpha| {slack:.2e})")
    assert all(v <= 1e-6 for v in e.values()), e
    assert through <= 2.0 * slack + 1e-6 * np.max(np.abs(mr)) and speed <= 2.0 * slack + 1e-6 * np.max(np.abs(dmr))


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_fit_predict_is_fit_then_predict(dtype):
    c, _ = case("matern52_d3_last")
    dt = np.float32 if dtype == "float32" else np.float64
    Xs = np.asarray(c["Xs"], dtype=dt)
    with make_gp(c, dtype=dtype) as gp:
        fit_case(gp, c, "matern52_d3_last", dt)
        m0, v0 = gp.predict(Xs)
        a0 = gp.alpha_.copy()
    with make_gp(c, dtype=dtype) as gp:
        a = lambda v: np.asarray(v, dtype=dt)  # noqa: E731
        m1, v1 = gp.fit_predict(a(c["X"]), a(c["y"]), Xs, derivatives=(a(c["Xd"]), c["dims"], a(c["yd"])),
                                derivative_noise=c["sn2_deriv"])
        assert np.array_equal(gp.observation_kinds_, c["kinds"])
        a1 = gp.alpha_
        m2, v2 = gp.predict(Xs)
    tol = 1e-9 if dtype == "float64" else 1e-3      # fp32: tests/test_fp32_gpu.py's level between its two routes
    em, ev, ea = rel_max(m1, np.float64(m0)), float(np.max(np.abs(np.float64(v1) - v0))) / c["sf2"], rel_max(a1, np.float64(a0))
    print(f"fit_predict {dtype}: mean {em:.2e} var {ev:.2e} alpha {ea:.2e}")
    assert em <= tol and ev <= tol and ea <= tol
    assert rel_max(m2, np.float64(m0)) <= tol


def test_kinds_all_minus_one_is_the_plain_fit():
    c, _ = case("rbf_d3_last")
    X, y, Xs, d = c["X"], c["y"], c["Xs"], c["X"].shape[1]
    with make_gp(c) as plain:
        plain.fit(X, y)
        want = (plain.alpha_.copy(), plain.log_det_) + plain.predict(Xs) + plain.predict_gradient(Xs)
        assert np.array_equal(plain.observation_kinds_, np.full(len(X), -1))
    with make_gp(c) as gp:
        gp.fit(X, y, derivatives=(np.empty((0, d)), np.empty((0,), dtype=np.int64), np.empty((0,) + y.shape[1:])))
        assert np.array_equal(gp.observation_kinds_, np.full(len(X), -1))
        got = (gp.alpha_.copy(), gp.log_det_) + gp.predict(Xs) + gp.predict_gradient(Xs)
        errs = [float(np.max(np.abs(np.asarray(a) - b)) / np.max(np.abs(b))) for a, b in zip(got, want)]
        print("kinds all -1 against the plain fit:", " ".join(f"{v:.2e}" for v in errs))
        assert max(errs) <= 1e-12
        gp.update(X[:3] + 0.01, y[:3])                                  # no derivative row: appends as the plain model does
        assert np.array_equal(gp.observation_kinds_, np.full(len(X) + 3, -1))
        # a fit with derivative rows on the same handle, then cleared by a fit without derivatives
        fit_case(gp, case("rbf_d3_last")[0], "rbf_d3_last")
        assert np.array_equal(gp.observation_kinds_, c["kinds"])
        gp.fit(X, y)
        again = (gp.alpha_.copy(), gp.log_det_) + gp.predict(Xs) + gp.predict_gradient(Xs)
        assert all(np.array_equal(a, b) for a, b in zip(again, want))   # bit-identical to a handle that never set kinds
        assert np.array_equal(gp.observation_kinds_, np.full(len(X), -1))


def test_bad_kinds_are_refused_and_the_previous_ones_stay():
    c, _ = case("rbf_d3_last")
    p = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    with make_gp(c) as gp:
        fit_case(gp, c, "rbf_d3_last")
        before = gp.predict(c["Xs"])
        lib, h = gp._lib, gp._h
        bad = c["kinds"].copy()
        bad[7] = -2
        assert lib.gpx_set_observation_kinds(h, p(bad), bad.size, 0.0, _abi.MEM_HOST) == _abi.E_ARG
        for s in (-1e-3, float("nan"), float("inf")):
            assert lib.gpx_set_observation_kinds(h, p(c["kinds"]), bad.size, s, _abi.MEM_HOST) == _abi.E_ARG
        info = C.c_int64(-5)
        ls = np.asarray(c["ls"], dtype=np.float64)

        def fit(X, y, N):
            return lib.gpx_fit(h, p(X), p(y), N, 3, 2, _abi.dptr(ls), 3, c["sf2"], c["sn2"], c["jitter"], _abi.MEM_HOST, C.byref(info))

        X, y = np.ascontiguousarray(c["Xall"]), np.ascontiguousarray(c["yall"])
        assert fit(X, y, len(X) - 1) == _abi.E_ARG and "observation kinds" in lib.gpx_last_error(h).decode()   # N != n
        big = c["kinds"].copy()
        big[250] = 3                                                                                            # a kind >= d
        assert lib.gpx_set_observation_kinds(h, p(big), big.size, 0.0, _abi.MEM_HOST) == 0
        assert fit(X, y, len(X)) == _abi.E_ARG and info.value == -5
        after = gp.predict(c["Xs"])
        assert all(np.array_equal(a, b) for a, b in zip(before, after))
        assert np.array_equal(gp.observation_kinds_, c["kinds"])         # the fit keeps the kinds it was made with
        # kinds from device memory
        import torch
        kd = torch.as_tensor(c["kinds"], device=f"cuda:{gp.device}")
        assert lib.gpx_set_observation_kinds(h, C.c_void_p(kd.data_ptr()), kd.numel(), c["sn2_deriv"], _abi.MEM_DEVICE) == 0
        assert fit(X, y, len(X)) == 0 and info.value == 0
        again = gp.predict(c["Xs"])
        assert all(np.array_equal(a, b) for a, b in zip(before, again))


REFUSED_FITS = {
    "matern12": dict(kernel="matern12"),
    "mixed": dict(dtype="mixed"),
    "group": dict(devices=1, transport="local"),
    "communicator": dict(device=0, world=1, rank=0, comm="rccl"),
}


@pytest.mark.parametrize("which", list(REFUSED_FITS))
def test_refused_fits_keep_the_previous_fit(which):
    c, _ = case("rbf_d1_last")
    kw = dict(REFUSED_FITS[which])
    kernel = kw.pop("kernel", c["kernel"])
    der = (c["Xd"], c["dims"], c["yd"])
    with GP(kernel, c["ls"], c["sf2"], c["sn2"], jitter=c["jitter"], **kw) as gp:
        gp.fit(c["X"], c["y"])
        before = gp.predict(c["Xs"])
        with pytest.raises(GpxError) as e:
            gp.fit(c["X"], c["y"], derivatives=der, derivative_noise=c["sn2_deriv"])
        assert e.value.code == _abi.E_UNSUPPORTED and str(e.value)
        with pytest.raises(GpxError) as e:
            gp.fit_predict(c["X"], c["y"], c["Xs"], derivatives=der, derivative_noise=c["sn2_deriv"])
        assert e.value.code == _abi.E_UNSUPPORTED
        # the refused fit computed nothing: the handle still holds the fit before (Python's own flag aside)
        mean, var = np.empty_like(before[0]), np.empty_like(before[1])
        rc = gp._lib.gpx_predict(gp._h, C.c_void_p(c["Xs"].ctypes.data), len(c["Xs"]), C.c_void_p(mean.ctypes.data),
                                 C.c_void_p(var.ctypes.data), _abi.MEM_HOST)
        assert rc == 0 and np.array_equal(mean, before[0]) and np.array_equal(var, before[1])
        if which == "matern12":                     # kinds that are all -1 are the plain model there
            d = c["X"].shape[1]
            gp.fit(c["X"], c["y"], derivatives=(np.empty((0, d)), 0, np.empty((0,))))
            assert np.array_equal(gp.observation_kinds_, np.full(len(c["X"]), -1))
        after = gp.fit(c["X"], c["y"]).predict(c["Xs"])                   # cleared: fits as before
        assert all(np.array_equal(a, b) for a, b in zip(before, after))


def test_refused_calls_on_a_derivative_fit():
    c, _ = case("rbf_d1_last")
    with make_gp(c) as gp:
        fit_case(gp, c, "rbf_d1_last")
        before = gp.predict(c["Xs"])
        for call in (gp.lml_gradient, lambda: gp.update(c["X"][:4] + 0.01, c["y"][:4]),
                     lambda: gp.update(c["X"][:4] + 0.01, c["y"][:4], noise_weights=np.ones(4))):
            with pytest.raises(GpxError) as e:
                call()
            assert e.value.code == _abi.E_UNSUPPORTED and "derivative" in str(e.value)
        after = gp.predict(c["Xs"])
        assert all(np.array_equal(a, b) for a, b in zip(before, after))
        assert gp._N == len(c["kinds"])


def test_bit_identical_under_stream_delays(gpx):
    c, _ = case("matern32_d3_mixed")

    def run():
        with make_gp(c) as gp:
            fit_case(gp, c, "matern32_d3_mixed")
            return ((gp.alpha_.copy(), np.float64(gp.log_det_)) + gp.predict(c["Xs"]) + gp.predict(c["Xs"], return_cov=True) +
                    gp.predict_gradient(c["Xs"], with_value=True) + gp.score_blocks(c["Xq"], c["Yq"], SCORE_LG, return_parts=True))

    want = run()
    try:
        for seed in (1, 7):
            gpx.gpx_debug_set_delay(seed)
            got = run()
            assert all(np.array_equal(a, b) for a, b in zip(got, want)), seed
    finally:
        gpx.gpx_debug_set_delay(0)


def test_device_tensors_and_optimize():
    import torch
    c, ref = case("matern52_d1_last")
    dev = torch.device("cuda:0")
    t = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float64), device=dev)  # noqa: E731
    with make_gp(c) as gp:
        gp.fit(t(c["X"]), t(c["y"]), derivatives=(t(c["Xd"]), c["dims"], t(c["yd"])), derivative_noise=c["sn2_deriv"])
        mean, var = gp.predict(t(c["Xs"]))
        mr, vr = ref.predict(c["Xs"])
        assert mean.is_cuda and rel_max(mean.cpu().numpy(), mr) <= 1e-6
        der = (c["Xd"], c["dims"], c["yd"])
        lml0 = gp.log_marginal_likelihood(c["y"], derivatives=der)
        assert abs(lml0 - ref.lml()) <= 1e-6 * abs(ref.lml())
        res = gp.optimize(c["X"], c["y"], maxiter=3, derivatives=der, derivative_noise=c["sn2_deriv"])
        lml1 = gp.log_marginal_likelihood(c["y"], derivatives=der)
        print(f"optimize with derivative observations: LML {lml0:.4f} -> {lml1:.4f} in {res.nfev} evaluations")
        assert lml1 >= lml0 and abs(-res.fun - lml1) <= 1e-9 * abs(lml1)
        assert np.array_equal(gp.observation_kinds_, c["kinds"])
