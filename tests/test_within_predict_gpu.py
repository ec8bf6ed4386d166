"""GPU: predicting an observed path itself, f + g_p (gpx_predict_paths, gpx_predict_cov_paths, gpx_sample_posterior_paths,
gpx_predict_grad_paths; GP.predict / predict_gradient / sample_y with ``path_ids=``) against the dense fp64 reference of
tests/within_predict_ref.py.

Shapes: ``within_ref.problem(P=12, L=33)``, N = 396 — seven 64-tiles whose id ranges straddle paths — with the rows sorted by
path and shuffled, and one d = 3 case with ARD lengthscales of both terms.  M = 70 and 200 query points with mixed ids.

Bounds.  Derivative matrices (gpx_kernel_path_grad_matrix): tests/test_within_gpu.py's matrix bounds scaled by the
derivative, 1e-12 (sf2 + sg2) / min l in fp64 and 1e-5 (sf2 + sg2) / min l in fp32 (min over l and l_path).  Values: that file's
predict bounds — mean 1e-6 of the largest entry, variance 1e-6 relative to max(|ref|, 1e-6 sf2); fp32 2e-3 and 2e-3 (sf2 +
sg2).  Gradient: tests/test_predict_grad_gpu.py's — dmean 1e-6 of the largest entry, dvar 1e-6 relative to max(|ref|, 1e-6
prior_j).  Between routes of one handle: 1e-9 (means) and 1e-10 (variances) of that file.  Leave-out / bring-back on the
device: the forecast bounds of tests/test_within_gpu.py, 1e-10 kappa max(1, resid) and 1e-10 kappa (sf2 + sg2).  Every test
prints its figures before it asserts."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest
from scipy.linalg import cholesky

from gaussianprocesspathmodelling_amd import GP, _abi
from gaussianprocesspathmodelling_amd._abi import GpxError

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import within_predict_ref as wpr  # noqa: E402
import within_ref as wr  # noqa: E402

pytestmark = pytest.mark.gpu

SF2, SG2, NOISE = 1.5, 0.4, 1e-2
DIFFERENTIABLE = ("rbf", "matern52", "matern32")
KERNELS = DIFFERENTIABLE + ("matern12",)


def rel_max(got, ref):
    return float(np.max(np.abs(np.asarray(got, dtype=np.float64) - ref)) / np.max(np.abs(ref)))


def rel_floor(got, ref, floor):
    return float(np.max(np.abs(np.asarray(got, dtype=np.float64) - ref) / np.maximum(np.abs(ref), floor)))


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


# ---- the derivative matrices ------------------------------------------------------------------------------------------
def _grad_matrix(kernel, dtype, A, ga, B, gb, ls, lsp, expect=0):
    lib = _abi.load()
    A, B = np.ascontiguousarray(A, dtype=np.float64), np.ascontiguousarray(B, dtype=np.float64)
    ga, gb = np.ascontiguousarray(ga, dtype=np.int32), np.ascontiguousarray(gb, dtype=np.int32)
    ls, lsp = np.ascontiguousarray(ls, dtype=np.float64), np.ascontiguousarray(lsp, dtype=np.float64)
    G = np.full((A.shape[1], len(A), len(B)), 7.0)
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))  # noqa: E731
    rc = lib.gpx_kernel_path_grad_matrix(_abi.KERNEL_IDS[kernel], _abi.DTYPE_IDS[dtype], _abi.dptr(A), ip(ga), len(A),
                                         _abi.dptr(B), ip(gb), len(B), A.shape[1], _abi.dptr(ls), ls.size, SF2, _abi.dptr(lsp),
                                         lsp.size, SG2, _abi.dptr(G))
    assert rc == expect
    return G


def _matrix_case(d, m, n, order):
    """m rows against n columns, 6 paths and some -1; 'sorted': runs of one id, rows ascending and columns descending, so
    most tiles cannot hold a same-path pair and take the plain path; 'shuffled': every tile can"""
    rng = np.random.default_rng(100 * d + m + n)
    A, B = rng.uniform(0.0, 1.0, (m, d)), rng.uniform(0.0, 1.0, (n, d))
    c = min(m, n, 40)
    B[:c] = A[:c] + 0.01 * rng.standard_normal((c, d))                 # close pairs ...
    B[0] = A[0]                                                        # ... and a coincident one, on one path
    ga, gb = rng.integers(-1, 6, m), rng.integers(-1, 6, n)
    gb[:c] = ga[:c]
    ga[0] = gb[0] = 2
    if order == "sorted":
        ia, ib = np.argsort(ga, kind="stable"), np.argsort(-gb, kind="stable")
        A, ga, B, gb = A[ia], ga[ia], B[ib], gb[ib]
    ls = np.linspace(0.3, 0.6, d) if d > 1 else np.array([0.3])
    lsp = np.linspace(0.2, 0.1, d) if d > 1 else np.array([0.1])
    return A, ga, B, gb, ls, lsp


SIZES = ((1, 1), (63, 65), (65, 63), (130, 130), (1, 130), (130, 1))


@pytest.mark.parametrize("d", [1, 2, 3, 5])
@pytest.mark.parametrize("kernel", DIFFERENTIABLE)
def test_kernel_path_grad_matrix_fp64(kernel, d):
    worst, pairs = 0.0, 0
    for m, n in SIZES:
        for order in ("shuffled", "sorted"):
            A, ga, B, gb, ls, lsp = _matrix_case(d, m, n, order)
            got = _grad_matrix(kernel, "float64", A, ga, B, gb, ls, lsp)
            ref = wpr.path_cov_dx(A, ga, B, gb, kernel, ls, SF2, lsp, SG2)
            pairs += int(((ga[:, None] == gb[None, :]) & (ga[:, None] >= 0)).sum())
            e = float(np.max(np.abs(got - ref))) * min(ls.min(), lsp.min()) / (SF2 + SG2)
            worst = max(worst, e)
    print(f"path grad matrix fp64 {kernel} d={d}: error min(l) / (sf2 + sg2) {worst:.2e} ({pairs} same-path pairs)")
    assert pairs > 1000 and worst <= 1e-12


@pytest.mark.parametrize("d", [1, 2, 3, 5])
@pytest.mark.parametrize("kernel", DIFFERENTIABLE)
def test_kernel_path_grad_matrix_fp32(kernel, d):
    worst = 0.0
    f = lambda a: np.asarray(a, dtype=np.float32).astype(np.float64)  # noqa: E731  (the inputs the fp32 builder sees)
    for m, n in SIZES:
        for order in ("shuffled", "sorted"):
            A, ga, B, gb, ls, lsp = _matrix_case(d, m, n, order)
            got = _grad_matrix(kernel, "float32", A, ga, B, gb, ls, lsp)
            ref = wpr.path_cov_dx(f(A), ga, f(B), gb, kernel, ls, SF2, lsp, SG2)
            worst = max(worst, float(np.max(np.abs(got - ref))) * min(ls.min(), lsp.min()) / (SF2 + SG2))
    print(f"path grad matrix fp32 {kernel} d={d}: error min(l) / (sf2 + sg2) {worst:.2e}")
    assert worst <= 1e-5


def test_kernel_path_grad_matrix_without_a_same_path_pair_is_the_plain_matrix():
    A, ga, B, gb, ls, lsp = _matrix_case(3, 130, 130, "shuffled")
    lib = _abi.load()
    plain = np.empty((3, 130, 130))
    assert lib.gpx_kernel_deriv_matrix(_abi.KERNEL_IDS["matern32"], _abi.dptr(A), 130, _abi.dptr(B), 130, 3, _abi.dptr(ls), 3,
                                       SF2, _abi.dptr(plain)) == 0
    assert np.array_equal(_grad_matrix("matern32", "float64", A, np.full(130, -1), B, gb, ls, lsp), plain)
    assert np.array_equal(_grad_matrix("matern32", "float64", A, ga + 100, B, gb, ls, lsp), plain)   # no range overlap
    assert np.all(plain[:, 0, 0] == 0.0)                                     # the coincident pair: no slope
    # Tile by tile: a 64 x 64 tile whose row and column id ranges do not overlap is the plain build's bit for bit; on the
    # others a pair of two paths gets no second term (equal to rounding: those tiles sum r^2 beside r_path^2)
    lo = lambda g: g[g >= 0].min() if np.any(g >= 0) else np.iinfo(np.int64).max  # noqa: E731
    for order in ("shuffled", "sorted"):
        A, ga, B, gb, ls, lsp = _matrix_case(3, 130, 130, order)
        assert lib.gpx_kernel_deriv_matrix(_abi.KERNEL_IDS["matern32"], _abi.dptr(A), 130, _abi.dptr(B), 130, 3, _abi.dptr(ls),
                                           3, SF2, _abi.dptr(plain)) == 0
        got = _grad_matrix("matern32", "float64", A, ga, B, gb, ls, lsp)
        same = np.broadcast_to((ga[:, None] == gb[None, :]) & (ga[:, None] >= 0), got.shape)
        tiles = {True: 0, False: 0}
        for i0 in range(0, 130, 64):
            for j0 in range(0, 130, 64):
                ra, rb = ga[i0:i0 + 64], gb[j0:j0 + 64]
                overlap = bool(lo(ra) <= rb.max() and lo(rb) <= ra.max())
                tiles[overlap] += 1
                if not overlap:
                    assert np.array_equal(got[:, i0:i0 + 64, j0:j0 + 64], plain[:, i0:i0 + 64, j0:j0 + 64]), (order, i0, j0)
        print(f"{order}: {tiles[False]} of 9 tiles cannot hold a same-path pair")
        assert np.max(np.abs(got[~same] - plain[~same])) <= 1e-12 * (SF2 + SG2) / lsp.min()
        assert np.any(got[same] != plain[same])
        assert order != "shuffled" or np.all(got[:, 0, 0] == 0.0)           # (rows and columns 0: the coincident pair)
    assert tiles[False] >= 2                                                 # 'sorted': runs of one id
    G = _grad_matrix("matern12", "float64", A, ga, B, gb, ls, lsp, expect=_abi.E_UNSUPPORTED)
    assert np.all(G == 7.0)


# ---- the posterior ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _case(name):
    """'sorted': 12 x 33, d = 1, ids in runs.  'shuffled': the same rows in random order.  'ard3': d = 3, ARD lengthscales of
    both terms, rows shuffled.  Each with the query points (200; the first 70 serve as the small call) and their ids:
    training ids, -1, a fresh id (99) and id 0 mixed."""
    if name == "ard3":
        p = wr.problem(P=12, L=33, seed=4, d=3, ls=(0.25, 0.5, 0.6), ls_path=(0.1, 0.2, 0.3))
        p.update(ls=np.array([0.25, 0.5, 0.6]), lsp=np.array([0.1, 0.2, 0.3]))
    else:
        p = wr.problem(P=12, L=33, seed=3)
        p.update(ls=np.array([0.25]), lsp=np.array([0.1]))
    rng = np.random.default_rng(11)
    if name != "sorted":
        perm = rng.permutation(len(p["X"]))
        p.update(X=np.ascontiguousarray(p["X"][perm]), Y=np.ascontiguousarray(p["Y"][perm]),
                 ids=np.ascontiguousarray(p["ids"][perm]))
    d = p["X"].shape[1]
    Xq = p["X"][rng.choice(len(p["X"]), 200, replace=False)] + 0.01 * rng.standard_normal((200, d))
    gq = rng.choice(np.array([-1, 0, 3, 7, 11, 99]), 200).astype(np.int32)
    gq[:6] = (3, -1, 99, 0, 3, 11)
    p.update(Xq=np.ascontiguousarray(Xq), gq=gq)
    return p


def _gp(p, kernel="matern32", dtype="float64", noise=NOISE, **kw):
    return GP(kernel, p["ls"], SF2, noise, dtype=dtype, **kw)


def _fit(gp, p, dt=np.float64, rows=slice(None)):
    return gp.fit(p["X"][rows].astype(dt), p["Y"][rows].astype(dt), path_ids=p["ids"][rows], path_variance=SG2,
                  path_lengthscale=p["lsp"])


def _ref(p, kernel, noise, jitter):
    return wr.fit_ref(p["X"], p["ids"], p["Y"], kernel, p["ls"], SF2, noise, p["lsp"], SG2, jitter=jitter)


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("name", ["sorted", "shuffled", "ard3"])
def test_values_fp64(name, kernel):
    p = _case(name)
    with _gp(p, kernel) as gp:
        _fit(gp, p)
        jit = gp.jitter_used_
        ref = _ref(p, kernel, NOISE, jit)
        for M in (70, 200):
            Xq, gq = p["Xq"][:M], p["gq"][:M]
            mean, var = gp.predict(Xq, path_ids=gq)
            mean_only = gp.predict(Xq, return_var=False, path_ids=gq)
            mean_c, cov = gp.predict(Xq, return_cov=True, path_ids=gq)
            mr, cr = wpr.predict_path(ref, Xq, gq)
            e = {"mean": rel_max(mean, mr), "var": rel_floor(var, np.diag(cr), 1e-6 * SF2),
                 "cov": float(np.max(np.abs(cov - cr))) / (SF2 + SG2), "mean_only": rel_max(mean_only, np.asarray(mean)),
                 "mean_cov": rel_max(mean_c, np.asarray(mean)),
                 "diag": float(np.max(np.abs(np.diag(cov) - var))) / (SF2 + SG2)}
            print(f"values fp64 {name} {kernel} M={M}: " + " ".join(f"{k} {v:.2e}" for k, v in e.items()))
            assert mean.shape == (M, 2) and var.shape == (M,) and cov.shape == (M, M)
            assert e["mean"] <= 1e-6 and e["var"] <= 1e-6 and e["cov"] <= 1e-6
            assert e["mean_only"] <= 1e-9 and e["mean_cov"] <= 1e-9 and e["diag"] <= 1e-10
            assert np.array_equal(cov, cov.T), "cov is not exactly symmetric"
            # the ids mean something: a training path is known better than f at its own points, a fresh one worse
            vf = gp.predict(Xq)[1]
            assert np.all(var[gq == -1] == vf[gq == -1]) and np.all(var[gq == 99] > vf[gq == 99] + 0.5 * SG2)


@pytest.mark.parametrize("name", ["sorted", "ard3"])
def test_values_fp32(name):
    p = _case(name)
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)  # noqa: E731
    with _gp(p, dtype="float32", noise=5e-2) as gp:
        _fit(gp, p, np.float32)
        jit = gp.jitter_used_
        mean, var = gp.predict(f32(p["Xq"]), path_ids=p["gq"])
        _, cov = gp.predict(f32(p["Xq"]), return_cov=True, path_ids=p["gq"])
        dm, dv = gp.predict_gradient(f32(p["Xq"]), path_ids=p["gq"])
    assert mean.dtype == np.float32 and cov.dtype == np.float32 and dm.dtype == np.float32
    ref = _ref(p, "matern32", 5e-2, jit)
    mr, cr = wpr.predict_path(ref, p["Xq"], p["gq"])
    dmr, dvr = wpr.predict_path_grad(ref, p["Xq"], p["gq"])
    prior = wpr.grad_priors(ref, p["gq"], p["X"].shape[1])
    e = {"mean": rel_max(mean, mr), "var": float(np.max(np.abs(var - np.diag(cr)))) / (SF2 + SG2),
         "cov": float(np.max(np.abs(cov - cr))) / (SF2 + SG2), "dmean": rel_max(dm, dmr),
         "dvar": float(np.max(np.abs(dv - dvr) / prior))}
    print(f"values fp32 {name}: " + " ".join(f"{k} {v:.2e}" for k, v in e.items()))
    assert e["mean"] <= 2e-3 and e["var"] <= 2e-3 and e["cov"] <= 2e-3
    assert e["dmean"] <= 5e-3 and e["dvar"] <= 5e-3                       # tests/test_predict_grad_gpu.py's fp32 level


# ---- routes -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fitted():
    p = _case("shuffled")
    with _gp(p) as gp:
        yield _fit(gp, p), p


def test_ids_all_minus_one_take_the_plain_route_bit_for_bit(fitted):
    gp, p = fitted
    Xq, none = p["Xq"], np.full(200, -1, dtype=np.int32)
    z = np.random.default_rng(1).standard_normal((3, 200, 2))
    before = gp.predict(Xq)
    assert _same(gp.predict(Xq, path_ids=none), before) and _same(gp.predict(Xq, path_ids=-1), before)
    assert np.array_equal(gp.predict(Xq, return_var=False, path_ids=none), gp.predict(Xq, return_var=False))
    assert _same(gp.predict(Xq, return_cov=True, path_ids=none), gp.predict(Xq, return_cov=True))
    assert _same(gp.predict_gradient(Xq, with_value=True, path_ids=none), gp.predict_gradient(Xq, with_value=True))
    assert _same(gp.predict_gradient(Xq, path_ids=none), gp.predict_gradient(Xq))
    assert np.array_equal(gp.sample_y(Xq, 3, z=z, include_noise=True, path_ids=none),
                          gp.sample_y(Xq, 3, z=z, include_noise=True))
    # without variances the ids take the batch route, the plain call the matrix-free product: equal to rounding
    a, b = gp.predict_gradient(Xq, return_var=False, path_ids=none), gp.predict_gradient(Xq, return_var=False)
    assert np.max(np.abs(a - b)) <= 1e-9 * np.max(np.abs(b))
    gp.predict(Xq, path_ids=p["gq"])
    gp.predict(Xq, return_cov=True, path_ids=p["gq"])
    gp.predict_gradient(Xq, path_ids=p["gq"])
    assert _same(gp.predict(Xq), before), "predict changed after calls with path ids"


def test_batches_give_the_same_bits(fitted, monkeypatch):
    gp, p = fitted
    rng = np.random.default_rng(2)
    Xq = np.concatenate([p["Xq"], p["Xq"][:100] + 0.003])
    gq = np.concatenate([p["gq"], rng.permutation(p["gq"])[:100]])
    a = gp.predict(Xq, path_ids=gq) + gp.predict_gradient(Xq, with_value=True, path_ids=gq)
    monkeypatch.setenv("GPX_PRED_BATCH", "128")
    b = gp.predict(Xq, path_ids=gq) + gp.predict_gradient(Xq, with_value=True, path_ids=gq)
    assert _same(a, b)


def test_a_point_does_not_depend_on_the_other_points(fitted):
    gp, p = fitted
    Xq, gq = p["Xq"], p["gq"]
    mean, var = gp.predict(Xq, path_ids=gq)
    m4, v4, dm, dv = gp.predict_gradient(Xq, with_value=True, path_ids=gq)
    for i in (0, 63, 64, 131, 199):
        m1, v1 = gp.predict(Xq[i:i + 1], path_ids=gq[i:i + 1])
        assert np.array_equal(m1[0], mean[i]) and v1[0] == var[i], i
        a = gp.predict_gradient(Xq[i:i + 1], with_value=True, path_ids=int(gq[i]))
        assert _same([x[0] for x in a], (m4[i], v4[i], dm[i], dv[i])), i
    m65, v65 = gp.predict(Xq[:65], path_ids=gq[:65])
    assert np.array_equal(m65, mean[:65]) and np.array_equal(v65, var[:65])


# ---- the gradient -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", DIFFERENTIABLE)
@pytest.mark.parametrize("name", ["sorted", "shuffled", "ard3"])
def test_gradient_fp64(name, kernel):
    p = _case(name)
    d = p["X"].shape[1]
    with _gp(p, kernel) as gp:
        _fit(gp, p)
        ref = _ref(p, kernel, NOISE, gp.jitter_used_)
        for M in (70, 200):
            Xq, gq = p["Xq"][:M], p["gq"][:M]
            m0, v0 = gp.predict(Xq, path_ids=gq)
            dm, dv = gp.predict_gradient(Xq, path_ids=gq)
            mean, var, dm2, dv2 = gp.predict_gradient(Xq, with_value=True, path_ids=gq)
            dm_only = gp.predict_gradient(Xq, return_var=False, path_ids=gq)
            mo, dmo = gp.predict_gradient(Xq, return_var=False, with_value=True, path_ids=gq)
            dmr, dvr = wpr.predict_path_grad(ref, Xq, gq)
            prior = wpr.grad_priors(ref, gq, d)
            em, ev = rel_max(dm, dmr), float(np.max(np.abs(dv - dvr) / np.maximum(np.abs(dvr), 1e-6 * prior)))
            print(f"gradient fp64 {name} {kernel} M={M}: dmean {em:.2e} (of max) dvar rel {ev:.2e}")
            assert dm.shape == (M, d, 2) and dv.shape == (M, d)
            assert em <= 1e-6 and ev <= 1e-6
            scale = np.max(np.abs(dm))
            assert np.max(np.abs(dm_only - dm)) <= 1e-9 * scale and np.max(np.abs(dmo - dm)) <= 1e-9 * scale
            assert np.max(np.abs(dm2 - dm)) <= 1e-9 * scale and np.max(np.abs(dv2 - dv)) <= 1e-10 * np.max(prior)
            assert np.max(np.abs(mean - m0)) <= 1e-9 * np.max(np.abs(m0)) and np.max(np.abs(mo - m0)) <= 1e-9 * np.max(np.abs(m0))
            assert np.max(np.abs(var - v0)) <= 1e-10 * (SF2 + SG2)


def test_gradient_on_matern12_is_refused():
    p = _case("sorted")
    with _gp(p, "matern12") as gp:
        _fit(gp, p)
        before = gp.predict(p["Xq"], path_ids=p["gq"])
        with pytest.raises(GpxError, match="not differentiable") as ei:
            gp.predict_gradient(p["Xq"], path_ids=p["gq"])
        assert ei.value.code == _abi.E_UNSUPPORTED
        assert _same(gp.predict(p["Xq"], path_ids=p["gq"]), before)


# ---- leave a path out, bring it back: the library on both sides --------------------------------------------------------
@pytest.mark.parametrize("name", ["sorted", "shuffled"])
def test_forecast_of_a_left_out_path_is_the_prediction_of_that_path(name):
    p = _case(name)
    mine = p["ids"] == 3
    tq = np.linspace(0.03, 0.97, 13).reshape(-1, 1)
    with _gp(p) as gp:
        _fit(gp, p, rows=~mine)
        jit = gp.jitter_used_
        fm, fc = gp.forecast_blocks(p["X"][mine], p["Y"][mine], tq, blocks=1, include_noise=True)
        _fit(gp, p)
        assert gp.jitter_used_ == jit
        mean, cov = gp.predict(tq, path_ids=3, return_cov=True)
    rest = wr.fit_ref(p["X"][~mine], p["ids"][~mine], p["Y"][~mine], "matern32", p["ls"], SF2, NOISE, p["lsp"], SG2, jitter=jit)
    sch = wr.forecast_schur(rest, p["X"][mine], p["Y"][mine], tq, 1, NOISE)       # kappa and the residual of the bounds
    kappa, resid = float(sch["kappa"][0]), float(sch["resid"][0])
    em, ec = float(np.max(np.abs(fm - mean))), float(np.max(np.abs(fc[0] - cov)))
    bm, bc = 1e-10 * kappa * max(1.0, resid), 1e-10 * kappa * (SF2 + SG2)
    print(f"leave out / bring back {name}: mean {em:.2e} (bound {bm:.2e}) cov {ec:.2e} (bound {bc:.2e}) kappa {kappa:.4g}")
    assert em <= bm and ec <= bc


# ---- samples ----------------------------------------------------------------------------------------------------------
def test_samples_are_mean_plus_factor_times_z(fitted):
    gp, p = fitted
    Xq, gq = p["Xq"][:70], p["gq"][:70]
    z = np.random.default_rng(3).standard_normal((5, 70, 2))
    out = gp.sample_y(Xq, 5, include_noise=True, z=z, path_ids=gq)
    j = gp.sample_jitter_
    mean, cov = gp.predict(Xq, return_cov=True, path_ids=gq)
    Ls = cholesky(cov + (NOISE + j) * np.eye(70), lower=True)
    ref = mean[:, :, None] + np.einsum("mn,snc->mcs", Ls, z)
    e = float(np.max(np.abs(out - ref))) / float(np.max(np.abs(ref)))
    print(f"samples with path ids: {e:.2e} (of max), jitter {j:.2e}")
    assert out.shape == (70, 2, 5) and e <= 1e-9             # tests/test_posterior_gpu.py's bound of the plain call
    plain = gp.sample_y(Xq, 5, include_noise=True, z=z)
    assert np.max(np.abs(out - plain)) > 0.1                  # ... and they are samples of the paths, not of f


# ---- after an append --------------------------------------------------------------------------------------------------
def test_a_path_that_came_with_an_update_is_predicted_as_in_a_fit_of_all_rows():
    p = _case("sorted")
    old = p["ids"] < 8
    Xq, gq = p["Xq"], np.where(p["gq"] == 3, 10, p["gq"]).astype(np.int32)
    with _gp(p) as gp:
        _fit(gp, p, rows=old)
        gp.update(p["X"][~old], p["Y"][~old], path_ids=p["ids"][~old])
        assert np.array_equal(gp.path_ids_, p["ids"])
        m1, v1 = gp.predict(Xq, path_ids=10)
        m2, v2 = gp.predict(Xq, path_ids=gq)
        dm, dv = gp.predict_gradient(Xq, path_ids=gq)
        with _gp(p) as full:
            _fit(full, p)
            f1, f2 = full.predict(Xq, path_ids=10), full.predict(Xq, path_ids=gq)
            fdm, fdv = full.predict_gradient(Xq, path_ids=gq)
            vf = full.predict(Xq)[1]
    e = {"mean10": rel_floor(m1, f1[0], 1e-6), "var10": rel_floor(v1, f1[1], 1e-6 * SF2), "mean": rel_floor(m2, f2[0], 1e-6),
         "var": rel_floor(v2, f2[1], 1e-6 * SF2), "dmean": rel_max(dm, fdm), "dvar": rel_max(dv, fdv)}
    print("after an update: " + " ".join(f"{k} {v:.2e}" for k, v in e.items()))
    assert all(v <= 1e-9 for v in e.values()), e
    near = np.abs(Xq[:, 0][:, None] - p["X"][p["ids"] == 10][:, 0][None, :]).min(axis=1) < 0.005
    assert near.sum() > 3 and np.all(v1[near] < vf[near])    # path 10 is known, not fresh: surer than f near its points


# ---- refusals ---------------------------------------------------------------------------------------------------------
def _calls(gp, Xq, ids):
    z = np.zeros((1, len(Xq), 2))
    return [lambda: gp.predict(Xq, path_ids=ids), lambda: gp.predict(Xq, return_var=False, path_ids=ids),
            lambda: gp.predict(Xq, return_cov=True, path_ids=ids), lambda: gp.predict_gradient(Xq, path_ids=ids),
            lambda: gp.sample_y(Xq, 1, z=z, path_ids=ids)]


def test_fits_without_path_ids_and_bad_ids_are_refused():
    p = _case("sorted")
    Xq, gq = p["Xq"][:70], p["gq"][:70]
    with _gp(p) as gp:
        gp.fit(p["X"], p["Y"])
        before = gp.predict(Xq) + gp.predict_gradient(Xq)
        for call in _calls(gp, Xq, gq) + _calls(gp, Xq, -1):
            with pytest.raises(GpxError, match="path ids") as ei:
                call()
            assert ei.value.code == _abi.E_UNSUPPORTED
        assert _same(gp.predict(Xq) + gp.predict_gradient(Xq), before)
        gp.fit(p["X"], p["Y"], path_ids=p["ids"], path_variance=0.0, path_lengthscale=p["lsp"])    # the plain model
        for call in _calls(gp, Xq, gq):
            with pytest.raises(GpxError, match="path ids") as ei:
                call()
            assert ei.value.code == _abi.E_UNSUPPORTED
        assert _same(gp.predict(Xq) + gp.predict_gradient(Xq), before)
        _fit(gp, p)
        before = gp.predict(Xq, path_ids=gq) + gp.predict(Xq)
        bad = gq.copy()
        bad[37] = -2
        for call in _calls(gp, Xq, bad) + _calls(gp, Xq, -2):
            with pytest.raises(GpxError, match="below -1") as ei:
                call()
            assert ei.value.code == _abi.E_ARG
        for wrong in (gq[:69], gq.astype(np.float64), np.zeros((70, 1), dtype=np.int32)):
            with pytest.raises(ValueError):
                gp.predict(Xq, path_ids=wrong)
        assert _same(gp.predict(Xq, path_ids=gq) + gp.predict(Xq), before)
        null = gp._lib.gpx_predict_paths(gp._h, C.c_void_p(Xq.ctypes.data), None, 70, C.c_void_p(before[0].ctypes.data), None,
                                         _abi.MEM_HOST)
        assert null == _abi.E_ARG and _same(gp.predict(Xq, path_ids=gq) + gp.predict(Xq), before)


# ---- device tensors ---------------------------------------------------------------------------------------------------
def test_device_tensors_in_device_tensors_out(fitted):
    torch = pytest.importorskip("torch")
    gp, p = fitted
    Xq, gq = p["Xq"], p["gq"]
    dev = torch.device("cuda", gp.device)
    tX, tg = torch.as_tensor(Xq, device=dev), torch.as_tensor(gq, device=dev)
    z = np.random.default_rng(5).standard_normal((2, 200, 2))
    host = gp.predict(Xq, path_ids=gq) + gp.predict(Xq, return_cov=True, path_ids=gq) + \
        gp.predict_gradient(Xq, with_value=True, path_ids=gq) + (gp.sample_y(Xq, 2, z=z, include_noise=True, path_ids=gq),)
    for ids in (tg, gq, tg.cpu()):                            # ids as a device tensor, an array, a host tensor
        got = gp.predict(tX, path_ids=ids) + gp.predict(tX, return_cov=True, path_ids=ids) + \
            gp.predict_gradient(tX, with_value=True, path_ids=ids) + \
            (gp.sample_y(tX, 2, z=z, include_noise=True, path_ids=ids),)
        assert all(t.is_cuda for t in got)
        assert _same([t.cpu().numpy() for t in got], host)
    bad = tg.clone()
    bad[5] = -7
    with pytest.raises(GpxError, match="below -1"):
        gp.predict(tX, path_ids=bad)
