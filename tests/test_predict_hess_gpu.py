"""GPU: the posterior second derivatives — ``GP.predict_hessian`` (gpx_predict_hess) and ``gpx_kernel_hess_matrix`` —
against the fp64 closed-form reference (tests/hess_ref.py), against finite differences of the GPU's own
``predict_gradient``, and for internal consistency (two routes, batching, device tensors, no side effects, refusals)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from gaussianprocesspathmodelling_amd import GP, GpxError, _abi
from oracle.gp_oracle import synthetic_problem

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from deriv_ref import lengthscales  # noqa: E402
from dobs_ref import DobsGP  # noqa: E402
from hess_ref import (expand, hess_ref, hess_ref_kinds, kernel_hess, kinds_hess, pairs,  # noqa: E402
                      prior_hess_var)

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KERNELS = ("rbf", "matern52")
# fp32: the project's bound for fp32 posteriors, of the largest |hmean| and of the prior (DESIGN.md §3.4p has the measured errors)
FP32_TOL = 5e-3


def golden_case(name):
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    ls = g["lengthscale"]
    return (g["X"], g["y"], g["Xs"], str(g["kernel"]), ls[0] if ls.size == 1 else ls, float(g["variance"]),
            float(g["noise"]), float(g["jitter"]))


def synthetic_case(N, d, M, k, kernel, ls, seed):
    X, y, Xs = synthetic_problem(N, d, M, seed=seed)
    if k == 2:
        y = np.stack([y, np.cos(2.0 * X.sum(axis=1))], axis=1)
    return X, y, Xs, kernel, ls, 1.5, 1e-2, 1.5e-10


# the smallest shapes that cross every boundary: one query point; N and M no multiples of the tile, ARD, two targets; more
# than one 128-row batch tile and d = 3; d = 5, the runtime-d kernels
SHAPES = {
    "d1_M1_k1": (1000, 1, 1, 1, 0.3, 3),
    "ard_d2_M77_k2": (777, 2, 77, 2, (0.3, 0.2), 4),
    "ard_d3_M300_k2": (1500, 3, 300, 2, (0.3, 0.2, 0.25), 5),
    "d5_M100_k1": (900, 5, 100, 1, 0.5, 9),
}
CASES = {n: (lambda n=n: golden_case(n)) for n in ("G1", "G2", "G3")}
for _kernel in KERNELS:
    for _name, (_N, _d, _M, _k, _ls, _seed) in SHAPES.items():
        CASES[f"{_kernel}_{_name}"] = (lambda a=(_N, _d, _M, _k, _kernel, _ls, _seed): synthetic_case(*a))


@pytest.fixture(scope="module")
def refs():
    cache = {}

    def get(name):
        if name not in cache:
            c = CASES[name]()
            cache[name] = c + (hess_ref(*c),)
        return cache[name]
    return get


def as_mpk(a, M, d2):
    return np.asarray(a).reshape(M, d2, -1)


def errors(hm, hv, hmr, hvr, prior):
    M, d2 = hvr.shape
    em = np.max(np.abs(as_mpk(hm, M, d2) - hmr)) / np.max(np.abs(hmr))
    ev = np.max(np.abs(hv - hvr) / np.maximum(np.abs(hvr), 1e-6 * prior[None, :]))
    return em, ev


@pytest.mark.parametrize("name", list(CASES))
def test_hessian_fp64(refs, name):
    X, y, Xs, kernel, ls, sf2, sn2, jit, (hmr, hvr) = refs(name)
    M, d = Xs.shape
    d2 = d * (d + 1) // 2
    prior = prior_hess_var(kernel, ls, sf2, d)
    with GP(kernel, ls, sf2, sn2, jitter=jit) as gp:
        gp.fit(X, y)
        m0, v0 = gp.predict(Xs)
        hm, hv = gp.predict_hessian(Xs)
        hm_only = gp.predict_hessian(Xs, return_var=False)                  # the matrix-free route
        hm2, hv2 = gp.predict_hessian(Xs)
        hm_only2 = gp.predict_hessian(Xs, return_var=False)
        hf, hvf = gp.predict_hessian(Xs, full=True)
        m1, v1 = gp.predict(Xs)
    k = 1 if np.ndim(y) == 1 else y.shape[1]
    assert hm.shape == ((M, d2) if np.ndim(y) == 1 else (M, d2, k)) and hv.shape == (M, d2)
    assert hm.dtype == np.float64 and hv.dtype == np.float64 and hm_only.shape == hm.shape
    em, ev = errors(hm, hv, hmr, hvr, prior)
    print(f"{name}: N={len(X)} M={M} d={d} k={k} hmean err {em:.2e} (of max), hvar rel err {ev:.2e}")
    assert em <= 1e-6 and ev <= 1e-6
    assert np.max(np.abs(hm_only - hm)) <= 1e-9 * np.max(np.abs(hm))       # matrix-free = z^T V route
    assert np.array_equal(hm2, hm) and np.array_equal(hv2, hv) and np.array_equal(hm_only2, hm_only)   # reproducible
    assert np.array_equal(m0, m1) and np.array_equal(v0, v1)                # the fit is only read
    assert hf.shape == (M, d, d) + hm.shape[2:] and hvf.shape == (M, d, d)
    assert np.array_equal(hf, expand(hm, d)) and np.array_equal(hvf, expand(hv, d))
    assert np.array_equal(hf, np.swapaxes(hf, 1, 2))


@pytest.mark.parametrize("name", list(CASES))
def test_hessian_fp32(refs, name):
    X, y, Xs, kernel, ls, sf2, sn2, jit, (hmr, hvr) = refs(name)
    M, d = Xs.shape
    d2 = d * (d + 1) // 2
    prior = prior_hess_var(kernel, ls, sf2, d)
    with GP(kernel, ls, sf2, sn2, jitter=jit, dtype="float32") as gp:
        gp.fit(X, y)
        hm, hv = gp.predict_hessian(Xs)
        hmo = gp.predict_hessian(Xs, return_var=False)
    assert hm.dtype == np.float32 and hv.dtype == np.float32
    em = np.max(np.abs(as_mpk(hm, M, d2) - hmr)) / np.max(np.abs(hmr))
    emo = np.max(np.abs(as_mpk(hmo, M, d2) - hmr)) / np.max(np.abs(hmr))
    ev = np.max(np.abs(hv - hvr) / prior[None, :])
    print(f"fp32 {name}: hmean err {em:.2e} / matrix-free {emo:.2e} (of max), hvar err {ev:.2e} (of prior)")
    assert em <= FP32_TOL and emo <= FP32_TOL and ev <= FP32_TOL


def test_against_finite_differences_of_predict_gradient():
    X, y, Xs = synthetic_problem(800, 2, 40, seed=12)
    ls = (0.35, 0.25)
    l = lengthscales(ls, 2)
    with GP("rbf", ls, 1.3, 1e-2) as gp:
        gp.fit(X, y)
        H = gp.predict_hessian(Xs, return_var=False, full=True)            # (M, d, d)
        for j in range(2):
            h = 1e-3 * l[j]
            Xp, Xm = Xs.copy(), Xs.copy()
            Xp[:, j] += h
            Xm[:, j] -= h
            fd = (gp.predict_gradient(Xp, return_var=False) - gp.predict_gradient(Xm, return_var=False)) / (2 * h)
            for i in range(2):
                err = np.max(np.abs(fd[:, i] - H[:, i, j])) / np.max(np.abs(H[:, i, j]))
                print(f"H[{i}][{j}]: finite-difference err {err:.2e} (of max)")
                assert err <= 1e-5


@pytest.mark.parametrize("kernel", KERNELS)
def test_far_query_returns_the_prior(kernel):
    X, y, Xs = synthetic_problem(500, 2, 20, seed=14)
    ls = (0.3, 0.2)
    far = np.array([[1.0 + 20 * 0.3, 1.0 + 20 * 0.2]])                     # 20 l beyond the unit box in every dimension
    prior = prior_hess_var(kernel, ls, 1.4, 2)
    with GP(kernel, ls, 1.4, 1e-2) as gp:
        gp.fit(X, y)
        hm_in = gp.predict_hessian(Xs, return_var=False)
        hm, hv = gp.predict_hessian(far)
        hmo = gp.predict_hessian(far, return_var=False)
    scale = np.max(np.abs(hm_in))
    print(f"{kernel}: far |hmean| / inside {np.max(np.abs(hm)) / scale:.2e}, hvar / prior - 1 {np.max(np.abs(hv[0] / prior - 1)):.2e}")
    assert np.max(np.abs(hv[0] - prior) / prior) <= 1e-12
    assert np.max(np.abs(hm)) <= 1e-12 * scale and np.max(np.abs(hmo)) <= 1e-12 * scale


def test_batched_equals_unbatched(refs, monkeypatch):
    X, y, Xs, kernel, ls, sf2, sn2, jit, _ = refs("rbf_ard_d3_M300_k2")
    with GP(kernel, ls, sf2, sn2, jitter=jit) as gp:
        gp.fit(X, y)
        a = gp.predict_hessian(Xs)
        monkeypatch.setenv("GPX_PRED_BATCH", "128")
        b = gp.predict_hessian(Xs)
    for u, v in zip(a, b):
        assert np.max(np.abs(u - v)) <= 1e-12 * np.max(np.abs(u))


def test_device_tensors():
    torch = pytest.importorskip("torch")
    X, y, Xs = synthetic_problem(600, 2, 90, seed=21)
    y2 = np.stack([y, -0.5 * y + X[:, 0]], 1)
    with GP("matern52", 0.3, 1.2, 5e-2) as gp:
        gp.fit(X, y2)
        ref = gp.predict_hessian(Xs)
        refo = gp.predict_hessian(Xs, return_var=False)
        reff = gp.predict_hessian(Xs, full=True)
        Xt = torch.from_numpy(Xs).to("cuda:0")
        out = gp.predict_hessian(Xt)
        outo = gp.predict_hessian(Xt, return_var=False)
        outf = gp.predict_hessian(Xt, full=True)
    for t, a in zip(out + (outo,) + outf, ref + (refo,) + reff):
        assert t.is_cuda and t.device == Xt.device and tuple(t.shape) == a.shape
        assert np.array_equal(t.cpu().numpy(), a)


def test_noise_weights():
    X, y, Xs = synthetic_problem(700, 2, 50, seed=23)
    w = np.random.default_rng(1).uniform(0.2, 5.0, len(X))
    ls, sf2, sn2 = (0.3, 0.25), 1.5, 1e-2
    hmr, hvr = hess_ref(X, y, Xs, "matern52", ls, sf2, sn2, 1e-10 * sf2, w=w)
    prior = prior_hess_var("matern52", ls, sf2, 2)
    with GP("matern52", ls, sf2, sn2) as gp:
        gp.fit(X, y, noise_weights=w)
        hm, hv = gp.predict_hessian(Xs)
        hmo = gp.predict_hessian(Xs, return_var=False)
    em, ev = errors(hm, hv, hmr, hvr, prior)
    print(f"noise weights: hmean err {em:.2e}, hvar rel err {ev:.2e}")
    assert em <= 1e-6 and ev <= 1e-6 and np.max(np.abs(hmo - hm)) <= 1e-9 * np.max(np.abs(hm))


@pytest.mark.parametrize("kernel", KERNELS)
def test_fit_with_derivative_rows(kernel):
    """600 values and 150 derivative rows, d = 2: the columns of the derivative rows hold the kernel's third derivative"""
    rng = np.random.default_rng(31)
    X, y, Xs = synthetic_problem(600, 2, 70, seed=31)
    Xd = rng.uniform(0, 1, (150, 2))
    dims = rng.integers(0, 2, 150)
    yd = np.where(dims == 0, 2 * np.pi * np.cos(2 * np.pi * Xd[:, 0]), -1.5 * np.sin(3.0 * Xd[:, 1])) + 0.2 * rng.standard_normal(150)
    ls, sf2, sn2, snd = (0.3, 0.25), 1.5, 1e-2, 5e-2
    ref = DobsGP(kernel, ls, sf2, sn2, snd, 1e-10 * sf2).fit(np.concatenate([X, Xd]),
                                                              np.concatenate([np.full(600, -1), dims]), np.concatenate([y, yd]))
    hmr, hvr = hess_ref_kinds(ref, Xs)
    prior = prior_hess_var(kernel, ls, sf2, 2)
    with GP(kernel, ls, sf2, sn2) as gp:
        gp.fit(X, y, derivatives=(Xd, dims, yd), derivative_noise=snd)
        m0, v0 = gp.predict(Xs)
        hm, hv = gp.predict_hessian(Xs)
        hmo = gp.predict_hessian(Xs, return_var=False)                      # (no matrix-free product on such a fit)
        m1, v1 = gp.predict(Xs)
    em, ev = errors(hm, hv, hmr, hvr, prior)
    print(f"{kernel}, derivative rows: hmean err {em:.2e} (of max), hvar rel err {ev:.2e}")
    assert em <= 1e-6 and ev <= 1e-6
    assert np.array_equal(hmo, hm) and np.array_equal(m0, m1) and np.array_equal(v0, v1)


def kernel_hess_matrix(gpx, kernel, A, B, ls, sf2, kinds=None, dtype="float64"):
    d = A.shape[1]
    lsa = np.ascontiguousarray(np.atleast_1d(np.asarray(ls, dtype=np.float64)))
    G = np.zeros((d * (d + 1) // 2, len(A), len(B)))
    kb = None if kinds is None else np.ascontiguousarray(kinds, dtype=np.int32)
    rc = gpx.gpx_kernel_hess_matrix(_abi.KERNEL_IDS[kernel], _abi.DTYPE_IDS[dtype], _abi.dptr(A), None, len(A), _abi.dptr(B),
                                    None if kb is None else kb.ctypes.data_as(C.POINTER(C.c_int32)), len(B), d,
                                    _abi.dptr(lsa), lsa.size, sf2, None, 1, 0.0, _abi.dptr(G))
    assert rc == 0
    return G


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("d,ls", [(1, 0.3), (2, (0.3, 0.5)), (3, 0.4), (3, (0.2, 0.5, 0.35)), (6, 0.6)])
def test_kernel_hess_matrix(gpx, kernel, d, ls):
    rng = np.random.default_rng(d)
    A, B = rng.uniform(0, 1, (70, d)), rng.uniform(0, 1, (130, d))
    B[5] = A[3]
    sf2 = 1.7
    l = lengthscales(ls, d)
    G = kernel_hess_matrix(gpx, kernel, A, B, ls, sf2)
    ref = kernel_hess(A, B, kernel, ls, sf2)
    err = np.max(np.abs(G - ref)) / np.max(np.abs(ref))
    print(f"{kernel} d={d}: plain build err {err:.2e} (of max)")
    assert err <= 1e-13
    g0 = sf2 * (1.0 if kernel == "rbf" else 5.0 / 3.0)
    for b, (i, j) in enumerate(zip(*pairs(d))):                             # the coincident pair
        if i == j:
            assert abs(G[b, 3, 5] + g0 / l[i] ** 2) <= 1e-15 * g0 / l[i] ** 2
        else:
            assert G[b, 3, 5] == 0.0
    # the KINDS build: derivative columns hold the third derivative; the first tile of 64 columns has values only and
    # gives the plain build's bits
    kinds = np.concatenate([np.full(64, -1), rng.integers(-1, d, 66)])
    kinds[70] = 0
    Gk = kernel_hess_matrix(gpx, kernel, A, B, ls, sf2, kinds=kinds)
    refk = kinds_hess(A, B, kinds, kernel, ls, sf2)
    errk = np.max(np.abs(Gk - refk)) / np.max(np.abs(refk))
    print(f"{kernel} d={d}: build with kinds err {errk:.2e} (of max)")
    assert errk <= 1e-13
    assert np.array_equal(Gk[:, :, :64], G[:, :, :64])


REFUSED = {
    "mixed": (dict(dtype="mixed"), "rbf", 2, {}),
    "one_rank_group": (dict(devices=1, transport="local"), "rbf", 2, {}),
    "basis": ({}, "rbf", 2, dict(basis="linear")),
    "matern32": ({}, "matern32", 2, {}),
    "matern12": ({}, "matern12", 2, {}),
    "d9": ({}, "rbf", 9, {}),
}


@pytest.mark.parametrize("name", list(REFUSED))
def test_refusals_keep_the_fit(name):
    kw, kernel, d, fit_kw = REFUSED[name]
    X, y, Xs = synthetic_problem(600, d, 90, seed=21)
    with GP(kernel, 0.4, 1.2, 5e-2, **kw) as gp:
        gp.fit(X, y, **fit_kw)
        m0, v0 = gp.predict(Xs)
        for rv in (True, False):
            with pytest.raises(GpxError) as e:
                gp.predict_hessian(Xs, return_var=rv)
            assert e.value.code == _abi.E_UNSUPPORTED
        if name in ("matern32", "matern12"):
            assert "not twice differentiable" in str(e.value)
        if name == "d9":
            assert "d > 8" in str(e.value)
        m1, v1 = gp.predict(Xs)
        assert np.array_equal(m0, m1) and np.array_equal(v0, v1)


def test_before_fit_and_bad_shape_raise():
    with GP("rbf", 0.3) as gp:
        with pytest.raises(RuntimeError, match="before a successful fit"):
            gp.predict_hessian(np.zeros((3, 2)))
        X, y, Xs = synthetic_problem(300, 2, 10, seed=1)
        gp.fit(X, y)
        with pytest.raises(ValueError, match=r"Xs must be \(M, 2\)"):
            gp.predict_hessian(np.zeros((3, 3)))
