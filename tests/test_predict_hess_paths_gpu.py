"""GPU: the second derivatives of an observed path itself — ``GP.predict_hessian(path_ids=)`` (gpx_predict_hess_paths), the
builder with path ids (gpx_kernel_hess_matrix) — against the dense reference of tests/hess_ref.py, and
``PathModel.predict_hessian`` / ``acceleration`` / ``curvature`` for units and on a half circle of known curvature."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from gaussianprocesspathmodelling_amd import GP, GpxError, _abi
from gaussianprocesspathmodelling_amd import paths as gpaths

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import within_ref as wr  # noqa: E402
from deriv_ref import grad_ref  # noqa: E402
from hess_ref import hess_ref, hess_ref_paths, path_hess, prior_hess_var  # noqa: E402

pytestmark = pytest.mark.gpu

P, L = 12, 33
LS = {1: 0.25, 3: (0.25, 0.4, 0.3)}
LS_PATH = {1: 0.1, 3: (0.1, 0.2, 0.15)}
SF2, SG2, SN2, JIT = 1.5, 0.4, 1e-2, 1.5e-10


@pytest.fixture(scope="module")
def worlds():
    """12 paths of 33 points drawn from the hierarchical model, its reference fit, and 60 query points whose ids mix -1,
    observed paths and a path nobody has seen (id 40) — computed once per (kernel, d)"""
    cache = {}

    def get(kernel, d):
        if (kernel, d) not in cache:
            w = wr.problem(P=P, L=L, kernel=kernel, ls=LS[d], sf2=SF2, ls_path=LS_PATH[d], sg2=SG2, sn2=SN2, seed=3 + d, d=d)
            fit = wr.fit_ref(w["X"], w["ids"], w["Y"], kernel, LS[d], SF2, SN2, LS_PATH[d], SG2, jitter=JIT)
            rng = np.random.default_rng(11)
            Xq = w["X"][rng.choice(len(w["X"]), 60, replace=False)] + 0.01 * rng.standard_normal((60, d))
            gq = rng.integers(-1, P, 60).astype(np.int32)
            gq[:4] = (-1, 40, 0, P - 1)
            cache[(kernel, d)] = (w, fit, Xq, gq)
        return cache[(kernel, d)]
    return get


def fitted(kernel, d, w):
    gp = GP(kernel, LS[d], SF2, SN2, jitter=JIT)
    gp.fit(w["X"], w["Y"], path_ids=w["ids"], path_variance=SG2, path_lengthscale=LS_PATH[d])
    return gp


@pytest.mark.parametrize("kernel", ["rbf", "matern52"])
@pytest.mark.parametrize("d", [1, 3])
def test_paths_against_the_reference(worlds, kernel, d):
    w, fit, Xq, gq = worlds(kernel, d)
    hmr, hvr = hess_ref_paths(fit, Xq, gq)
    prior = prior_hess_var(kernel, LS[d], SF2, d)
    with fitted(kernel, d, w) as gp:
        m0, v0 = gp.predict(Xq)
        hm, hv = gp.predict_hessian(Xq, path_ids=gq)
        hmo = gp.predict_hessian(Xq, return_var=False, path_ids=gq)
        hm2, hv2 = gp.predict_hessian(Xq, path_ids=gq)
        one = gp.predict_hessian(Xq, path_ids=5)
        m1, v1 = gp.predict(Xq)
    em = np.max(np.abs(hm - hmr)) / np.max(np.abs(hmr))
    ev = np.max(np.abs(hv - hvr) / np.maximum(np.abs(hvr), 1e-6 * prior[None, :]))
    print(f"{kernel} d={d}: hmean err {em:.2e} (of max), hvar rel err {ev:.2e}")
    assert em <= 1e-6 and ev <= 1e-6
    assert np.array_equal(hmo, hm) and np.array_equal(hm2, hm) and np.array_equal(hv2, hv)
    assert np.array_equal(m0, m1) and np.array_equal(v0, v1)
    r5 = hess_ref_paths(fit, Xq, 5)
    assert np.max(np.abs(one[0] - r5[0])) <= 1e-6 * np.max(np.abs(r5[0]))
    assert np.max(np.abs(one[1] - r5[1]) / np.maximum(np.abs(r5[1]), 1e-6 * prior[None, :])) <= 1e-6


@pytest.mark.parametrize("d", [1, 3])
def test_all_minus_one_is_the_plain_batch_route(worlds, d):
    w, fit, Xq, _ = worlds("matern52", d)
    none = np.full(len(Xq), -1, dtype=np.int32)
    with fitted("matern52", d, w) as gp:
        hm, hv = gp.predict_hessian(Xq)
        hmp, hvp = gp.predict_hessian(Xq, path_ids=none)
    assert np.array_equal(hmp, hm) and np.array_equal(hvp, hv)
    hmr, _ = hess_ref_paths(fit, Xq, -1)
    assert np.max(np.abs(hm - hmr)) <= 1e-6 * np.max(np.abs(hmr))


def test_paths_call_needs_a_fit_with_path_ids(worlds):
    w, _, Xq, gq = worlds("rbf", 1)
    with GP("rbf", LS[1], SF2, SN2) as gp:
        gp.fit(w["X"], w["Y"])
        m0, v0 = gp.predict(Xq)
        with pytest.raises(GpxError) as e:
            gp.predict_hessian(Xq, path_ids=gq)
        assert e.value.code == _abi.E_UNSUPPORTED and "path ids" in str(e.value)
        m1, v1 = gp.predict(Xq)
    assert np.array_equal(m0, m1) and np.array_equal(v0, v1)


@pytest.mark.parametrize("kernel", ["rbf", "matern52"])
@pytest.mark.parametrize("d", [1, 2, 3, 6])
def test_kernel_hess_matrix_with_path_ids(gpx, kernel, d):
    rng = np.random.default_rng(40 + d)
    A, B = rng.uniform(0, 1, (70, d)), rng.uniform(0, 1, (130, d))
    B[5] = A[3]
    ga, gb = rng.integers(-1, 4, 70).astype(np.int32), rng.integers(-1, 4, 130).astype(np.int32)
    ga[3] = gb[5] = 2
    gb[64:128] = -1                                                          # a tile that cannot hold a same-path pair
    ls, lsp = np.linspace(0.3, 0.6, d), np.linspace(0.15, 0.2, d)
    pi = lambda v: v.ctypes.data_as(C.POINTER(C.c_int32))  # noqa: E731
    G, G0 = np.zeros((d * (d + 1) // 2, 70, 130)), np.zeros((d * (d + 1) // 2, 70, 130))
    rc = gpx.gpx_kernel_hess_matrix(_abi.KERNEL_IDS[kernel], 0, _abi.dptr(A), pi(ga), 70, _abi.dptr(B), pi(gb), 130, d,
                                    _abi.dptr(ls), d, 1.7, _abi.dptr(lsp), d, 0.6, _abi.dptr(G))
    assert rc == 0
    ref = path_hess(A, ga, B, gb, kernel, ls, 1.7, lsp, 0.6)
    err = np.max(np.abs(G - ref)) / np.max(np.abs(ref))
    print(f"{kernel} d={d}: build with path ids err {err:.2e} (of max)")
    assert err <= 1e-13
    rc = gpx.gpx_kernel_hess_matrix(_abi.KERNEL_IDS[kernel], 0, _abi.dptr(A), None, 70, _abi.dptr(B), None, 130, d,
                                    _abi.dptr(ls), d, 1.7, None, 1, 0.0, _abi.dptr(G0))
    assert rc == 0
    assert np.array_equal(G[:, :, 64:128], G0[:, :, 64:128])                  # the plain build's bits


# ---- path models -----------------------------------------------------------------------------------------------------------
R, T_END = 1000.0, 1280.0
HP = dict(kernel="rbf", lengthscale=0.3, variance=1.0, noise=1e-4)


def half_circle(seed=5):
    """5 paths of 33 points on x = R cos(pi s), y = R sin(pi s), s = t / T_END, with unit noise: curvature 1 / R,
    counter-clockwise"""
    rng = np.random.default_rng(seed)
    t, keys = gpaths.Trajectories(), []
    tt = np.arange(L, dtype=float) * (T_END / (L - 1))
    for p in range(5):
        tr = gpaths.Trajectory()
        for i in range(L):
            s = tt[i] / T_END
            tr.add_point(tt[i], R * np.cos(np.pi * s) + rng.normal(0, 1), R * np.sin(np.pi * s) + rng.normal(0, 1))
        t.add_trajectory(f"C{p}", tr)
        keys.append(f"C{p}")
    return t, keys


@pytest.fixture(scope="module")
def circle():
    t, keys = half_circle()
    models = gpaths.fit_path_models(t, {0: keys}, **HP)
    yield t, keys, models[0]
    models[0].close()


def curvature_of(v, a):
    return (v[:, 0] * a[:, 1] - v[:, 1] * a[:, 0]) / (v[:, 0] ** 2 + v[:, 1] ** 2) ** 1.5


def test_acceleration_units(circle):
    t, keys, m = circle
    q = np.linspace(100.0, 1200.0, 23)
    acc, av = m.acceleration(q)
    hm, hv = m.predict_hessian(q)
    assert acc.shape == av.shape == (23, 2) and hm.shape == hv.shape == (23, 1, 2)
    assert np.array_equal(hm[:, 0, :], acc) and np.array_equal(hv[:, 0, :], av)
    qn = ((q - m.in_lo[0]) / m.in_span[0]).reshape(-1, 1)
    gm, gv = m.gp.predict_hessian(qn)                                        # normalised units
    scale = m.y_std / m.in_span[0] ** 2
    assert np.max(np.abs(acc - gm[:, 0, :] * scale)) <= 1e-12 * np.max(np.abs(acc))
    assert np.max(np.abs(av - gv[:, :1] * scale ** 2)) <= 1e-12 * np.max(np.abs(av))
    assert np.all(av > 0)
    ao = m.acceleration(q, return_var=False)                                 # the matrix-free route
    assert np.max(np.abs(ao - acc)) <= 1e-9 * np.max(np.abs(acc))
    with pytest.raises(ValueError, match="'t'"):
        gpaths.PathModel(m.gp, m.keys, m.in_lo, m.in_span, m.y_mean, m.y_std, ("x",), m.targets).acceleration(q)
    with pytest.raises(ValueError, match="two targets"):
        gpaths.PathModel(m.gp, m.keys, m.in_lo, m.in_span, m.y_mean[:1], m.y_std[:1], m.inputs, ("x",)).curvature(q)


def test_curvature_of_a_half_circle(circle):
    t, keys, m = circle
    q = np.linspace(0.25, 0.75, 41) * T_END
    kappa = m.curvature(q)
    assert kappa.shape == (41,)
    own = curvature_of(m.velocity(q, return_var=False), m.acceleration(q, return_var=False))
    assert np.max(np.abs(kappa - own)) <= 1e-12 * np.max(np.abs(own))
    # the CPU reference of the same model, in the model's own normalisation
    X, Y, (lo, span) = gpaths.to_gp_inputs(t, keys)
    Yn = (Y - m.y_mean) / m.y_std
    qn = ((q - lo[0]) / span[0]).reshape(-1, 1)
    a = (HP["kernel"], HP["lengthscale"], HP["variance"], HP["noise"], m.gp.jitter_used_)
    v_ref = grad_ref(X, Yn, qn, *a)[0][:, 0, :] * m.y_std / span[0]
    a_ref = hess_ref(X, Yn, qn, *a)[0][:, 0, :] * m.y_std / span[0] ** 2
    k_ref = curvature_of(v_ref, a_ref)
    err = np.max(np.abs(kappa - k_ref) / np.abs(k_ref))
    print(f"half circle: kappa R in [{np.min(kappa) * R:.4f}, {np.max(kappa) * R:.4f}] (reference "
          f"[{np.min(k_ref) * R:.4f}, {np.max(k_ref) * R:.4f}]), rel err to the reference {err:.2e}")
    assert err <= 1e-6
    assert np.all(kappa * R >= 0.95) and np.all(kappa * R <= 1.05)             # counter-clockwise: positive
