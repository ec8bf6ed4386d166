"""GPU: the posterior gradient — ``GP.predict_gradient`` (gpx_predict_grad), ``gpx_kernel_grad_matrix`` and
``PathModel.velocity`` — against the fp64 closed-form reference (tests/deriv_ref.py), against finite differences of the
GPU's own ``predict``, and for internal consistency (two routes, batching, timing perturbation, no side effects)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from gaussianprocesspathmodelling_amd import GP, GpxError, _abi
from gaussianprocesspathmodelling_amd import paths as gpaths
from oracle.gp_oracle import synthetic_problem

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from deriv_ref import grad_ref, kernel_grad, lengthscales, prior_grad_var  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


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


CASES = {
    "G1": lambda: golden_case("G1"),
    "G2": lambda: golden_case("G2"),
    "G3": lambda: golden_case("G3"),
    "rbf_d1_M1_k1": lambda: synthetic_case(1000, 1, 1, 1, "rbf", 0.3, 3),
    "matern_ard_d2_M77_k2": lambda: synthetic_case(777, 2, 77, 2, "matern52", (0.3, 0.2), 4),
    "rbf_ard_d3_M300_k2": lambda: synthetic_case(1500, 3, 300, 2, "rbf", (0.3, 0.2, 0.25), 5),
    "matern_d3_M300_k1": lambda: synthetic_case(2000, 3, 300, 1, "matern52", 0.25, 6),
    "matern_d1_M2048_k2": lambda: synthetic_case(4096, 1, 2048, 2, "matern52", 0.1, 7),
    "rbf_N8192_M2048": lambda: synthetic_case(8192, 3, 2048, 1, "rbf", 0.25, 8),
    "rbf_ard_d5_M100_k2": lambda: synthetic_case(900, 5, 100, 2, "rbf", (0.5, 0.4, 0.6, 0.45, 0.55), 9),  # runtime-d path
}


@pytest.fixture(scope="module")
def refs():
    cache = {}

    def get(name):
        if name not in cache:
            c = CASES[name]()
            cache[name] = c + (grad_ref(*c),)
        return cache[name]
    return get


def as_mdk(a, M, d):
    return np.asarray(a).reshape(M, d, -1)


@pytest.mark.parametrize("name", list(CASES))
def test_gradient_fp64(refs, name):
    X, y, Xs, kernel, ls, sf2, sn2, jit, (dmr, dvr) = refs(name)
    M, d = Xs.shape
    prior = prior_grad_var(kernel, ls, sf2, d)
    with GP(kernel, ls, sf2, sn2, jitter=jit) as gp:
        gp.fit(X, y)
        m0, v0 = gp.predict(Xs)
        dm, dv = gp.predict_gradient(Xs)
        dm_only = gp.predict_gradient(Xs, return_var=False)               # the matrix-free route
        mean, var, dm2, dv2 = gp.predict_gradient(Xs, with_value=True)
        mo, dmo = gp.predict_gradient(Xs, return_var=False, with_value=True)
        dm3, dv3 = gp.predict_gradient(Xs)
        mp = gp.predict(Xs, return_var=False)
        m1, v1 = gp.predict(Xs)
    k = 1 if np.ndim(y) == 1 else y.shape[1]
    assert dm.shape == ((M, d) if k == 1 and np.ndim(y) == 1 else (M, d, k)) and dv.shape == (M, d)
    assert dm.dtype == np.float64 and dm_only.shape == dm.shape and mean.shape == m0.shape and var.shape == (M,)
    em = np.max(np.abs(as_mdk(dm, M, d) - dmr)) / np.max(np.abs(dmr))
    ev = np.max(np.abs(dv - dvr) / np.maximum(np.abs(dvr), 1e-6 * prior[None, :]))
    print(f"{name}: N={len(X)} M={M} d={d} k={k} dmean err {em:.2e} (of max), dvar rel err {ev:.2e}")
    assert em <= 1e-6 and ev <= 1e-6
    scale = np.max(np.abs(dm))
    assert np.max(np.abs(dm_only - dm)) <= 1e-9 * scale                  # matrix-free = z^T V route
    assert np.array_equal(dmo, dm_only) and np.array_equal(mo, mp)      # mean: predict's own mean-only path
    assert np.max(np.abs(dm2 - dm)) <= 1e-9 * scale and np.max(np.abs(dv2 - dv)) <= 1e-10 * np.max(prior)
    assert np.max(np.abs(mean - m0)) <= 1e-9 * np.max(np.abs(m0))       # = predict's mean and variance
    assert np.max(np.abs(var - v0)) <= 1e-10 * sf2
    assert np.array_equal(dm3, dm) and np.array_equal(dv3, dv)           # reproducible
    assert np.array_equal(m0, m1) and np.array_equal(v0, v1)             # the fit is only read


@pytest.mark.parametrize("name", list(CASES))
def test_gradient_fp32(refs, name):
    X, y, Xs, kernel, ls, sf2, sn2, jit, (dmr, dvr) = refs(name)
    M, d = Xs.shape
    prior = prior_grad_var(kernel, ls, sf2, d)
    with GP(kernel, ls, sf2, sn2, jitter=jit, dtype="float32") as gp:
        gp.fit(X, y)
        dm, dv = gp.predict_gradient(Xs)
        dmo = gp.predict_gradient(Xs, return_var=False)
    assert dm.dtype == np.float32 and dv.dtype == np.float32
    em = np.max(np.abs(as_mdk(dm, M, d) - dmr)) / np.max(np.abs(dmr))
    emo = np.max(np.abs(as_mdk(dmo, M, d) - dmr)) / np.max(np.abs(dmr))
    ev = np.max(np.abs(dv - dvr) / prior[None, :])
    print(f"fp32 {name}: dmean err {em:.2e} / matrix-free {emo:.2e} (of max), dvar err {ev:.2e} (of prior)")
    assert em <= 5e-3 and emo <= 5e-3 and ev <= 5e-3


@pytest.mark.parametrize("kernel", ["rbf", "matern52"])
@pytest.mark.parametrize("d,ls", [(1, 0.3), (2, (0.3, 0.5)), (3, 0.4), (3, (0.2, 0.5, 0.35)), (6, 0.6)])
def test_kernel_grad_matrix(gpx, kernel, d, ls):
    rng = np.random.default_rng(d)
    A, B = rng.uniform(0, 1, (70, d)), rng.uniform(0, 1, (130, d))
    B[5] = A[3]
    sf2 = 1.7
    lsa = lengthscales(ls, d) if np.ndim(ls) else np.array([float(ls)])
    G = np.zeros((d, 70, 130))
    rc = gpx.gpx_kernel_grad_matrix(_abi.KERNEL_IDS[kernel], _abi.dptr(A), 70, _abi.dptr(B), 130, d, _abi.dptr(lsa),
                                    lsa.size, sf2, _abi.dptr(G))
    assert rc == 0
    ref = kernel_grad(A, B, kernel, ls, sf2)
    assert np.max(np.abs(G - ref)) <= 1e-13 * np.max(np.abs(ref))
    assert np.all(G[:, 3, 5] == 0.0)


def test_batched_equals_unbatched(refs, monkeypatch):
    X, y, Xs, kernel, ls, sf2, sn2, jit, _ = refs("rbf_ard_d3_M300_k2")
    with GP(kernel, ls, sf2, sn2, jitter=jit) as gp:
        gp.fit(X, y)
        a = gp.predict_gradient(Xs, with_value=True)
        monkeypatch.setenv("GPX_PRED_BATCH", "128")
        b = gp.predict_gradient(Xs, with_value=True)
    for u, v in zip(a, b):
        assert np.max(np.abs(u - v)) <= 1e-12 * np.max(np.abs(u))


@pytest.mark.parametrize("kernel,ls", [("rbf", 0.3), ("matern52", (0.35, 0.25))])
def test_against_finite_differences_of_predict(kernel, ls):
    X, y, Xs = synthetic_problem(800, 2, 40, seed=12)
    sf2, sn2 = 1.3, 1e-2
    l = lengthscales(ls, 2)
    prior = prior_grad_var(kernel, ls, sf2, 2)
    with GP(kernel, ls, sf2, sn2) as gp:
        gp.fit(X, y)
        dm, dv = gp.predict_gradient(Xs)
        for j in range(2):
            h = 1e-3 * l[j]
            Xp, Xm = Xs.copy(), Xs.copy()
            Xp[:, j] += h
            Xm[:, j] -= h
            fd = (gp.predict(Xp, return_var=False) - gp.predict(Xm, return_var=False)) / (2 * h)
            assert np.max(np.abs(fd - dm[:, j])) <= 1e-5 * np.max(np.abs(dm[:, j]))
            h = 3e-3 * l[j]
            Xp, Xm = Xs.copy(), Xs.copy()
            Xp[:, j] += h
            Xm[:, j] -= h
            _, cov = gp.predict(np.concatenate([Xp, Xm]), return_cov=True)
            M = len(Xs)
            fdv = (np.diag(cov)[:M] + np.diag(cov)[M:] - 2 * np.diag(cov[:M, M:])) / (4 * h * h)
            err = np.max(np.abs(fdv - dv[:, j])) / prior[j]
            print(f"{kernel} dim {j}: finite-difference variance err {err:.2e} (of prior)")
            assert err <= 1e-4


def test_device_tensors():
    torch = pytest.importorskip("torch")
    X, y, Xs = synthetic_problem(600, 2, 90, seed=21)
    y2 = np.stack([y, -0.5 * y + X[:, 0]], 1)
    with GP("matern52", 0.3, 1.2, 5e-2) as gp:
        gp.fit(X, y2)
        ref = gp.predict_gradient(Xs, with_value=True)
        refo = gp.predict_gradient(Xs, return_var=False)
        Xt = torch.from_numpy(Xs).to("cuda:0")
        out = gp.predict_gradient(Xt, with_value=True)
        outo = gp.predict_gradient(Xt, return_var=False)
    for t, a in zip(out + (outo,), ref + (refo,)):
        assert t.is_cuda and t.device == Xt.device and tuple(t.shape) == a.shape
        assert np.array_equal(t.cpu().numpy(), a)


@pytest.mark.parametrize("kw", [dict(dtype="mixed"), dict(devices=1, transport="local")])
def test_refused_handles_keep_their_fit(kw):
    X, y, Xs = synthetic_problem(600, 2, 90, seed=21)
    with GP("matern52", 0.3, 1.2, 5e-2, **kw) as gp:
        gp.fit(X, y)
        m0, v0 = gp.predict(Xs)
        for rv in (True, False):
            with pytest.raises(GpxError) as e:
                gp.predict_gradient(Xs, return_var=rv)
            assert e.value.code == _abi.E_UNSUPPORTED
        m1, v1 = gp.predict(Xs)
        assert np.array_equal(m0, m1) and np.array_equal(v0, v1)


def test_before_fit_and_bad_shape_raise():
    with GP("rbf", 0.3) as gp:
        with pytest.raises(RuntimeError, match="before a successful fit"):
            gp.predict_gradient(np.zeros((3, 2)))
        X, y, Xs = synthetic_problem(300, 2, 10, seed=1)
        gp.fit(X, y)
        with pytest.raises(ValueError, match=r"Xs must be \(M, 2\)"):
            gp.predict_gradient(np.zeros((3, 3)))


def test_bit_identical_under_stream_delays(gpx):
    X, y, Xs = synthetic_problem(4096, 3, 700, seed=31)
    with GP("rbf", (0.3, 0.25, 0.35), 1.1, 1e-2) as gp:
        gp.fit(X, y)
        ref = gp.predict_gradient(Xs, with_value=True)
        try:
            for seed in (1, 7, 123):
                gpx.gpx_debug_set_delay(seed)
                out = gp.predict_gradient(Xs, with_value=True)
                assert all(np.array_equal(a, b) for a, b in zip(out, ref)), seed
        finally:
            gpx.gpx_debug_set_delay(0)


def straight_paths(seed=3, speed=(1.25, -0.6)):
    rng = np.random.default_rng(seed)
    t = gpaths.Trajectories()
    tt = np.arange(33, dtype=float) * 40.0
    keys = []
    for p in range(6):
        tr = gpaths.Trajectory()
        ox, oy = rng.normal(0, 20, 2)
        for i in range(33):
            tr.add_point(tt[i], 100.0 + ox + speed[0] * tt[i] + rng.normal(0, 3),
                         400.0 + oy + speed[1] * tt[i] + rng.normal(0, 3))
        t.add_trajectory(f"P{p}", tr)
        keys.append(f"P{p}")
    return t, {0: keys}


def test_path_velocity_recovers_constant_speed():
    speed = np.array([1.25, -0.6])
    t, clusters = straight_paths(speed=tuple(speed))
    models = gpaths.fit_path_models(t, clusters, kernel="rbf", lengthscale=0.5, variance=1.0, noise=0.01)
    try:
        m = models[0]
        q = np.linspace(200.0, 1080.0, 23)
        v, vv = m.velocity(q)
        assert v.shape == (23, 2) and vv.shape == (23, 2)
        zscore = np.abs(v - speed[None, :]) / np.sqrt(vv)
        print(f"velocity: max |v - speed| = {np.max(np.abs(v - speed)):.3e}, max z = {zscore.max():.2f}")
        assert np.all(vv > 0) and np.all(zscore <= 3.0)
        dm, dv = m.predict_gradient(q)
        assert dm.shape == (23, 1, 2) and np.array_equal(dm[:, 0, :], v) and np.array_equal(dv[:, 0, :], vv)
        vo = m.velocity(q, return_var=False)                                # the matrix-free route
        assert np.max(np.abs(vo - v)) <= 1e-9 * np.max(np.abs(v))
    finally:
        for mm in models.values():
            mm.close()


def test_path_velocity_matches_finite_differences_of_predict():
    rng = np.random.default_rng(4)
    t = gpaths.Trajectories()
    tt = np.arange(33, dtype=float) * 40.0
    for p in range(5):
        tr = gpaths.Trajectory()
        for i in range(33):
            s = tt[i] / 1280.0
            tr.add_point(tt[i], 1500.0 * s + 200.0 * np.sin(3 * s) + rng.normal(0, 10),
                         900.0 * s * s + rng.normal(0, 10))
        t.add_trajectory(f"Q{p}", tr)
    models = gpaths.fit_path_models(t, {0: [f"Q{p}" for p in range(5)]}, kernel="matern52", lengthscale=0.3,
                                    variance=1.0, noise=0.02)
    try:
        m = models[0]
        q = np.linspace(50.0, 1230.0, 31)
        v = m.velocity(q, return_var=False)
        h = 1e-3 * 0.3 * m.in_span[0]
        fd = (m.predict(q + h, return_var=False) - m.predict(q - h, return_var=False)) / (2 * h)
        assert np.max(np.abs(fd - v)) <= 1e-5 * np.max(np.abs(v))
        with pytest.raises(ValueError):
            gpaths.PathModel(m.gp, m.keys, m.in_lo, m.in_span, m.y_mean, m.y_std, ("x",), m.targets).velocity(q)
    finally:
        for mm in models.values():
            mm.close()


def test_close_frees_the_gradient_buffers():
    """``close()`` returns the scratch of ``predict_gradient`` to the device.  The V buffer of this call holds three row
    blocks (value and two partials) of M = 2048 rows of N + skew fp64 columns: 3 * 2048 * (4096 + 16) * 8 bytes, about
    200 MB.  Free device memory after the close must be within half of that (100 MB) of what it was before the model
    existed: the bound comes from the buffer's size, it is not a measurement.

    One model is fitted and closed before the first reading: the first use of the library in a process costs device
    memory that no handle owns (code objects, queues, kernel scratch: 172 MB measured, the same with and without the
    leak, constant over any number of models), and a test that runs alone would count it."""
    import torch

    N, d, M = 4096, 2, 2048
    X, y, Xs = synthetic_problem(N, d, M, seed=11)
    with GP("matern52", 0.3, 1.5, 1e-2, jitter=0.0, device=0) as warm:
        warm.fit(X, y).predict(Xs)
    torch.cuda.synchronize()
    free_before = torch.cuda.mem_get_info(0)[0]
    gp = GP("matern52", 0.3, 1.5, 1e-2, jitter=0.0, device=0)
    try:
        gp.fit(X, y).predict_gradient(Xs, return_var=True, with_value=True)
    finally:
        gp.close()
    torch.cuda.synchronize()
    free_after = torch.cuda.mem_get_info(0)[0]
    gv_bytes = 3 * M * (N + 16) * 8
    print(f"free before {free_before}  after close {free_after}  not returned {free_before - free_after}  GV {gv_bytes}")
    assert free_before - free_after <= gv_bytes // 2
