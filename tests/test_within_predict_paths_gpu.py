"""GPU: PathModel.predict / sample / predict_gradient / velocity with ``path=key`` on a within-path cluster model — the
posterior of one observed path itself (cluster mean plus its own deviation) in raw units, against the dense reference of
tests/within_predict_ref.py and against the plain methods' shapes and units."""
import os
import sys

import numpy as np
import pytest

from gaussianprocesspathmodelling_amd import paths as gpaths

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import within_predict_ref as wpr  # noqa: E402
import within_ref as wr  # noqa: E402

pytestmark = pytest.mark.gpu

HP = dict(kernel="matern52", lengthscale=0.3, variance=1.0, noise=0.01)
PATH_VAR, PATH_LS = 0.1, 1.0
L, T_END = gpaths.PATH_LENGTH, 1280.0


def _world(seed=33, n=6):
    """one cluster of n paths of 33 points around a smooth curve, each with an offset of its own (100 raw units, against a
    noise of 15)"""
    rng = np.random.default_rng(seed)
    t, keys = gpaths.Trajectories(), []
    tt = np.linspace(0.0, T_END, L)
    s = tt / T_END
    for p in range(n):
        ox, oy = rng.normal(0, 100, 2)
        tr = gpaths.Trajectory()
        for i in range(L):
            tr.add_point(tt[i], ox + 1500.0 * s[i] + 200.0 * np.sin(3 * s[i]) + rng.normal(0, 15),
                         oy + 900.0 * s[i] * s[i] + rng.normal(0, 15))
        t.add_trajectory(f"P{p}", tr)
        keys.append(f"P{p}")
    return t, keys, tt


@pytest.fixture(scope="module")
def world():
    t, keys, tt = _world()
    models = gpaths.fit_path_models(t, {0: keys}, within_path=True, path_variance=PATH_VAR, path_lengthscale=PATH_LS, **HP)
    plain = gpaths.fit_path_models(t, {0: keys}, **HP)
    yield t, keys, tt, models[0], plain[0]
    models[0].close()
    plain[0].close()


def _rms(a, b):
    return float(np.sqrt(np.mean((a - b) ** 2)))


def test_a_path_is_closer_to_its_own_observations_than_the_cluster_mean(world):
    t, keys, tt, pm, _ = world
    Xn, Y, _ = gpaths.to_gp_inputs(t, keys)                                 # inputs mapped to [0, 1], targets raw
    Yn = (Y - pm.y_mean) / pm.y_std
    ids = np.repeat(np.arange(len(keys)), L).astype(np.int32)
    fit = wr.fit_ref(Xn, ids, Yn, HP["kernel"], HP["lengthscale"], HP["variance"], HP["noise"], PATH_LS, PATH_VAR,
                     jitter=pm.gp.jitter_used_)
    for i, key in ((2, "P2"), (5, "P5")):
        own = t.as_array([key])[0][:, 1:]                                   # (L, 2) raw observations
        rows = slice(i * L, (i + 1) * L)
        # first on the reference, in normalised units ...
        rp = _rms(wpr.predict_path(fit, Xn[rows], i)[0], Yn[rows])
        rf = _rms(wr.predict_f(fit, Xn[rows])[0], Yn[rows])
        assert rp < 0.5 * rf, (rp, rf)
        # ... then on the device, in raw units
        mp, vp = pm.predict(tt, path=key)
        mf, vf = pm.predict(tt)
        ep, ef = _rms(mp, own), _rms(mf, own)
        print(f"{key}: RMS error to its own observations {ep:.4g} as the path, {ef:.4g} as the cluster mean "
              f"(reference, normalised: {rp:.4g} / {rf:.4g})")
        assert mp.shape == mf.shape == (L, 2) and vp.shape == vf.shape == (L, 2)
        assert ep < 0.5 * ef
        want = wpr.predict_path(fit, Xn[rows], i)
        assert np.max(np.abs(mp - (want[0] * pm.y_std + pm.y_mean))) <= 1e-6 * np.max(np.abs(mp))
        wv = np.diag(want[1])[:, None] * (pm.y_std ** 2)[None, :]
        assert np.max(np.abs(vp - wv) / np.maximum(wv, 1e-6 * np.max(pm.y_std ** 2))) <= 1e-6


def test_velocity_of_a_path_matches_central_differences_of_its_prediction(world):
    """step and bound of tests/test_predict_grad_gpu.py::test_path_velocity_matches_finite_differences_of_predict"""
    t, keys, tt, pm, _ = world
    q = np.linspace(50.0, 1230.0, 31)
    v = pm.velocity(q, return_var=False, path="P4")
    h = 1e-3 * HP["lengthscale"] * pm.in_span[0]
    fd = (pm.predict(q + h, return_var=False, path="P4") - pm.predict(q - h, return_var=False, path="P4")) / (2 * h)
    e = float(np.max(np.abs(fd - v)) / np.max(np.abs(v)))
    print(f"velocity of P4 vs central differences: {e:.2e} (of max)")
    assert e <= 1e-5
    assert np.max(np.abs(v - pm.velocity(q, return_var=False))) > 1e-3 * np.max(np.abs(v))   # not the cluster mean's


def test_units_and_shapes_are_the_plain_methods(world):
    t, keys, tt, pm, _ = world
    q = np.linspace(0.0, T_END, 17)
    for kw in ({}, {"path": "P1"}):
        mean, var = pm.predict(q, **kw)
        mc, cov = pm.predict(q, return_cov=True, **kw)
        dm, dv = pm.predict_gradient(q, **kw)
        v, vv = pm.velocity(q, **kw)
        s = pm.sample(q, 4, seed=7, **kw)
        assert mean.shape == var.shape == (17, 2) and cov.shape == (2, 17, 17) and pm.predict(q, return_var=False, **kw).shape == (17, 2)
        assert dm.shape == dv.shape == (17, 1, 2) and v.shape == vv.shape == (17, 2) and s.shape == (4, 17, 2)
        assert np.array_equal(dm[:, 0, :], v) and np.array_equal(dv[:, 0, :], vv)
        assert np.max(np.abs(mc - mean)) <= 1e-9 * np.max(np.abs(mean))
        assert np.max(np.abs(np.einsum("cii->ic", cov) - var)) <= 1e-9 * np.max(var)
    # samples of the path pass near its points; with include_noise they scatter as its observations do
    own = t.as_array(["P1"])[0][:, 1:]
    s = pm.sample(tt, 64, seed=3, path="P1")
    sd = np.sqrt(pm.predict(tt, path="P1")[1])
    assert np.all(np.abs(s.mean(0) - pm.predict(tt, path="P1")[0]) <= 5.0 * sd / np.sqrt(64) + 1e-6 * np.abs(own).max())
    assert _rms(s.mean(0), own) < 0.5 * _rms(pm.sample(tt, 64, seed=3).mean(0), own)


def test_keys_and_models_that_have_no_paths_of_their_own(world):
    t, keys, tt, pm, plain = world
    q = np.linspace(0.0, T_END, 5)
    for call in (pm.predict, pm.predict_gradient, pm.velocity, lambda q, path: pm.sample(q, 2, path=path)):
        with pytest.raises(KeyError):
            call(q, path="nobody")
    for call in (plain.predict, plain.predict_gradient, plain.velocity, lambda q, path: plain.sample(q, 2, path=path)):
        with pytest.raises(ValueError, match="within_path"):
            call(q, path="P1")
    assert plain.predict(q)[0].shape == (5, 2)                               # path=None stays every model's call
