"""GPU: path models with within-path deviations (paths.fit_path_models(within_path=True)), PathModel.forecast and
paths.forecast_paths on synthetic clusters whose paths carry a persistent per-path offset: two clusters of 10 training and 4
held-out paths of 33 points around smooth curves, every path shifted by its own offset (standard deviation 150 map units per
coordinate, against 15 of point noise).  A cluster-mean prediction cannot know a new path's offset; a forecast from the
path's first 20 points can.

The offset scale was picked on the CPU with the reference alone (tests/within_ref.py on the normalised data, ``_reference``
below, seed as here): the forecast's mean squared error over the held-out paths' last 13 points is 7.3e2 / 1.4e3 map
units^2 (cluster 0 / 1) against 3.4e4 / 4.0e4 of the cluster mean — factors of 47 and 28 — and the weight of a held-out
path's true cluster is 1 to within 1e-300 (the clusters lie 4000 units apart: log-likelihoods of about -200 against -900 and
less).  Both inequalities of the tests hold with that margin before any GPU number enters."""
import os
import sys

import numpy as np
import pytest

from gaussianprocesspathmodelling_amd import paths as gpaths

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import within_ref as wr  # noqa: E402

pytestmark = pytest.mark.gpu

HP = dict(kernel="matern32", lengthscale=0.3, variance=1.0, noise=0.01)
PATH_VAR, PATH_LS = 0.1, 1.0
L, LO, TRAIN, HELD = gpaths.PATH_LENGTH, 20, 10, 4


def _world(seed=21):
    rng = np.random.default_rng(seed)
    t = gpaths.Trajectories()
    groups = {0: [], 1: []}
    tt = np.arange(L, dtype=float) * 40.0
    for g in (0, 1):
        for p in range(TRAIN + HELD):
            tr = gpaths.Trajectory()
            ox, oy = rng.normal(0, 150, 2)                                  # the path's own persistent offset
            for i in range(L):
                s = i / (L - 1.0)
                tr.add_point(tt[i], 4000.0 * g + ox + 1500.0 * s + 200.0 * np.sin(3 * s + g) + rng.normal(0, 15),
                             2500.0 * g + oy + 900.0 * s * s + rng.normal(0, 15))
            t.add_trajectory(f"G{g}P{p}", tr)
            groups[g].append(f"G{g}P{p}")
    return t, groups


def _reference(t, train_keys, held_arr):
    """forecast (refit form) and cluster-mean prediction of one cluster's model for the held-out paths, in raw units, and
    the prefix log-densities (P, k) in raw units"""
    arr = t.as_array(train_keys)
    tt, Y = arr[:, :, 0].reshape(-1, 1), arr[:, :, 1:3].reshape(-1, 2)
    lo, span = tt.min(), tt.max() - tt.min()
    mu, sd = Y.mean(axis=0), Y.std(axis=0)
    X, Yn = (tt - lo) / span, (Y - mu) / sd
    ids = np.repeat(np.arange(len(train_keys)), L)
    P = len(held_arr)
    Xo = ((held_arr[:, :LO, 0] - lo) / span).reshape(-1, 1)
    Xp = ((held_arr[:, LO:, 0] - lo) / span).reshape(-1, 1)
    Yo = ((held_arr[:, :LO, 1:3] - mu) / sd).reshape(-1, 2)
    train = dict(X=X, ids=ids, Y=Yn, kernel=HP["kernel"], ls=HP["lengthscale"], sf2=HP["variance"], sn2=HP["noise"],
                 ls_path=PATH_LS, sg2=PATH_VAR, jitter=1e-10 * HP["variance"])
    ref = wr.forecast_refit(train, Xo, Yo, Xp, P, HP["noise"])
    fit = wr.fit_ref(X, ids, Yn, HP["kernel"], HP["lengthscale"], HP["variance"], HP["noise"], PATH_LS, PATH_VAR,
                     jitter=1e-10 * HP["variance"])
    fmean = wr.predict_f(fit, Xp)[0]
    return (ref["mean"].reshape(P, L - LO, 2) * sd + mu, fmean.reshape(P, L - LO, 2) * sd + mu,
            ref["logp"] - LO * np.log(sd)[None, :], ref["cov"][:, None] * (sd ** 2)[None, :, None, None])


@pytest.fixture(scope="module")
def world():
    t, groups = _world()
    train = {g: groups[g][:TRAIN] for g in groups}
    held = {g: groups[g][TRAIN:] for g in groups}
    models = gpaths.fit_path_models(t, train, within_path=True, path_variance=PATH_VAR, path_lengthscale=PATH_LS, **HP)
    yield t, train, held, models
    for m in models.values():
        m.close()


def test_a_forecast_beats_the_cluster_mean(world):
    t, train, held, models = world
    for g, m in models.items():
        assert m.within_path and m.gp.path_variance == PATH_VAR
        arr = t.as_array(held[g])
        mean, cov = m.forecast(arr[:, :LO], arr[0, LO:, 0])
        assert mean.shape == (HELD, L - LO, 2) and cov.shape == (HELD, 2, L - LO, L - LO)
        cluster = m.predict(arr[0, LO:, 0], return_var=False)
        truth = arr[:, LO:, 1:3]
        mse_f, mse_c = float(np.mean((mean - truth) ** 2)), float(np.mean((cluster[None] - truth) ** 2))
        rm, rc, _, rcov = _reference(t, train[g], arr)
        ref_f, ref_c = float(np.mean((rm - truth) ** 2)), float(np.mean((rc - truth) ** 2))
        print(f"cluster {g}: forecast mse {mse_f:.4g} (reference {ref_f:.4g}), cluster mean mse {mse_c:.4g} (reference "
              f"{ref_c:.4g}); margin of the reference {ref_c / ref_f:.3g}")
        assert ref_f * 10 < ref_c                     # the reference alone, with a clear margin
        assert mse_f < mse_c
        # and the numbers are the reference's: 1e-6 of the largest entry (tests/test_dobs_paths_gpu.py's level)
        assert np.max(np.abs(mean - rm)) <= 1e-6 * np.max(np.abs(rm))
        assert np.max(np.abs(cov - rcov)) <= 1e-6 * np.max(np.abs(rcov))


def test_forecast_paths_weighs_the_true_cluster(world):
    t, train, held, models = world
    keys = held[0] + held[1]
    arr = t.as_array(keys)
    w, means, covs = gpaths.forecast_paths(arr[:, :LO], arr[:, LO:, 0], models)
    assert w.shape == (2 * HELD, 2) and np.allclose(w.sum(axis=1), 1.0)
    assert list(means) == list(models) and means[0].shape == (2 * HELD, L - LO, 2)
    assert covs[1].shape == (2 * HELD, 2, L - LO, L - LO)
    true = np.r_[np.zeros(HELD, dtype=int), np.ones(HELD, dtype=int)]
    LLref = np.stack([_reference(t, train[g], arr)[2].sum(axis=1) for g in models], axis=1)
    wref = np.exp(LLref - LLref.max(axis=1, keepdims=True))
    wref /= wref.sum(axis=1, keepdims=True)
    print(f"weight of the true cluster: at least {w[np.arange(2 * HELD), true].min():.6g} (reference "
          f"{wref[np.arange(2 * HELD), true].min():.6g})")
    assert np.all(wref[np.arange(2 * HELD), true] > 0.5) and np.all(w[np.arange(2 * HELD), true] > 0.5)
    # the prefix log-likelihoods behind the weights are log_likelihood's of the prefixes
    for c, m in enumerate(models.values()):
        _, _, logp = m.forecast(arr[:, :LO], arr[:, LO:, 0], return_logp=True)
        ll = m.log_likelihood(arr[:, :LO])
        assert np.max(np.abs(logp - ll)) <= 1e-6 * np.max(np.abs(ll))


def test_add_paths_is_refused_on_a_within_path_model(world):
    t, train, held, models = world
    with pytest.raises(ValueError, match="within-path"):
        models[0].add_paths(t, held[0])
    assert models[0].keys == train[0]
    with pytest.raises(ValueError):
        gpaths.fit_path_models(t, {0: train[0]}, within_path=True, velocities={train[0][0]: np.zeros((L, 2))}, **HP)
