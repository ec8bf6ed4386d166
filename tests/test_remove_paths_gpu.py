"""GPU: PathModel.remove_paths — paths taken out of a cluster's model (GP.remove underneath) on a plain, a step-weighted and
a within-path model, against a fit of the remaining paths under the model's normalisation (which the first fit fixed, as
for add_paths: tests/test_append_gpu.py).  Bars: against a fresh fit of the library on the remaining rows 1e-9 of the
largest entry, against the dense fp64 oracle 1e-6 of it (test_add_paths_matches_the_oracle_on_all_paths' level)."""
import os
import sys

import numpy as np
import pytest

from gaussianprocesspathmodelling_amd import GP
from gaussianprocesspathmodelling_amd import paths as gpaths
from oracle.gp_oracle import OracleGP

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_paths_gpu import _synthetic_groups  # noqa: E402

pytestmark = pytest.mark.gpu

HP = dict(kernel="matern52", lengthscale=0.3, variance=1.0, noise=0.02)
Q = np.linspace(-50.0, 1400.0, 57)


def relmax(a, b):
    return float(np.max(np.abs(np.asarray(a) - b)) / np.max(np.abs(b)))


def rows_of(t, pm, keys):
    """the rows of `keys` under pm's normalisation"""
    X, Y, _ = gpaths.to_gp_inputs(t, keys, normalise=False)
    return np.ascontiguousarray((X - pm.in_lo) / pm.in_span), np.ascontiguousarray((Y - pm.y_mean) / pm.y_std)


def fresh_predict(pm, Xn, Yn, **fit_kw):
    with GP(HP["kernel"], HP["lengthscale"], HP["variance"], HP["noise"]) as gf:
        gf.fit(Xn, Yn, **fit_kw)
        mean, var = gf.predict(pm._queries(Q))
        return mean * pm.y_std + pm.y_mean, var[:, None] * pm.y_std ** 2, gf.log_det_


@pytest.fixture(scope="module")
def world():
    t, truth = _synthetic_groups(n_groups=1, per_group=9, seed=6)
    return t, truth[0]


@pytest.mark.parametrize("step_noise", [False, True])
def test_remove_paths_plain_and_step_weighted(world, step_noise):
    t, keys = world
    gone, left = [keys[2], keys[5], keys[6]], [q for i, q in enumerate(keys) if i not in (2, 5, 6)]
    pm = gpaths.fit_path_models(t, {0: keys}, step_noise=step_noise, **HP)[0]
    try:
        with pytest.raises(KeyError):
            pm.remove_paths([keys[2], "no such path"])
        assert pm.keys == keys                                     # nothing was removed
        assert pm.remove_paths([keys[5], keys[2]]).remove_paths([keys[6]]) is pm and pm.keys == left
        Xn, Yn = rows_of(t, pm, left)
        w = pm._tiled_weights(len(Xn), "test")
        assert (w is not None) == step_noise
        fm, fv, fld = fresh_predict(pm, Xn, Yn, noise_weights=w)
        mean, var = pm.predict(Q)
        fig = (relmax(mean, fm), relmax(var, fv), abs(pm.gp.log_det_ - fld) / abs(fld))
        print(f"remove_paths step_noise={step_noise}: mean {fig[0]:.2e} var {fig[1]:.2e} logdet {fig[2]:.2e} against a fresh fit")
        assert max(fig) <= 1e-9
        if not step_noise:
            o = OracleGP(HP["kernel"], HP["lengthscale"], HP["variance"], HP["noise"], jitter=pm.gp.jitter_used_).fit(Xn, Yn)
            om, ov = o.predict(pm._queries(Q))
            om, ov = om * pm.y_std + pm.y_mean, ov[:, None] * pm.y_std ** 2
            assert relmax(mean, om) <= 1e-6 and relmax(var, ov) <= 1e-6
        # the removed paths come back at the end: the model of all paths again, in the new order
        pm.add_paths(t, gone)
        assert pm.keys == left + gone
        Xa, Ya = rows_of(t, pm, left + gone)
        fm, fv, _ = fresh_predict(pm, Xa, Ya, noise_weights=pm._tiled_weights(len(Xa), "test"))
        mean, var = pm.predict(Q)
        assert relmax(mean, fm) <= 1e-9 and relmax(var, fv) <= 1e-9
    finally:
        pm.close()


def test_remove_paths_within_path_and_fresh_ids_afterwards(world):
    t, keys = world
    first, later = keys[:7], keys[7:]
    L = gpaths.PATH_LENGTH
    pm = gpaths.fit_path_models(t, {0: first}, within_path=True, path_variance=0.1, path_lengthscale=1.0, **HP)[0]
    try:
        assert pm.remove_paths([first[1], first[4]]) is pm
        left = [q for i, q in enumerate(first) if i not in (1, 4)]
        ids = np.repeat(np.array([0, 2, 3, 5, 6], dtype=np.int32), L)
        assert pm.keys == left and np.array_equal(pm.gp.path_ids_, ids)
        with pytest.raises(KeyError):
            pm.predict(Q, path=first[1])                           # a removed key is unknown
        Xn, Yn = rows_of(t, pm, left)
        fm, fv, fld = fresh_predict(pm, Xn, Yn, path_ids=ids, path_variance=0.1, path_lengthscale=1.0)
        mean, var = pm.predict(Q)
        fig = (relmax(mean, fm), relmax(var, fv), abs(pm.gp.log_det_ - fld) / abs(fld))
        print(f"remove_paths within_path: mean {fig[0]:.2e} var {fig[1]:.2e} logdet {fig[2]:.2e} against a fresh fit")
        assert max(fig) <= 1e-9
        # appended paths get ids that no path has had: 7 and 8, not the freed 1 and 4
        pm.append_paths(t, later)
        assert pm.keys == left + later and [pm._ids[q] for q in later] == [7, 8]
        ids2 = np.concatenate([ids, np.repeat(np.array([7, 8], dtype=np.int32), L)])
        assert np.array_equal(pm.gp.path_ids_, ids2)
        Xa, Ya = rows_of(t, pm, left + later)
        with GP(HP["kernel"], HP["lengthscale"], HP["variance"], HP["noise"]) as gf:
            gf.fit(Xa, Ya, path_ids=ids2, path_variance=0.1, path_lengthscale=1.0)
            for key, pid in ((left[1], 2), (later[0], 7)):         # a path that stayed, a path that came afterwards
                m1 = pm.predict(Q, return_var=False, path=key)
                m2 = gf.predict(pm._queries(Q), return_var=False, path_ids=pid) * pm.y_std + pm.y_mean
                print(f"predict(path={key!r}) after remove + append: {relmax(m1, m2):.2e} against a fresh fit")
                assert relmax(m1, m2) <= 1e-9
    finally:
        pm.close()


def test_remove_paths_is_refused_on_a_model_with_velocities(world):
    t, keys = world
    L = gpaths.PATH_LENGTH
    pm = gpaths.fit_path_models(t, {0: keys[:4]}, velocities={keys[0]: np.zeros((L, 2))}, **HP)[0]
    try:
        with pytest.raises(ValueError, match="velocities"):
            pm.remove_paths([keys[1]])
        assert pm.keys == keys[:4] and pm.gp._N == 5 * L
        pm.gp.remove(np.arange(L, 2 * L))                          # GP.remove(indices) remains available
        assert pm.gp._N == 4 * L
    finally:
        pm.close()
