"""GPU: gpx_score_blocks / GP.score_blocks / the path likelihoods against the fp64 reference of tests/score_ref.py.

Error bound (per block g, first-order error propagation through S_g^-1): |got - ref| <= eps kappa_g (Lg + maha_g) for logp,
maha and logdet, kappa_g the 2-norm condition number of the reference's S_g, eps = 1e-10 for fp64 handles (the level at
which tests/test_posterior_gpu.py holds fp64 variances, 1e-10 sf2) and 1e-4 for fp32 handles (that suite's fp32 level).
With sf2 = 1.5 and diag_add = sn2 = 1e-2, kappa_g <= 9601 (score_ref.kappa_bound).  Every test prints the largest ratio of
an observed error to its bound before it asserts."""
import os
import sys

import numpy as np
import pytest

from gaussianprocesspathmodelling_amd import GP, _abi
from gaussianprocesspathmodelling_amd import paths as gpaths

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from score_ref import LOG_2PI, kappa_bound, problem, score_ref  # noqa: E402

pytestmark = pytest.mark.gpu

SF2 = 1.5
LS = {1: 1.0, 3: (1.0, 1.5, 2.0)}
BLOCKS = (1, 15, 16, 17, 33, 64)          # 15 / 16 / 17: a tile edge of the Gram; 33: PATH_LENGTH; 64: the cap
KERNELS = ("rbf", "matern52", "matern32", "matern12")


def _ratios(got, ref, Lg, eps):
    """largest |got - ref| / bound over the blocks, for (logp, maha, logdet)"""
    logp, maha, logdet = (np.asarray(a, dtype=np.float64) for a in got)
    G = len(ref["kappa"])
    bound = eps * ref["kappa"][:, None] * (Lg + ref["maha"])
    return (float(np.max(np.abs(logp.reshape(G, -1) - ref["logp"]) / bound)),
            float(np.max(np.abs(maha.reshape(G, -1) - ref["maha"]) / bound)),
            float(np.max(np.abs(logdet - ref["logdet"]) / bound.min(axis=1))))


def _parity(kernel, d, k, dtype, sn2, eps):
    N = 1500 if (d == 3 and k == 2) else 300         # 1500: three column slices of V^T; 300: not a multiple of 128
    npdt = np.float32 if dtype == "float32" else np.float64
    worst = 0.0
    with GP(kernel, LS[d], SF2, sn2, dtype=dtype) as gp:
        fitted = False
        for Lg in BLOCKS:
            X, Y, Xq, Yq = (a.astype(npdt) for a in problem(N, d, k, 5, Lg, seed=100 * d + k))
            if not fitted:
                gp.fit(X, Y[:, 0] if k == 1 else Y)
                fitted = True
            got = gp.score_blocks(Xq, Yq[:, 0] if k == 1 else Yq, Lg, return_parts=True)
            assert got[0].shape == ((5,) if k == 1 else (5, k)) and got[2].shape == (5,) and got[0].dtype == npdt
            ref = score_ref(X, Y, Xq, Yq, Lg, kernel, LS[d], SF2, sn2, sn2, jitter=gp.jitter_used_)
            assert np.all(ref["kappa"] <= kappa_bound(Lg, SF2, sn2))
            r = _ratios(got, ref, Lg, eps)
            print(f"score parity {dtype} {kernel} d={d} k={k} N={N} Lg={Lg}: error / bound logp {r[0]:.3g} maha {r[1]:.3g} "
                  f"logdet {r[2]:.3g} (kappa max {ref['kappa'].max():.3g})")
            worst = max(worst, *r)
    print(f"score parity {dtype} {kernel} d={d} k={k}: largest error / bound {worst:.3g}")
    assert worst <= 1.0


@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("d", [1, 3])
@pytest.mark.parametrize("kernel", KERNELS)
def test_parity_with_the_reference_fp64(kernel, d, k):
    _parity(kernel, d, k, "float64", 1e-2, 1e-10)


@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("d", [1, 3])
@pytest.mark.parametrize("kernel", KERNELS)
def test_parity_with_the_reference_fp32(kernel, d, k):
    _parity(kernel, d, k, "float32", 5e-2, 1e-4)


# ---- one fitted model for the consistency / independence / isolation tests ---------------------------------------------
@pytest.fixture(scope="module")
def fitted():
    """N = 1500 (three column slices), d = 3 ARD, two targets, 40 blocks of 33 points"""
    X, Y, Xq, Yq = problem(1500, 3, 2, 40, 33, seed=7)
    gp = GP("matern32", LS[3], SF2, 1e-2).fit(X, Y)
    yield gp, X, Y, Xq, Yq
    gp.close()


def test_single_points_are_predicts_normal_density(fitted):
    gp, X, Y, Xq, Yq = fitted
    mean, var = gp.predict(Xq[:40], include_noise=True)
    logp, maha, logdet = gp.score_blocks(Xq[:40], Yq[:40], 1, return_parts=True)
    want_maha = (Yq[:40] - mean) ** 2 / var[:, None]
    want = -0.5 * want_maha - 0.5 * np.log(var)[:, None] - 0.5 * LOG_2PI
    bound = 1e-10 * 1.0 * (1 + want_maha)            # kappa of a 1 x 1 block is 1
    r = max(np.max(np.abs(logp - want) / bound), np.max(np.abs(maha - want_maha) / bound),
            np.max(np.abs(logdet - np.log(var)) / bound.min(axis=1)))
    print(f"score Lg=1 vs predict: largest error / bound {r:.3g}")
    assert r <= 1.0


def test_one_block_is_the_density_of_predicts_joint_covariance(fitted):
    gp, X, Y, Xq, Yq = fitted
    from scipy.linalg import cholesky, solve_triangular
    Lg = 48
    q, yq = Xq[100:100 + Lg], Yq[100:100 + Lg]
    mean, cov = gp.predict(q, return_cov=True, include_noise=True)
    ev = np.linalg.eigvalsh(cov)
    Ls = cholesky(cov, lower=True)
    w = solve_triangular(Ls, yq - mean, lower=True)
    ref = {"kappa": np.array([ev[-1] / ev[0]]), "maha": np.sum(w * w, axis=0)[None, :],
           "logdet": np.array([2.0 * np.sum(np.log(np.diag(Ls)))])}
    ref["logp"] = -0.5 * ref["maha"] - 0.5 * ref["logdet"][:, None] - 0.5 * Lg * LOG_2PI
    r = _ratios(gp.score_blocks(q, yq, Lg, return_parts=True), ref, Lg, 1e-10)
    print(f"score G=1 Lg=48 vs predict(return_cov): error / bound logp {r[0]:.3g} maha {r[1]:.3g} logdet {r[2]:.3g}")
    assert max(r) <= 1.0


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def test_a_block_does_not_depend_on_the_others(fitted):
    gp, X, Y, Xq, Yq = fitted
    full = gp.score_blocks(Xq, Yq, 33, return_parts=True)
    assert full[0].shape == (40, 2) and np.all(np.isfinite(full[0]))
    for b in (0, 17, 39):
        sl = slice(33 * b, 33 * (b + 1))
        alone = gp.score_blocks(Xq[sl], Yq[sl], 33, return_parts=True)
        assert _same(alone, [a[b:b + 1] for a in full]), f"block {b} alone differs from block {b} among 40"
    # block 17 at another position of another call
    order = np.r_[np.arange(33 * 17, 33 * 18), np.arange(0, 33 * 5)]
    moved = gp.score_blocks(Xq[order], Yq[order], 33, return_parts=True)
    assert _same([a[:1] for a in moved], [a[17:18] for a in full])


def test_batches_of_whole_blocks_give_the_same_bits(fitted, monkeypatch):
    gp, X, Y, Xq, Yq = fitted
    full = gp.score_blocks(Xq, Yq, 33, return_parts=True)
    monkeypatch.setenv("GPX_PRED_BATCH", "128")      # 3 blocks = 99 rows per batch: blocks would straddle 128-row edges
    small = gp.score_blocks(Xq, Yq, 33, return_parts=True)
    assert _same(small, full)


def test_results_do_not_depend_on_stream_timing(fitted):
    gp, X, Y, Xq, Yq = fitted
    lib = _abi.load()
    full = gp.score_blocks(Xq, Yq, 33, return_parts=True)
    try:
        for seed in (1, 2):
            lib.gpx_debug_set_delay(seed)
            assert _same(gp.score_blocks(Xq, Yq, 33, return_parts=True), full), f"delay seed {seed}"
    finally:
        lib.gpx_debug_set_delay(0)


def test_predict_is_unchanged_by_a_score_call(fitted):
    gp, X, Y, Xq, Yq = fitted
    before = gp.predict(Xq[:500])
    gp.score_blocks(Xq, Yq, 33)
    assert _same(gp.predict(Xq[:500]), before)


def test_a_singular_block_is_isolated(fitted):
    gp, X, Y, Xq, Yq = fitted
    rng = np.random.default_rng(3)
    G, Lg, bad = 9, 8, 4
    start = rng.uniform(0.0, 10.0, (G, 1, 3))
    q = start + 0.5 * np.arange(Lg)[None, :, None] * rng.choice([-1.0, 1.0], (G, 1, 3))
    yq = rng.standard_normal((G, Lg, 2))
    good = gp.score_blocks(np.delete(q, bad, axis=0).reshape(-1, 3), np.delete(yq, bad, axis=0).reshape(-1, 2), Lg,
                           include_noise=False, return_parts=True)
    assert gp.score_info_ == 0 and all(np.all(np.isfinite(a)) for a in good)
    q[bad] = q[bad, :1]                                # eight identical points: the latent covariance has rank 1
    got = gp.score_blocks(q.reshape(-1, 3), yq.reshape(-1, 2), Lg, include_noise=False, return_parts=True, on_bad="nan")
    assert gp.score_info_ in (0, bad + 1)
    if gp.score_info_:
        assert all(np.all(np.isnan(a[bad])) for a in got)
        with pytest.raises(np.linalg.LinAlgError, match=f"block {bad} "):
            gp.score_blocks(q.reshape(-1, 3), yq.reshape(-1, 2), Lg, include_noise=False)
    else:
        assert all(np.all(np.isfinite(a[bad])) for a in got)
    assert _same([np.delete(a, bad, axis=0) for a in got], good)


@pytest.mark.parametrize("kw", [{"dtype": "mixed"}, {"devices": [0], "transport": "local"}])
def test_mixed_and_group_handles_are_refused(kw):
    X, Y, Xq, Yq = problem(300, 1, 1, 4, 16, seed=11)
    with GP("rbf", 1.0, SF2, 1e-2, **kw) as gp:
        gp.fit(X, Y[:, 0])
        before = gp.predict(Xq)
        with pytest.raises(_abi.GpxError) as e:
            gp.score_blocks(Xq, Yq[:, 0], 16)
        assert e.value.code == _abi.E_UNSUPPORTED
        assert _same(gp.predict(Xq), before)


def test_device_tensors_in_device_tensors_out(fitted):
    import torch
    gp, X, Y, Xq, Yq = fitted
    want = gp.score_blocks(Xq[:330], Yq[:330], 33)
    dev = torch.device("cuda", gp.device)
    got = gp.score_blocks(torch.as_tensor(Xq[:330], device=dev), torch.as_tensor(Yq[:330], device=dev), 33)
    assert got.is_cuda and np.array_equal(got.cpu().numpy(), want)


# ---- paths ---------------------------------------------------------------------------------------------------------------
def _two_clusters(per_group=18, seed=9):
    rng = np.random.default_rng(seed)
    t = gpaths.Trajectories()
    groups = {0: [], 1: []}
    tt = np.arange(33, dtype=float) * 40.0
    for g in (0, 1):
        for p in range(per_group):
            tr = gpaths.Trajectory()
            ox, oy = rng.normal(0, 60, 2)
            for i in range(33):
                s = i / 32.0
                tr.add_point(tt[i], 4000.0 * g + ox + 1500.0 * s + 200.0 * np.sin(3 * s + g) + rng.normal(0, 15),
                             2500.0 * g + oy + 900.0 * s * s + rng.normal(0, 15))
            t.add_trajectory(f"G{g}P{p}", tr)
            groups[g].append(f"G{g}P{p}")
    return t, groups


def test_paths_are_assigned_to_the_cluster_that_explains_them():
    t, groups = _two_clusters()
    train = {g: groups[g][:12] for g in groups}
    held = groups[0][12:] + groups[1][12:]
    hp = dict(kernel="matern32", lengthscale=0.3, variance=1.0, noise=0.05)
    models = gpaths.fit_path_models(t, train, **hp)
    try:
        keys, LL = gpaths.path_log_likelihood_matrix(t, models, keys=held)
        assert keys == held and LL.shape == (12, 2)
        assert gpaths.assign_paths(t, models, keys=held) == {0: groups[0][12:], 1: groups[1][12:]}
        arr = t.as_array(held)
        worst = 0.0
        for c, (cid, m) in enumerate(models.items()):
            ll = m.log_likelihood(arr)
            assert ll.shape == (12, 2) and np.array_equal(ll.sum(axis=1), LL[:, c])
            X, Yraw, (lo, span) = gpaths.to_gp_inputs(t, train[cid])
            mu, sd = Yraw.mean(0), Yraw.std(0)
            ref = score_ref(X, (Yraw - mu) / sd, (arr[:, :, :1].reshape(-1, 1) - lo) / span,
                            (arr[:, :, 1:].reshape(-1, 2) - mu) / sd, 33, hp["kernel"], hp["lengthscale"], hp["variance"],
                            hp["noise"], hp["noise"], jitter=m.gp.jitter_used_)
            want = ref["logp"] - 33 * np.log(sd)[None, :]      # raw units: the Jacobian of the standardisation
            bound = 1e-10 * ref["kappa"][:, None] * (33 + ref["maha"])
            worst = max(worst, float(np.max(np.abs(ll - want) / bound)))
        print(f"path log-likelihood vs reference: largest error / bound {worst:.3g}")
        assert worst <= 1.0
    finally:
        for m in models.values():
            m.close()
