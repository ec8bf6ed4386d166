"""GPU: the mixed-precision mode (BASELINE.json configs[4]): fp32 factorisation
on the fp32 MFMA engine, alpha refined in fp64 against the matrix-free fp64 kernel, posterior
mean in fp64.  The refined mean is pinned against the fp64 oracle at a stated tolerance: 1e-6
elementwise (north_star's own bar) after 3 iterations on these problems, where the pure-fp32
path of test_fp32_gpu.py is only good to ~1e-3; the variance keeps fp32 accuracy (by design:
it is never refined — GP docstring).  The default is ADAPTIVE (refine until the relative residual is
<= 1e-10 or stops contracting); the same bar at the config's own size (N = 65536, where 3
iterations are NOT enough) is tests/test_full_size_gpu.py."""
import numpy as np
import pytest

from gaussianprocesspathmodelling_amd import GP, GpxError
from oracle.gp_oracle import OracleGP, synthetic_problem

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("N,M,k,kernel,ls,noise", [
    (2500, 130, 1, "matern52", (0.3, 0.2, 0.25), 1e-2),
    (4000, 300, 2, "rbf", (0.3, 0.2, 0.25), 1e-2),
    (1000, 77, 1, "rbf", 0.25, 1e-2),
    (2700, 90, 5, "rbf", 0.25, 1e-2),          # 3 .. 8 targets: the KC = 8 instantiation of the refinement kernels; three
    (3300, 64, 8, "matern52", 0.3, 1e-2),      # panels, the last one 640 / 256 wide (streaming few-right-hand-side solves)
])
def test_refined_mean_meets_the_fp64_bar(N, M, k, kernel, ls, noise):
    X, y, Xs = synthetic_problem(N, 3, M, seed=N)
    Y = y if k == 1 else np.stack([np.cos((c + 1) * y) if c else y for c in range(k)], axis=1)
    ref = OracleGP(kernel, ls, 1.5, noise, jitter=0.0).fit(X, Y)
    mr, vr = ref.predict(Xs)
    with GP(kernel, ls, 1.5, noise, jitter=0.0, dtype="mixed", refine=3) as gp:
        mean, var = gp.fit(X, Y).predict(Xs)
        tm = gp.timings_
        assert gp.info_ == 0 and mean.dtype == np.float64 and var.dtype == np.float64
        em = np.max(np.abs(mean - mr) / np.maximum(np.abs(mr), 1e-6))
        ea = np.max(np.abs(gp.alpha_ - ref.alpha_)) / np.max(np.abs(ref.alpha_))
        ev = np.max(np.abs(var - vr)) / 1.5
        print(f"mixed N={N} {kernel} k={k}: residual {tm['refine_resid0']:.1e} -> {tm['refine_resid']:.1e}, "
              f"mean rel {em:.1e}, alpha {ea:.1e}, var err/sf2 {ev:.1e}")
        assert tm["refine_resid"] < 1e-3 * tm["refine_resid0"]      # the refinement converges
        assert em <= 1e-6 and ea <= 1e-7                             # fp64-grade mean and alpha
        assert ev <= 2e-3                                            # variance: fp32 accuracy
        m_only = gp.predict(Xs, return_var=False)
        assert np.array_equal(m_only, mean)


def test_default_refinement_is_adaptive_and_meets_the_bar():
    X, y, Xs = synthetic_problem(4000, 3, 300, seed=11)
    ref = OracleGP("rbf", (0.3, 0.2, 0.25), 1.5, 1e-2, jitter=0.0).fit(X, y)
    mr, _ = ref.predict(Xs)
    with GP("rbf", (0.3, 0.2, 0.25), 1.5, 1e-2, jitter=0.0, dtype="mixed") as gp:      # refine=0: adaptive
        mean, _ = gp.fit(X, y).predict(Xs)
        tm = gp.timings_
        em = np.max(np.abs(mean - mr) / np.maximum(np.abs(mr), 1e-6))
        print(f"adaptive: {tm['refine_iters']:.0f} iterations, residual {tm['refine_resid0']:.1e} -> {tm['refine_resid']:.1e}, mean rel {em:.1e}")
        assert 1 <= tm["refine_iters"] <= 12 and tm["refine_resid"] <= 1e-10 and em <= 1e-6
        st = gp.get_state()
        assert st["refine"] == 0
    with GP("rbf", 0.25, dtype="mixed", refine=4) as gp:
        assert GP.from_state(gp.get_state()).refine == 4


def test_each_refinement_step_contracts_the_residual():
    X, y, Xs = synthetic_problem(3000, 3, 50, seed=3)
    res = []
    for it in (1, 2, 4):
        with GP("rbf", 0.25, 1.5, 1e-2, jitter=0.0, dtype="mixed", refine=it) as gp:
            gp.fit(X, y)
            res.append(gp.timings_["refine_resid"])
    assert res[1] < 0.1 * res[0] and res[2] <= res[1]


def test_mixed_limits():
    X, y, _ = synthetic_problem(300, 3, 1, seed=1)
    with GP("rbf", 0.3, dtype="mixed") as gp:
        with pytest.raises(GpxError, match="8 target"):
            gp.fit(X, np.zeros((300, 9)))
        gp.fit(X, y)
        with pytest.raises(GpxError):
            gp.lml_gradient()


@pytest.mark.parametrize("N,M,block,k", [(3000, 100, 256, 1), (3000, 100, 512, 3), (5000, 64, 2048, 1), (300, 40, 0, 2),
                                         (1024, 10, 128, 8), (4096, 200, 1024, 1)])
def test_refinement_across_panel_widths(N, M, block, k):
    """The refinement's streaming few-right-hand-side solves work with the fit's block inverses: every panel width up to
    1024 and its multiples (2048: 1024-sub-blocks of the wide inverses; other widths above 1024: the slab path), a single panel, a ragged last panel, 1 .. 8 targets — adaptive default, 1e-6 on the mean."""
    X, y, Xs = synthetic_problem(N, 3, M, seed=N + block)
    Y = y if k == 1 else np.stack([np.cos((c + 1) * y) if c else y for c in range(k)], axis=1)
    ref = OracleGP("rbf", 0.25, 1.5, 1e-2, jitter=0.0).fit(X, Y)
    mr, vr = ref.predict(Xs)
    with GP("rbf", 0.25, 1.5, 1e-2, jitter=0.0, dtype="mixed", block=block) as gp:
        mean, var = gp.fit(X, Y).predict(Xs)
        em = np.max(np.abs(mean - mr) / np.maximum(np.abs(mr), 1e-6))
        ea = np.max(np.abs(gp.alpha_ - ref.alpha_)) / np.max(np.abs(ref.alpha_))
        assert gp.info_ == 0 and em <= 1e-6 and ea <= 1e-7
        assert 1 <= gp.timings_["refine_iters"] <= 12 and gp.timings_["refine_resid"] <= 2e-10


@pytest.mark.parametrize("ndev,N,M,k,kernel,nb,repl", [
    (2, 2500, 130, 1, "matern52", 256, 1), (4, 4000, 300, 2, "rbf", 256, 0), (3, 2700, 90, 5, "rbf", 128, 0),
    (4, 3300, 64, 8, "matern52", 512, 1), (8, 3000, 100, 1, "rbf", 128, 0), (2, 9000, 200, 1, "rbf", 0, -1),
])
def test_mixed_mode_on_a_shard_meets_the_fp64_bar(monkeypatch, ndev, N, M, k, kernel, nb, repl):
    """Round 4: mixed precision on the row-block shard (it was unsharded only).  The fp32 factorisation is sharded; the
    fp64 refinement of alpha is the same replicated matrix-free work on every rank, its fp32 solves local (replicated
    factor: the streaming few-right-hand-side solver with the block inverses every rank keeps) or collective (factor
    only held distributed: the sweeps of the alpha solve).  Adaptive default: 1e-6 on the mean, 1e-7 on alpha against
    the fp64 oracle; variance fp32-grade, through the sharded fp32 predict."""
    if nb:
        monkeypatch.setenv("GPX_NB_SHARD", str(nb))
    else:
        monkeypatch.delenv("GPX_NB_SHARD", raising=False)
    if repl >= 0:
        monkeypatch.setenv("GPX_SHARD_REPLICATE", str(repl))
    ls, noise = (0.3, 0.2, 0.25), 1e-2
    X, y, Xs = synthetic_problem(N, 3, M, seed=N + ndev)
    Y = y if k == 1 else np.stack([np.cos((c + 1) * y) if c else y for c in range(k)], axis=1)
    ref = OracleGP(kernel, ls, 1.5, noise, jitter=0.0).fit(X, Y)
    mr, vr = ref.predict(Xs)
    with GP(kernel, ls, 1.5, noise, jitter=0.0, dtype="mixed", devices=ndev, oversubscribe=True) as gp:
        mean, var = gp.fit(X, Y).predict(Xs)
        tm = gp.timings_
        assert gp.info_ == 0 and mean.dtype == np.float64 and var.dtype == np.float64
        em = np.max(np.abs(mean - mr) / np.maximum(np.abs(mr), 1e-6))
        ea = np.max(np.abs(gp.alpha_ - ref.alpha_)) / np.max(np.abs(ref.alpha_))
        ev = np.max(np.abs(var - vr)) / 1.5
        print(f"mixed shard P={ndev} N={N} repl={repl}: {tm['refine_iters']:.0f} iterations, residual "
              f"{tm['refine_resid0']:.1e} -> {tm['refine_resid']:.1e}, mean rel {em:.1e}, alpha {ea:.1e}, var err/sf2 {ev:.1e}")
        assert em <= 1e-6 and ea <= 1e-7 and ev <= 2e-3
        assert 1 <= tm["refine_iters"] <= 12 and tm["refine_resid"] <= 2e-10
        m_only = gp.predict(Xs, return_var=False)
        assert np.array_equal(m_only, mean)
        m2, v2 = gp.fit(X, Y).predict(Xs)            # refit on the same group
        assert np.array_equal(m2, mean) and np.array_equal(v2, var)
