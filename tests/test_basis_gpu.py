"""GPU: explicit basis functions (gpx_set_basis / GP.fit(basis=)) against the dense fp64 reference of tests/basis_ref.py.

Bounds.  Those the suite already holds the same quantities to: mean and variance the 1e-6 contract at the head of
tests/test_gp_parity_gpu.py (|d mean| <= 1e-6 max(|ref|, 1e-6), |d var| <= 1e-6 max(ref, 1e-6 sf2)), alpha 1e-7 of its largest
entry, the likelihood 1e-9 relative, its gradient 1e-8 of its largest entry, the joint covariance 1e-6 as
tests/test_posterior_gpu.py (relative to max(|ref|, 1e-6 sf2)); fp32 handles the 2e-3 of tests/test_fp32_gpu.py (mean: of its
largest entry; variance: of sf2); fit_predict against fit + predict 1e-9 as tests/test_fit_predict_gpu.py; samples 1e-9 of the
largest as tests/test_posterior_gpu.py; block scores eps kappa_g (Lg + maha_g), eps = 1e-10, as tests/test_score_gpu.py, and
forecasts the forms of tests/test_within_gpu.py (mean eps kappa_g max(1, max |yo - mean_o|), covariance eps kappa_g s_g) with
s_g the largest prior variance of the block's rows in place of sf2: with a basis the prior of a row is not bounded by sf2
(it gains |u|^2).
beta_ and beta_cov_ have no precedent: BETA_TOL / BETA_COV_TOL are a decade above the largest error measured on an MI355X
over every fit of this file (profiles/basis_parity.json; cond(H^T K^-1 H) is 1e1 - 4e2 there), relative to the largest
entry of the reference's.  Every test prints its figures before it asserts."""
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
import basis_ref as br  # noqa: E402

pytestmark = pytest.mark.gpu

KERNEL, SF2, SN2 = "rbf", 1.5, 1e-2
BETA_TOL, BETA_COV_TOL = 1.5e-11, 7e-13         # fp64 handles: measured at most 1.38e-12 and 6.83e-14
BETA_TOL_F32, BETA_COV_TOL_F32 = 2e-3, 3e-5     # fp32 handles: measured at most 1.71e-4 and 2.99e-6
SHAPES = {
    "ragged": dict(N=300, d=2, k=2, M=70, block=0, ls=(0.3, 0.4), batch=None),        # ragged tiles, two targets
    "panels": dict(N=1500, d=3, k=1, M=200, block=256, ls=(0.3, 0.2, 0.25), batch=128),  # several panels, predict batches
    "p63": dict(N=300, d=31, k=1, M=40, block=0, ls=2.0, batch=None),                 # quadratic: k + p = 64, the limit
}


@functools.lru_cache(maxsize=None)
def _data(shape):
    s = SHAPES[shape]
    return br.trend_problem(s["N"], s["d"], s["k"], s["M"], seed=s["N"] + s["d"])


@functools.lru_cache(maxsize=None)
def _weights(shape):
    return np.exp(np.random.default_rng(5).uniform(np.log(0.1), np.log(10.0), SHAPES[shape]["N"]))


@functools.lru_cache(maxsize=None)
def _ref(shape, basis, weighted=False):
    X, Y, Xs = _data(shape)
    ref = br.BasisGP(KERNEL, SHAPES[shape]["ls"], SF2, SN2, basis).fit(X, Y, _weights(shape) if weighted else None)
    mean, cov = ref.joint(Xs)
    return ref, mean, cov


def _gp(shape, **kw):
    return GP(KERNEL, SHAPES[shape]["ls"], SF2, SN2, jitter=0.0, block=SHAPES[shape]["block"], **kw)


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def _mean_var_errors(mean, var, mr, vr):
    dm = np.abs(np.asarray(mean, np.float64).reshape(mr.shape) - mr) / np.maximum(np.abs(mr), 1e-6)
    dv = np.abs(np.asarray(var, np.float64) - vr) / np.maximum(vr, 1e-6 * SF2)
    return float(dm.max()), float(dv.max())


def _beta_errors(gp, ref):
    eb = np.max(np.abs(gp.beta_.reshape(ref.beta.shape) - ref.beta)) / np.abs(ref.beta).max()
    ec = np.max(np.abs(gp.beta_cov_ - ref.beta_cov)) / np.abs(ref.beta_cov).max()
    return float(eb), float(ec)


def _check_fit(gp, shape, basis, weighted=False, tag=""):
    """every quantity of a fitted fp64 model against the reference"""
    X, Y, Xs = _data(shape)
    ref, mr, cr = _ref(shape, basis, weighted)
    mean, var = gp.predict(Xs)
    em, ev = _mean_var_errors(mean, var, mr, np.diag(cr))
    ea = np.max(np.abs(gp.alpha_.reshape(ref.alpha.shape) - ref.alpha)) / np.abs(ref.alpha).max()
    eb, ec = _beta_errors(gp, ref)
    lml = gp.log_marginal_likelihood(Y)
    el = abs(lml - ref.lml()) / abs(ref.lml())
    lml2, grad = gp.lml_gradient()
    want = ref.lml_gradient()
    eg = np.max(np.abs(grad - want)) / np.abs(want).max()
    m2, cov = gp.predict(Xs, return_cov=True)
    ecov = np.max(np.abs(cov - cr) / np.maximum(np.abs(cr), 1e-6 * SF2))
    m_only = gp.predict(Xs, return_var=False)
    eo = np.max(np.abs(m_only - mean)) / max(1.0, np.abs(mean).max())
    print(f"basis parity {tag}{shape} {basis}: mean {em:.2e} var {ev:.2e} alpha {ea:.2e} beta {eb:.2e} beta_cov {ec:.2e} "
          f"lml {el:.2e} grad {eg:.2e} cov {ecov:.2e} mean-only {eo:.2e} cond(A) {np.linalg.cond(ref.A):.3g}")
    assert gp.basis_ == basis and gp.beta_.shape == ((ref.beta.shape[0],) if ref.y1d else ref.beta.shape)
    assert em <= 1e-6 and ev <= 1e-6
    assert ea <= 1e-7
    assert eb <= BETA_TOL and ec <= BETA_COV_TOL
    assert el <= 1e-9 and abs(lml2 - lml) <= 1e-10 * abs(lml)
    assert eg <= 1e-8
    assert ecov <= 1e-6 and np.array_equal(cov, cov.T)
    assert np.max(np.abs(np.diag(cov) - var)) <= 1e-10 * max(SF2, var.max())
    assert np.max(np.abs(m2 - mean)) <= 1e-9 * np.abs(mean).max()
    assert eo <= 1e-9
    assert abs(gp.log_det_ - ref.logdet) <= 1e-9 * max(1.0, abs(ref.logdet))
    return mean, var


@pytest.mark.parametrize("basis", br.BASES)
@pytest.mark.parametrize("shape", ["ragged", "panels"])
def test_parity_with_the_reference(shape, basis, monkeypatch):
    X, Y, Xs = _data(shape)
    with _gp(shape) as gp:
        gp.fit(X, Y, basis=basis)
        assert gp.info_ == 0 and gp.get_state()["fitted"]["basis"] == basis
        mean, var = _check_fit(gp, shape, basis)
        if SHAPES[shape]["batch"]:          # 128 rows is the smallest batch: M = 200 goes through two, 3 M / 2 through three
            X3 = np.concatenate([Xs, Xs[:100] + 0.01])
            full = gp.predict(X3)
            monkeypatch.setenv("GPX_PRED_BATCH", str(SHAPES[shape]["batch"]))
            assert _same(gp.predict(Xs), (mean, var))
            assert _same(gp.predict(X3), full)
            assert np.array_equal(gp.predict(X3, return_var=False), gp.predict(X3, return_var=False))
            _check_fit(gp, shape, basis, tag="batched ")


def test_the_largest_basis_that_fits_the_bordered_rows_and_the_two_refusals_at_the_fit():
    """d = 31, quadratic, k = 1: p = 63 and k + p = 64 is accepted; k = 2 is refused, and so is N < p, both before
    anything is computed: the previous fit still predicts the same bits"""
    X, Y, Xs = _data("p63")
    with _gp("p63") as gp:
        gp.fit(X, Y, basis="quadratic")
        assert gp.beta_.shape == (63,) and gp.beta_cov_.shape == (63, 63)
        mean, var = _check_fit(gp, "p63", "quadratic")
        with pytest.raises(GpxError) as e:
            gp.fit(X, np.stack([Y, Y], axis=1), basis="quadratic")
        msg = str(e.value)
        assert e.value.code == _abi.E_ARG and "k = 2" in msg and "p = 63" in msg and "64" in msg
        assert _same(gp.predict(Xs), (mean, var))
        with pytest.raises(GpxError) as e:
            gp.fit_predict(X, np.stack([Y, Y], axis=1), Xs, basis="quadratic")
        assert e.value.code == _abi.E_ARG
        assert _same(gp.predict(Xs), (mean, var))
        with pytest.raises(GpxError) as e:
            gp.fit(X[:40], Y[:40], basis="quadratic")                 # N = 40 < p = 63
        assert e.value.code == _abi.E_ARG and "N >= p" in str(e.value)
        assert _same(gp.predict(Xs), (mean, var))
    X2, Y2, Xs2 = _data("ragged")
    with _gp("ragged") as gp:
        before = gp.fit(X2, Y2, basis="linear").predict(Xs2)
        with pytest.raises(GpxError) as e:
            gp.fit(X2[:4], Y2[:4], basis="quadratic")                 # N = 4, d = 2: p = 5
        assert e.value.code == _abi.E_ARG
        assert _same(gp.predict(Xs2), before) and gp.basis_ == "linear"


def test_bad_values_of_the_set_call_keep_the_previous_setting():
    X, Y, Xs = _data("ragged")
    with _gp("ragged") as gp:
        b, p = C.c_int32(-7), C.c_int32(-7)
        assert gp._lib.gpx_get_basis(gp._h, C.byref(b), C.byref(p), None, None) == _abi.E_ARG   # no fit yet
        assert gp._lib.gpx_set_basis(gp._h, _abi.BASIS_IDS["linear"]) == 0
        for bad in (4, -1, 99):
            assert gp._lib.gpx_set_basis(gp._h, bad) == _abi.E_ARG
        gp._basis_set = "linear"                                      # (what the raw call above left in the handle)
        gp.fit(X, Y, basis="linear")
        assert gp.basis_ == "linear" and gp.beta_.shape == (3, 2)
        gp.fit(X, Y)
        beta = np.full(4, 9.0)
        assert gp._lib.gpx_get_basis(gp._h, C.byref(b), C.byref(p), _abi.dptr(beta), None) == 0
        assert b.value == 0 and p.value == 0 and np.array_equal(beta, np.full(4, 9.0))          # nothing else written
        assert gp.basis_ is None and gp.beta_.shape == (0, 2) and "basis" not in gp.get_state()["fitted"]


@pytest.mark.parametrize("basis", br.BASES)
def test_fit_predict_is_fit_then_predict(basis):
    X, Y, Xs = _data("panels")
    ref, mr, cr = _ref("panels", basis)
    with _gp("panels") as gp:
        m2, v2 = gp.fit(X, Y, basis=basis).predict(Xs)
        a2, b2 = gp.alpha_.copy(), gp.beta_.copy()
        mean, var = gp.fit_predict(X, Y, Xs, basis=basis)
        em, ev = _mean_var_errors(mean, var, mr, np.diag(cr))
        rm = np.max(np.abs(mean - m2) / np.maximum(np.abs(m2), 1e-6))
        rv = np.max(np.abs(var - v2) / np.maximum(v2, 1e-6 * SF2))
        print(f"fit_predict {basis}: against the reference mean {em:.2e} var {ev:.2e}; against the two calls {rm:.2e} {rv:.2e}")
        assert gp.info_ == 0 and em <= 1e-6 and ev <= 1e-6
        assert (rm <= 1e-9 or np.max(np.abs(mean - m2)) <= 1e-10 * np.max(np.abs(m2))) and rv <= 1e-9
        assert np.array_equal(gp.alpha_, a2) and np.array_equal(gp.beta_, b2) and gp.basis_ == basis
        assert _same(gp.predict(Xs), (m2, v2))


@pytest.mark.parametrize("basis", ["constant", "quadratic"])
def test_fp32_handles(basis):
    X, Y, Xs = _data("ragged")
    ref, mr, cr = _ref("ragged", basis)
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)  # noqa: E731
    with _gp("ragged", dtype="float32") as gp:
        mean, var = gp.fit(f32(X), f32(Y), basis=basis).predict(f32(Xs))
        m2, cov = gp.predict(f32(Xs), return_cov=True)
        em = np.max(np.abs(mean - mr)) / np.abs(mr).max()
        ev = np.max(np.abs(var - np.diag(cr))) / SF2
        ec = np.max(np.abs(cov.astype(np.float64) - cr)) / SF2
        eb, ebc = _beta_errors(gp, ref)
        print(f"fp32 basis parity {basis}: mean {em:.2e} (of max|mean|) var {ev:.2e} cov {ec:.2e} (of sf2) beta {eb:.2e} "
              f"beta_cov {ebc:.2e}")
        assert mean.dtype == np.float32 and var.dtype == np.float32 and gp.beta_.dtype == np.float64
        assert em <= 2e-3 and ev <= 2e-3 and ec <= 2e-3 and np.array_equal(cov, cov.T)
        assert eb <= BETA_TOL_F32 and ebc <= BETA_COV_TOL_F32


def test_samples_are_the_mean_plus_the_factor_of_the_corrected_covariance_times_z():
    X, Y, Xs = _data("ragged")
    M, S, k = len(Xs), 5, 2
    z = np.random.default_rng(3).standard_normal((S, M, k))
    with _gp("ragged") as gp:
        gp.fit(X, Y, basis="linear")
        out = gp.sample_y(Xs, S, include_noise=True, z=z)
        mean, cov = gp.predict(Xs, return_cov=True)
        j = gp.sample_jitter_
    assert out.shape == (M, k, S) and np.array_equal(cov, cov.T)
    Ls = cholesky(cov + (SN2 + j) * np.eye(M), lower=True)
    want = mean[:, :, None] + np.einsum("mn,snc->mcs", Ls, z)
    err = np.max(np.abs(out - want)) / np.max(np.abs(want))
    print(f"samples vs mean + chol(cov) z: {err:.2e}")
    assert err <= 1e-9


@functools.lru_cache(maxsize=None)
def _blocks():
    """5 blocks of 33 = 20 observed + 13 forecast rows, d = 3, one target"""
    return br.block_queries(5, 33, 3, 1, seed=17)


@pytest.fixture(scope="module")
def scored():
    X, Y, _ = _data("panels")
    gp = _gp("panels").fit(X, Y, basis="quadratic")
    yield gp
    gp.close()


def test_block_scores_against_the_dense_reference(scored):
    gp = scored
    Xq, Yq = _blocks()
    ref = _ref("panels", "quadratic")[0].score(Xq, Yq, 33, SN2)
    logp, maha, logdet = gp.score_blocks(Xq, Yq[:, 0], 33, return_parts=True)
    bound = 1e-10 * ref["kappa"][:, None] * (33 + ref["maha"])
    r = (np.max(np.abs(logp[:, None] - ref["logp"]) / bound), np.max(np.abs(maha[:, None] - ref["maha"]) / bound),
         np.max(np.abs(logdet - ref["logdet"]) / bound.min(axis=1)))
    print(f"basis block scores: error / bound logp {r[0]:.3g} maha {r[1]:.3g} logdet {r[2]:.3g} "
          f"(kappa max {ref['kappa'].max():.3g})")
    assert max(r) <= 1.0


def test_block_forecasts_against_the_dense_reference(scored):
    gp = scored
    Xq, Yq = _blocks()
    B = Xq.reshape(5, 33, 3)
    Xo, Xp, Yo = B[:, :20].reshape(-1, 3), B[:, 20:].reshape(-1, 3), Yq.reshape(5, 33, 1)[:, :20].reshape(-1, 1)
    ref = _ref("panels", "quadratic")[0].forecast(Xo, Yo, Xp, 5, SN2)
    mean, cov, logp = gp.forecast_blocks(Xo, Yo[:, 0], Xp, blocks=5, return_logp=True)
    mean2, var = gp.forecast_blocks(Xo, Yo[:, 0], Xp, blocks=5, return_cov=False)
    kap = ref["kappa"]
    bm = 1e-10 * kap * np.maximum(1.0, ref["resid"])
    bc = 1e-10 * kap * ref["scale"]
    bl = 1e-10 * kap[:, None] * (20 + ref["maha"])
    r = (np.max(np.abs(mean.reshape(5, 13, 1) - ref["mean"]) / bm[:, None, None]),
         np.max(np.abs(cov - ref["cov"]) / bc[:, None, None]),
         np.max(np.abs(var.reshape(5, 13) - np.einsum("gii->gi", ref["cov"])) / bc[:, None]),
         np.max(np.abs(logp[:, None] - ref["logp"]) / bl))
    print(f"basis block forecasts: error / bound mean {r[0]:.3g} cov {r[1]:.3g} var {r[2]:.3g} logp {r[3]:.3g} "
          f"(kappa max {kap.max():.3g})")
    assert max(r) <= 1.0 and np.array_equal(mean, mean2)


def test_a_block_does_not_depend_on_the_others_its_position_or_the_batch(scored, monkeypatch):
    gp = scored
    Xq, Yq = _blocks()
    y = Yq[:, 0]

    def both(idx, G):
        B = Xq[idx].reshape(G, 33, 3)
        Xo, Xp, Yo = B[:, :20].reshape(-1, 3), B[:, 20:].reshape(-1, 3), y[idx].reshape(G, 33)[:, :20].reshape(-1)
        return (gp.score_blocks(Xq[idx], y[idx], 33, return_parts=True),
                gp.forecast_blocks(Xo, Yo, Xp, blocks=G, return_logp=True))

    full_s, full_f = both(np.arange(165), 5)
    sl = np.arange(33 * 3, 33 * 4)
    alone_s, alone_f = both(sl, 1)                                   # block 3 alone
    assert _same(alone_s, [a[3:4] for a in full_s])
    assert np.array_equal(alone_f[0], full_f[0][13 * 3:13 * 4]) and np.array_equal(alone_f[1][0], full_f[1][3])
    assert np.array_equal(alone_f[2], full_f[2][3:4])
    order = np.r_[sl, np.arange(0, 66)]                              # ... and first of another call
    moved_s, moved_f = both(order, 3)
    assert _same([a[:1] for a in moved_s], [a[3:4] for a in full_s])
    assert np.array_equal(moved_f[0][:13], full_f[0][13 * 3:13 * 4]) and np.array_equal(moved_f[1][0], full_f[1][3])
    monkeypatch.setenv("GPX_PRED_BATCH", "128")                      # 3 blocks = 99 rows per batch
    small_s, small_f = both(np.arange(165), 5)
    assert _same(small_s, full_s) and _same(small_f, full_f)


@pytest.mark.parametrize("basis", ["constant", "quadratic"])
def test_noise_weights_compose(basis):
    X, Y, Xs = _data("ragged")
    with _gp("ragged") as gp:
        gp.fit(X, Y, basis=basis, noise_weights=_weights("ragged"))
        _check_fit(gp, "ragged", basis, weighted=True, tag="weighted ")


def test_optimize_with_a_basis_climbs_the_profile_likelihood():
    """data with a linear trend plus a smooth term: the search with basis="linear" ends no lower than it starts, its final
    gradient is the central difference of the profile likelihood, and it does not end where the zero-mean search ends"""
    X, Y, _ = br.trend_problem(200, 1, 1, 1, seed=8)
    Y = Y + 25.0 * X[:, 0]
    start = dict(lengthscale=0.5, variance=1.0, noise=0.1)
    with GP(KERNEL, jitter=1e-10, **start) as gp:
        l0 = gp.fit(X, Y, basis="linear").log_marginal_likelihood(Y)
        res = gp.optimize(X, Y, basis="linear", maxiter=25)
        l1, grad = gp.lml_gradient()
        ls_basis = gp.lengthscale.copy()
        v0 = np.log(np.concatenate([gp.lengthscale, [gp.variance, gp.noise]]))
        assert gp.basis_ == "linear" and abs(l1 + res.fun) <= 1e-9 * abs(l1)
    print(f"optimize(basis='linear'): lml {l0:.3f} -> {l1:.3f}, lengthscale {ls_basis}")
    assert l1 >= l0
    h = 1e-4
    for i in range(3):
        f = []
        for sgn in (+1, -1):
            v = v0.copy()
            v[i] += sgn * h
            with GP(KERNEL, np.exp(v[:1]), float(np.exp(v[1])), float(np.exp(v[2])), jitter=1e-10) as g2:
                f.append(g2.fit(X, Y, basis="linear").log_marginal_likelihood(Y))
        fd = (f[0] - f[1]) / (2 * h)
        # (at an optimum the gradient is near 0 and cannot scale its own bound: the central difference's truncation
        # error h^2 / 6 |f'''| is about 1e-8 N, so the floor of the scale is 1)
        assert abs(fd - grad[i]) <= 2e-5 * max(np.abs(grad).max(), 1.0), (i, fd, grad[i])
    with GP(KERNEL, jitter=1e-10, **start) as gp:
        gp.optimize(X, Y, maxiter=25)
        print(f"optimize(basis=None): lengthscale {gp.lengthscale}")
        assert gp.basis_ is None and not np.allclose(gp.lengthscale, ls_basis, rtol=1e-3)


def test_a_handle_without_a_basis_returns_the_same_bits_before_and_after_one():
    X, Y, Xs = _data("ragged")
    with _gp("ragged") as gp:
        gp.fit(X, Y)
        first = gp.predict(Xs) + (gp.predict(Xs, return_var=False), gp.alpha_.copy(), gp.predict(Xs, return_cov=True)[1])
        ld = gp.log_det_
        state = gp.get_state()
        with_basis = gp.fit(X, Y, basis="linear").predict(Xs)
        assert not np.array_equal(with_basis[0], first[0])
        gp.fit(X, Y, basis=None)
        last = gp.predict(Xs) + (gp.predict(Xs, return_var=False), gp.alpha_.copy(), gp.predict(Xs, return_cov=True)[1])
        assert _same(first, last) and gp.log_det_ == ld and gp.get_state() == state and gp.basis_ is None
        m, v = gp.fit_predict(X, Y, Xs)
        gp.fit_predict(X, Y, Xs, basis="constant")
        assert _same(gp.fit_predict(X, Y, Xs), (m, v))


# ---- refusals ----------------------------------------------------------------------------------------------------------
REFUSED_HANDLES = {
    "mixed": dict(dtype="mixed"),
    "group": dict(devices=1, transport="local"),
    "communicator": dict(device=0, world=1, rank=0, comm="rccl"),
}


def _raw_predict(gp, Xs, like):
    mean, var = np.empty_like(like[0]), np.empty_like(like[1])
    rc = gp._lib.gpx_predict(gp._h, C.c_void_p(Xs.ctypes.data), len(Xs), C.c_void_p(mean.ctypes.data),
                             C.c_void_p(var.ctypes.data), _abi.MEM_HOST)
    assert rc == 0
    return mean, var


@pytest.mark.parametrize("which", list(REFUSED_HANDLES))
def test_handles_that_do_not_serve_a_basis_keep_the_previous_fit(which):
    X, Y, Xs = _data("ragged")
    with GP(KERNEL, SHAPES["ragged"]["ls"], SF2, SN2, **REFUSED_HANDLES[which]) as gp:
        gp.fit(X, Y)
        before = gp.predict(Xs)
        for call in (lambda: gp.fit(X, Y, basis="linear"), lambda: gp.fit_predict(X, Y, Xs, basis="linear")):
            with pytest.raises(GpxError) as e:
                call()
            assert e.value.code == _abi.E_UNSUPPORTED and "basis" in str(e.value)
            assert _same(_raw_predict(gp, Xs, before), before)       # the refused fit computed nothing
            assert _same(gp.predict(Xs), before)
        assert _same(gp.fit(X, Y).predict(Xs), before)               # cleared: fits as before


def test_a_basis_with_observation_kinds_or_path_ids_is_refused():
    X, Y, Xs = _data("ragged")
    with _gp("ragged") as gp:
        before = gp.fit(X, Y, basis="constant").predict(Xs)
        der = (X[:5], 0, np.zeros((5, 2)))
        ids = np.arange(len(X), dtype=np.int32) // 10
        for kw in (dict(derivatives=der), dict(path_ids=ids, path_variance=0.3)):
            with pytest.raises(GpxError) as e:
                gp.fit(X, Y, basis="constant", **kw)
            assert e.value.code == _abi.E_UNSUPPORTED and "basis" in str(e.value)
            assert _same(_raw_predict(gp, Xs, before), before)
        got = gp.fit(X, Y, basis="constant", path_ids=ids, path_variance=0.0).predict(Xs)   # ids without effect: allowed
        assert _same(got, before)


def test_calls_a_fit_with_a_basis_refuses():
    X, Y, Xs = _data("ragged")
    with _gp("ragged") as gp:
        gp.fit(X, Y, basis="linear")
        before = gp.predict(Xs)
        N = len(X)
        calls = {
            "update": lambda: gp.update(X[:3] + 0.01, Y[:3]),
            "update weighted": lambda: gp.update(X[:3] + 0.01, Y[:3], noise_weights=np.ones(3)),
            "remove": lambda: gp.remove(0, 5),
            "predict_gradient": lambda: gp.predict_gradient(Xs),
            "predict path_ids": lambda: gp.predict(Xs, path_ids=0),
            "predict_cov path_ids": lambda: gp.predict(Xs, return_cov=True, path_ids=0),
            "sample path_ids": lambda: gp.sample_y(Xs, 2, path_ids=0),
            "predict_gradient path_ids": lambda: gp.predict_gradient(Xs, path_ids=0),
        }
        for name, call in calls.items():
            with pytest.raises(GpxError) as e:
                call()
            assert e.value.code == _abi.E_UNSUPPORTED and "basis" in str(e.value), name
            assert _same(gp.predict(Xs), before) and gp._N == N, name
        info = C.c_int64(0)
        p = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
        xn, yn = np.ascontiguousarray(X[:3] + 0.01), np.ascontiguousarray(Y[:3])
        rc = gp._lib.gpx_append_rows(gp._h, p(xn), p(yn), None, None, None, 3, _abi.MEM_HOST, C.byref(info))
        assert rc == _abi.E_UNSUPPORTED and b"basis" in gp._lib.gpx_last_error(gp._h)
        assert _same(gp.predict(Xs), before)
        # the gradient calls are served: on such a fit the three are one
        l0, g0 = gp.lml_gradient()
        l1, g1 = gp.lml_gradient(derivative_noise=True)
        l2, g2 = gp.lml_gradient(path=True)
        assert l0 == l1 == l2 and np.array_equal(g0, g1[:len(g0)]) and np.array_equal(g0, g2[:len(g0)])
