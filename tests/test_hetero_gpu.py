"""GPU: per-observation noise weights (K = sf2 k(X,X) + diag(sn2 w_i + jitter); include/gpx.h) through
fit, predict, fit_predict, the LML gradient, optimize, update, score_blocks and the mixed mode, against the dense fp64
reference of tests/hetero_ref.py (itself checked in tests/test_hetero_ref.py).

Standard inputs (hetero_ref): X uniform in [0, 1]^d, sf2 = 1.5, sn2 = 1e-2, length scale 0.3, the default jitter, weights
log-uniform in [0.1, 10] with every 97th one 0.  cond(K) <= 2.1e6 at N = 1153 (RBF; less for the Matern families), and the
weights move alpha by 25 times its largest entry (tests/test_hetero_ref.py): no build that drops or mis-indexes the vector
passes the parity bars.  Shapes: N = 300 (one panel, ragged 64-tile) and N = 1153 with block = 128 (ten panels, ragged).
Bars are the project's own: alpha 1e-7 of its largest entry, logdet and LML 1e-9 (tests/test_gp_parity_gpu.py), mean and
variance the 1e-6 contract with its floors, two routes of the library against each other 1e-9
(tests/test_fit_predict_gpu.py, tests/test_append_gpu.py)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from gaussianprocesspathmodelling_amd import GP, _abi

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hetero_ref as hr  # noqa: E402
from score_ref import kappa_bound  # noqa: E402
from score_ref import problem as score_problem  # noqa: E402

pytestmark = pytest.mark.gpu

SF2, SN2 = hr.SF2, hr.SN2
KERNELS = ("rbf", "matern52", "matern32", "matern12")
SHAPES = [(300, 2, 0), (1153, 3, 128)]          # N, d, block
M = 200


def rel(a, b, floor):
    return float(np.max(np.abs(np.asarray(a) - b) / np.maximum(np.abs(b), floor)))


def amax(a, b):
    """largest difference relative to the largest entry"""
    return float(np.max(np.abs(np.asarray(a) - b)) / np.max(np.abs(b)))


_CACHE = {}


def case(kernel, N, d, k, is_ard):
    """inputs and the reference's numbers, computed once per case and never modified"""
    key = (kernel, N, d, k, is_ard)
    if key not in _CACHE:
        ls = hr.ard(d) if is_ard else hr.LS
        X, y, Xs = hr.problem(N, d, M, k, seed=N + k)
        w = hr.weights(N, seed=N + k + 1)
        ref = hr.HeteroGP(kernel, ls, SF2, SN2, 1e-10 * SF2).fit(X, y, w)
        mean, var = ref.predict(Xs)
        for a in (X, y, Xs, w, mean, var):
            a.setflags(write=False)
        _CACHE[key] = dict(ls=ls, X=X, y=y, Xs=Xs, w=w, ref=ref, mean=mean, var=var)
    return _CACHE[key]


def check_fit(gp, c, mean, var, tag):
    ref = c["ref"]
    fig = {"alpha": amax(gp.alpha_, ref.alpha_), "logdet": abs(gp.log_det_ - ref.logdet) / abs(ref.logdet),
           "lml": abs(gp.log_marginal_likelihood(c["y"]) - ref.lml()) / abs(ref.lml()),
           "mean": rel(mean, c["mean"], 1e-6), "var": rel(var, c["var"], 1e-6 * SF2)}
    print(tag, " ".join(f"{n} {v:.2e}" for n, v in fig.items()))
    assert gp.info_ == 0 and gp.jitter_used_ == gp.jitter
    assert fig["alpha"] <= 1e-7 and fig["logdet"] <= 1e-9 and fig["lml"] <= 1e-9, (tag, fig)
    assert fig["mean"] <= 1e-6 and fig["var"] <= 1e-6, (tag, fig)


# ---- 1. parity ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,is_ard", [(1, False), (3, True)])
@pytest.mark.parametrize("N,d,block", SHAPES)
@pytest.mark.parametrize("kernel", KERNELS)
def test_parity_with_the_reference_fp64(kernel, N, d, block, k, is_ard):
    c = case(kernel, N, d, k, is_ard)
    with GP(kernel, c["ls"], SF2, SN2, block=block) as gp:
        mean, var = gp.fit(c["X"], c["y"], noise_weights=c["w"]).predict(c["Xs"])
        check_fit(gp, c, mean, var, f"hetero parity {kernel} N={N} k={k} numpy:")
        assert np.array_equal(gp.noise_weights_, c["w"])


@pytest.mark.parametrize("k,is_ard", [(1, False), (3, True)])
@pytest.mark.parametrize("N,d,block", SHAPES)
@pytest.mark.parametrize("kernel", KERNELS)
def test_parity_with_the_reference_fp64_device_tensors(kernel, N, d, block, k, is_ard):
    torch = pytest.importorskip("torch")
    c = case(kernel, N, d, k, is_ard)
    with GP(kernel, c["ls"], SF2, SN2, block=block) as gp:
        mean, var = gp.fit(c["X"], c["y"], noise_weights=c["w"]).predict(c["Xs"])
        host = (mean.copy(), var.copy(), gp.alpha_.copy(), gp.log_det_)
        dev = torch.device("cuda", 0)
        Xd, yd, Xsd, wd = (torch.from_numpy(np.array(c[n])).to(dev) for n in ("X", "y", "Xs", "w"))
        md, vd = gp.fit(Xd, yd, noise_weights=wd).predict(Xsd)
        assert md.is_cuda and vd.is_cuda
        check_fit(gp, c, md.cpu().numpy(), vd.cpu().numpy(), f"hetero parity {kernel} N={N} k={k} device:")
        # the same arithmetic from another kind of memory: the same bits
        assert np.array_equal(md.cpu().numpy(), host[0]) and np.array_equal(vd.cpu().numpy(), host[1])
        assert np.array_equal(gp.alpha_, host[2]) and gp.log_det_ == host[3] and np.array_equal(gp.noise_weights_, c["w"])


# ---- 2. ones are nothing ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float64", "float32", "mixed"])
def test_weights_of_one_change_no_bit(dtype):
    N, d, k = 1153, 3, 2
    X, y, Xs = hr.problem(N, d, M, k, seed=5)
    noise = SN2 if dtype == "float64" else 1e-1
    kw = dict(kernel="matern52", lengthscale=hr.ard(d), variance=SF2, noise=noise, dtype=dtype, block=256)

    def run(gp, w):
        mean, var = gp.fit(X, y, noise_weights=w).predict(Xs)
        out = [gp.alpha_.copy(), np.float64(gp.log_det_), mean, var]
        if dtype == "float64":
            lml, grad = gp.lml_gradient()
            out += [np.float64(lml), grad]
        return out

    with GP(**kw) as gp:
        fresh = run(gp, None)
    with GP(**kw) as gp:
        ones = run(gp, np.ones(N))
        assert np.array_equal(gp.noise_weights_, np.ones(N))
    with GP(**kw) as gp:
        weighted = run(gp, hr.weights(N, seed=6, lo=0.25, hi=4.0, zeros=False))
        cleared = run(gp, None)                      # the same handle after its weights were cleared
        assert np.array_equal(gp.noise_weights_, np.ones(N))
    assert not np.array_equal(weighted[0], fresh[0])
    for name, other in (("ones", ones), ("set and cleared", cleared)):
        for a, b in zip(other, fresh):
            assert np.array_equal(a, b), (dtype, name)


# ---- 3. one pass -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float64", "float32", "mixed"])
@pytest.mark.parametrize("N,d,block", SHAPES)
def test_fit_predict_sees_the_same_weights_as_the_two_calls(N, d, block, dtype):
    c = case("matern52", N, d, 3, True)
    npdt = np.float32 if dtype == "float32" else np.float64
    noise = SN2 if dtype == "float64" else 1e-1
    w = np.array(c["w"]) if dtype == "float64" else hr.weights(N, seed=9, lo=0.25, hi=4.0, zeros=False)
    X, y, Xs, w = (np.asarray(a, dtype=npdt) for a in (c["X"], c["y"], c["Xs"], w))
    with GP("matern52", c["ls"], SF2, noise, dtype=dtype, block=block) as gp:
        m2, v2 = gp.fit(X, y, noise_weights=w).predict(Xs)
        a2, ld2 = gp.alpha_.copy(), gp.log_det_
        mean, var = gp.fit_predict(X, y, Xs, noise_weights=w)
        assert gp.info_ == 0 and np.array_equal(gp.noise_weights_, w)
        if dtype == "float64":
            check_fit(gp, c, mean, var, f"hetero fit_predict N={N}:")
            assert rel(mean, m2, 1e-6) <= 1e-9 or np.max(np.abs(mean - m2)) <= 1e-10 * np.max(np.abs(m2))
            assert rel(var, v2, 1e-6 * SF2) <= 1e-9
            assert gp.log_det_ == ld2 and np.array_equal(gp.alpha_, a2)
        elif dtype == "float32":      # the bars of test_fit_predict_fp32_and_device_tensors
            assert mean.dtype == np.float32
            assert np.max(np.abs(mean - m2)) <= 2e-2 * np.max(np.abs(m2)) and np.max(np.abs(var - v2)) <= 2e-3 * 1.5
        else:                         # mixed: the call IS the two calls
            assert np.array_equal(mean, m2) and np.array_equal(var, v2) and np.array_equal(gp.alpha_, a2)
        # and none of them is the unweighted model
        m0, _ = gp.fit_predict(X, y, Xs)
        assert np.max(np.abs(m0 - mean)) > 1e-3 * np.max(np.abs(mean))
        assert np.array_equal(gp.noise_weights_, np.ones(N, dtype=npdt))


# ---- 4. gradient -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,d,block", SHAPES)
@pytest.mark.parametrize("kernel", KERNELS)
def test_lml_gradient_with_weights(kernel, N, d, block):
    k, is_ard = (3, True) if kernel in ("rbf", "matern32") else (1, False)
    c = case(kernel, N, d, k, is_ard)
    ref = c["ref"]
    want = ref.lml_gradient()
    with GP(kernel, c["ls"], SF2, SN2, block=block) as gp:
        lml, grad = gp.fit(c["X"], c["y"], noise_weights=c["w"]).lml_gradient()
        el, eg = abs(lml - ref.lml()) / abs(ref.lml()), float(np.max(np.abs(grad - want)) / np.max(np.abs(want)))
        print(f"hetero gradient {kernel} N={N} k={k}: lml {el:.2e} grad {eg:.2e} of its largest entry; noise entry "
              f"{grad[-1]:.8g} (reference {want[-1]:.8g})")
        assert el <= 1e-9 and eg <= 1e-8
        # the noise entry against a central difference of the library's own LML in log noise
        h, f = 1e-4, []
        for sgn in (+1, -1):
            with GP(kernel, c["ls"], SF2, float(np.exp(np.log(SN2) + sgn * h)), jitter=gp.jitter, block=block) as g2:
                f.append(g2.fit(c["X"], c["y"], noise_weights=c["w"]).log_marginal_likelihood(c["y"]))
        fd = (f[0] - f[1]) / (2 * h)
        print(f"hetero gradient {kernel} N={N}: noise entry {grad[-1]:.8g}, central difference {fd:.8g}")
        assert abs(fd - grad[-1]) <= 2e-5 * np.abs(grad).max()


def test_optimize_keeps_the_weights():
    c = case("rbf", 300, 2, 1, False)
    with GP("rbf", 0.5, 1.0, 0.05) as gp:
        res = gp.optimize(c["X"], c["y"], noise_weights=c["w"], maxiter=5)
        assert np.array_equal(gp.noise_weights_, c["w"])
        ref = hr.HeteroGP("rbf", gp.lengthscale, gp.variance, gp.noise, gp.jitter_used_).fit(c["X"], c["y"], c["w"])
        lml = gp.log_marginal_likelihood(c["y"])
        print(f"hetero optimize: lml {lml:.6f} reference {ref.lml():.6f} after {res.nit} iterations")
        assert abs(lml - ref.lml()) <= 1e-8 * abs(ref.lml()) and abs(-res.fun - ref.lml()) <= 1e-8 * abs(ref.lml())
        start = hr.HeteroGP("rbf", 0.5, 1.0, 0.05, 1e-10).fit(c["X"], c["y"], c["w"]).lml()
        assert lml > start


# ---- 5. update -------------------------------------------------------------------------------------------------------------
def _figures(gp, Xs):
    mean, var = gp.predict(Xs)
    return dict(mean=mean, var=var, alpha=gp.alpha_.copy(), logdet=gp.log_det_)


def _check_update(o, c, fresh, tag):
    """the measures and bars of tests/test_append_gpu.py's check()"""
    ref = c["ref"]
    fig = {"mean/ref": rel(o["mean"], c["mean"], 1e-6), "var/ref": rel(o["var"], c["var"], 1e-6 * SF2),
           "alpha/ref": amax(o["alpha"], ref.alpha_), "logdet/ref": abs(o["logdet"] - ref.logdet) / abs(ref.logdet),
           "mean/fresh": rel(o["mean"], fresh["mean"], 1e-6), "var/fresh": rel(o["var"], fresh["var"], 1e-6 * SF2),
           "alpha/fresh": amax(o["alpha"], fresh["alpha"]),
           "logdet/fresh": abs(o["logdet"] - fresh["logdet"]) / abs(fresh["logdet"])}
    print(tag, " ".join(f"{n} {v:.2e}" for n, v in fig.items()))
    for n, v in fig.items():
        bar = 1e-9 if n.endswith("/fresh") or n == "logdet/ref" else 1e-7 if n == "alpha/ref" else 1e-6
        assert v <= bar, (tag, n, v, bar)


@pytest.mark.parametrize("reserve", [0, 2048])
def test_update_with_weights(reserve):
    N0, m, d = 1000, 200, 3                    # block = 128: the restart begins at R0 = 896, inside the fitted weights
    N = N0 + m
    X, y, Xs = hr.problem(N, d, M, 3, seed=15)
    w = hr.weights(N, seed=16)
    ls = hr.ard(d)
    for a in (X, y, Xs, w):
        a.setflags(write=False)

    def reference(wts):
        r = hr.HeteroGP("matern52", ls, SF2, SN2, 1e-10 * SF2).fit(X, y, wts)
        mean, var = r.predict(Xs)
        return dict(ref=r, mean=mean, var=var)

    with GP("matern52", ls, SF2, SN2, block=128) as gp:
        fresh = _figures(gp.fit(X, y, noise_weights=w), Xs)
        w1 = np.concatenate([w[:N0], np.ones(m)])
        fresh1 = _figures(gp.fit(X, y, noise_weights=w1), Xs)
    with GP("matern52", ls, SF2, SN2, block=128) as gp:
        if reserve:
            gp.reserve(reserve)
        gp.fit(X[:N0], y[:N0], noise_weights=w[:N0])
        assert gp.update(X[N0:], y[N0:], noise_weights=w[N0:]) is gp
        assert np.array_equal(gp.noise_weights_, w) and gp.alpha_.shape[0] == N
        _check_update(_figures(gp, Xs), reference(w), fresh, f"hetero update reserve={reserve}:")
        # update without weights on a weighted model: ones for the new points
        gp.fit(X[:N0], y[:N0], noise_weights=w[:N0]).update(X[N0:], y[N0:])
        assert np.array_equal(gp.noise_weights_, w1)
        _check_update(_figures(gp, Xs), reference(w1), fresh1, f"hetero update reserve={reserve}, no new weights:")
        # weights for the new points of a model that had none
        gp.fit(X[:N0], y[:N0]).update(X[N0:], y[N0:], noise_weights=w[N0:])
        w2 = np.concatenate([np.ones(N0), w[N0:]])
        assert np.array_equal(gp.noise_weights_, w2)
        with GP("matern52", ls, SF2, SN2, block=128) as g2:
            fresh2 = _figures(g2.fit(X, y, noise_weights=w2), Xs)
        _check_update(_figures(gp, Xs), reference(w2), fresh2, f"hetero update reserve={reserve}, first weights:")


def test_failed_weighted_append_keeps_the_model_and_its_weights():
    """The recipe of test_failed_append_keeps_the_model with a noise level: K of the 300 fitted points is exactly diagonal,
    1 + 0.5 w_i (every off-diagonal exp underflows); the point -100 twice with weight 0 (exact observations) gives the Schur
    block [[1, 1], [1, 1]]: the second pivot is exactly 0, info = 302."""
    X = 100.0 * np.arange(300, dtype=np.float64)[:, None]
    y = np.sin(np.arange(300, dtype=np.float64))
    w = hr.weights(300, seed=17, zeros=False)
    Xs = X[:50] + 0.3
    twice = np.array([[-100.0], [-100.0]])
    apart = np.array([[-100.0], [-200.0]])
    ynew, wnew = np.array([0.5, -0.25]), np.array([0.0, 0.0])
    with GP("rbf", 1.0, 1.0, noise=0.5, jitter=0.0) as gp:
        m0, v0 = gp.fit(X, y, noise_weights=w).predict(Xs)
        a0, ld0 = gp.alpha_.copy(), gp.log_det_
        assert np.max(np.abs(a0 - y / (1.0 + 0.5 * w))) <= 1e-12
        info = C.c_int64(-1)
        p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
        rc = gp._lib.gpx_append_weighted(gp._h, p(twice), p(ynew), p(wnew), 2, _abi.MEM_HOST, C.byref(info))
        assert rc == 0 and info.value == 302
        with pytest.raises(np.linalg.LinAlgError, match="unchanged"):
            gp.update(twice, ynew, noise_weights=wnew)
        assert gp.get_state()["fitted"]["N"] == 300 and np.array_equal(gp.noise_weights_, w)
        m1, v1 = gp.predict(Xs)
        assert rel(m1, m0, 1e-6) <= 1e-9 and rel(v1, v0, 1e-6) <= 1e-9
        assert np.max(np.abs(gp.alpha_ - a0)) <= 1e-9 * np.max(np.abs(a0)) and abs(gp.log_det_ - ld0) <= 1e-9
        gp.update(apart, ynew, noise_weights=np.array([2.0, 0.0]))       # two distinct far points: positive definite
        assert np.array_equal(gp.noise_weights_, np.concatenate([w, [2.0, 0.0]]))
        assert np.max(np.abs(gp.alpha_[300:] - ynew / np.array([2.0, 1.0]))) <= 1e-12


def test_update_with_weights_float32():
    """the bars of test_single_append_float32"""
    N0, m = 1000, 200
    N = N0 + m
    X, y, Xs = hr.problem(N, 3, 90, 1, seed=18)
    w = hr.weights(N, seed=19, lo=0.25, hi=4.0, zeros=False)
    ls, noise = hr.ard(3), 1e-1
    ref = hr.HeteroGP("rbf", ls, SF2, noise, 0.0).fit(X, y, w)
    mr, vr = ref.predict(Xs)
    f32 = lambda a: np.asarray(a, dtype=np.float32)  # noqa: E731
    with GP("rbf", ls, SF2, noise, jitter=0.0, dtype="float32", block=256) as gp:
        m1, v1 = gp.fit(f32(X), f32(y), noise_weights=f32(w)).predict(f32(Xs))
        a1, ld1 = gp.alpha_.copy(), gp.log_det_
        gp.fit(f32(X[:N0]), f32(y[:N0]), noise_weights=f32(w[:N0])).update(f32(X[N0:]), f32(y[N0:]), noise_weights=f32(w[N0:]))
        mean, var = gp.predict(f32(Xs))
        assert mean.dtype == np.float32 and gp.alpha_.shape == (N,) and np.array_equal(gp.noise_weights_, f32(w))
        em, ev = np.max(np.abs(mean - mr)) / np.max(np.abs(mr)), np.max(np.abs(var - vr)) / 1.5
        el = abs(gp.log_det_ - ref.logdet) / abs(ref.logdet)
        print(f"hetero fp32 update: mean {em:.2e} var {ev:.2e} logdet {el:.2e}")
        assert em <= 2e-3 and ev <= 2e-3 and el <= 1e-3
        assert np.max(np.abs(mean - m1)) <= 1e-3 * np.max(np.abs(m1)) and np.max(np.abs(var - v1)) <= 1e-3 * 1.5
        assert np.max(np.abs(gp.alpha_ - a1)) <= 2e-3 * np.max(np.abs(a1)) and abs(gp.log_det_ - ld1) <= 1e-4 * abs(ld1)


# ---- 6. score --------------------------------------------------------------------------------------------------------------
def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("G,Lg", [(5, 33), (3, 64)])
def test_weighted_score_against_the_reference(G, Lg):
    """the error measure of tests/test_score_gpu.py: |got - ref| <= 1e-10 kappa_g (Lg + maha_g), kappa_g the condition
    number of the reference's S_g — which is bounded by score_ref.kappa_bound at the smallest per-point diagonal value"""
    N, d, k = 700, 3, 2
    ls = (1.0, 1.5, 2.0)
    X, Y, Xq, Yq = score_problem(N, d, k, G + 4, Lg, seed=23)
    w = hr.weights(N, seed=24)
    wq = np.exp(np.random.default_rng(25).uniform(np.log(0.5), np.log(2.0), (G + 4) * Lg))
    with GP("matern32", ls, SF2, SN2) as gp:
        gp.fit(X, Y, noise_weights=w)
        ref = hr.HeteroGP("matern32", ls, SF2, SN2, gp.jitter_used_).fit(X, Y, w).score(Xq[:G * Lg], Yq[:G * Lg], Lg, SN2,
                                                                                      wq[:G * Lg])
        assert np.all(ref["kappa"] <= kappa_bound(Lg, SF2, ref["dmin"]))
        logp, maha, logdet = gp.score_blocks(Xq[:G * Lg], Yq[:G * Lg], Lg, return_parts=True, noise_weights=wq[:G * Lg])
        bound = 1e-10 * ref["kappa"][:, None] * (Lg + ref["maha"])
        r = (float(np.max(np.abs(logp - ref["logp"]) / bound)), float(np.max(np.abs(maha - ref["maha"]) / bound)),
             float(np.max(np.abs(logdet - ref["logdet"]) / bound.min(axis=1))))
        print(f"hetero score G={G} Lg={Lg}: error / bound logp {r[0]:.3g} maha {r[1]:.3g} logdet {r[2]:.3g} "
              f"(kappa max {ref['kappa'].max():.3g})")
        assert max(r) <= 1.0
        # the weights are seen: the unweighted score of the same blocks is another number
        plain = gp.score_blocks(Xq[:G * Lg], Yq[:G * Lg], Lg, return_parts=True)
        assert np.max(np.abs(plain[0] - logp)) > 1e-3
        # weights of one are no weights
        assert _same(gp.score_blocks(Xq[:G * Lg], Yq[:G * Lg], Lg, return_parts=True, noise_weights=np.ones(G * Lg)), plain)
        # a block does not depend on the others: alone, and inside a larger call at another position
        full = gp.score_blocks(Xq, Yq, Lg, return_parts=True, noise_weights=wq)
        assert _same([a[:G] for a in full], (logp, maha, logdet))
        b = G + 2
        sl = slice(Lg * b, Lg * (b + 1))
        alone = gp.score_blocks(Xq[sl], Yq[sl], Lg, return_parts=True, noise_weights=wq[sl])
        assert _same(alone, [a[b:b + 1] for a in full])


# ---- 7. mixed --------------------------------------------------------------------------------------------------------------
def test_mixed_refines_against_the_weighted_kernel():
    """N = 1153, weights in [0.25, 4] and none of them 0, so that the fp32 factorisation succeeds: cond(K) of the reference
    is 1.34e5 for these inputs (RBF; smallest eigenvalue 2.6e-3 ~ sn2 min(w), largest 354), against 1 / eps_fp32 = 1.7e7.
    The fp64 refinement runs against K with the weighted diagonal: with the scalar one it would converge to another alpha
    (or not at all), and the mean would miss the fp64 handle's by far more than the bar of tests/test_mixed_gpu.py."""
    N, d, k = 1153, 3, 2
    X, y, Xs = hr.problem(N, d, M, k, seed=N)
    w = hr.weights(N, seed=N + 1, lo=0.25, hi=4.0, zeros=False)
    ev = np.linalg.eigvalsh(hr.HeteroGP("rbf", hr.LS, SF2, SN2, 1e-10 * SF2).gram(X, w))
    print(f"hetero mixed: cond(K) = {ev[-1] / ev[0]:.3g}")
    assert ev[-1] / ev[0] <= 2e5
    with GP("rbf", hr.LS, SF2, SN2, block=128) as g64:
        m64 = g64.fit(X, y, noise_weights=w).predict(Xs, return_var=False)
        a64 = g64.alpha_.copy()
    with GP("rbf", hr.LS, SF2, SN2, dtype="mixed", block=128) as gp:
        mean, var = gp.fit(X, y, noise_weights=w).predict(Xs)
        tm = gp.timings_
        em = float(np.max(np.abs(mean - m64) / np.maximum(np.abs(m64), 1e-6)))
        ea = amax(gp.alpha_, a64)
        print(f"hetero mixed: refine_resid {tm['refine_resid']:.2e} after {tm['refine_iters']:.0f} iterations, mean {em:.2e} "
              f"alpha {ea:.2e}")
        assert gp.info_ == 0 and np.array_equal(gp.noise_weights_, w)
        assert tm["refine_resid"] <= 1e-10
        assert em <= 1e-6 and ea <= 1e-7


# ---- 8. rules --------------------------------------------------------------------------------------------------------------
def test_argument_rules_and_refusals():
    torch = pytest.importorskip("torch")
    c = case("rbf", 300, 2, 1, False)
    X, y, Xs, w = c["X"], c["y"], c["Xs"], c["w"]
    N = len(X)
    with GP("rbf", hr.LS, SF2, SN2) as gp:
        with pytest.raises(RuntimeError):
            gp.noise_weights_
        m0, v0 = gp.fit(X, y, noise_weights=w).predict(Xs)
        bad_neg, bad_nan, bad_inf = np.array(w), np.array(w), np.array(w)
        bad_neg[7], bad_nan[N - 1], bad_inf[0] = -1e-300, np.nan, np.inf
        dev = torch.device("cuda", 0)
        for bad, exc in ((w[:-1], ValueError), (np.stack([w, w], 1), ValueError), (torch.from_numpy(np.array(w)).to(dev), ValueError),
                         (bad_neg, _abi.GpxError), (bad_nan, _abi.GpxError), (bad_inf, _abi.GpxError)):
            with pytest.raises(exc) as e:
                gp.fit(X, y, noise_weights=bad)
            assert exc is ValueError or e.value.code == _abi.E_ARG
            # nothing happened: the model, and the weights it was made with, are as before
            assert np.array_equal(gp.noise_weights_, w)
            m1, v1 = gp.predict(Xs)
            assert np.array_equal(m1, m0) and np.array_equal(v1, v0)
        # the same through device memory: the validation kernel
        Xd, yd = torch.from_numpy(np.array(X)).to(dev), torch.from_numpy(np.array(y)).to(dev)
        for bad in (bad_neg, bad_nan, bad_inf):
            with pytest.raises(_abi.GpxError) as e:
                gp.fit(Xd, yd, noise_weights=torch.from_numpy(bad).to(dev))
            assert e.value.code == _abi.E_ARG and np.array_equal(gp.noise_weights_, w)
        # the handle kept the weights of the last accepted call: a fit through the C ABI alone still uses them
        info, ls = C.c_int64(0), np.array([hr.LS])
        Xc, yc = np.ascontiguousarray(X), np.ascontiguousarray(y)
        rc = gp._lib.gpx_fit(gp._h, Xc.ctypes.data_as(C.c_void_p), yc.ctypes.data_as(C.c_void_p), N, 2, 1, _abi.dptr(ls), 1,
                             SF2, SN2, gp.jitter, _abi.MEM_HOST, C.byref(info))
        assert rc == 0 and info.value == 0
        gp._alpha = None
        assert amax(gp.alpha_, c["ref"].alpha_) <= 1e-7
        # ... and refuses a fit of another size before anything is computed
        rc = gp._lib.gpx_fit(gp._h, Xc.ctypes.data_as(C.c_void_p), yc.ctypes.data_as(C.c_void_p), N - 1, 2, 1, _abi.dptr(ls), 1,
                             SF2, SN2, gp.jitter, _abi.MEM_HOST, C.byref(info))
        assert rc == _abi.E_ARG and b"noise weights" in gp._lib.gpx_last_error(gp._h)
        assert np.array_equal(gp.predict(Xs)[0], m0)                    # the fit before it is still there
        # update and score: wrong length, wrong kind, bad values
        with pytest.raises(ValueError):
            gp.update(Xs[:5], np.zeros(5), noise_weights=np.ones(4))
        with pytest.raises(_abi.GpxError) as e:
            gp.update(Xs[:5], np.zeros(5), noise_weights=np.array([1.0, 1.0, -1.0, 1.0, 1.0]))
        assert e.value.code == _abi.E_ARG and gp.get_state()["fitted"]["N"] == N
        with pytest.raises(ValueError):
            gp.score_blocks(Xs[:8], np.zeros(8), 4, noise_weights=np.ones(7))
        with pytest.raises(_abi.GpxError) as e:
            gp.score_blocks(Xs[:8], np.zeros(8), 4, noise_weights=np.r_[np.ones(7), np.nan])
        assert e.value.code == _abi.E_ARG


def test_groups_refuse_weights_and_fit_without_them():
    c = case("rbf", 300, 2, 1, False)
    X, y, Xs, w = c["X"], c["y"], c["Xs"], c["w"]
    with GP("rbf", hr.LS, SF2, SN2) as gp:
        want = gp.fit(X, y).predict(Xs)
    with GP("rbf", hr.LS, SF2, SN2, devices=1, transport="local") as gp:
        with pytest.raises(_abi.GpxError) as e:
            gp.fit(X, y, noise_weights=w)
        assert e.value.code == _abi.E_UNSUPPORTED and "weights" in str(e.value)
        with pytest.raises(_abi.GpxError) as e:
            gp.fit_predict(X, y, Xs, noise_weights=w)
        assert e.value.code == _abi.E_UNSUPPORTED
        mean, var = gp.fit(X, y).predict(Xs)
        assert amax(mean, want[0]) <= 1e-9 and amax(var, want[1]) <= 1e-9     # (the sharded schedule: another summation order)
        assert np.array_equal(gp.noise_weights_, np.ones(len(X)))


def test_lml_gradient_of_a_weighted_float32_model_is_refused_as_without_weights():
    c = case("rbf", 300, 2, 1, False)
    f32 = lambda a: np.asarray(a, dtype=np.float32)  # noqa: E731
    w = hr.weights(300, seed=31, lo=0.25, hi=4.0, zeros=False)
    with GP("rbf", hr.LS, SF2, 1e-1, dtype="float32") as gp:
        codes = []
        for wts in (None, f32(w)):
            gp.fit(f32(c["X"]), f32(c["y"]), noise_weights=wts)
            with pytest.raises(_abi.GpxError) as e:
                gp.lml_gradient()
            codes.append(e.value.code)
        assert codes == [_abi.E_UNSUPPORTED, _abi.E_UNSUPPORTED]
