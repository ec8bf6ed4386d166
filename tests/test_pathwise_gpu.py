"""GPU: pathwise posterior function samples — the evaluation kernel alone (``gpx_pathwise_eval_raw``) against NumPy inside a
derived rounding bound, ``GP.sample_functions`` end to end against the dense reference of tests/pathwise_ref.py, the seed /
``z`` twins, bit-for-bit reproducibility, the lifetime of a draw and the refusals."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

from gaussianprocesspathmodelling_amd import GP, GpxError, _abi

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pathwise_ref as pw  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53
FAMILIES = ["rbf", "matern52", "matern32", "matern12"]
# one decade above the largest difference measured between a seeded draw and its z twin (profiles/pathwise_parity.json),
# as a fraction of max |out|; the project's bar for the same quantity by another route is 1e-9
TWIN_BAR = 1.64e-12


def eval_raw(gpx, kernel, dtype, Xq, X, ls, sf2, Omega, W, V):
    lsa = np.ascontiguousarray(np.atleast_1d(np.asarray(ls, dtype=np.float64)))
    out = np.zeros((len(W), len(Xq)))
    arrs = [np.ascontiguousarray(a, dtype=np.float64) for a in (Xq, X, Omega, W, V)]
    rc = gpx.gpx_pathwise_eval_raw(_abi.KERNEL_IDS[kernel], _abi.DTYPE_IDS[dtype], _abi.dptr(arrs[0]), len(Xq),
                                   _abi.dptr(arrs[1]), len(X), X.shape[1], _abi.dptr(lsa), lsa.size, sf2, _abi.dptr(arrs[2]),
                                   len(Omega), _abi.dptr(arrs[3]), _abi.dptr(arrs[4]), len(W), _abi.dptr(out))
    assert rc == 0, gpx.gpx_last_error(None)
    return out


def raw_case(M, N, F, Cn, d, ard, kernel, seed):
    rng = np.random.default_rng(seed)
    Xq, X = rng.uniform(0, 1, (M, d)), rng.uniform(0, 1, (N, d))
    ls = tuple(rng.uniform(0.2, 0.6, d)) if ard else 0.3
    g, chin, W, V = pw.split(rng.standard_normal(pw.n_normals(kernel, F, d, Cn, N)), kernel, F, d, Cn, N)
    return Xq, X, ls, 1.7, pw.frequencies(g, chin), W, V


# M in {1, 77, 200} x N in {130, 333} x F in {1, 5, 64} x C in {1, 3, 17, 70} x d in {1, 3, 5}, scalar and ARD, four
# families: every value of every axis appears, the tile edges (M, C not multiples of 16 / 64; N, 2F not multiples of the
# 64-item stage) and the run-time-d kernel (d = 5) with each family
RAW_CASES = [
    (1, 130, 1, 1, 1, False, "rbf"), (77, 333, 5, 3, 3, True, "matern52"), (200, 130, 64, 17, 5, True, "matern32"),
    (77, 130, 64, 70, 1, False, "matern12"), (200, 333, 5, 70, 3, False, "rbf"), (1, 333, 64, 17, 5, False, "matern52"),
    (200, 333, 1, 3, 1, False, "matern32"), (77, 130, 5, 1, 3, True, "matern12"), (200, 130, 64, 70, 5, True, "rbf"),
    (77, 333, 64, 17, 3, False, "matern12"), (1, 130, 5, 3, 5, True, "matern12"), (200, 333, 64, 3, 2, True, "matern52"),
    (77, 333, 1, 70, 5, False, "matern32"), (200, 130, 5, 17, 1, False, "matern52"),
    # more than one split on either axis (2048 training points / 2048 feature items each), the last ones partly filled
    (77, 4200, 1100, 3, 2, True, "matern52"), (1, 2049, 1025, 17, 1, False, "rbf"),
]


@pytest.mark.parametrize("case", RAW_CASES, ids=lambda c: "M{}_N{}_F{}_C{}_d{}_{}_{}".format(*c[:5], "ard" if c[5] else "iso", c[6]))
def test_evaluation_kernel_fp64_inside_its_rounding_bound(gpx, case):
    """|out - ref| <= (N + 2F + 16) 2^-53 A1 + (d + 2) 2^-53 A2 per element: worst-case summation of the N + 2F terms
    (A1 = the sum of their magnitudes) plus the rounding of the phases (A2 weighs each feature by |theta|)"""
    M, N, F, Cn, d, ard, kernel = case
    Xq, X, ls, sf2, Om, W, V = raw_case(*case, seed=11)
    out = eval_raw(gpx, kernel, "float64", Xq, X, ls, sf2, Om, W, V)
    ref = pw.evaluate_columns(kernel, Xq, X, ls, sf2, Om, W, V)
    amp = np.sqrt(sf2 / F)
    Wabs = np.abs(W[:, :F]) + np.abs(W[:, F:])                                             # (C, F)
    th = np.abs(pw.phases(pw.scaled(Xq, ls), Om))                                          # (M, F)
    A1 = amp * Wabs.sum(axis=1)[:, None] + np.abs(V) @ pw.kernel_matrix(kernel, Xq, X, ls, sf2).T
    A2 = amp * Wabs @ th.T
    bound = (N + 2 * F + 16) * U * A1 + (d + 2) * U * A2
    ratio = np.max(np.abs(out - ref) / bound)
    print(f"{case}: max |out - ref| / bound = {ratio:.3f}, max |out - ref| = {np.max(np.abs(out - ref)):.2e}")
    assert ratio <= 1.0


@pytest.mark.parametrize("case", RAW_CASES[1::3], ids=lambda c: "M{}_N{}_F{}_C{}_d{}_{}".format(*c[:5], c[6]))
def test_evaluation_kernel_fp32(gpx, case):
    """the fp32 kernel (phases still fp64) at the project's fp32 bar: 2e-3 of max |ref|"""
    M, N, F, Cn, d, ard, kernel = case
    Xq, X, ls, sf2, Om, W, V = raw_case(*case, seed=12)
    out = eval_raw(gpx, kernel, "float32", Xq, X, ls, sf2, Om, W, V)
    ref = pw.evaluate_columns(kernel, Xq, X, ls, sf2, Om, W, V)
    err = np.max(np.abs(out - ref)) / np.max(np.abs(ref))
    print(f"{case}: fp32 err {err:.2e} of max |ref|")
    assert err <= 2e-3


def test_fp32_phases_survive_large_frequencies(gpx):
    """Cauchy frequencies (Matern-1/2) scaled up until |theta| passes 1e4: an fp32 phase would have no digits left"""
    Xq, X, ls, sf2, Om, W, V = raw_case(77, 130, 64, 3, 1, False, "matern12", seed=13)
    Om = Om * (2e4 / np.max(np.abs(Om)) * 0.3)                                            # u <= 1 / 0.3
    assert np.max(np.abs(pw.phases(pw.scaled(Xq, ls), Om))) > 1e4
    out = eval_raw(gpx, "matern12", "float32", Xq, X, ls, sf2, Om, W, V)
    ref = pw.evaluate_columns("matern12", Xq, X, ls, sf2, Om, W, V)
    err = np.max(np.abs(out - ref)) / np.max(np.abs(ref))
    print(f"fp32 with |theta| up to {np.max(np.abs(pw.phases(pw.scaled(Xq, ls), Om))):.3g}: err {err:.2e}")
    assert err <= 2e-3


# ---- end to end -----------------------------------------------------------------------------------------------------------

def problem(N, d, k, seed, M=77):
    rng = np.random.default_rng(seed)
    X = rng.uniform(0, 1, (N, d))
    y = np.sin(5.0 * X.sum(axis=1)) + 0.1 * rng.standard_normal(N)
    if k == 2:
        y = np.stack([y, np.cos(3.0 * X[:, 0]) + 0.1 * rng.standard_normal(N)], axis=1)
    w = rng.uniform(0.5, 2.0, N)
    return X, y, rng.uniform(-0.1, 1.1, (M, d)), w


def as_smk(f, k):
    """GP.sample_y's shape (M, S) | (M, k, S) -> (S, M, k)"""
    return f.T[:, :, None] if f.ndim == 2 else f.transpose(2, 0, 1)


E2E = [(130, 1, 1, False, "rbf", 0.25), (130, 2, 2, True, "matern52", (0.3, 0.4)), (333, 3, 1, True, "matern32", 0.35),
       (333, 2, 2, False, "matern12", (0.4, 0.3)), (333, 1, 2, True, "rbf", 0.2), (130, 3, 1, False, "matern52", 0.4)]


@pytest.mark.parametrize("N,d,k,weighted,kernel,ls", E2E)
def test_functions_match_the_dense_reference(N, d, k, weighted, kernel, ls):
    """caller-supplied z: the device's functions are the dense reference's, 1e-6 of max |ref| (the project's bar for
    posterior quantities against a dense reference at this noise level)"""
    X, y, Xs, w = problem(N, d, k, seed=N + d)
    S, F, sf2, sn2 = 5, 48, 1.5, 1e-2
    z = np.random.default_rng(5).standard_normal(pw.n_normals(kernel, F, d, S * k, N))
    with GP(kernel, ls, sf2, sn2) as gp:
        gp.fit(X, y, noise_weights=w if weighted else None)
        fs = gp.sample_functions(S, n_features=F, z=z)
        assert (fs.n_samples, fs.n_features) == (S, F)
        f = fs(Xs)
        jit = gp.jitter_used_
    assert f.shape == ((77, S) if k == 1 else (77, k, S))
    ref = pw.evaluate(pw.draw(kernel, X, y, ls, sf2, sn2, z, S, F, w=w if weighted else None, jitter=jit), Xs)
    err = np.max(np.abs(as_smk(f, k) - ref)) / np.max(np.abs(ref))
    print(f"N={N} d={d} k={k} weighted={weighted} {kernel}: err {err:.2e} of max |ref|")
    assert err <= 1e-6


@pytest.mark.parametrize("N,k,weighted", [(130, 1, False), (333, 2, True), (333, 1, False), (130, 2, True)])
def test_zero_normals_give_the_posterior_mean(N, k, weighted):
    """all-zero z: every function is K* alpha, within N 2^-53 sum_n |k| |alpha| of gp.predict's mean"""
    X, y, Xs, w = problem(N, 2, k, seed=3 * N + k)
    kernel, ls, sf2, sn2, S, F = "rbf", (0.3, 0.45), 1.5, 1e-2, 2, 16
    with GP(kernel, ls, sf2, sn2) as gp:
        gp.fit(X, y, noise_weights=w if weighted else None)
        f = as_smk(gp.sample_functions(S, n_features=F, z=np.zeros(pw.n_normals(kernel, F, 2, S * k, N)))(Xs), k)
        mean = gp.predict(Xs, return_var=False).reshape(len(Xs), k)
        alpha = gp.alpha_.reshape(N, k)
    bound = N * U * (np.abs(pw.kernel_matrix(kernel, Xs, X, ls, sf2)) @ np.abs(alpha))
    ratio = max(np.max(np.abs(f[s] - mean) / bound) for s in range(S))
    print(f"N={N} k={k} weighted={weighted}: max |f - mean| / bound = {ratio:.3f}")
    assert ratio <= 1.0


def test_seed_and_z_twins():
    """random_state = r against z = the reference's Philox normals of seed r: the same functions, up to the device's
    log / sin / cos in the Box-Muller step.  The largest difference is recorded in profiles/pathwise_parity.json; the
    bar is one decade above it (and far below 1e-9, above which a difference would be a bug)."""
    worst = 0.0
    for kernel, d, k, r in (("rbf", 1, 1, 7), ("matern52", 2, 2, 123456789), ("matern12", 3, 1, 2 ** 40 + 5)):
        N, S, F = 130, 4, 40
        X, y, Xs, _ = problem(N, d, k, seed=d)
        with GP(kernel, 0.3, 1.5, 1e-2) as gp:
            gp.fit(X, y)
            a = gp.sample_functions(S, n_features=F, random_state=r)(Xs)
            b = gp.sample_functions(S, n_features=F, z=pw.normals(r, kernel, F, d, S * k, N))(Xs)
        diff = np.max(np.abs(a - b)) / np.max(np.abs(a))
        print(f"{kernel} d={d} k={k} seed={r}: twins differ by {diff:.2e} of max |out|")
        worst = max(worst, diff)
    rec = json.load(open(os.path.join(ROOT, "profiles", "pathwise_parity.json")))
    assert rec["largest_difference_of_max_out"] < TWIN_BAR <= 10.0 * rec["largest_difference_of_max_out"] < 1e-9
    assert worst <= TWIN_BAR


def test_bit_for_bit():
    N, d, k, S, F = 333, 2, 2, 5, 40
    X, y, Xs, _ = problem(N, d, k, seed=9, M=200)
    with GP("matern52", (0.3, 0.4), 1.5, 1e-2) as gp:
        gp.fit(X, y)
        m0, v0 = gp.predict(Xs)
        s0 = gp.sample_y(Xs[:40], 3, random_state=4)
        l0, g0 = gp.lml_gradient()
        fs = gp.sample_functions(S, n_features=F, random_state=21)
        a = fs(Xs)
        assert np.array_equal(a, fs(Xs))                                                   # twice
        assert np.array_equal(np.concatenate([fs(Xs[:77]), fs(Xs[77:])]), a)               # in two halves
        assert np.array_equal(fs(Xs, samples=slice(0, 3)), a[..., :3])                     # a slice of the samples
        assert np.array_equal(fs(Xs, samples=slice(2, 5)), a[..., 2:5])
        assert np.array_equal(fs(Xs[5:6]), a[5:6])                                         # one point alone
        m1, v1 = gp.predict(Xs)                                                            # the fit is only read
        s1 = gp.sample_y(Xs[:40], 3, random_state=4)
        l1, g1 = gp.lml_gradient()
        assert np.array_equal(m0, m1) and np.array_equal(v0, v1) and np.array_equal(s0, s1)
        assert l0 == l1 and np.array_equal(g0, g1)
        b = gp.sample_functions(3, n_features=F, random_state=21)(Xs)                      # the first S' of a larger draw
        assert np.array_equal(b, a[..., :3])
        big = gp.sample_functions(40, n_features=F, random_state=21)(Xs)                   # 80 columns: two 64-column blocks
        assert np.array_equal(big[..., :5], a)


def test_more_query_points_than_one_batch():
    """M beyond the 8192 rows of a batch: the batches' results are those of the points evaluated on their own, and the
    dense reference's"""
    N, d, k, S, F, M = 130, 1, 2, 3, 24, 8192 + 333
    X, y, _, _ = problem(N, d, k, seed=14)
    Xs = np.random.default_rng(15).uniform(-0.1, 1.1, (M, d))
    z = np.random.default_rng(16).standard_normal(pw.n_normals("matern32", F, d, S * k, N))
    with GP("matern32", 0.3, 1.5, 1e-2) as gp:
        gp.fit(X, y)
        fs = gp.sample_functions(S, n_features=F, z=z)
        a = fs(Xs)
        assert np.array_equal(a[8100:8300], fs(Xs[8100:8300])) and np.array_equal(a[-1:], fs(Xs[-1:]))
        jit = gp.jitter_used_
    ref = pw.evaluate(pw.draw("matern32", X, y, 0.3, 1.5, 1e-2, z, S, F, jitter=jit), Xs)
    assert np.max(np.abs(as_smk(a, k) - ref)) <= 1e-6 * np.max(np.abs(ref))


def test_more_training_points_than_one_launch_of_the_draw():
    """N beyond the 8192 training points the draw's feature pass takes per launch, and beyond one 2048-point split of the
    evaluation: against the dense reference (one N = 8392 solve on the CPU)"""
    N, d, k, S, F = 8192 + 200, 2, 1, 2, 16
    X, y, Xs, _ = problem(N, d, k, seed=18)
    z = np.random.default_rng(19).standard_normal(pw.n_normals("matern32", F, d, S, N))
    with GP("matern32", 0.3, 1.5, 5e-2) as gp:
        gp.fit(X, y)
        f = gp.sample_functions(S, n_features=F, z=z)(Xs)
        jit = gp.jitter_used_
    ref = pw.evaluate(pw.draw("matern32", X, y, 0.3, 1.5, 5e-2, z, S, F, jitter=jit), Xs)
    err = np.max(np.abs(as_smk(f, k) - ref)) / np.max(np.abs(ref))
    print(f"N={N}: err {err:.2e} of max |ref|")
    assert err <= 1e-6


def test_device_tensors_in_device_tensors_out():
    import torch
    X, y, Xs, _ = problem(130, 2, 1, seed=2)
    with GP("rbf", 0.3, 1.5, 1e-2, device=0) as gp:
        gp.fit(X, y)
        fs = gp.sample_functions(3, n_features=32, random_state=1)
        a = fs(Xs)
        t = fs(torch.as_tensor(Xs, device="cuda:0"))
        assert t.is_cuda and tuple(t.shape) == a.shape == (77, 3)
        assert np.array_equal(t.cpu().numpy(), a)


def test_float32_handle():
    """a GPX_F32 model: fp32 factor and fp32 kernel, held to the fp64 dense reference at the project's fp32 bar"""
    N, d, k, S, F = 333, 2, 1, 4, 48
    X, y, Xs, _ = problem(N, d, k, seed=6)
    z = np.random.default_rng(8).standard_normal(pw.n_normals("matern32", F, d, S, N)).astype(np.float32)
    with GP("matern32", 0.35, 1.5, 5e-2, dtype="float32") as gp:
        gp.fit(X, y)
        f = gp.sample_functions(S, n_features=F, z=z)(Xs)
        jit = gp.jitter_used_
    assert f.dtype == np.float32
    ref = pw.evaluate(pw.draw("matern32", X.astype(np.float32), y.astype(np.float32), 0.35, 1.5, 5e-2, z, S, F, jitter=jit), Xs.astype(np.float32))
    err = np.max(np.abs(as_smk(f, 1) - ref)) / np.max(np.abs(ref))
    print(f"float32 handle: err {err:.2e} of max |ref|")
    assert err <= 2e-3


def test_a_changed_model_ends_the_draw():
    N, d, k, S, F = 130, 1, 1, 3, 32
    X, y, Xs, _ = problem(N + 40, d, k, seed=4)
    with GP("rbf", 0.25, 1.5, 1e-2) as gp:
        gp.fit(X[:N], y[:N])
        fs = gp.sample_functions(S, n_features=F, random_state=1)
        fs(Xs)
        gp.update(X[N:], y[N:])
        with pytest.raises(RuntimeError, match="model changed"):
            fs(Xs)
        z = np.random.default_rng(1).standard_normal(pw.n_normals("rbf", F, d, S, N + 40))
        f = gp.sample_functions(S, n_features=F, z=z)                                      # a new draw: the changed model's
        ref = pw.evaluate(pw.draw("rbf", X, y, 0.25, 1.5, 1e-2, z, S, F, jitter=gp.jitter_used_), Xs)
        assert np.max(np.abs(as_smk(f(Xs), 1) - ref)) <= 1e-6 * np.max(np.abs(ref))
        gp.remove(0, 10)
        with pytest.raises(RuntimeError, match="model changed"):
            f(Xs)
        z = z[:pw.n_normals("rbf", F, d, S, N + 30)]
        f = gp.sample_functions(S, n_features=F, z=z)
        ref = pw.evaluate(pw.draw("rbf", X[10:], y[10:], 0.25, 1.5, 1e-2, z, S, F, jitter=gp.jitter_used_), Xs)
        assert np.max(np.abs(as_smk(f(Xs), 1) - ref)) <= 1e-6 * np.max(np.abs(ref))
        gp.fit(X[:N], y[:N])
        with pytest.raises(RuntimeError, match="model changed"):
            f(Xs)
        older = gp.sample_functions(S, n_features=F, random_state=1)
        newer = gp.sample_functions(S, n_features=F, random_state=2)                       # one draw is live per model
        with pytest.raises(RuntimeError):
            older(Xs)
        newer(Xs)
        newer.close()
        with pytest.raises(RuntimeError):
            newer(Xs)
        # the C call without a live draw: GPX_E_ARG, and the message says so
        out = np.zeros((1, len(Xs), 1))
        rc = gp._lib.gpx_pathwise_eval(gp._h, C.c_void_p(Xs.ctypes.data), len(Xs), 0, 1, C.c_void_p(out.ctypes.data),
                                       _abi.MEM_HOST)
        assert rc == _abi.E_ARG and b"no live draw" in gp._lib.gpx_last_error(gp._h)


def test_release_scratch_keeps_the_draw():
    X, y, Xs, _ = problem(130, 2, 1, seed=5)
    with GP("matern52", 0.3, 1.5, 1e-2) as gp:
        gp.fit(X, y)
        fs = gp.sample_functions(3, n_features=32, random_state=3)
        a = fs(Xs)
        gp._check(gp._lib.gpx_release_scratch(gp._h))
        assert np.array_equal(fs(Xs), a)


def refused_fit(name):
    rng = np.random.default_rng(17)
    X, y, Xs, _ = problem(200, 2, 1, seed=17)
    if name == "derivatives":
        return X, y, Xs, dict(derivatives=(rng.uniform(0, 1, (20, 2)), rng.integers(0, 2, 20), rng.standard_normal(20)),
                              derivative_noise=5e-2)
    if name == "path_ids":
        return X, y, Xs, dict(path_ids=np.arange(200) // 20, path_variance=0.3)
    return X, y, Xs, (dict(basis="linear") if name == "basis" else {})


REFUSED = {"mixed": (dict(dtype="mixed"), "GPX_MIXED"), "one_rank_group": (dict(devices=1, transport="local"), "device groups"),
           "derivatives": ({}, "derivative observations"), "path_ids": ({}, "path ids"), "basis": ({}, "basis")}


@pytest.mark.parametrize("name", list(REFUSED))
def test_refusals_keep_the_fit(name):
    kw, word = REFUSED[name]
    X, y, Xs, fit_kw = refused_fit(name)
    with GP("rbf", 0.4, 1.2, 5e-2, **kw) as gp:
        gp.fit(X, y, **fit_kw)
        m0, v0 = gp.predict(Xs)
        with pytest.raises(GpxError) as e:
            gp.sample_functions(3, n_features=16)
        assert e.value.code == _abi.E_UNSUPPORTED and word in str(e.value)
        m1, v1 = gp.predict(Xs)
        assert np.array_equal(m0, m1) and np.array_equal(v0, v1)
