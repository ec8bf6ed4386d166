"""GPU: the deferred product in the left block column of the two-level Cholesky (GPX_DEFER_LEFT).

While the panels left of c1 (the panel boundary nearest c / 2) run, the 128-tile rows of A21 are updated in columns
[t0, c1) only; behind the side step of the last of those panels ONE product at K = c1,
A21[:, c1:c] -= L21[:, 0:c1] L11[c1:c, 0:c1]^T, makes up for it — through strassen_nt where the level is on.  The path is
forced at a few thousand rows with ``GPX_TWO_LEVEL_FROM=1024 GPX_STRASSEN_MIN=128`` as in tests/test_two_level_gpu.py.

Shapes (the smallest that reach every branch):
  potrf3072   gpx_potrf n = 3072, block 512: c = 1536, three panels, c1 = 1024 (not c / 2), np = 1536, no bordered rows;
  n4500       GP.fit N = 4500, default block: Npad = 4608, nb = 1024, c = 2048, c1 = 1024, product 2560 x 1024 x 1024, the 64
              right-hand-side rows stay right-looking; temporaries in panel buffer 0;
  n2900_b512  GP.fit N = 2900, block 512: Npad = 2944, c = 1536, c1 = 1024, np = 1408 rows: 128 of them peeled off by
              strassen_nt; temporaries in panel buffer 1;
  n4500_wide  N = 4500 with GPX_NB_WIDE_FROM=2048: phase 1 is a single panel, nothing is deferred.

Bars.  Errors are those of tests/test_two_level_gpu.py against OracleGP.  profiles/deferred_left_parity.json records them
on exactly these inputs with the path off and on.  A bar is one decade above the largest error recorded with the path on,
never looser than the full-size bars (1e-6, 1e-6, 1e-8, 1e-12); where that would sit less than a decade above the
path-off error the full-size bar holds: see BARS.  Factor errors are against the oracle's LAPACK factor (chol_lower),
with the path off and with it on — never against the code under test.  Every test prints its figures before it asserts."""
import contextlib
import ctypes as C

import numpy as np
import pytest

from gaussianprocesspathmodelling_amd import GP, _abi
from oracle.gp_oracle import OracleGP, chol_lower, kernel_matrix, synthetic_problem

pytestmark = pytest.mark.gpu

SF2, SN2, LS, M = 1.5, 1e-2, 0.25, 300
SWITCHES = ("GPX_TWO_LEVEL_FROM", "GPX_STRASSEN_MIN", "GPX_STRASSEN_DIAG", "GPX_STRASSEN_SINGLE", "GPX_NB_WIDE_FROM",
            "GPX_NB_PRED", "GPX_DEFER_LEFT", "GPX_CU_SELF_RESERVE")
STRASSEN = {"GPX_TWO_LEVEL_FROM": "1024", "GPX_STRASSEN_MIN": "128"}
SPLIT = {"GPX_TWO_LEVEL_FROM": "1024", "GPX_STRASSEN_MIN": "0"}
OFF, ON = {"GPX_DEFER_LEFT": "0"}, {"GPX_DEFER_LEFT": "1"}
# (mean, variance, alpha, log-det), from profiles/deferred_left_parity.json (n4500 and n2900_b512, Strassen level on).
# Largest errors with the path on 1.242e-10, 3.249e-11, 4.567e-12, 1.181e-15; with it off 1.251e-10, 3.323e-11, 4.137e-12,
# 7.44e-16.  Mean and variance: a decade above the path-on error is less than a decade above the path-off error, so the
# full-size bar (1e-6) holds.  Alpha and log-det: one decade above the path-on error, both below the full-size bars.
BARS = (1e-6, 1e-6, 4.57e-11, 1.19e-14)

CASES = {   # name: (N, block, extra environment, Npad, c, c1)
    "n4500": (4500, 0, {}, 4608, 2048, 1024),
    "n4500_wide": (4500, 0, {"GPX_NB_WIDE_FROM": "2048"}, 4608, 2048, 0),
    "n2900_b512": (2900, 512, {}, 2944, 1536, 1024),
}


@contextlib.contextmanager
def switches(env):
    with pytest.MonkeyPatch.context() as mp:
        for name in SWITCHES:
            mp.delenv(name, raising=False)
        for name, value in env.items():
            mp.setenv(name, value)
        yield


_REF = {}


def reference(N):
    """the problem, OracleGP's outputs and its factor, once per size"""
    if N not in _REF:
        X, y, Xs = synthetic_problem(N, 3, M, seed=N)
        og = OracleGP("rbf", LS, SF2, SN2, jitter=0.0).fit(X, y)
        mean, var = og.predict(Xs)
        # og.L_ is scipy's cholesky(K, lower=True) of K + sn2 I: the call chol_lower makes
        _REF[N] = dict(X=X, y=y, Xs=Xs, mean=mean, var=var, alpha=og.alpha_, logdet=og.log_det_, L=np.tril(og.L_))
    return _REF[N]


def errors(alpha, logdet, r, mean, var):
    mean, var, alpha = np.asarray(mean, np.float64), np.asarray(var, np.float64), np.asarray(alpha, np.float64)
    return (float(np.max(np.abs(mean - r["mean"]) / np.maximum(np.abs(r["mean"]), 1e-6))),
            float(np.max(np.abs(var - r["var"]) / np.maximum(r["var"], 1e-6 * SF2))),
            float(np.max(np.abs(alpha - r["alpha"])) / np.max(np.abs(r["alpha"]))),
            abs(logdet - r["logdet"]) / abs(r["logdet"]))


def read_factor(gp, n):
    """rows [0, n) of the handle's K buffer, lower triangle (as tests/test_two_level_gpu.py reads it)"""
    ptr, ld, cap = C.c_void_p(0), C.c_int64(0), C.c_int64(0)
    gp._check(gp._lib.gpx_factor_info(gp._h, C.byref(ptr), C.byref(ld), C.byref(cap)))
    hip = _abi._preload_torch_hip_runtime() or C.CDLL("libamdhip64.so")
    out = np.empty((n, ld.value))
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    assert hip.hipMemcpy(out.ctypes.data, ptr.value, out.nbytes, 2) == 0   # device to host
    return np.tril(out[:, :n])


def one_fit(gp, r, npad):
    mean, var = gp.fit(r["X"], r["y"]).predict(r["Xs"])
    assert gp.info_ == 0
    return dict(L=read_factor(gp, npad), mean=mean.copy(), var=var.copy(), alpha=gp.alpha_.copy(), logdet=gp.log_det_)


_RUNS = {}


def fit_run(case, env):
    """one fit + predict of a case under the switches `env`, once per (case, env)"""
    key = (case, tuple(sorted(env.items())))
    if key not in _RUNS:
        N, block, extra, npad = CASES[case][:4]
        r = reference(N)
        with switches({**extra, **env}), GP("rbf", LS, SF2, SN2, jitter=0.0, block=block) as gp:
            out = one_fit(gp, r, npad)
        out["errors"] = errors(out["alpha"], out["logdet"], r, out["mean"], out["var"])
        _RUNS[key] = out
    return _RUNS[key]


def check_structure(name, L0, L1, ref, n, c, c1):
    """L0 / L1: the factor with the path off / on (n rows of it are the matrix proper); ref: LAPACK's"""
    assert np.array_equal(L0[:c, :c], L1[:c, :c]), "L11 changed"
    assert np.array_equal(L0[c:, :c1], L1[c:, :c1]), "L21 left of c1 changed"
    assert not np.array_equal(L0[c:, c1:c], L1[c:, c1:c]), "the deferred product did not run"
    scale = np.max(np.abs(ref))
    e0 = np.max(np.abs(L0[c:n, c1:n] - ref[c:n, c1:n])) / scale
    e1 = np.max(np.abs(L1[c:n, c1:n] - ref[c:n, c1:n])) / scale
    print(f"deferred left {name}: factor error of L21[:, c1:c] and L22 against LAPACK, path off {e0:.3e}, on {e1:.3e}")
    assert e1 <= 10 * e0


def test_potrf_structure(gpx):
    n, c, c1 = 3072, 1536, 1024
    rng = np.random.default_rng(n)
    Xp = rng.uniform(size=(n, 3))
    K = kernel_matrix(Xp, Xp, "rbf", LS, SF2)
    K[np.diag_indices(n)] += SN2
    ref = chol_lower(K)
    Ls = []
    for env in (OFF, ON):
        A = np.tril(K) + np.triu(np.full((n, n), 777.0), 1)
        info = C.c_int64(-1)
        with switches({**STRASSEN, **env}):
            assert gpx.gpx_potrf(_abi.dptr(A), n, 512, C.byref(info)) == 0
        assert info.value == 0
        Ls.append(np.tril(A))
    check_structure("potrf3072", Ls[0], Ls[1], ref, n, c, c1)


@pytest.mark.parametrize("case", ["n4500", "n2900_b512"])
def test_fit_structure(case):
    N, _, _, _, c, c1 = CASES[case]
    check_structure(case, fit_run(case, {**STRASSEN, **OFF})["L"], fit_run(case, {**STRASSEN, **ON})["L"],
                    reference(N)["L"], N, c, c1)


def test_single_panel_left_column_defers_nothing():
    """GPX_NB_WIDE_FROM=2048: c = nb, no panel boundary inside the left block column: bit-identical to the path off"""
    a, b = fit_run("n4500_wide", {**STRASSEN, **OFF}), fit_run("n4500_wide", {**STRASSEN, **ON})
    for q in ("L", "mean", "var", "alpha"):
        assert np.array_equal(a[q], b[q]), q
    assert a["logdet"] == b["logdet"]


def test_default_is_on_with_the_level_and_off_without():
    """unset: the path of GPX_DEFER_LEFT=1 where the Strassen level is in force, that of 0 where it is not"""
    for env, same in ((STRASSEN, ON), (SPLIT, OFF)):
        a, b = fit_run("n4500", env), fit_run("n4500", {**env, **same})
        assert np.array_equal(a["L"], b["L"]), (env, same)


@pytest.mark.parametrize("case", ["n4500", "n2900_b512"])
def test_deferred_fit_matches_the_oracle(case):
    e0, e = fit_run(case, {**STRASSEN, **OFF})["errors"], fit_run(case, {**STRASSEN, **ON})["errors"]
    print(f"deferred left {case}, path off: mean {e0[0]:.3e} var {e0[1]:.3e} alpha {e0[2]:.3e} logdet {e0[3]:.3e}")
    print(f"deferred left {case}, path on:  mean {e[0]:.3e} var {e[1]:.3e} alpha {e[2]:.3e} logdet {e[3]:.3e}")
    assert all(x <= bar for x, bar in zip(e, BARS)), (e, BARS)


def test_classical_deferred_fit_matches_the_oracle():
    """GPX_DEFER_LEFT=1 without the level: one classical product.  The bars of test_split_only_fit_matches_the_oracle
    (1e-6 elementwise, alpha 1e-7, log-det 1e-9).  At N = 4500 a single panel lies left of c1, so the classical product
    is that panel's own update (the same addends in the same order); that the path runs shows at block 512, where the
    product sums two panels' addends before it subtracts them."""
    e = fit_run("n4500", {**SPLIT, **ON})["errors"]
    print(f"deferred left classical n4500: mean {e[0]:.3e} var {e[1]:.3e} alpha {e[2]:.3e} logdet {e[3]:.3e}")
    assert e[0] <= 1e-6 and e[1] <= 1e-6 and e[2] <= 1e-7 and e[3] <= 1e-9
    N, _, _, _, c, c1 = CASES["n2900_b512"]
    check_structure("n2900_b512 classical", fit_run("n2900_b512", {**SPLIT, **OFF})["L"],
                    fit_run("n2900_b512", {**SPLIT, **ON})["L"], reference(N)["L"], N, c, c1)


@pytest.mark.parametrize("k", [1, 4])
def test_self_reserving_launches_give_the_same_deferred_fit(k):
    """GPX_CU_SELF_RESERVE=k reaches the deferred product: at n2900_b512 strassen_nt peels 128 rows off through the
    classical launch, which then goes out in its self-reserving form (with rest_split / 2 = 8 every panel of phase 1 is
    chain-bound, so the reserve mode is on throughout).  The same arithmetic per tile under another launch geometry:
    bit-identical to the plain launches, as test_schedule_variants_give_the_same_factorisation asserts for the one-level
    fit."""
    a = fit_run("n2900_b512", {**STRASSEN, **ON})
    b = fit_run("n2900_b512", {**STRASSEN, **ON, "GPX_CU_SELF_RESERVE": str(k)})
    for q in ("L", "mean", "var", "alpha"):
        assert np.array_equal(a[q], b[q]), q


def test_deferred_fit_is_repeatable_bit_for_bit():
    """two fits on one handle, one on a fresh handle"""
    N, block, extra, npad = CASES["n4500"][:4]
    r = reference(N)
    runs = []
    with switches({**extra, **STRASSEN, **ON}):
        with GP("rbf", LS, SF2, SN2, jitter=0.0, block=block) as gp:
            runs += [one_fit(gp, r, npad), one_fit(gp, r, npad)]
        with GP("rbf", LS, SF2, SN2, jitter=0.0, block=block) as gp:
            runs.append(one_fit(gp, r, npad))
    for other in runs[1:]:
        for q in ("L", "mean", "var"):
            assert np.array_equal(runs[0][q], other[q]), q


def test_deferred_fit_does_not_depend_on_stream_timing():
    """the orderings of the deferred product (copy stream, STRIP_D on the chain, the panel buffer's next writer): random
    delays in front of a third of all launches (gpx_debug_set_delay), two seeds, bit-identical to the undisturbed run"""
    N, block, extra, npad = CASES["n4500"][:4]
    r = reference(N)
    lib = _abi.load()
    base = fit_run("n4500", {**STRASSEN, **ON})
    try:
        with switches({**extra, **STRASSEN, **ON}), GP("rbf", LS, SF2, SN2, jitter=0.0, block=block) as gp:
            for seed in (1, 123456789):
                lib.gpx_debug_set_delay(seed)
                got = one_fit(gp, r, npad)
                lib.gpx_debug_set_delay(0)
                for q in ("L", "mean", "var", "alpha"):
                    assert np.array_equal(base[q], got[q]), f"seed {seed}: {q} changed under timing perturbation"
                assert base["logdet"] == got["logdet"], f"seed {seed}"
    finally:
        lib.gpx_debug_set_delay(0)
