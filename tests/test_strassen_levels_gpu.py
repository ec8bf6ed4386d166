"""GPU: the second Strassen level of strassen_nt (GPX_STRASSEN_MIN_TWO).

Each of the seven half-size products of a Strassen level takes another level when its own quadrants are at least
``GPX_STRASSEN_MIN_TWO`` rows and columns (default 4096, i.e. first-level products of 8192 and more: N = 65536).  The switch is
read at the start of every call, so the path is forced here at a few thousand rows, on top of the switches
tests/test_two_level_gpu.py forces: ``GPX_TWO_LEVEL_FROM=1024 GPX_STRASSEN_MIN=128 GPX_STRASSEN_MIN_TWO=128``.

Shapes.  gpx_gemm_nt (m, n, k), k-step 16:
  (512, 512, 64), (512, 512, 128)   halves 256, quadrants 128: the smallest shapes that take both levels with nothing
                                    peeled (the half's k is two / four k-steps)
  (896, 640, 112)                   first-level halves 384 x 256 (128 rows and columns peeled); the second level takes 256
                                    rows of the 384 and peels 128; k remainders at both levels (112 = 96 + 16, 48 = 32 + 16)
  (1024, 512, 1024)
GP.fit: N = 4500 with GPX_NB_WIDE_FROM=2048 (Npad = 4608, c = 2048; off-diagonal block of the deep update 1280 x 1280 x
2048, halves 640: the second level takes 512 and peels 128; a single panel left of c, so nothing is deferred there) and
N = 2900, block 512 (Npad = 2944, c = 1536, c1 = 1024; the deep update's block 768 x 640 x 1536 with halves 384 x 256, and
the deferred product 1408 x 512 x 1024 with halves 640 x 256: rows peeled at both levels in either).

Bars (BARS, GEMM_BAR) follow the rule of tests/test_two_level_gpu.py: one decade above the largest two-level error that
profiles/strassen_l2_parity.json (tools/strassen_l2_parity.py, these inputs) records, never looser than the full-size
bars (1e-6, 1e-6, 1e-8, 1e-12); where that would sit less than a decade above the one-level error the existing bar holds.
Every test prints its figures before it asserts them."""
import contextlib
import ctypes as C

import numpy as np
import pytest

from gaussianprocesspathmodelling_amd import GP, _abi
from oracle.gp_oracle import OracleGP, synthetic_problem

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
SF2, SN2, LS, M = 1.5, 1e-2, 0.25, 300
SWITCHES = ("GPX_TWO_LEVEL_FROM", "GPX_STRASSEN_MIN", "GPX_STRASSEN_MIN_TWO", "GPX_STRASSEN_DIAG", "GPX_STRASSEN_SINGLE",
            "GPX_NB_WIDE_FROM", "GPX_NB_PRED", "GPX_DEFER_LEFT")
ONE = {"GPX_TWO_LEVEL_FROM": "1024", "GPX_STRASSEN_MIN": "128"}                              # the new switch unset
ONE0 = {**ONE, "GPX_STRASSEN_MIN_TWO": "0"}
TWO = {**ONE, "GPX_STRASSEN_MIN_TWO": "128"}
# (mean, variance, alpha, log-det), from profiles/strassen_l2_parity.json.  Largest errors with two levels 8.427e-11,
# 3.470e-11, 5.911e-12, 8.86e-16; with one level 1.242e-10, 3.470e-11, 4.698e-12, 1.181e-15.  Variance and alpha: one
# decade above the two-level error, both below the full-size bars.  Mean and log-det: that would be less than a decade
# above the one-level error, so the existing bars hold: the full-size 1e-6 and 1e-12.
BARS = (1e-6, 3.48e-10, 5.92e-11, 1e-12)
# gpx_gemm_nt: the largest difference from NumPy over max|A| max|B| k eps in that file is 0.0857 classical, 0.1304 with one
# level and 0.2090 with two; one decade above the last
GEMM_BAR = 2.1
GEMM_SHAPES = [(512, 512, 64), (512, 512, 128), (896, 640, 112), (1024, 512, 1024)]

CASES = {   # name: (N, block, extra environment, Npad, c)
    "n4500_wide": (4500, 0, {"GPX_NB_WIDE_FROM": "2048"}, 4608, 2048),
    "n2900_b512": (2900, 512, {}, 2944, 1536),
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
    """the problem, OracleGP's outputs and its factor (LAPACK's), once per size"""
    if N not in _REF:
        X, y, Xs = synthetic_problem(N, 3, M, seed=N)
        og = OracleGP("rbf", LS, SF2, SN2, jitter=0.0).fit(X, y)
        mean, var = og.predict(Xs)
        _REF[N] = dict(X=X, y=y, Xs=Xs, mean=mean, var=var, alpha=og.alpha_, logdet=og.log_det_, L=np.tril(og.L_))
    return _REF[N]


def errors(alpha, logdet, r, mean, var):
    """the error definitions of tests/test_full_size_gpu.py"""
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
    return dict(L=read_factor(gp, npad), mean=mean.copy(), var=var.copy(), alpha=gp.alpha_.copy(), logdet=gp.log_det_,
                timings=dict(gp.timings_))


_RUNS = {}


def fit_run(case, env):
    """one fit + predict of a case under the switches `env`, once per (case, env)"""
    key = (case, tuple(sorted(env.items())))
    if key not in _RUNS:
        N, block, extra, npad = CASES[case][:4]
        r = reference(N)
        with switches({**extra, **env}), GP("rbf", LS, SF2, SN2, jitter=0.0, block=block, profile=True) as gp:
            out = one_fit(gp, r, npad)
        out["errors"] = errors(out["alpha"], out["logdet"], r, out["mean"], out["var"])
        _RUNS[key] = out
    return _RUNS[key]


def same_bits(a, b, what=("L", "mean", "var", "alpha")):
    for q in what:
        assert np.array_equal(a[q], b[q]), q
    assert a["logdet"] == b["logdet"]


def gemm_inputs(m, n, k):
    rng = np.random.default_rng(m + n + k)
    return rng.standard_normal((m, k)), rng.standard_normal((n, k)), rng.standard_normal((m, n))


def gemm_run(gpx, m, n, k, env):
    A, B, C0 = gemm_inputs(m, n, k)
    Cg = C0.copy()
    with switches(env):
        assert gpx.gpx_gemm_nt(_abi.dptr(Cg), m, n, _abi.dptr(A), _abi.dptr(B), k, 0) == 0
    unit = np.max(np.abs(A)) * np.max(np.abs(B)) * k * EPS
    return Cg, float(np.max(np.abs(Cg - (C0 - A @ B.T))) / unit)


def strassen_flops(m, n, k, min2):
    """the flops strassen_nt executes in fp64 (k-step 16): 2 m n k where classical, 7/8 of that on the part that takes one
    level, 49/64 on the part that takes both"""
    full = 2.0 * m * n * k
    m0, n0, k0 = m // 256 * 256, n // 256 * 256, k // 32 * 32
    if min(m0, n0, k0) == 0:
        return full
    mh, nh, kh = m0 // 2, n0 // 2, k0 // 2
    m2, n2, k2 = mh // 256 * 256, nh // 256 * 256, kh // 32 * 32
    second = min2 > 0 and k2 > 0 and min(m2, n2) > 0 and min(m2, n2) // 2 >= min2
    return full - 2.0 * m0 * n0 * k0 / 8 - (7 * 2.0 * m2 * n2 * k2 / 8 if second else 0.0)


@pytest.mark.parametrize("m, n, k", GEMM_SHAPES)
def test_gemm_nt_on_two_levels(gpx, m, n, k):
    _, e0 = gemm_run(gpx, m, n, k, {"GPX_STRASSEN_MIN": "0"})
    C1, e1 = gemm_run(gpx, m, n, k, {"GPX_STRASSEN_MIN": "128", "GPX_STRASSEN_MIN_TWO": "0"})
    C2, e2 = gemm_run(gpx, m, n, k, {"GPX_STRASSEN_MIN": "128", "GPX_STRASSEN_MIN_TWO": "128"})
    print(f"strassen_nt {m}x{n}x{k}: classical {e0:.3e}, one level {e1:.3e}, two levels {e2:.3e} (of max|A| max|B| k eps)")
    assert not np.array_equal(C1, C2), "the second level did not run"
    assert e2 <= GEMM_BAR


@pytest.mark.parametrize("m, n, k", GEMM_SHAPES)
def test_gemm_nt_switch_off_is_one_level(gpx, m, n, k):
    """GPX_STRASSEN_MIN_TWO=0 and the switch unset (default 4096: far above these quadrants): both one level, the same bits"""
    Cu, _ = gemm_run(gpx, m, n, k, {"GPX_STRASSEN_MIN": "128"})
    C0, _ = gemm_run(gpx, m, n, k, {"GPX_STRASSEN_MIN": "128", "GPX_STRASSEN_MIN_TWO": "0"})
    assert np.array_equal(Cu, C0)


@pytest.mark.parametrize("case", list(CASES))
def test_fit_matches_the_oracle(case):
    e1, e = fit_run(case, ONE0)["errors"], fit_run(case, TWO)["errors"]
    print(f"Strassen levels {case}, one: mean {e1[0]:.3e} var {e1[1]:.3e} alpha {e1[2]:.3e} logdet {e1[3]:.3e}")
    print(f"Strassen levels {case}, two: mean {e[0]:.3e} var {e[1]:.3e} alpha {e[2]:.3e} logdet {e[3]:.3e}")
    assert all(x <= bar for x, bar in zip(e, BARS)), (e, BARS)


@pytest.mark.parametrize("case", list(CASES))
def test_factor_against_lapack(case):
    """lower triangle with a positive diagonal, L L^T = K to the bar of the gpx_potrf tests (8 n eps in the Frobenius
    norm), and the factor itself no further from LAPACK's than ten times what one level is"""
    N = CASES[case][0]
    ref = reference(N)["L"]
    L1, L2 = fit_run(case, ONE0)["L"][:N, :N], fit_run(case, TWO)["L"][:N, :N]
    assert not np.array_equal(L1, L2), "the second level did not run"
    assert np.all(np.diag(L2) > 0) and np.all(np.isfinite(L2))
    K = ref @ ref.T
    berr = np.linalg.norm(L2 @ L2.T - K) / np.linalg.norm(K)
    scale = np.max(np.abs(ref))
    f1, f2 = np.max(np.abs(L1 - ref)) / scale, np.max(np.abs(L2 - ref)) / scale
    print(f"Strassen levels {case}: backward error {berr:.2e} (bar {8 * N * EPS:.2e}); factor error one level {f1:.3e}, two {f2:.3e}")
    assert berr <= 8 * N * EPS
    assert f2 <= 10 * f1


@pytest.mark.parametrize("case", list(CASES))
def test_syrk_flops_count_the_flops_executed(case):
    """no one-level trailing update of these fits is large enough to be booked, so syrk_flops is the deep update's: two
    triangles at K = c and the block between them, 49/64 where both levels ran: this is what shows that the level ran"""
    _, _, _, npad, c = CASES[case]
    np_ = npad - c
    hh = np_ // 2 // 128 * 128
    tri = float(hh * (hh + 1) * c + (np_ - hh) * (np_ - hh + 1) * c)
    for env, min2, launches in ((ONE0, 0, 9), (TWO, 128, 51)):
        tm = fit_run(case, env)["timings"]
        want = tri + strassen_flops(np_ - hh, hh, c, min2)
        print(f"{case} MIN2={min2}: syrk_flops {tm['syrk_flops']:.6e} (expected {want:.6e}), launches {tm['syrk_launches']}")
        assert tm["syrk_flops"] == want and tm["syrk_launches"] == launches
    assert strassen_flops(np_ - hh, hh, c, 128) < strassen_flops(np_ - hh, hh, c, 0)


@pytest.mark.parametrize("case", list(CASES))
def test_fit_is_repeatable_bit_for_bit(case):
    """two fits on one handle, one on a fresh handle"""
    N, block, extra, npad = CASES[case][:4]
    r = reference(N)
    base = fit_run(case, TWO)
    with switches({**extra, **TWO}):
        with GP("rbf", LS, SF2, SN2, jitter=0.0, block=block) as gp:
            runs = [one_fit(gp, r, npad), one_fit(gp, r, npad)]
    for other in runs:
        same_bits(base, other)


@pytest.mark.parametrize("case", list(CASES))
def test_fit_does_not_depend_on_stream_timing(case):
    """random delays in front of a third of all launches (gpx_debug_set_delay), two seeds: bit-identical"""
    N, block, extra, npad = CASES[case][:4]
    r = reference(N)
    lib = _abi.load()
    base = fit_run(case, TWO)
    try:
        with switches({**extra, **TWO}), GP("rbf", LS, SF2, SN2, jitter=0.0, block=block) as gp:
            for seed in (1, 123456789):
                lib.gpx_debug_set_delay(seed)
                got = one_fit(gp, r, npad)
                lib.gpx_debug_set_delay(0)
                same_bits(base, got)
    finally:
        lib.gpx_debug_set_delay(0)


def test_default_untouched_at_small_n():
    """the new switch unset (default 4096) and GPX_STRASSEN_MIN_TWO=0: the same one-level fit bit for bit"""
    same_bits(fit_run("n4500_wide", ONE), fit_run("n4500_wide", ONE0))


def test_fp32_takes_one_level_only():
    """fp32 takes the first level only with GPX_STRASSEN_SINGLE=1 and the second never"""
    r = reference(4500)
    outs = []
    for env in (ONE0, TWO):
        with switches({**env, "GPX_STRASSEN_SINGLE": "1"}), \
                GP("rbf", LS, SF2, SN2, jitter=0.0, dtype="float32", profile=True) as gp:
            mean, var = gp.fit(r["X"], r["y"]).predict(r["Xs"])
            assert gp.info_ == 0 and mean.dtype == np.float32
            assert gp.timings_["syrk_launches"] == 9
            outs.append(dict(mean=mean.copy(), var=var.copy(), alpha=gp.alpha_.copy(), logdet=gp.log_det_))
    same_bits(outs[0], outs[1], what=("mean", "var", "alpha"))


def test_fit_predict_takes_no_level():
    """gpx_fit_predict (query rows ride through the factorisation) stays on the one-level schedule"""
    r = reference(4500)
    outs = []
    for env in (ONE0, TWO):
        with switches({**CASES["n4500_wide"][2], **env}), GP("rbf", LS, SF2, SN2, jitter=0.0) as gp:
            mean, var = gp.fit_predict(r["X"], r["y"], r["Xs"])
            assert gp.info_ == 0
            outs.append(dict(mean=mean.copy(), var=var.copy(), logdet=gp.log_det_))
    same_bits(outs[0], outs[1], what=("mean", "var"))
