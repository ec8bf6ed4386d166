"""GPU: the two-level Cholesky (chol_two_level_enqueue) and its Strassen level (strassen_nt).

By default the split applies from Npad = 65536 on (``GPX_TWO_LEVEL_FROM``) and a Strassen level to quadrants of at least
4096 (``GPX_STRASSEN_MIN``); the switches are read at the start of every call, so the path is forced here at a few
thousand rows, as tests/test_wide_panels_gpu.py forces the wide panels:

  split only   ``GPX_TWO_LEVEL_FROM=1024``: left block column, ONE deep update at K = c, right block.  Classical
               products only, so the bars are the ones the one-level path is held to.
  Strassen     also ``GPX_STRASSEN_MIN=128``: the off-diagonal block of the deep update takes one Strassen level;
               ``GPX_STRASSEN_DIAG=1``: the off-diagonal blocks of its two diagonal halves as well.

Shapes: gpx_potrf n = 3072, block 512 (c = 1536; off-diagonal block 768 x 768 x 1536, quadrants 384 x 384 x 768);
GP.fit N = 4500 with the default block and with GPX_NB_WIDE_FROM=2048 (Npad = 4608, c = 2048, right block 2560, halves
1280); N = 2900, block 512 (Npad = 2944, c = 1536, right block 1408, off-diagonal block 768 x 640: the last 128 columns
are peeled off and done classically).

Bars.  Errors are those of tests/test_full_size_gpu.py (mean and variance elementwise relative with floors 1e-6 and
1e-6 sf2, alpha over its largest entry, log-det relative), against OracleGP.  profiles/two_level_parity.json records them
for the one-level path and for the Strassen path on exactly these inputs.  A Strassen bar is one decade above the largest
Strassen error recorded, never looser than the full-size bars (1e-6, 1e-6, 1e-8, 1e-12); where that would sit less than a
decade above the one-level path's error the existing bar of tests/test_wide_panels_gpu.py / the full-size bar holds:
see BARS.  Every test prints its figures before it asserts them."""
import contextlib
import ctypes as C

import numpy as np
import pytest

from gaussianprocesspathmodelling_amd import GP, _abi
from oracle.gp_oracle import OracleGP, chol_lower, kernel_matrix, synthetic_problem

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
SF2, SN2, LS, M = 1.5, 1e-2, 0.25, 300
SWITCHES = ("GPX_TWO_LEVEL_FROM", "GPX_STRASSEN_MIN", "GPX_STRASSEN_DIAG", "GPX_STRASSEN_SINGLE", "GPX_NB_WIDE_FROM", "GPX_NB_PRED")
SPLIT = {"GPX_TWO_LEVEL_FROM": "1024", "GPX_STRASSEN_MIN": "0"}
STRASSEN = {"GPX_TWO_LEVEL_FROM": "1024", "GPX_STRASSEN_MIN": "128"}
DIAG = {"GPX_TWO_LEVEL_FROM": "1024", "GPX_STRASSEN_MIN": "128", "GPX_STRASSEN_DIAG": "1"}
# (mean, variance, alpha, log-det), from profiles/two_level_parity.json.  Largest Strassen errors 1.251e-10, 3.470e-11,
# 4.698e-12, 7.43e-16; the one-level path's 9.59e-11, 3.470e-11, 4.24e-12, 1.11e-15.  One decade above the Strassen
# errors for the first three (all below the full-size bars); for the log-det that would be 7.4e-15, less than a decade
# above the one-level path's error, so the existing bar holds: the full-size 1e-12.
BARS = (1.26e-9, 3.48e-10, 4.70e-11, 1e-12)

CASES = {   # name: (N, block, extra environment)
    "n4500": (4500, 0, {}),
    "n4500_wide": (4500, 0, {"GPX_NB_WIDE_FROM": "2048"}),
    "n2900_b512": (2900, 512, {}),
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
    """the problem and OracleGP's outputs, once per size"""
    if N not in _REF:
        X, y, Xs = synthetic_problem(N, 3, M, seed=N)
        og = OracleGP("rbf", LS, SF2, SN2, jitter=0.0).fit(X, y)
        mean, var = og.predict(Xs)
        _REF[N] = dict(X=X, y=y, Xs=Xs, mean=mean, var=var, alpha=og.alpha_, logdet=og.log_det_)
    return _REF[N]


def errors(gp, r, mean, var):
    mean, var, alpha = np.asarray(mean, np.float64), np.asarray(var, np.float64), np.asarray(gp.alpha_, np.float64)
    return (float(np.max(np.abs(mean - r["mean"]) / np.maximum(np.abs(r["mean"]), 1e-6))),
            float(np.max(np.abs(var - r["var"]) / np.maximum(r["var"], 1e-6 * SF2))),
            float(np.max(np.abs(alpha - r["alpha"])) / np.max(np.abs(r["alpha"]))),
            abs(gp.log_det_ - r["logdet"]) / abs(r["logdet"]))


def fit_errors(case, env, **kw):
    N, block, extra = CASES[case]
    r = reference(N)
    with switches({**extra, **env}), GP("rbf", LS, SF2, SN2, jitter=0.0, block=block, **kw) as gp:
        mean, var = gp.fit(r["X"], r["y"]).predict(r["Xs"])
        assert gp.info_ == 0
        return errors(gp, r, mean, var), gp.timings_


def spd(n):
    rng = np.random.default_rng(n)
    Xp = rng.uniform(size=(n, 3))
    K = kernel_matrix(Xp, Xp, "rbf", LS, SF2)
    K[np.diag_indices(n)] += SN2
    return K


@pytest.mark.parametrize("env", [SPLIT, STRASSEN], ids=["split", "strassen"])
def test_potrf_on_two_levels(gpx, env):
    """n = 3072, block 512: the bars of tests/test_kernels_gpu.py::test_potrf_backward_error"""
    n = 3072
    K = spd(n)
    A = np.tril(K) + np.triu(np.full((n, n), 777.0), 1)
    info = C.c_int64(-1)
    with switches(env):
        assert gpx.gpx_potrf(_abi.dptr(A), n, 512, C.byref(info)) == 0
    assert info.value == 0
    L = np.tril(A)
    berr = np.linalg.norm(L @ L.T - K) / np.linalg.norm(K)
    ref = chol_lower(K)
    ferr = np.max(np.abs(L - ref)) / np.max(np.abs(ref))
    print(f"potrf two-level {env}: backward error {berr:.2e} (bar {8 * n * EPS:.2e}), factor error {ferr:.2e} (bar 1e-9)")
    assert berr <= 8 * n * EPS
    assert ferr <= 1e-9


@pytest.mark.parametrize("case", list(CASES))
def test_split_only_fit_matches_the_oracle(case):
    """classical products only: the bars of tests/test_wide_panels_gpu.py (1e-6 elementwise, alpha 1e-7, log-det 1e-9)"""
    e, _ = fit_errors(case, SPLIT)
    print(f"two-level split {case}: mean {e[0]:.2e} var {e[1]:.2e} alpha {e[2]:.2e} logdet {e[3]:.2e}")
    assert e[0] <= 1e-6 and e[1] <= 1e-6 and e[2] <= 1e-7 and e[3] <= 1e-9


@pytest.mark.parametrize("case, env", [("n4500", STRASSEN), ("n4500_wide", STRASSEN), ("n2900_b512", STRASSEN),
                                       ("n4500_wide", DIAG)],
                         ids=["n4500", "n4500_wide", "n2900_b512", "n4500_wide_diag"])
def test_strassen_fit_matches_the_oracle(case, env):
    e, _ = fit_errors(case, env)
    print(f"two-level Strassen {case}: mean {e[0]:.2e} var {e[1]:.2e} alpha {e[2]:.2e} logdet {e[3]:.2e}")
    assert all(x <= bar for x, bar in zip(e, BARS)), (e, BARS)


def test_strassen_fit_fp32():
    """the level of tests/test_fp32_gpu.py, against the fp64 oracle"""
    N = 4500
    r = reference(N)
    with switches({**STRASSEN, "GPX_STRASSEN_SINGLE": "1"}), GP("rbf", LS, SF2, SN2, jitter=0.0, dtype="float32", profile=True) as gp:
        mean, var = gp.fit(r["X"], r["y"]).predict(r["Xs"])
        assert gp.info_ == 0 and mean.dtype == np.float32
        assert gp.timings_["syrk_launches"] == 9     # the level ran: two triangles and seven products
        em = np.max(np.abs(mean - r["mean"])) / np.max(np.abs(r["mean"]))
        ev = np.max(np.abs(var - r["var"])) / SF2
        el = abs(gp.log_det_ - r["logdet"]) / abs(r["logdet"])
    print(f"two-level Strassen fp32: mean {em:.2e} var {ev:.2e} logdet {el:.2e}")
    assert em <= 2e-3 and ev <= 2e-3 and el <= 1e-3


def read_factor(gp, n):
    """rows [0, n) of the handle's K buffer (the factor's lower triangle and whatever lies above it)"""
    ptr, ld, cap = C.c_void_p(0), C.c_int64(0), C.c_int64(0)
    gp._check(gp._lib.gpx_factor_info(gp._h, C.byref(ptr), C.byref(ld), C.byref(cap)))
    hip = _abi._preload_torch_hip_runtime() or C.CDLL("libamdhip64.so")
    out = np.empty((n, ld.value))
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    assert hip.hipMemcpy(out.ctypes.data, ptr.value, out.nbytes, 2) == 0   # device to host
    return np.tril(out[:, :n])


def test_strassen_fit_is_repeatable_bit_for_bit():
    N = 4500
    r = reference(N)
    runs = []
    with switches({**CASES["n4500_wide"][2], **DIAG}):
        with GP("rbf", LS, SF2, SN2, jitter=0.0) as gp:
            for _ in range(2):
                mean, var = gp.fit(r["X"], r["y"]).predict(r["Xs"])
                runs.append((read_factor(gp, 4608), mean.copy(), var.copy()))
        with GP("rbf", LS, SF2, SN2, jitter=0.0) as gp:
            mean, var = gp.fit(r["X"], r["y"]).predict(r["Xs"])
            runs.append((read_factor(gp, 4608), mean.copy(), var.copy()))
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            assert np.array_equal(a, b)


@pytest.mark.parametrize("m, n, k", [(512, 512, 96), (640, 512, 80)], ids=["even", "ragged"])
def test_strassen_nt_alone(gpx, m, n, k):
    """gpx_gemm_nt with GPX_STRASSEN_MIN=128 against NumPy.  The bar is measured against the classical launch on the same
    inputs: one decade over its error, both relative to max|A| max|B| k eps (recorded in profiles/two_level_parity.json)."""
    rng = np.random.default_rng(m + n + k)
    A, B, C0 = rng.standard_normal((m, k)), rng.standard_normal((n, k)), rng.standard_normal((m, n))
    ref = C0 - A @ B.T
    unit = np.max(np.abs(A)) * np.max(np.abs(B)) * k * EPS
    err = {}
    for name, env in (("classical", {"GPX_STRASSEN_MIN": "0"}), ("strassen", {"GPX_STRASSEN_MIN": "128"})):
        Cg = C0.copy()
        with switches(env):
            assert gpx.gpx_gemm_nt(_abi.dptr(Cg), m, n, _abi.dptr(A), _abi.dptr(B), k, 0) == 0
        err[name] = float(np.max(np.abs(Cg - ref)) / unit)
    print(f"strassen_nt {m}x{n}x{k}: classical {err['classical']:.3e}, Strassen {err['strassen']:.3e} (of max|A| max|B| k eps)")
    assert err["strassen"] != err["classical"], "the Strassen level did not run"
    assert err["strassen"] <= 10 * err["classical"]


def test_syrk_flops_count_the_flops_executed():
    """N = 4500, wide panels: no one-level trailing update is large enough to be booked, so syrk_flops is the deep
    update's: two triangles at K = c, and the 1280 x 1280 x 2048 block between them at 7/8"""
    c, np_, hh = 2048, 2560, 1280
    tri = hh * (hh + 1) * c + (np_ - hh) * (np_ - hh + 1) * c
    rect = 2.0 * (np_ - hh) * hh * c
    _, tm = fit_errors("n4500_wide", SPLIT, profile=True)
    print(f"split: syrk_flops {tm['syrk_flops']:.6e}, launches {tm['syrk_launches']}")
    assert tm["syrk_flops"] == float(np_ * (np_ + 1) * c) and tm["syrk_launches"] == 1
    _, tm = fit_errors("n4500_wide", STRASSEN, profile=True)
    print(f"Strassen: syrk_flops {tm['syrk_flops']:.6e}, launches {tm['syrk_launches']}")
    assert tm["syrk_flops"] == tri + rect * 7 / 8 and tm["syrk_launches"] == 9
