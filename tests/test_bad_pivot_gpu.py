"""GPU: the failure path of the Cholesky in every schedule — WHICH pivot is reported, and that the factor above it is valid.

include/gpx.h adopts LAPACK's potrf convention: info = p > 0 means the leading minor of order p is the first that is not
positive definite; rows [0, p - 1) of the factor are then the factor of that minor.  The index is put together by
potf2_lds (gidx0 + j + bad), the 128-wide diagonal kernel (a second call at gidx0 + 64), the two-level schedule (gidx0 + c),
and it depends on every update having reached a pivot before it is tested; a slip in any of them shows in a non-zero info
only.  The inputs (tests/bad_pivot_ref.py) make the failing pivot a matter of mathematics — a diagonal entry of -1 or NaN
in a positive definite matrix, a NaN input row in a well-conditioned fit — so the assertions are equalities with LAPACK's
info; tests/test_bad_pivot_ref.py holds the tables to LAPACK on the CPU.

Bars.  The prefix is held to what the whole factor of the same schedule is held to: |L L^T - K| / |K| <= 8 p0 eps in the
Frobenius norm and max |L - ref| <= 1e-9 max |ref| (tests/test_kernels_gpu.py::test_potrf_backward_error,
tests/test_two_level_gpu.py::test_potrf_on_two_levels, tests/test_strassen_levels_gpu.py::test_factor_against_lapack), with
K the reference matrix built on the CPU and ref LAPACK's factor of it.  fp32 fits: the project has no bar for an fp32
factor; the same backward-error bar with fp32's eps (the kernel matrix itself is rounded to fp32, one eps relative, and a
Cholesky's backward error is bounded by a small multiple of p0 eps); the forward error is printed only (cond(K) eps_32 is
of order 1e-2 here).  GPX_MIXED handles and device groups give no access to their factor (gpx_factor_info refuses them):
the index only.  Every test prints its figures before it asserts them.

After a failed fit gpx_factor_info refuses the handle, so a fit case first fits the clean problem on the same handle, takes
the factor's address (it changes only when a fit has to reallocate, include/gpx.h) and reads the rows from there."""
import contextlib
import ctypes as C

import numpy as np
import pytest

import bad_pivot_ref as bp
from bad_pivot_ref import EPS, EPS32, LS, SF2, SN2
from gaussianprocesspathmodelling_amd import GP, _abi
from oracle.gp_oracle import chol_lower, synthetic_problem

pytestmark = pytest.mark.gpu


@contextlib.contextmanager
def switches(env):
    with pytest.MonkeyPatch.context() as mp:
        for name in bp.SWITCHES:
            mp.delenv(name, raising=False)
        for name, value in env.items():
            mp.setenv(name, value)
        yield


# ---- gpx_potrf -----------------------------------------------------------------------------------------------------------
_INFO_REF = {}


def info_ref(n, bad):
    if (n, bad) not in _INFO_REF:
        _INFO_REF[n, bad] = bp.lapack_info(bp.indefinite(n, bad))
    return _INFO_REF[n, bad]


def potrf_figures(env, n, block, bad):
    """-> (rc, info, backward error and factor error of the prefix, or None where it is empty)"""
    K = bp.indefinite(n, bad)
    A = np.tril(K)
    A[np.triu_indices(n, 1)] = 777.0                                # poison the upper triangle
    info = C.c_int64(-7)
    with switches(env):
        rc = _abi.load().gpx_potrf(_abi.dptr(A), n, block, C.byref(info))
    p0 = bp.first_bad(bad)
    return rc, int(info.value), (bp.prefix_errors(A, bp.spd(n), bp.spd_factor(n), p0) if p0 else None)


POTRF = bp.potrf_cases()


@pytest.mark.parametrize("env, n, block, bad", [c[1:] for c in POTRF], ids=[c[0] for c in POTRF])
def test_potrf_reports_the_first_bad_pivot_above_a_valid_factor(gpx, env, n, block, bad):
    p0 = bp.first_bad(bad)
    rc, info, prefix = potrf_figures(env, n, block, bad)
    print(f"potrf n {n} block {block} {env} bad {bad}: rc {rc}, info {info} (LAPACK {info_ref(n, bad)})")
    assert rc == 0
    assert info >= 0, "a negative word is the parked stream's timeout, not a pivot"
    assert info == info_ref(n, bad) == p0 + 1
    if prefix:
        print(f"  prefix [0, {p0}): backward error {prefix[0]:.2e} (bar {8 * p0 * EPS:.2e}), factor error {prefix[1]:.2e} (bar 1e-9)")
        assert prefix[0] <= 8 * p0 * EPS
        assert prefix[1] <= 1e-9


# ---- fits ------------------------------------------------------------------------------------------------------------------
def factor_address(gp):
    ptr, ld, cap = C.c_void_p(0), C.c_int64(0), C.c_int64(0)
    gp._check(gp._lib.gpx_factor_info(gp._h, C.byref(ptr), C.byref(ld), C.byref(cap)))
    return ptr.value, ld.value


def device_rows(gp, address, n):
    """rows [0, n) of the K buffer at `address`, lower triangle (tests/test_deferred_left_gpu.py::read_factor)"""
    ptr, ld = address
    hip = _abi._preload_torch_hip_runtime() or C.CDLL("libamdhip64.so")
    out = np.empty((n, ld), dtype=gp._np_dtype)
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    assert hip.hipMemcpy(out.ctypes.data, ptr, out.nbytes, 2) == 0   # device to host
    return np.tril(out[:, :n])


def failing_fit(gp, prob, p0, read=True):
    """the clean fit (for the factor's address) where the factor is to be read, then the fit with the NaN row on the same
    handle -> (info, growth of handover_retries, the factor's address or None)"""
    address = None
    if read:
        gp.fit(prob["X"], prob["y"], **prob["fit"])
        assert gp.info_ == 0
        address = factor_address(gp)
    retries = gp.timings_["handover_retries"]
    Xn, kw = bp.with_nan_row(prob, p0)
    with pytest.raises(np.linalg.LinAlgError):                    # (rc != 0 raises GpxError instead)
        gp.fit(Xn, prob["y"], **kw)
    with pytest.raises(RuntimeError):
        gp.predict(prob["X"][:3])
    return gp.info_, gp.timings_["handover_retries"] - retries, address


def value_and_derivative_rows(prob):
    return np.concatenate([prob["X"], prob["fit"]["derivatives"][0]]) if "derivatives" in prob["fit"] else prob["X"]


def fit_figures(name):
    """-> (info, growth of handover_retries, prefix errors or None, eps of the factor's element type)"""
    case = bp.FIT_CASES[name]
    p0 = case["p0"]
    prob = bp.fit_problem(case["N"], case["variant"])
    with switches(case["env"]), GP("rbf", LS, SF2, SN2, jitter=0.0, block=case["block"], max_tries=1, **case["kw"]) as gp:
        info, grew, address = failing_fit(gp, prob, p0, case["read"])
        L = device_rows(gp, address, p0) if address and p0 else None
        eps = EPS32 if case["kw"].get("dtype") == "float32" else EPS
    prefix = None
    if L is not None:
        K = prob["gram"](value_and_derivative_rows(prob)[:p0])
        prefix = bp.prefix_errors(L, K, chol_lower(K), p0)
    return info, grew, prefix, eps


@pytest.mark.parametrize("name", list(bp.FIT_CASES))
def test_fit_with_a_nan_row_reports_that_row_above_a_valid_factor(name):
    case = bp.FIT_CASES[name]
    p0 = case["p0"]
    info, grew, prefix, eps = fit_figures(name)
    print(f"fit {name}: info {info} (NaN row {p0}), handover retries + {grew}")
    assert info >= 0 and grew == 0
    assert info == p0 + 1
    assert (prefix is not None) == (case["read"] and p0 > 0)
    if prefix:
        fp64 = eps == EPS
        print(f"  prefix [0, {p0}): backward error {prefix[0]:.2e} (bar {8 * p0 * eps:.2e}), factor error {prefix[1]:.2e}"
              + (" (bar 1e-9)" if fp64 else " (fp32: no bar)"))
        assert prefix[0] <= 8 * p0 * eps
        assert prefix[1] <= 1e-9 or not fp64


def test_fit_predict_with_a_nan_row_predicts_nothing():
    """tests/test_fit_predict_gpu.py::test_fit_predict_reports_a_bad_pivot_and_falls_back_where_unsupported with a pivot that
    is decided: N = 2048, M = 100, the query rows ride through the factorisation as bordered rows"""
    N, M, p0 = (bp.FIT_PREDICT[q] for q in ("N", "M", "p0"))
    X, y, Xs = synthetic_problem(N, 3, M, seed=9)
    X[p0, :] = np.nan
    with switches({}), GP("rbf", LS, SF2, SN2, jitter=0.0, max_tries=1) as gp:
        retries = gp.timings_["handover_retries"]
        with pytest.raises(np.linalg.LinAlgError):
            gp.fit_predict(X, y, Xs)
        print(f"fit_predict: info {gp.info_}")
        assert gp.info_ > 0
        assert gp.info_ == p0 + 1
        assert gp.timings_["handover_retries"] == retries
        with pytest.raises(RuntimeError):
            gp.predict(Xs)


def strassen_nan_row_figures():
    """-> (info, growth of handover_retries, prefix errors of rows [0, info - 1))"""
    case = bp.STRASSEN_NAN_ROW
    prob = bp.fit_problem(case["N"])
    with switches(bp.STRASSEN), GP("rbf", LS, SF2, SN2, jitter=0.0, block=case["block"], max_tries=1) as gp:
        info, grew, address = failing_fit(gp, prob, case["p0"])
        rows = min(max(info - 1, 0), case["npad"])
        L = device_rows(gp, address, rows) if rows else None
    K = prob["gram"](prob["X"][:rows])
    return info, grew, (bp.prefix_errors(L, K, chol_lower(K), rows) if rows else None)


def test_a_nan_row_right_of_c_under_a_strassen_level():
    """The one case that is not an equality with p0 + 1.  Row p0 >= c of A21 is NaN before the
    deferred product, whose Strassen level adds it to the row half a block away (bad_pivot_ref.strassen_partner_rows: row
    c + 324 for p0 = c + 964), which lies above p0: the first failing pivot is the smaller of the two.  Rows left of c never
    read row p0, so c < info <= p0 + 1 whatever the level does; the factor above the reported pivot is valid."""
    case = bp.STRASSEN_NAN_ROW
    p0, c = case["p0"], case["c"]
    info, grew, prefix = strassen_nan_row_figures()
    partners = bp.strassen_partner_rows(p0, c, case["npad"] - c)
    print(f"Strassen level, NaN row {p0}: info {info}, rows the operand sums reach {sorted(partners)}, retries + {grew}")
    assert grew == 0
    assert c < info <= p0 + 1
    assert info == min(partners) + 1
    rows = info - 1
    print(f"  prefix [0, {rows}): backward error {prefix[0]:.2e} (bar {8 * rows * EPS:.2e}), factor error {prefix[1]:.2e} (bar 1e-9)")
    assert prefix[0] <= 8 * rows * EPS
    assert prefix[1] <= 1e-9


# ---- a failed multi-panel fit leaves nothing behind ------------------------------------------------------------------------
HISTORY = {   # name: (N of the failed and the first clean fit, block, environment, constructor keywords)
    "n2900_b512_level2": (2900, 512, bp.LEVEL_TWO, {}),
    "n2900_b512_fp32": (2900, 512, {**bp.LEVEL_TWO, "GPX_STRASSEN_SINGLE": "1"}, {"dtype": "float32"}),
    "n4500_wide": (4500, 0, {"GPX_NB_WIDE_FROM": "2048"}, {}),
}
HISTORY_P0, HISTORY_SMALL = 2000, 1000


def observe(gp, N):
    X, y, Xs = synthetic_problem(N, 3, 300, seed=N)
    mean, var = gp.fit(X, y).predict(Xs)
    assert gp.info_ == 0
    npad = (N + 127) // 128 * 128
    return dict(mean=mean.copy(), var=var.copy(), alpha=gp.alpha_.copy(), logdet=gp.log_det_,
                L=device_rows(gp, factor_address(gp), npad))


@pytest.mark.parametrize("name", list(HISTORY))
def test_a_failed_multi_panel_fit_leaves_nothing_behind(name):
    """The contract of tests/test_handle_history_gpu.py::test_a_failed_call_leaves_no_trace at the sizes where the scratch
    exists: after a fit that failed at row 2000 every scratch buffer of the handle (panel buffers, block inverses, the
    second level's temporaries, the K buffer's padding and right-hand-side rows) holds NaN; the clean fit of the same size
    and a smaller one after it have the bits of a fresh handle under the same switches."""
    N, block, env, kw = HISTORY[name]
    with switches(env):
        fresh = {}
        for n in (N, HISTORY_SMALL):
            with GP("rbf", LS, SF2, SN2, jitter=0.0, block=block, **kw) as gp:
                fresh[n] = observe(gp, n)
        with GP("rbf", LS, SF2, SN2, jitter=0.0, block=block, **kw) as gp:
            X, y, _ = synthetic_problem(N, 3, 300, seed=N)
            X[HISTORY_P0, :] = np.nan
            gp.max_tries = 1
            with pytest.raises(np.linalg.LinAlgError):
                gp.fit(X, y)
            print(f"history {name}: the failed fit reports {gp.info_}")
            assert gp.info_ > 0
            if "GPX_STRASSEN_MIN" not in env:                   # (with a level on: test_a_nan_row_right_of_c_...)
                assert gp.info_ == HISTORY_P0 + 1
            gp.max_tries = 3
            for n in (N, HISTORY_SMALL):
                got = observe(gp, n)
                for q in ("mean", "var", "alpha", "L"):
                    assert np.array_equal(got[q], fresh[n][q]), f"{name}: {q} of the N = {n} fit after the failed one"
                assert got["logdet"] == fresh[n]["logdet"], f"{name}: log-det of the N = {n} fit after the failed one"


