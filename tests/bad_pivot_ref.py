"""Inputs whose first failing Cholesky pivot is decided by the mathematics, not by rounding, the tables of positions the
GPU tests (tests/test_bad_pivot_gpu.py) run through every schedule, and the CPU reference for the pivot index.

Matrix level.  K = sf2 rbf(X, X) + 1e-2 I on uniform points (the matrix of tests/test_kernels_gpu.py::
test_potrf_backward_error) is positive definite, so is every leading minor of it.  With K[p0, p0] = -1 the leading minor of
order p0 is untouched and pivot p0 is -1 - |l_p0|^2 < 0 whatever the rounding: LAPACK's info is p0 + 1.  With K[p0, p0] = NaN
the pivot is NaN.  With two bad diagonals the smaller index decides.

Fit level.  The library refuses negative noise and negative weights, so no indefinite K can be passed to a fit; a row of X
that is NaN makes row and column p0 of K NaN and nothing else: no row above p0 reads it, pivot p0 is NaN.

The reference.  ``lapack_info`` is ``scipy.linalg.lapack.dpotrf`` on the matrix itself wherever its lower triangle is
finite (every case of the tables below).  Reference LAPACK tests a pivot with ``AJJ.LE.ZERO.OR.DISNAN(AJJ)``; the
OpenBLAS ``potrf`` SciPy ships tests ``ajj <= 0`` only and returns info = 0 for a NaN pivot, so for a matrix with non-finite
entries the routine applies LAPACK to the finite leading minor (rows before the first one with a non-finite entry in its
lower triangle) and LAPACK's documented test to the one pivot that follows: ``not (a_rr - |l_r|^2 > 0)``."""
import numpy as np
from scipy.linalg import solve_triangular
from scipy.linalg.lapack import dpotrf

from oracle.gp_oracle import chol_lower, kernel_matrix, synthetic_problem

EPS = np.finfo(np.float64).eps
EPS32 = float(np.finfo(np.float32).eps)
SF2, SN2, LS = 1.5, 1e-2, 0.25

# every switch a case may set: cleared before a case's own are set
SWITCHES = ("GPX_TWO_LEVEL_FROM", "GPX_STRASSEN_MIN", "GPX_STRASSEN_MIN_TWO", "GPX_STRASSEN_DIAG", "GPX_STRASSEN_SINGLE",
            "GPX_NB_WIDE_FROM", "GPX_NB_PRED", "GPX_DEFER_LEFT", "GPX_CU_SELF_RESERVE", "GPX_DIAG_STEP", "GPX_FUSED_STRIP",
            "GPX_SPLIT_STRIP", "GPX_CHAIN_FLAG", "GPX_NB_SHARD", "GPX_SHARD_REPLICATE")
# as tests/test_two_level_gpu.py, tests/test_deferred_left_gpu.py and tests/test_strassen_levels_gpu.py force the paths
SPLIT = {"GPX_TWO_LEVEL_FROM": "1024", "GPX_STRASSEN_MIN": "0"}
STRASSEN = {"GPX_TWO_LEVEL_FROM": "1024", "GPX_STRASSEN_MIN": "128"}
DIAG = {"GPX_TWO_LEVEL_FROM": "1024", "GPX_STRASSEN_MIN": "128", "GPX_STRASSEN_DIAG": "1"}
LEVEL_TWO = {**STRASSEN, "GPX_STRASSEN_MIN_TWO": "128"}

# ---- gpx_potrf -----------------------------------------------------------------------------------------------------------
# one-level, n = 1024, block 256.  0, 7, 8: the 8-column step offsets of potf2_lds; 63, 64, 127: the halves of the 128-wide
# diagonal kernel; 128, 255, 256: block and panel ends; 1023: the last row
ONE_LEVEL = {   # name: (environment, positions)
    "default": ({}, (0, 7, 8, 63, 64, 127, 128, 200, 255, 256, 1023)),
    "diag64": ({"GPX_DIAG_STEP": "64"}, (0, 63, 64, 127, 128, 256, 1023)),
    "fused": ({"GPX_FUSED_STRIP": "1"}, (127, 256, 1023)),
    "unsplit": ({"GPX_SPLIT_STRIP": "0"}, (127, 256, 1023)),
    "events": ({"GPX_CHAIN_FLAG": "0"}, (127, 256, 1023)),
    "reserve4": ({"GPX_CU_SELF_RESERVE": "4"}, (127, 256, 1023)),
}
ONE_LEVEL_N, ONE_LEVEL_BLOCK = 1024, 256
# two-level, n = 3072, block 512: c = 1536, c1 = 1024, hh = 768.  100, 1023, 1024, 1300, 1535: phase 1 on either side of c1;
# 1536: the right block's first row; 1605: the second half of a 128 block there; 2303, 2304: the Strassen half boundary
# c + hh; 3071: the last row
TWO_LEVEL = {
    "split": SPLIT,
    "strassen": STRASSEN,
    "diag": DIAG,
    "strassen_defer0": {**STRASSEN, "GPX_DEFER_LEFT": "0"},
    "strassen_defer1": {**STRASSEN, "GPX_DEFER_LEFT": "1"},
    "split_defer1": {**SPLIT, "GPX_DEFER_LEFT": "1"},
    "strassen_level2": LEVEL_TWO,
}
TWO_LEVEL_N, TWO_LEVEL_BLOCK = 3072, 512
TWO_LEVEL_P0 = (100, 1023, 1024, 1300, 1535, 1536, 1605, 2303, 2304, 3071)
# wide panels: panel ends and the last row
WIDE_N, WIDE_BLOCK, WIDE_P0 = 4608, 2048, (2047, 2048, 4607)
NAN = float("nan")


def potrf_cases():
    """-> [(id, environment, n, block, ((index, value on the diagonal), ...))]: the table, then the NaN diagonals and the
    pairs of bad pivots"""
    cases = []
    for name, (env, positions) in ONE_LEVEL.items():
        cases += [(f"one_level_{name}-{p0}", env, ONE_LEVEL_N, ONE_LEVEL_BLOCK, ((p0, -1.0),)) for p0 in positions]
    for name, env in TWO_LEVEL.items():
        cases += [(f"two_level_{name}-{p0}", env, TWO_LEVEL_N, TWO_LEVEL_BLOCK, ((p0, -1.0),)) for p0 in TWO_LEVEL_P0]
    cases += [(f"wide-{p0}", {}, WIDE_N, WIDE_BLOCK, ((p0, -1.0),)) for p0 in WIDE_P0]
    cases += [("nan_one_level-200", {}, ONE_LEVEL_N, ONE_LEVEL_BLOCK, ((200, NAN),)),
              ("nan_strassen-1605", STRASSEN, TWO_LEVEL_N, TWO_LEVEL_BLOCK, ((1605, NAN),)),
              ("pair_one_level-130-700", {}, ONE_LEVEL_N, ONE_LEVEL_BLOCK, ((130, -1.0), (700, -1.0))),
              ("pair_strassen-900-2000", STRASSEN, TWO_LEVEL_N, TWO_LEVEL_BLOCK, ((900, -1.0), (2000, -1.0))),
              ("pair_strassen-1600-2400", STRASSEN, TWO_LEVEL_N, TWO_LEVEL_BLOCK, ((1600, -1.0), (2400, -1.0)))]
    return cases


def first_bad(bad):
    return min(i for i, _ in bad)


_SPD, _FACTOR = {}, {}


def spd(n):
    """the positive definite matrix, once per n (read-only)"""
    if n not in _SPD:
        rng = np.random.default_rng(n)
        Xp = rng.uniform(size=(n, 3))
        K = kernel_matrix(Xp, Xp, "rbf", LS, SF2)
        K[np.diag_indices(n)] += SN2
        K.setflags(write=False)
        _SPD[n] = K
    return _SPD[n]


def spd_factor(n):
    """LAPACK's factor of spd(n), once per n (read-only).  Row i of a Cholesky factor depends on the leading minor of order
    i + 1 only, so its leading p0 x p0 block is the factor of spd(n)[:p0, :p0]: the prefix reference of every position."""
    if n not in _FACTOR:
        L = chol_lower(spd(n))
        L.setflags(write=False)
        _FACTOR[n] = L
    return _FACTOR[n]


def indefinite(n, bad):
    K = np.array(spd(n))
    for i, v in bad:
        K[i, i] = v
    return K


def lapack_info(K):
    """info of LAPACK's dpotrf(lower) on K; only the lower triangle is read (see the module docstring for non-finite K)"""
    K = np.asarray(K, dtype=np.float64)
    n = K.shape[0]
    rows = np.flatnonzero(~np.all(np.isfinite(np.tril(K)), axis=1))
    r = int(rows[0]) if rows.size else n
    L, info = dpotrf(K[:r, :r], lower=1) if r else (np.zeros((0, 0)), 0)
    if info != 0 or r == n:
        return int(info)
    l = solve_triangular(L, K[r, :r], lower=True, check_finite=False) if r else np.zeros(0)
    pivot = K[r, r] - l @ l
    assert not pivot > 0, "a non-finite row whose pivot is positive"
    return r + 1


def prefix_errors(L, K, ref, p0):
    """rows and columns [0, p0) of a factor L against the matrix K and LAPACK's factor `ref` of it: the measures of
    tests/test_kernels_gpu.py::test_potrf_backward_error -> (|L L^T - K| / |K| in the Frobenius norm, max |L - ref| / max |ref|)"""
    Lp, Kp, Rp = np.tril(np.asarray(L[:p0, :p0], dtype=np.float64)), K[:p0, :p0], ref[:p0, :p0]
    return (float(np.linalg.norm(Lp @ Lp.T - Kp) / np.linalg.norm(Kp)),
            float(np.max(np.abs(Lp - Rp)) / np.max(np.abs(Rp))))


# ---- fits with one NaN input row ---------------------------------------------------------------------------------------
# name: dict(N, p0, block, constructor keywords, environment, variant, exact).  variant: the Gram build of the fit ("plain",
# "weights", "kinds", "paths"); what = "info" where the factor cannot be read back (gpx_factor_info refuses GPX_MIXED handles
# and device groups)
def _fit(N, p0, block=256, env=None, kw=None, variant="plain", read=True):
    return dict(N=N, p0=p0, block=block, env=env or {}, kw=kw or {}, variant=variant, read=read)


FIT_CASES = {
    **{f"n1000_{dt}-{p0}": _fit(1000, p0, kw={"dtype": dt}, read=dt != "mixed")
       for dt in ("float64", "float32", "mixed") for p0 in (0, 300, 999)},
    "n970-969": _fit(970, 969),
    **{f"n300_{v}-150": _fit(300, 150, variant=v) for v in ("plain", "weights", "kinds", "paths")},
    **{f"n1000_shard_repl{r}-700": _fit(1000, 700, block=0, env={"GPX_NB_SHARD": "128", "GPX_SHARD_REPLICATE": str(r)},
                                        kw={"devices": 2, "oversubscribe": True}, read=False) for r in (0, 1)},
    **{f"n4500_split-{p0}": _fit(4500, p0, block=0, env=SPLIT) for p0 in (1000, 3000)},
    **{f"n2900_b512_strassen-{p0}": _fit(2900, p0, block=512, env=STRASSEN) for p0 in (500, 1300)},
}
FIT_PREDICT = dict(N=2048, M=100, p0=1500)
# the one case that is not an equality: a NaN row right of c under a Strassen level
STRASSEN_NAN_ROW = dict(N=2900, block=512, p0=2500, npad=2944, c=1536, c1=1024)
KINDS_VALUES = 150     # the "kinds" variant: 150 value rows, then 150 derivative rows: row 150 is the first derivative row
PATH_SG2, PATH_LS = 0.4, 0.5


def strassen_partner_rows(p0, c, rows):
    """Rows of A21 that a NaN row p0 >= c of it reaches through the operand sums of the deferred product's one Strassen
    level (strassen_nt on all `rows` 128-tile rows of A21 as one chunk: m0 = rows / 256 * 256, halves of mh = m0 / 2):
    M1 = (A1 + A4)(B1 + B4)^T lands in C11 and C22, so row r of either half is NaN in both.  The deep update's level works on
    rows [c + hh, n) against [c, c + hh): its sums move a NaN between rows of the lower half only — all of them below the
    partner found here — or between columns."""
    r = p0 - c
    mh = rows // 256 * 256 // 2
    if r >= 2 * mh:
        return {p0}                                     # a peeled row: classical
    return {c + r % mh, c + r % mh + mh}


def fit_problem(N, variant="plain"):
    """the clean problem of a fit case -> dict(X, y, fit keywords, K(rows) -> the reference Gram matrix of X[:rows])"""
    X, y, _ = synthetic_problem(N, 3, 1, seed=N)
    if variant == "plain":
        return dict(X=X, y=y, fit={}, gram=lambda Xr: _gram(Xr))
    if variant == "weights":
        w = np.random.default_rng(N + 1).uniform(0.5, 2.0, N)
        return dict(X=X, y=y, fit={"noise_weights": w}, gram=lambda Xr: _gram(Xr, SN2 * w[:len(Xr)]))
    if variant == "kinds":
        nv = KINDS_VALUES
        rng = np.random.default_rng(N + 2)
        return dict(X=X[:nv], y=y[:nv], gram=lambda Xr: _gram(Xr),
                    fit={"derivatives": (X[nv:], rng.integers(0, 3, N - nv), rng.standard_normal(N - nv)),
                         "derivative_noise": 1e-2})
    if variant == "paths":
        from within_ref import path_cov
        ids = (np.arange(N) % 7).astype(np.int32)

        def gram(Xr):
            n = len(Xr)
            return path_cov(Xr, ids[:n], Xr, ids[:n], "rbf", LS, SF2, PATH_LS, PATH_SG2) + SN2 * np.eye(n)
        return dict(X=X, y=y, fit={"path_ids": ids, "path_variance": PATH_SG2, "path_lengthscale": PATH_LS}, gram=gram)
    raise ValueError(variant)


def _gram(Xr, noise=SN2):
    K = kernel_matrix(Xr, Xr, "rbf", LS, SF2)
    K[np.diag_indices(len(Xr))] += noise
    return K


def with_nan_row(prob, p0):
    """the problem with input row p0 (counted over value rows, then derivative rows) set to NaN -> (X, fit keywords)"""
    X, fit = np.array(prob["X"]), dict(prob["fit"])
    if p0 < len(X):
        X[p0, :] = np.nan
    else:
        Xd, dims, yd = fit["derivatives"]
        Xd = np.array(Xd)
        Xd[p0 - len(X), :] = np.nan
        fit["derivatives"] = (Xd, dims, yd)
    return X, fit
