"""CPU: the inputs of tests/test_bad_pivot_gpu.py have the failing pivot the tables say, by LAPACK (tests/bad_pivot_ref.py),
and the tables still hold every position that reaches an index path of its own."""
import numpy as np
import pytest
from scipy.linalg.lapack import dpotrf

import bad_pivot_ref as bp


def test_the_tables_hold_every_position():
    one = {name: positions for name, (_, positions) in bp.ONE_LEVEL.items()}
    assert one == {"default": (0, 7, 8, 63, 64, 127, 128, 200, 255, 256, 1023), "diag64": (0, 63, 64, 127, 128, 256, 1023),
                   "fused": (127, 256, 1023), "unsplit": (127, 256, 1023), "events": (127, 256, 1023),
                   "reserve4": (127, 256, 1023)}
    env = {name: e for name, (e, _) in bp.ONE_LEVEL.items()}
    assert env == {"default": {}, "diag64": {"GPX_DIAG_STEP": "64"}, "fused": {"GPX_FUSED_STRIP": "1"},
                   "unsplit": {"GPX_SPLIT_STRIP": "0"}, "events": {"GPX_CHAIN_FLAG": "0"},
                   "reserve4": {"GPX_CU_SELF_RESERVE": "4"}}
    assert (bp.ONE_LEVEL_N, bp.ONE_LEVEL_BLOCK) == (1024, 256)
    two, on = {"GPX_TWO_LEVEL_FROM": "1024"}, {"GPX_STRASSEN_MIN": "128"}
    assert bp.TWO_LEVEL == {
        "split": {**two, "GPX_STRASSEN_MIN": "0"}, "strassen": {**two, **on}, "diag": {**two, **on, "GPX_STRASSEN_DIAG": "1"},
        "strassen_defer0": {**two, **on, "GPX_DEFER_LEFT": "0"}, "strassen_defer1": {**two, **on, "GPX_DEFER_LEFT": "1"},
        "split_defer1": {**two, "GPX_STRASSEN_MIN": "0", "GPX_DEFER_LEFT": "1"},
        "strassen_level2": {**two, **on, "GPX_STRASSEN_MIN_TWO": "128"}}
    assert (bp.TWO_LEVEL_N, bp.TWO_LEVEL_BLOCK) == (3072, 512)
    assert bp.TWO_LEVEL_P0 == (100, 1023, 1024, 1300, 1535, 1536, 1605, 2303, 2304, 3071)
    assert (bp.WIDE_N, bp.WIDE_BLOCK, bp.WIDE_P0) == (4608, 2048, (2047, 2048, 4607))
    cases = bp.potrf_cases()
    assert len(cases) == 11 + 7 + 4 * 3 + 7 * 10 + 3 + 5 and len({c[0] for c in cases}) == len(cases)
    extra = {c[0]: (c[1], c[2], c[3], tuple(i for i, _ in c[4]), tuple(np.isnan(v) for _, v in c[4])) for c in cases[-5:]}
    assert extra == {"nan_one_level-200": ({}, 1024, 256, (200,), (True,)),
                     "nan_strassen-1605": (bp.STRASSEN, 3072, 512, (1605,), (True,)),
                     "pair_one_level-130-700": ({}, 1024, 256, (130, 700), (False, False)),
                     "pair_strassen-900-2000": (bp.STRASSEN, 3072, 512, (900, 2000), (False, False)),
                     "pair_strassen-1600-2400": (bp.STRASSEN, 3072, 512, (1600, 2400), (False, False))}
    assert all(set(c[1]) <= set(bp.SWITCHES) for c in cases)
    fits = {name: (c["N"], c["p0"], c["block"], c["variant"]) for name, c in bp.FIT_CASES.items()}
    want = {f"n1000_{dt}-{p0}": (1000, p0, 256, "plain") for dt in ("float64", "float32", "mixed") for p0 in (0, 300, 999)}
    want.update({"n970-969": (970, 969, 256, "plain"), "n300_plain-150": (300, 150, 256, "plain"),
                 "n300_weights-150": (300, 150, 256, "weights"), "n300_kinds-150": (300, 150, 256, "kinds"),
                 "n300_paths-150": (300, 150, 256, "paths"), "n1000_shard_repl0-700": (1000, 700, 0, "plain"),
                 "n1000_shard_repl1-700": (1000, 700, 0, "plain"), "n4500_split-1000": (4500, 1000, 0, "plain"),
                 "n4500_split-3000": (4500, 3000, 0, "plain"), "n2900_b512_strassen-500": (2900, 500, 512, "plain"),
                 "n2900_b512_strassen-1300": (2900, 1300, 512, "plain")})
    assert fits == want
    assert all(set(c["env"]) <= set(bp.SWITCHES) for c in bp.FIT_CASES.values())
    assert bp.FIT_CASES["n4500_split-3000"]["env"] == bp.SPLIT and bp.FIT_CASES["n2900_b512_strassen-500"]["env"] == bp.STRASSEN
    assert bp.FIT_CASES["n1000_shard_repl1-700"]["env"] == {"GPX_NB_SHARD": "128", "GPX_SHARD_REPLICATE": "1"}
    assert bp.FIT_PREDICT == dict(N=2048, M=100, p0=1500)
    assert (bp.STRASSEN_NAN_ROW["N"], bp.STRASSEN_NAN_ROW["block"], bp.STRASSEN_NAN_ROW["p0"]) == (2900, 512, 2500)
    assert bp.KINDS_VALUES == 150                                    # row 150 of the "kinds" variant is a derivative row


_DISTINCT = sorted({(n, bad) for _, _, n, _, bad in bp.potrf_cases()}, key=lambda c: (c[0], [i for i, _ in c[1]], str(c[1])))


@pytest.mark.parametrize("n, bad", _DISTINCT, ids=[f"n{n}-" + "-".join(str(i) for i, _ in bad) + ("nan" if np.isnan(bad[0][1]) else "")
                                                  for n, bad in _DISTINCT])
def test_lapack_reports_the_tabled_pivot(n, bad):
    K = bp.indefinite(n, bad)
    want = bp.first_bad(bad) + 1
    assert bp.lapack_info(K) == want
    if np.all(np.isfinite(K)):
        assert dpotrf(K, lower=1)[1] == want                        # (the same call: lapack_info adds nothing for a finite matrix)


def test_the_positive_definite_matrix_is_positive_definite():
    for n in (bp.ONE_LEVEL_N, bp.TWO_LEVEL_N):
        assert bp.lapack_info(bp.spd(n)) == 0
        L = bp.spd_factor(n)
        # the leading block of the factor is the factor of the leading minor: the prefix reference
        for p0 in (200, n // 2):
            Lp = np.linalg.cholesky(bp.spd(n)[:p0, :p0])
            assert np.max(np.abs(Lp - L[:p0, :p0])) <= 1e-11 * np.max(np.abs(Lp))


def test_lapack_info_on_non_finite_input_is_the_documented_test():
    """against the unblocked algorithm with LAPACK's pivot test (dpotf2: AJJ.LE.ZERO.OR.DISNAN(AJJ)) written out"""
    def potf2(K):
        n = len(K)
        L = np.zeros_like(K)
        for j in range(n):
            ajj = K[j, j] - L[j, :j] @ L[j, :j]
            if ajj <= 0 or np.isnan(ajj):
                return j + 1
            L[j, j] = np.sqrt(ajj)
            L[j + 1:, j] = (K[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
        return 0
    K = np.array(bp.spd(bp.ONE_LEVEL_N)[:96, :96])
    assert potf2(K) == bp.lapack_info(K) == 0
    for p0, q0 in ((0, None), (40, None), (95, None), (70, 30)):
        A = K.copy()
        A[p0, :] = A[:, p0] = np.nan
        if q0 is not None:
            A[q0, q0] = -1.0
        assert potf2(A) == bp.lapack_info(A) == min(p0, p0 if q0 is None else q0) + 1
        A = K.copy()
        A[p0, p0] = np.nan
        assert potf2(A) == bp.lapack_info(A) == p0 + 1


@pytest.mark.parametrize("name", list(bp.FIT_CASES))
def test_a_nan_input_row_is_the_first_failing_pivot(name):
    """K of the fit with the NaN row: rows [0, p0) are those of the clean problem, row and column p0 are NaN"""
    case = bp.FIT_CASES[name]
    N, p0 = case["N"], case["p0"]
    prob = bp.fit_problem(N, case["variant"])
    Xn, fit = bp.with_nan_row(prob, p0)
    rows = np.concatenate([Xn, fit["derivatives"][0]]) if case["variant"] == "kinds" else Xn
    assert rows.shape == (N, 3)
    bad = np.flatnonzero(~np.all(np.isfinite(rows), axis=1))
    assert list(bad) == [p0]
    K = np.full((p0 + 1, p0 + 1), np.nan)
    if case["variant"] == "plain":
        K = bp._gram(rows[:p0 + 1])                                 # the NaN row goes through the kernel itself
        assert np.all(np.isnan(K[p0, :])) and np.all(np.isnan(K[:, p0]))
    else:
        K[:p0, :p0] = prob["gram"](rows[:p0])
    assert np.all(np.isfinite(K[:p0, :p0]))
    assert bp.lapack_info(K) == p0 + 1


def test_partner_rows_of_the_strassen_case():
    c = bp.STRASSEN_NAN_ROW
    rows = c["npad"] - c["c"]
    assert rows == 1408
    # m0 = 1280, halves of 640: row 2500 - 1536 = 964 of A21 lies in the lower half, its partner is row 324
    assert bp.strassen_partner_rows(c["p0"], c["c"], rows) == {1860, 2500}
    assert bp.strassen_partner_rows(1536 + 1300, 1536, rows) == {1536 + 1300}       # a peeled row has no partner
    assert bp.strassen_partner_rows(1536 + 5, 1536, rows) == {1541, 2181}
