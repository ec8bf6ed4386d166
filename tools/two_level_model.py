"""CPU model of the two-level Cholesky with a Strassen level in its deep update, in float64.

The accuracy side of the schedule before any kernel: the bench's problem (oracle.gp_oracle.synthetic_problem, RBF,
lengthscale 0.25, sf2 1.5, sn2 1e-2) at N = 4096 and 8192, factorised

  blocked      right-looking in panels of nb (what the library's one-level schedule computes, up to summation order),
  two_level    split at the panel boundary c nearest N / 2: left block column, ONE update A22 -= L21 L21^T, right block,
  strassen     the same with one Strassen level on the off-diagonal block of that update,
  strassen2    and on the off-diagonal blocks of its two diagonal halves as well,
  deferred     strassen, and in the left block column the panels left of c1 (the panel boundary nearest c / 2) leave
               A21[:, c1:c] alone: ONE product A21[:, c1:c] -= L21[:, :c1] L11[c1:c, :c1]^T behind them (GPX_DEFER_LEFT),
  deferred_strassen   the same with that product through a Strassen level (in two row halves, as at N = 65536),
  strassen_l2, deferred_strassen_l2   strassen / deferred_strassen with a second level in each of the seven products of
               every Strassen level (GPX_STRASSEN_MIN_TWO),

each followed by z = L^-1 y, alpha = L^-T z, mean = K* alpha, var = k** - |L^-1 K*^T|^2 and log det.  Errors are those of
tests/test_full_size_gpu.py against OracleGP (LAPACK): mean and variance elementwise relative (floors 1e-6, 1e-6 sf2),
alpha over its largest entry, log-det relative.  Writes profiles/two_level_model.json.

    python tools/two_level_model.py [--out profiles/two_level_model.json]
"""
import argparse
import json
import os
import sys

import numpy as np
from scipy.linalg import cholesky, solve_triangular

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle.gp_oracle import OracleGP, kernel_matrix, synthetic_problem  # noqa: E402

KERNEL, LS, SF2, SN2 = "rbf", 0.25, 1.5, 1e-2


def strassen_nt(C, A, B, levels=1, targets=None):
    """C -= A B^T with `levels` Strassen levels (dimensions multiples of 2^levels); the products and targets of
    csrc/gpx_blas.hip.  targets: [(C, s), ...] instead of C — every one takes s * A B^T (the second level: the sums of a
    product of the first land in its targets' quadrants, in the order M1 .. M7, nothing in between is rounded twice)"""
    if targets is None:
        targets = [(C, -1.0)]
    m, n, k = A.shape[0] // 2, B.shape[0] // 2, A.shape[1] // 2
    A1, A2, A3, A4 = A[:m, :k], A[:m, k:], A[m:, :k], A[m:, k:]
    B1, B2, B3, B4 = B[:n, :k], B[:n, k:], B[n:, :k], B[n:, k:]
    q11, q12, q21, q22 = (np.s_[:m, :n], np.s_[:m, n:], np.s_[m:, :n], np.s_[m:, n:])

    def product(X, Y, *where):  # where: (quadrant, sign of the product in A B^T)
        tg = [(T[q], s * t) for T, s in targets for q, t in where]
        if levels > 1:
            strassen_nt(None, X, Y, levels - 1, tg)
        else:
            M = X @ Y.T
            for Tq, st in tg:
                Tq += st * M
    product(A1 + A4, B1 + B4, (q11, 1.0), (q22, 1.0))
    product(A3 + A4, B1, (q21, 1.0), (q22, -1.0))
    product(A1, B3 - B4, (q12, 1.0), (q22, 1.0))
    product(A4, B2 - B1, (q11, 1.0), (q21, 1.0))
    product(A1 + A2, B4, (q11, -1.0), (q12, 1.0))
    product(A3 - A1, B1 + B3, (q22, 1.0))
    product(A2 - A4, B2 + B4, (q11, 1.0))


def chol_blocked(A, nb, rows_below=0, defer=None, slevels=1):
    """right-looking, in place: the leading n x n block of A (n = A.shape[0] - rows_below) is factorised, the rows below it
    ride along as bordered rows (solved and updated, never factorised).  defer = "classical" / "strassen": the deferred
    product of the bordered rows' columns [c1, n)"""
    n = A.shape[0] - rows_below
    c1 = min(max(1, (n // 2 + nb // 2) // nb) * nb, n - nb) if defer else 0
    for o in range(0, n, nb):
        e = min(o + nb, n)
        A[o:e, o:e] = cholesky(A[o:e, o:e], lower=True)
        if e < A.shape[0]:
            A[e:, o:e] = solve_triangular(A[o:e, o:e], A[e:, o:e].T, lower=True).T
            if e < n and o < c1:
                A[e:n, e:n] -= A[e:n, o:e] @ A[e:n, o:e].T
                A[n:, e:c1] -= A[n:, o:e] @ A[e:c1, o:e].T
                if e == c1 and defer == "classical":
                    A[n:, c1:n] -= A[n:, :c1] @ A[c1:n, :c1].T
                elif e == c1:
                    h = rows_below // 2
                    strassen_nt(A[n:n + h, c1:n], A[n:n + h, :c1], A[c1:n, :c1], slevels)
                    strassen_nt(A[n + h:, c1:n], A[n + h:, :c1], A[c1:n, :c1], slevels)
            elif e < n:
                A[e:, e:n] -= A[e:, o:e] @ A[e:n, o:e].T
    return A


def deep_update(A22, L21, levels, slevels=1):
    """A22 -= L21 L21^T (lower triangle); `levels` levels of splitting, the off-diagonal blocks through strassen_nt with
    `slevels` Strassen levels"""
    n = A22.shape[0]
    if levels <= 0 or n < 4:
        A22 -= L21 @ L21.T
        return
    h = n // 2
    deep_update(A22[:h, :h], L21[:h], levels - 1, slevels)
    strassen_nt(A22[h:, :h], L21[h:], L21[:h], slevels)
    deep_update(A22[h:, h:], L21[h:], levels - 1, slevels)


def chol_two_level(K, nb, levels, defer=None, slevels=1):
    n = K.shape[0]
    c = max(1, (n // 2 + nb // 2) // nb) * nb
    A = K.copy()
    chol_blocked(A[:, :c], nb, rows_below=n - c, defer=defer, slevels=slevels)  # L11, L21 (A21 rides as bordered rows)
    deep_update(A[c:, c:], A[c:, :c], levels, slevels)
    chol_blocked(A[c:, c:], nb)
    return A


def outputs(L, y, Ks, kss):
    z = solve_triangular(L, y, lower=True)
    alpha = solve_triangular(L, z, lower=True, trans="T")
    V = solve_triangular(L, Ks.T, lower=True)
    return dict(mean=Ks @ alpha, var=kss - np.sum(V * V, axis=0), alpha=alpha, logdet=2.0 * np.sum(np.log(np.diag(L))))


def errors(o, r):
    return dict(mean=float(np.max(np.abs(o["mean"] - r["mean"]) / np.maximum(np.abs(r["mean"]), 1e-6))),
                var=float(np.max(np.abs(o["var"] - r["var"]) / np.maximum(r["var"], 1e-6 * SF2))),
                alpha=float(np.max(np.abs(o["alpha"] - r["alpha"])) / np.max(np.abs(r["alpha"]))),
                logdet=float(abs(o["logdet"] - r["logdet"]) / abs(r["logdet"])))


def run(N, M, nb):
    X, y, Xs = synthetic_problem(N, 3, M)
    og = OracleGP(KERNEL, LS, SF2, SN2, jitter=0.0).fit(X, y)
    mean, var = og.predict(Xs)
    ref = dict(mean=mean, var=var, alpha=og.alpha_, logdet=og.log_det_)
    K = kernel_matrix(X, X, KERNEL, LS, SF2)
    K[np.diag_indices(N)] += SN2
    Ks = kernel_matrix(Xs, X, KERNEL, LS, SF2)
    kss = np.full(M, SF2)
    row = {"N": N, "M": M, "nb": nb}
    for name, L in (("blocked", chol_blocked(K.copy(), nb)), ("two_level", chol_two_level(K, nb, 0)),
                    ("strassen", chol_two_level(K, nb, 1)), ("strassen2", chol_two_level(K, nb, 2)),
                    ("deferred", chol_two_level(K, nb, 1, "classical")),
                    ("deferred_strassen", chol_two_level(K, nb, 1, "strassen")),
                    ("strassen_l2", chol_two_level(K, nb, 1, slevels=2)),
                    ("deferred_strassen_l2", chol_two_level(K, nb, 1, "strassen", slevels=2))):
        row[name] = errors(outputs(np.tril(L), y, Ks, kss), ref)
    worst = max(row[s][q] / max(row["blocked"][q], 1e-17)
                for s in ("strassen", "strassen2", "deferred", "deferred_strassen", "strassen_l2", "deferred_strassen_l2")
                for q in row["blocked"])
    row["worst_ratio_to_blocked"] = worst
    return row


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "two_level_model.json"))
    ap.add_argument("--sizes", type=int, nargs="*", default=[4096, 8192])
    args = ap.parse_args()
    rows = [run(N, 512, 1024) for N in args.sizes]
    res = {"what": "tools/two_level_model.py: errors against OracleGP (fp64, NumPy), bench hyper-parameters",
           "bars_at_full_size": {"mean": 1e-6, "var": 1e-6, "alpha": 1e-8, "logdet": 1e-12},
           "rows": rows,
           "go": bool(all(r["worst_ratio_to_blocked"] < 100 for r in rows))}
    print(json.dumps(res, indent=1))
    json.dump(res, open(args.out, "w"), indent=1)
