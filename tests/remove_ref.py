"""NumPy mirror of the blocked row removal (csrc/gpx_update.hip, include/gpx.h: gpx_remove_rows).

Taking rows [a, b) out of the data leaves L11 and L31 of the factor as they are; the trailing block takes the positive
update L33' L33'^T = L33 L33^T + L32 L32^T, done in column panels of width w with the carry W = L32, and the bordered
rows z^T = (L^-1 y)^T ride through the same orthogonal transformations.  The functions here follow the library step by
step (panel Q, strip product, chunks of at most ``width`` removed columns from the highest rows down) in float64.
"""
import numpy as np


def panel_q(Ljj, Wj):
    """Q ((w + m) square, orthogonal) of one panel and the new diagonal block: [Ljj | Wj] Q = [Ljj' | 0]."""
    w, m = Wj.shape
    Lp = np.linalg.cholesky(Ljj @ Ljj.T + Wj @ Wj.T)
    V = np.linalg.solve(Ljj, Wj)
    C = np.linalg.cholesky(np.eye(m) + V.T @ V)
    LpinvT = np.linalg.inv(Lp).T
    CinvT = np.linalg.inv(C).T
    Q = np.block([[Ljj.T @ LpinvT, -V @ CinvT], [Wj.T @ LpinvT, CinvT]])
    return Q, Lp


def remove_pass(L, zT, a, m, w):
    """One pass: rows [a, a + m) out of the factor L (N x N, lower) and the bordered rows zT (k x N)."""
    N = L.shape[0]
    b = a + m
    n3 = N - b
    Lnew = np.zeros((N - m, N - m))
    znew = np.zeros((zT.shape[0], N - m))
    Lnew[:a, :a] = L[:a, :a]
    znew[:, :a] = zT[:, :a]
    if n3 == 0:
        return Lnew, znew
    Lnew[a:, :a] = L[b:, :a]
    W = L[b:, a:b].copy()
    z2 = zT[:, a:b].copy()
    L33 = np.tril(L[b:, b:])
    z3 = zT[:, b:]
    for j0 in range(0, n3, w):
        j1 = min(j0 + w, n3)
        Q, _ = panel_q(L33[j0:j1, j0:j1], W[j0:j1])
        wj = j1 - j0
        S = np.hstack([L33[j0:, j0:j1], W[j0:]]) @ Q
        Lnew[a + j0:, a + j0:a + j1] = S[:, :wj]
        W[j0:] = S[:, wj:]
        zS = np.hstack([z3[:, j0:j1], z2]) @ Q
        znew[:, a + j0:a + j1] = zS[:, :wj]
        z2 = zS[:, wj:]
    return np.tril(Lnew), znew


def remove_rows(L, zT, start, count, w=64, width=64):
    """Rows [start, start + count) out of (L, zT), in chunks of at most ``width`` columns from the highest rows down.
    Returns the new factor, the new bordered rows and the log-determinant 2 sum log diag."""
    hi = start + count
    while hi > start:
        lo = max(start, hi - width)
        L, zT = remove_pass(L, zT, lo, hi - lo, w)
        hi = lo
    return L, zT, 2.0 * np.sum(np.log(np.diag(L)))
