"""The blocked row removal (tests/remove_ref.py, the mirror of csrc/gpx_update.hip) against a dense Cholesky of the
remaining rows.  CPU only.

Bars.  Both factors come from backward-stable algorithms applied to the same matrix K_rem, so they differ by about
cond(K_rem) eps relative; the matrices here (RBF + 1e-2 noise, N = 700) have cond < 1e6, hence 1e-9 on the factor.
z = L^-1 y is large where the noise is small: its bar is relative to its largest entry.  The log-determinant is a sum of
N logs: 1e-9 absolute is four orders above its rounding."""
import numpy as np
import pytest

from remove_ref import panel_q, remove_rows


def _problem(N, k=2, seed=0):
    rng = np.random.default_rng(seed)
    X = rng.uniform(-2, 2, (N, 2))
    y = np.sin(X @ rng.standard_normal((2, k)))
    d2 = ((X[:, None, :] - X[None, :, :]) ** 2).sum(-1)
    K = 1.3 * np.exp(-0.5 * d2 / 0.6 ** 2) + 1e-2 * np.eye(N)
    return K, y


def _factor(K, y):
    L = np.linalg.cholesky(K)
    return L, np.linalg.solve(L, y).T


@pytest.fixture(scope="module")
def fitted():
    K, y = _problem(700)
    return K, y, _factor(K, y)


def test_panel_q_is_orthogonal_and_annihilates_the_carry():
    rng = np.random.default_rng(1)
    Ljj = np.tril(rng.standard_normal((13, 13))) + 4 * np.eye(13)
    Wj = rng.standard_normal((13, 5))
    Q, Lp = panel_q(Ljj, Wj)
    assert np.abs(Q.T @ Q - np.eye(18)).max() < 1e-13
    S = np.hstack([Ljj, Wj]) @ Q
    assert np.abs(S[:, :13] - Lp).max() < 1e-13
    assert np.abs(S[:, 13:]).max() < 1e-13


# (start, count, panel width w, most columns per pass): nothing aligned, count > w, several chunks, head and tail
@pytest.mark.parametrize("a,m,w,width", [(130, 37, 64, 64), (0, 37, 64, 64), (130, 100, 64, 64), (5, 5, 64, 64),
                                         (663, 37, 64, 64), (130, 37, 24, 16), (311, 150, 50, 64), (1, 698, 64, 64)])
def test_blocked_removal_matches_a_refit(fitted, a, m, w, width):
    K, y, (L, zT) = fitted
    keep = np.r_[0:a, a + m:K.shape[0]]
    Lr, zr = _factor(K[np.ix_(keep, keep)], y[keep])
    L1, z1, logdet = remove_rows(L, zT, a, m, w=w, width=width)
    assert L1.shape == Lr.shape
    assert np.abs(L1 - Lr).max() < 1e-9
    assert np.abs(z1 - zr).max() < 1e-9 * max(1.0, np.abs(zr).max())
    assert abs(logdet - 2.0 * np.sum(np.log(np.diag(Lr)))) < 1e-9


def test_removing_the_tail_is_a_truncation(fitted):
    K, y, (L, zT) = fitted
    L1, z1, _ = remove_rows(L, zT, 650, 50)
    assert np.array_equal(L1, L[:650, :650])
    assert np.array_equal(z1, zT[:, :650])
