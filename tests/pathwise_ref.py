"""NumPy reference of the pathwise posterior sampler (``gpx_pathwise_draw`` / ``gpx_pathwise_eval``; include/gpx.h):
the layout of its normals on the Philox stream of ``philox_ref``, frequencies and features, a dense draw and evaluation,
and the exact covariance of the sampler for a given set of frequencies."""
import numpy as np

import philox_ref

CHI_DOF = {"rbf": 0, "matern52": 5, "matern32": 3, "matern12": 1}   # q = 2 nu (0: Gaussian frequencies)
SQRT5, SQRT3 = 5.0 ** 0.5, 3.0 ** 0.5


def n_normals(kernel, F, d, C, N):
    return F * (d + CHI_DOF[kernel]) + C * (2 * F + N)


def normals(seed, kernel, F, d, C, N):
    """the flat stream a call with z = NULL draws: number i is normal number i of the Philox stream `seed`"""
    return philox_ref.normals(seed, np.arange(n_normals(kernel, F, d, C, N), dtype=np.uint64))


def split(z, kernel, F, d, C, N):
    """flat stream -> g (F, d), chi normals (F, q), W (C, 2F), E (C, N)"""
    q = CHI_DOF[kernel]
    z = np.asarray(z, dtype=np.float64).ravel()
    assert z.size == n_normals(kernel, F, d, C, N)
    head = z[:F * (d + q)].reshape(F, d + q)
    cols = z[F * (d + q):].reshape(C, 2 * F + N)
    return head[:, :d], head[:, d:], cols[:, :2 * F], cols[:, 2 * F:]


def frequencies(g, chin):
    """Omega (F, d) = g sqrt(q / chi), chi the sum of squares of the q chi normals in order; q = 0: g"""
    q = chin.shape[1]
    if q == 0:
        return g.copy()
    chi = np.zeros(len(g))
    for j in range(q):
        chi = chi + chin[:, j] * chin[:, j]
    with np.errstate(divide="ignore", invalid="ignore"):                # chi = 0 (an all-zero z): frequency 0
        return np.where(chi[:, None] > 0, g * np.sqrt(q / chi)[:, None], 0.0)


def scaled(X, ls):
    X = np.asarray(X, dtype=np.float64)
    X = X.reshape(-1, 1) if X.ndim == 1 else X
    return X / np.broadcast_to(np.asarray(ls, dtype=np.float64), (X.shape[1],))


def phases(U, Omega):
    """theta (M, F), summed over the dimensions in order"""
    th = np.zeros((len(U), len(Omega)))
    for j in range(U.shape[1]):
        th = th + U[:, j:j + 1] * Omega[None, :, j]
    return th


def features(X, ls, Omega, sf2):
    """Phi (M, 2F) = sqrt(sf2 / F) [cos theta | sin theta]"""
    th = phases(scaled(X, ls), Omega)
    return np.sqrt(sf2 / len(Omega)) * np.concatenate([np.cos(th), np.sin(th)], axis=1)


def kernel_matrix(kernel, A, B, ls, sf2):
    """sf2 k(A, B) in the operation order of csrc/gpx_cov.h"""
    Ua, Ub = scaled(A, ls), scaled(B, ls)
    r2 = np.zeros((len(Ua), len(Ub)))
    for j in range(Ua.shape[1]):
        df = Ua[:, j:j + 1] - Ub[None, :, j]
        r2 = r2 + df * df
    if kernel == "rbf":
        return sf2 * np.exp(-0.5 * r2)
    s = {"matern52": SQRT5, "matern32": SQRT3, "matern12": 1.0}[kernel] * np.sqrt(r2)
    poly = {"matern52": 1.0 + s + s * s / 3.0, "matern32": 1.0 + s, "matern12": 1.0}[kernel]
    return sf2 * (poly * np.exp(-s))


def k_y(kernel, X, ls, sf2, noise, w=None, jitter=0.0):
    n = len(X)
    w = np.ones(n) if w is None else np.asarray(w, dtype=np.float64)
    return kernel_matrix(kernel, X, X, ls, sf2) + np.diag(noise * w + jitter)


def draw(kernel, X, y, ls, sf2, noise, z, S, F, w=None, jitter=0.0):
    """the dense draw: Omega (F, d), W (C, 2F), V (C, N) = R K_y^-1 of include/gpx.h, from the flat stream z"""
    X = scaled(X, 1.0)
    y = np.asarray(y, dtype=np.float64).reshape(len(X), -1)
    N, d, k = len(X), X.shape[1], y.shape[1]
    C = S * k
    g, chin, W, E = split(z, kernel, F, d, C, N)
    Omega = frequencies(g, chin)
    wn = np.ones(N) if w is None else np.asarray(w, dtype=np.float64)
    prior = W @ features(X, ls, Omega, sf2).T                                   # (C, N)
    R = np.tile(y.T, (S, 1)) - prior - np.sqrt(noise * wn)[None, :] * E          # row col = s k + c
    V = np.linalg.solve(k_y(kernel, X, ls, sf2, noise, w, jitter), R.T).T
    return {"kernel": kernel, "X": X, "ls": ls, "sf2": sf2, "k": k, "S": S, "Omega": Omega, "W": W, "V": V}


def evaluate_columns(kernel, Xq, X, ls, sf2, Omega, W, V):
    """out (C, M) = W Phi(Xq)^T + V K(Xq, X)^T"""
    return W @ features(Xq, ls, Omega, sf2).T + V @ kernel_matrix(kernel, Xq, X, ls, sf2).T


def evaluate(dr, Xq):
    """the drawn functions at Xq: (S, M, k)"""
    out = evaluate_columns(dr["kernel"], Xq, dr["X"], dr["ls"], dr["sf2"], dr["Omega"], dr["W"], dr["V"])
    return np.ascontiguousarray(out.reshape(dr["S"], dr["k"], -1).transpose(0, 2, 1))


def posterior(kernel, X, y, Xq, ls, sf2, noise, w=None, jitter=0.0):
    """exact posterior mean (M, k) and latent covariance (M, M)"""
    Ky = k_y(kernel, X, ls, sf2, noise, w, jitter)
    Ks = kernel_matrix(kernel, Xq, X, ls, sf2)
    A = np.linalg.solve(Ky, Ks.T).T
    y = np.asarray(y, dtype=np.float64).reshape(len(Ky), -1)
    return A @ y, kernel_matrix(kernel, Xq, Xq, ls, sf2) - A @ Ks.T


def sampler_cov(kernel, X, Xq, ls, sf2, noise, Omega, w=None, jitter=0.0):
    """The exact covariance (M, M) of the sampler at Xq for the frequencies Omega: with A = K* K_y^-1 and K~ = Phi Phi^T,
    K~** - A K~X*^T - K~*X A^T + A (K~XX + noise diag(w)) A^T.  Its mean is the exact posterior mean A y."""
    n = len(scaled(X, 1.0))
    wn = np.ones(n) if w is None else np.asarray(w, dtype=np.float64)
    A = np.linalg.solve(k_y(kernel, X, ls, sf2, noise, w, jitter), kernel_matrix(kernel, Xq, X, ls, sf2).T).T
    Ps, Px = features(Xq, ls, Omega, sf2), features(X, ls, Omega, sf2)
    D = Ps - A @ Px
    return D @ D.T + (A * (noise * wn)[None, :]) @ A.T
