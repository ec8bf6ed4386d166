"""Inducing-point Gaussian process on one GPU: the collapsed variational bound of Titsias (2009), "SGPR".

For data with more observations than a dense Cholesky factor can hold — a trajectory cluster of tens of thousands of
paths is a million rows whose inputs are a 1-D time — ``m`` inducing points ``Z`` stand for the ``N`` observations.  The
fit costs O(N m^2) and O(m^2 + chunk m) memory; the observations stream through the device in chunks.  The model
(``include/gpx.h`` has the formulas, ``tests/sparse_ref.py`` the NumPy definition)::

    Kuu = variance k(Z, Z) + jitter I = L L^T        A = L^-1 variance k(Z, X) S^-1/2        B = I + A A^T

with ``S = diag(noise * noise_weights)``.  When ``Z`` covers the distinct inputs the posterior IS the exact one (40 paths
on a shared 33-step grid with ``Z`` = the grid and ``jitter=0``: mean to 2.5e-13, variance to 2.9e-12 relative).

``jitter`` goes on the diagonal of ``Kuu`` only.  It is a (tiny) change of the MODEL, not of the noise: on that grid
``jitter=1e-6`` already moves the variance by 9e-4 relative.  The default is ``1e-8 * variance``.

The hyperparameters are learnt on the bound itself: ``elbo_gradient()`` is its analytic gradient by the log lengthscales,
log variance and log noise on the GPU (one more streamed pass over the observations, which ``fit`` therefore keeps
references to), and ``optimize`` runs L-BFGS-B on it with ``Z`` fixed.  Learning them on a subsample with the dense ``GP``
optimises another objective: the bound has a trace term the marginal likelihood lacks.

Not part of this class: the gradient with respect to the inducing locations ``Z``, float32 / mixed precision, shards and
device groups, derivative observations, path ids, basis functions, and update / remove / loo on a sparse fit.  There is no
CPU fallback.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _abi
from .gp import _is_torch

MAX_TARGETS = 8


def choose_inducing(X, m, random_state=0):
    """``m`` inducing points for the inputs ``X`` (N, d), NumPy: for ``d == 1`` equally spaced over ``[min X, max X]``;
    otherwise a seeded subset of the distinct rows of ``X`` (all of them, sorted, when there are no more than ``m``)."""
    X = np.asarray(X, dtype=np.float64)
    m = int(m)
    if m < 1:
        raise ValueError("inducing must be >= 1")
    if X.shape[1] == 1:
        lo, hi = float(X.min()), float(X.max())
        return np.linspace(lo, hi, m).reshape(m, 1) if m > 1 else np.array([[0.5 * (lo + hi)]])
    U = np.unique(X, axis=0)
    if U.shape[0] <= m:
        return U
    idx = np.random.default_rng(random_state).choice(U.shape[0], size=m, replace=False)
    return U[np.sort(idx)]


class SparseGP:
    """``SparseGP(kernel, lengthscale, variance, noise, jitter=None, device=None, chunk=None)``: fit, predict, ``elbo``,
    ``elbo_gradient``, ``optimize``.

    kernel : "rbf" | "matern52" | "matern32" | "matern12"
    lengthscale : scalar (isotropic) or (d,) array (ARD)
    variance, noise : signal variance and observation-noise variance (``noise > 0``)
    jitter : added to the diagonal of ``Kuu``; None = ``1e-8 * variance`` (a change of model: see the module text)
    chunk : observations per streamed chunk (rounded up to a multiple of 128); None = the library's choice, a function
        of ``m`` alone.  Results depend on (m, chunk) at rounding level and on nothing else; two fits agree bit for bit.
    """

    def __init__(self, kernel="rbf", lengthscale=1.0, variance=1.0, noise=1e-2, jitter=None, device=None, chunk=None):
        if kernel not in _abi.KERNEL_IDS:
            raise ValueError(f"unknown kernel {kernel!r}; expected one of {sorted(_abi.KERNEL_IDS)}")
        self.kernel = kernel
        self.lengthscale = np.atleast_1d(np.asarray(lengthscale, dtype=np.float64)).copy()
        if self.lengthscale.ndim != 1 or not np.all(self.lengthscale > 0):
            raise ValueError("lengthscale must be a positive scalar or 1-D array")
        self.variance, self.noise = float(variance), float(noise)
        if not self.variance > 0 or not self.noise > 0:
            raise ValueError("need variance > 0 and noise > 0")
        self._jitter_default = jitter is None   # optimize() re-derives the default from the variance it learns
        self.jitter = 1e-8 * self.variance if jitter is None else float(jitter)
        if self.jitter < 0:
            raise ValueError("need jitter >= 0")
        self.chunk = 0 if chunk is None else int(chunk)
        if self.chunk < 0:
            raise ValueError("chunk must be >= 0")
        if device is None:
            import os
            device = int(os.environ.get("LOCAL_RANK", "0"))
        self.device = int(device)
        self._lib = _abi.load()
        cfg = _abi.GpxConfig(kernel=_abi.KERNEL_IDS[kernel], dtype=_abi.DTYPE_IDS["float64"], device=self.device, block=0,
                             rank=0, world=1, flags=0, ndev=0, devices=(C.c_int32 * _abi.MAX_GROUP)(), transport=0, refine=0)
        h = C.c_void_p()
        rc = self._lib.gpx_create(C.byref(h), C.byref(cfg))
        if rc != 0:
            raise _abi.GpxError(rc, self._lib.gpx_last_error(None).decode())
        self._h = h
        self._fitted = False
        self._obs = None
        self.info_ = 0
        self.inducing_ = None

    # -- plumbing ---------------------------------------------------------------------
    def _check(self, rc):
        if rc != 0:
            raise _abi.GpxError(rc, self._lib.gpx_last_error(self._h).decode())

    def close(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            self._lib.gpx_destroy(h)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _as_input(self, a, name):
        """-> (pointer, mem_kind, keepalive, torch_device_or_None, shape), float64"""
        if _is_torch(a):
            import torch
            t = a.detach().to(torch.float64).contiguous()
            if t.is_cuda:
                if t.device.index != self.device:
                    raise ValueError(f"{name} lives on cuda:{t.device.index}, handle on {self.device}")
                torch.cuda.current_stream(t.device).synchronize()
                return C.c_void_p(t.data_ptr()), _abi.MEM_DEVICE, t, t.device, tuple(t.shape)
            a = t.numpy()
        arr = np.ascontiguousarray(a, dtype=np.float64)
        return C.c_void_p(arr.ctypes.data), _abi.MEM_HOST, arr, None, arr.shape

    @staticmethod
    def _empty(shape, dev):
        if dev is not None:
            import torch
            return torch.empty(shape, dtype=torch.float64, device=dev)
        return np.empty(shape, dtype=np.float64)

    @staticmethod
    def _ptr(a):
        return C.c_void_p(a.data_ptr() if _is_torch(a) else a.ctypes.data)

    @staticmethod
    def _like(a, dev):
        """the NumPy array ``a`` in the kind of the call's inputs (a device tensor on ``dev``, or itself)"""
        if dev is None:
            return a
        import torch
        return torch.as_tensor(a, dtype=torch.float64, device=dev)

    # -- the model --------------------------------------------------------------------
    def fit(self, X, y, inducing, noise_weights=None, random_state=0):
        """Fit to ``X`` (N, d), ``y`` (N,) or (N, k <= 8).  ``inducing``: the points ``Z`` (m, d), or an int — that many
        equally spaced points over ``[min X, max X]`` for ``d == 1``, otherwise a subset of the distinct rows of ``X``
        drawn with ``random_state``.  ``noise_weights`` (N,), each finite and > 0, scale the noise per observation
        (``noise * w_n``); a waypoint, ``w = 0``, has no place in this model.  Raises ``numpy.linalg.LinAlgError`` when
        ``Kuu`` is not positive definite (``info_`` = the 1-based pivot: two identical inducing points with ``jitter=0``)."""
        px, kind, keepx, dev, sx = self._as_input(X, "X")
        if len(sx) != 2:
            raise ValueError("X must be (N, d)")
        N, d = sx
        if self.lengthscale.size not in (1, d):
            raise ValueError(f"lengthscale must be a scalar or have d = {d} entries")
        py, ky, keepy, _, sy = self._as_input(y, "y")
        if ky != kind:
            raise ValueError("X and y must both be host arrays or both device tensors")
        if len(sy) not in (1, 2) or sy[0] != N:
            raise ValueError(f"y must be ({N},) or ({N}, k)")
        self._y1d = len(sy) == 1
        k = 1 if self._y1d else sy[1]
        if not 1 <= k <= MAX_TARGETS:
            raise ValueError(f"SparseGP takes 1 <= k <= {MAX_TARGETS} target columns")
        pw = keepw = None
        if noise_weights is not None:
            pw, kw, keepw, _, sw = self._as_input(noise_weights, "noise_weights")
            if tuple(sw) != (N,):
                raise ValueError(f"noise_weights must be ({N},), one weight per observation")
            if kw != kind:
                raise ValueError("noise_weights must be of the same kind as X: both host arrays or both device tensors")
        if isinstance(inducing, (int, np.integer)):
            Xh = keepx.cpu().numpy() if dev is not None else keepx
            Z = choose_inducing(Xh, int(inducing), random_state)
        else:
            Z = inducing.detach().cpu().numpy() if _is_torch(inducing) else inducing
            Z = np.array(Z, dtype=np.float64, ndmin=2)
            if Z.ndim != 2 or Z.shape[1] != d or Z.shape[0] < 1:
                raise ValueError(f"inducing must be (m, {d}) or an int")
        Z = np.ascontiguousarray(Z)
        zin = self._like(Z, dev)
        info = C.c_int64(0)
        ls = self.lengthscale
        self._fitted, self._obs = False, None
        self._check(self._lib.gpx_sparse_fit(self._h, px, py, pw, N, d, k, self._ptr(zin), Z.shape[0], _abi.dptr(ls), ls.size,
                                             self.variance, self.noise, self.jitter, self.chunk, kind, C.byref(info)))
        self.info_ = int(info.value)
        if self.info_ != 0:
            what = "Kuu" if self.info_ <= Z.shape[0] else "I + A A^T"
            raise np.linalg.LinAlgError(f"{what} is not positive definite (pivot {self.info_}; m = {Z.shape[0]}): "
                                        "identical inducing points need jitter > 0")
        self.inducing_ = self._like(Z, dev)
        self._d, self._k, self._N = d, k, N
        self._obs = (px, py, pw, kind, (keepx, keepy, keepw))   # references, not copies: elbo_gradient() streams them again
        self._fitted = True
        return self

    def predict(self, Xs, return_var=True, include_noise=False, return_cov=False):
        """Posterior of the latent function at ``Xs`` (M, d): ``mean`` ((M,) for a 1-D ``y``, else (M, k)) and, with
        ``return_var``, the variance (M,); ``return_cov=True`` returns ``(mean, cov)`` with the joint (M, M) covariance
        instead.  ``include_noise`` adds ``noise`` (times 1: a query point has no weight).  NumPy in, NumPy out; a device
        tensor in, device tensors out."""
        if not self._fitted:
            raise RuntimeError("predict() before a successful fit()")
        pq, kq, keepq, devq, sq = self._as_input(Xs, "Xs")
        if len(sq) != 2 or sq[1] != self._d:
            raise ValueError(f"Xs must be (M, {self._d})")
        M = sq[0]
        mean = self._empty((M,) if self._y1d else (M, self._k), devq)
        if return_cov:
            cov = self._empty((M, M), devq)
            self._check(self._lib.gpx_sparse_predict_cov(self._h, pq, M, self._ptr(mean), self._ptr(cov), kq))
            if include_noise:
                if devq is not None:
                    cov.diagonal().add_(self.noise)
                else:
                    cov[np.diag_indices(M)] += self.noise
            return mean, cov
        var = self._empty((M,), devq) if return_var else None
        self._check(self._lib.gpx_sparse_predict(self._h, pq, M, self._ptr(mean), self._ptr(var) if return_var else None, kq))
        if not return_var:
            return mean
        if include_noise:
            var += self.noise
        return mean, var

    def elbo(self):
        """The collapsed bound per target column, (k,) float64 NumPy: ``elbo().sum()`` is a lower bound of the exact log
        marginal likelihood of the same data under the same hyperparameters, and equals it when ``Z`` covers the inputs."""
        if not self._fitted:
            raise RuntimeError("elbo() before a successful fit()")
        out = np.empty(self._k, dtype=np.float64)
        self._check(self._lib.gpx_sparse_elbo(self._h, _abi.dptr(out)))
        return out

    def elbo_gradient(self):
        """``(elbo().sum(), grad)``: the bound summed over the target columns and its gradient by the LOG parameters,
        ``grad`` (n_ls + 2,) float64 NumPy ordered as ``GP.lml_gradient``'s: the lengthscales, ``variance``, ``noise``.
        ``Z`` and ``jitter`` are constants.  Analytic, on the GPU: an O(m^3) stage and one more streamed pass over the
        observations ``fit`` was given — ``fit`` keeps references to them, not copies, so they must not have been
        changed in place since.  The fit is left as it is: ``predict`` afterwards returns the same bits."""
        if not self._fitted:
            raise RuntimeError("elbo_gradient() before a successful fit()")
        px, py, pw, kind, _ = self._obs
        elbo = np.empty(self._k, dtype=np.float64)
        grad = np.empty(self.lengthscale.size + 2, dtype=np.float64)
        self._check(self._lib.gpx_sparse_elbo_grad(self._h, px, py, pw, self._N, kind, _abi.dptr(elbo), _abi.dptr(grad)))
        return float(elbo.sum()), grad

    def optimize(self, X, y, inducing, params=("lengthscale", "variance", "noise"), bounds=(1e-4, 1e4), maxiter=40,
                 jac="analytic", noise_weights=None, random_state=0):
        """Learn the hyperparameters by maximising the bound ``elbo().sum()`` with L-BFGS-B in log space (the shape of
        ``GP.optimize``).  ``params`` chooses what moves ("lengthscale" moves every ARD entry).  An int ``inducing`` is
        resolved to ``Z`` once, as :meth:`fit` does, and ``Z`` then stays fixed through the search.  ``jac="analytic"``:
        every evaluation is one ``fit`` and one ``elbo_gradient`` on the GPU; ``jac="3-point"``: central differences of
        the bound, 2 p extra fits per gradient.  A trial point whose factorisation fails counts as very bad, it does
        not raise.  A ``jitter`` left at None in the constructor is re-derived as ``1e-8 * variance`` at every point; one
        that was given stays.  Leaves the model fitted at the best point found, with ``lengthscale``, ``variance`` and
        ``noise`` updated, and returns scipy's result with ``.fun == -elbo().sum()`` there."""
        from scipy.optimize import minimize
        known = ("lengthscale", "variance", "noise")
        names = [p for p in known if p in params]
        if not names or len(names) != len(tuple(params)):
            raise ValueError("params must be a non-empty subset of " + " / ".join(known))
        if jac not in ("analytic", "3-point"):
            raise ValueError('jac must be "analytic" or "3-point"')
        if isinstance(inducing, (int, np.integer)):
            Xh = X.detach().cpu().numpy() if _is_torch(X) else np.asarray(X, dtype=np.float64)
            inducing = choose_inducing(Xh, int(inducing), random_state)
        n_ls = self.lengthscale.size
        cols = []
        for p in names:
            cols.extend(range(n_ls) if p == "lengthscale" else [n_ls + ("variance", "noise").index(p)])
        analytic = jac == "analytic"

        def pack():
            v = []
            for p in names:
                v.extend(np.log(self.lengthscale) if p == "lengthscale" else [np.log(max(getattr(self, p), bounds[0]))])
            return np.asarray(v, dtype=np.float64)

        def unpack(v):
            i = 0
            for p in names:
                if p == "lengthscale":
                    self.lengthscale = np.exp(v[i:i + n_ls])
                    i += n_ls
                else:
                    setattr(self, p, float(np.exp(v[i])))
                    i += 1
            if self._jitter_default:
                self.jitter = 1e-8 * self.variance

        best = {"f": np.inf, "v": pack()}

        def objective(v):
            unpack(v)
            g = np.zeros(len(cols))
            try:
                self.fit(X, y, inducing, noise_weights=noise_weights)
                if analytic:
                    f, full = self.elbo_gradient()
                    f, g = -f, -full[cols]
                else:
                    f = -float(self.elbo().sum())
            except np.linalg.LinAlgError:
                f = 1e300
            if not np.isfinite(f) or not np.all(np.isfinite(g)):
                f, g = 1e300, np.zeros(len(cols))
            if f < best["f"]:
                best["f"], best["v"] = f, np.array(v, copy=True)
            return (f, g) if analytic else f

        v0 = pack()
        lo, hi = np.log(bounds[0]), np.log(bounds[1])
        res = minimize(objective, v0, method="L-BFGS-B", jac=True if analytic else "3-point", bounds=[(lo, hi)] * v0.size,
                       options={"maxiter": int(maxiter)} if analytic else {"maxiter": int(maxiter), "eps": 1e-4})
        unpack(best["v"])
        self.fit(X, y, inducing, noise_weights=noise_weights)
        res.x, res.fun = best["v"], -float(self.elbo().sum())
        return res

    @property
    def chunk_(self):
        """rows per chunk of the last fit"""
        c = C.c_int64(0)
        self._check(self._lib.gpx_sparse_info(self._h, None, None, None, C.byref(c)))
        return int(c.value)

    @property
    def timings_(self):
        t = _abi.GpxTimings()
        self._check(self._lib.gpx_get_timings(self._h, C.byref(t)))
        return t.as_dict()
