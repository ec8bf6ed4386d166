"""Exact Gaussian-process regression with a ``fit()`` / ``predict()`` surface.

This is the Python host side of the hot path.  The upstream reference
(``GPmap.py``) has no such class — its public names are ``trajectory``,
``trajectories``, ``readcsvfile`` (``GPmap.py:12,28,178``) — so the surface is the one
BASELINE.json's north_star names: hyper-parameters are fixed inputs, ``fit(X, y)``
factorises ``K = sf2 k(X,X) + (sn2 + jitter) I`` (``noise_weights``: ``+ diag(sn2 w_i + jitter)``) and solves for ``alpha``,
``predict(Xs)`` returns the posterior mean and (latent) variance.

All arithmetic runs in ``csrc/libgpx.so`` (hand-written HIP for gfx950) through the
ctypes C ABI of ``include/gpx.h``.  There is no CPU code path: without the library or
without a GPU, construction raises.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _abi


def _is_torch(x) -> bool:
    return type(x).__module__.split(".")[0] == "torch"


def check_path_args(path_ids, path_variance, path_lengthscale, n=None, d=None, derivatives=None):
    """Validation of ``fit(..., path_ids=, path_variance=, path_lengthscale=)`` -> ``(ids, variance, lengthscale)``: ``ids``
    None or a contiguous (N,) int32 array, ``lengthscale`` None (the model's own) or a 1-D float64 array.  Raises
    ``ValueError`` for ids that are not one integer >= -1 per observation, a negative or non-finite variance, a
    lengthscale that is not positive (or has neither 1 nor d entries), and for path ids together with ``derivatives``."""
    var = float(path_variance)
    if not np.isfinite(var) or var < 0:
        raise ValueError("path_variance must be finite and >= 0")
    lsp = None
    if path_lengthscale is not None:
        lsp = np.atleast_1d(np.asarray(path_lengthscale, dtype=np.float64)).copy()
        if lsp.ndim != 1 or lsp.size == 0 or not np.all(np.isfinite(lsp)) or not np.all(lsp > 0):
            raise ValueError("path_lengthscale must be a positive scalar or 1-D array")
        if d is not None and lsp.size not in (1, d):
            raise ValueError("path_lengthscale must be scalar or have d entries")
    if path_ids is None:
        return None, var, lsp
    if derivatives is not None:
        raise ValueError("path_ids cannot be combined with derivatives=: no builder evaluates both")
    if _is_torch(path_ids):
        path_ids = path_ids.detach().cpu().numpy()
    ids = np.asarray(path_ids)
    if ids.ndim != 1 or (n is not None and ids.shape[0] != n):
        raise ValueError("path_ids must be (N,), one id per observation")
    if not np.issubdtype(ids.dtype, np.integer):
        raise ValueError("path_ids must be integers")
    if ids.size and (ids.min() < -1 or ids.max() > np.iinfo(np.int32).max):
        raise ValueError("path_ids must be >= 0, or -1 for an observation that belongs to no path")
    return np.ascontiguousarray(ids, dtype=np.int32), var, lsp


class GP:
    """Exact GP regressor on one MI355X (or a row-block shard of several).

    Parameters
    ----------
    kernel : "rbf" | "matern52" | "matern32" | "matern12" — scikit-learn's ``RBF`` and ``Matern(nu=2.5 | 1.5 | 0.5)``
        (include/gpx.h).  Matern-3/2 is the usual prior for trajectories (a velocity, no acceleration);
        Matern-1/2 (exponential / Ornstein-Uhlenbeck) has no derivative, so :meth:`predict_gradient` raises
        ``GpxError`` for it; :meth:`predict_hessian` (second derivatives: acceleration, curvature) needs a twice
        differentiable prior and runs for "rbf" and "matern52" only.  Every other call runs for all four.
    lengthscale : float or array of d floats (ARD)
    variance : signal variance sf2
    noise : observation-noise variance sn2 (added to the diagonal).  ``fit(..., noise_weights=w)`` makes it the LEVEL of a
        per-observation noise ``sn2 * w_i`` (``w_i >= 0``, one per observation, shared by the targets; ``w_i = 0`` is an
        exact observation); absolute variances are ``noise=1.0, noise_weights=variances``.  ``lml_gradient`` and
        ``optimize`` learn the level, the weights are fixed data.  One device only (not ``devices=`` / ``world=``).
    jitter : extra diagonal term; default 1e-10 * variance
    dtype : "float64" | "float32" (everything, including the factorisation, in fp32:
        the precision study of BASELINE.json configs[4]; not a 1e-6 path) | "mixed" (float64 in and
        out; the factorisation in fp32 at twice the MFMA rate, alpha refined in fp64 against the
        matrix-free fp64 kernel: **fp64-grade posterior mean** (1e-6 elementwise at N = 65536,
        tests/test_full_size_gpu.py) but an **fp32-grade variance** — sf2 - ||L^-1 k*||^2 through
        the fp32 factor is never refined, so it carries absolute errors of ~3e-6 sf2, which is
        percents of a variance of 1e-4 sf2; use "float64" when the variance matters.  At most 8
        targets).  Every dtype also runs sharded (``devices=`` / ``world=``: the shard takes the handle's
        element type; round 4)
    refine : "mixed" only — 0 (default): refine until ||y - K alpha|| <= 1e-10 ||y|| or the residual
        stops contracting (at most 12 iterations; ``timings_["refine_iters"]`` says how many ran);
        n > 0: exactly n iterations
    device : HIP device ordinal (default: LOCAL_RANK or 0)
    devices : several GPUs from ONE ordinary Python process: an int n (devices
        0..n-1) or a list of HIP ordinals.  The Gram matrix is sharded in row blocks dealt over the devices (snake dealing: balanced row work)
        over them; one worker thread per device lives inside ``fit`` / ``predict``, which stay
        plain blocking calls — no launcher, no ``torch.distributed``.  ``devices=1`` / ``[i]`` is
        the single-GPU path on that device — unless ``transport`` is given explicitly: then it is a
        ONE-rank group (the group / RCCL code path on a single GPU; tests).
    transport : how the devices of a ``devices=`` group exchange panels: "rccl"
        (``ncclCommInitAll`` inside the process; distinct devices only), "local" (peer copies
        and hipEvents between the ranks' streams, nothing but HIP), None/"auto" = rccl when the
        devices are distinct, else local.
    oversubscribe : allow ``devices=n`` with fewer than n GPUs visible: ordinals wrap around, so
        several ranks share a GPU over the local transport (how the one-GPU tests run 2..8 ranks)
    block : Cholesky panel width nb (multiple of 128, at most 4096; 0 = the library's choice: 1024, and 2048 from
        N = 40960 on, where nothing of the serial chain is exposed any more)
    max_tries : jitter escalations (x10 each) before ``LinAlgError``
    profile : record per-launch timings of the Cholesky sub-phases
    world, rank : row-block shard of ONE Gram matrix over ``world`` processes (one per GPU).
        Every rank passes the same full X, y, Xs and receives the full mean / var.
    comm : "rccl" (RCCL on the library's stream; unique id shipped by torch.distributed),
        "host" (collectives on host buffers through torch.distributed, e.g. gloo), or
        None = pick from the initialised torch.distributed backend when world > 1.
        ``comm`` with world == 1 runs the sharded schedule on one rank (tests).
    """

    def __init__(self, kernel="rbf", lengthscale=1.0, variance=1.0, noise=1e-2, jitter=None,
                 dtype="float64", device=None, block=0, max_tries=3, profile=False,
                 world=1, rank=0, comm=None, group=None, devices=None, transport=None,
                 oversubscribe=False, refine=0):
        if kernel not in _abi.KERNEL_IDS:
            raise ValueError(f"unknown kernel {kernel!r}; expected one of {sorted(_abi.KERNEL_IDS)}")
        if dtype not in _abi.DTYPE_IDS:
            raise ValueError(f"unknown dtype {dtype!r}")
        self.kernel = kernel
        self.lengthscale = np.atleast_1d(np.asarray(lengthscale, dtype=np.float64)).copy()
        if self.lengthscale.ndim != 1 or not np.all(self.lengthscale > 0):
            raise ValueError("lengthscale must be a positive scalar or 1-D array")
        self.variance = float(variance)
        self.noise = float(noise)
        if not self.variance > 0 or self.noise < 0:
            raise ValueError("need variance > 0 and noise >= 0")
        self.jitter = 1e-10 * self.variance if jitter is None else float(jitter)
        self.dtype = dtype
        self._np_dtype = np.float32 if dtype == "float32" else np.float64
        self.block = int(block)
        self.max_tries = int(max_tries)
        self.refine = int(refine)
        if device is None:
            import os
            device = int(os.environ.get("LOCAL_RANK", "0"))
        self.device = int(device)
        self._lib = _abi.load()
        self.world, self.rank = int(world), int(rank)
        if transport not in _abi.TRANSPORT_IDS:
            raise ValueError(f"unknown transport {transport!r}; expected rccl / local / auto")
        self.devices = self._resolve_devices(devices, oversubscribe)
        self._is_group = len(self.devices) > 1 or (len(self.devices) == 1 and _abi.TRANSPORT_IDS[transport] != 0)
        if self._is_group and (self.world != 1 or comm is not None):
            raise ValueError("devices= (one process, several GPUs) and world=/comm= (one process per GPU) "
                             "are two different process models: pick one")
        if self.devices:
            self.device = self.devices[0]
            if self._is_group and transport != "local":
                _abi.prefer_torch_rccl()     # the group will load RCCL: torch's copy, after torch (see _abi)
        cfg = _abi.GpxConfig(kernel=_abi.KERNEL_IDS[kernel], dtype=_abi.DTYPE_IDS[dtype],
                             device=self.device, block=self.block, rank=self.rank, world=self.world,
                             flags=_abi.FLAG_PROFILE if profile else 0, ndev=len(self.devices),
                             devices=(C.c_int32 * _abi.MAX_GROUP)(*self.devices),
                             transport=_abi.TRANSPORT_IDS[transport], refine=int(refine))
        h = C.c_void_p()
        rc = self._lib.gpx_create(C.byref(h), C.byref(cfg))
        if rc != 0:
            raise _abi.GpxError(rc, self._lib.gpx_last_error(None).decode())
        self._h = h
        self._fitted = False
        self._weights_set = False  # gpx_set_noise_weights holds a vector for the next fits
        self._kinds_set = False    # gpx_set_observation_kinds holds kinds for the next fits
        self.derivative_noise = 0.0  # noise variance of the derivative rows of the last fit(derivatives=) (0 without any)
        self._groups_set = False   # gpx_set_path_groups holds path ids for the next fits
        self._basis_set = None     # gpx_set_basis holds a basis for the next fits (None: none)
        self._basis_fit = None     # the basis of the last successful fit
        self.path_variance = 0.0   # within-path variance sg2 of the last fit(path_ids=) (0 without any)
        self.path_lengthscale = None  # ... and its lengthscale(s) (None without path ids)
        self._n_path_ls = 1        # path lengthscales of the last fit: entries of lml_gradient(path=True) after path_variance
        self._alpha = None
        self.info_ = 0
        self.jitter_used_ = self.jitter
        self._host_comm = None
        self._has_comm = self.world > 1 or comm is not None
        if self._has_comm:
            self._init_comm(comm, group)

    def _resolve_devices(self, devices, oversubscribe):
        if devices is None:
            return []
        if isinstance(devices, (int, np.integer)):
            n = int(devices)
            if n < 1:
                raise ValueError("devices must be >= 1")
            devs = list(range(n))
        else:
            devs = [int(v) for v in devices]
            if not devs:
                raise ValueError("devices must not be empty")
        if len(devs) > _abi.MAX_GROUP:
            raise ValueError(f"at most {_abi.MAX_GROUP} devices per group")
        if oversubscribe:
            cnt = C.c_int(0)
            self._lib.gpx_device_count(C.byref(cnt))
            if cnt.value > 0:
                devs = [v % cnt.value for v in devs]
        return devs

    def _init_comm(self, comm, group):
        from . import dist as gdist
        if comm is None:
            import torch.distributed as tdist
            if not tdist.is_initialized():
                raise RuntimeError("world > 1 needs torch.distributed.init_process_group() first")
            comm = "rccl" if tdist.get_backend(group) == "nccl" else "host"
        try:
            if comm == "rccl":
                gdist.init_rccl(self._lib, self._h, self.rank, self.world, group)
            elif comm == "host":
                self._host_comm = gdist.HostCollectives(group)
                self._host_comm.attach(self._lib, self._h)
            else:
                raise ValueError(f"unknown comm {comm!r}")
        except Exception:
            self.close()
            raise

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
        """-> (pointer, mem_kind, keepalive, torch_device_or_None, shape)"""
        if _is_torch(a):
            import torch
            t = a.detach()
            tdt = torch.float32 if self.dtype == "float32" else torch.float64
            if t.dtype != tdt:
                t = t.to(tdt)
            t = t.contiguous()
            if t.is_cuda:
                if t.device.index != self.device:
                    raise ValueError(f"{name} lives on cuda:{t.device.index}, handle on {self.device}")
                torch.cuda.current_stream(t.device).synchronize()
                return C.c_void_p(t.data_ptr()), _abi.MEM_DEVICE, t, t.device, tuple(t.shape)
            a = t.numpy()
        arr = np.ascontiguousarray(a, dtype=self._np_dtype)
        return C.c_void_p(arr.ctypes.data), _abi.MEM_HOST, arr, None, arr.shape

    def _weights_input(self, w, n, kind, name, like):
        """per-point weights ``w`` (n,) -> pointer (None for ``w is None``) and keepalive; same kind as ``like``"""
        if w is None:
            return None, None
        pw, kw, keepw, devw, sw = self._as_input(w, name)
        if tuple(sw) != (n,):
            raise ValueError(f"{name} must be ({n},), one weight per point")
        if kw != kind:
            raise ValueError(f"{name} must be of the same kind as {like}: both host arrays or both device tensors")
        return pw, keepw

    def _set_noise_weights(self, w, n, kind):
        """the weights of the fits that follow (``gpx_set_noise_weights``); None clears them.  A refused vector
        (wrong length or kind: ValueError; negative or non-finite: GpxError) leaves the handle as it was."""
        pw, keepw = self._weights_input(w, n, kind, "noise_weights", "X")
        if pw is None and not self._weights_set:
            return  # (a model that never had weights makes no call at all)
        self._check(self._lib.gpx_set_noise_weights(self._h, pw, n if pw is not None else 0, kind))
        self._weights_set = pw is not None

    @property
    def noise_weights_(self):
        """Per-observation noise weights of the fitted model (N,), appended points included; ones without any."""
        if not self._fitted:
            raise RuntimeError("no fit")
        out = np.empty((self._N,), dtype=self._np_dtype)
        self._check(self._lib.gpx_get_noise_weights(self._h, C.c_void_p(out.ctypes.data)))
        return out

    def _set_observation_kinds(self, kinds, derivative_noise):
        """the kinds of the fits that follow (``gpx_set_observation_kinds``); None clears them"""
        if kinds is None:
            if self._kinds_set:
                self._check(self._lib.gpx_set_observation_kinds(self._h, None, 0, 0.0, _abi.MEM_HOST))
                self._kinds_set = False
            return  # (a model that never had kinds makes no call at all)
        self._check(self._lib.gpx_set_observation_kinds(self._h, C.c_void_p(kinds.ctypes.data), kinds.size,
                                                        float(derivative_noise), _abi.MEM_HOST))
        self._kinds_set = True

    def _set_path_groups(self, ids, variance, lengthscale):
        """the path ids of the fits that follow (``gpx_set_path_groups``); None clears them"""
        if ids is None:
            if self._groups_set:
                self._check(self._lib.gpx_set_path_groups(self._h, None, 0, 0.0, None, 0, _abi.MEM_HOST))
                self._groups_set = False
            self.path_variance, self.path_lengthscale = 0.0, None
            self._n_path_ls = 1 if lengthscale is None else int(np.size(lengthscale))
            return  # (a model that never had path ids makes no call at all)
        lsp = self.lengthscale if lengthscale is None else lengthscale
        lsp = np.ascontiguousarray(lsp, dtype=np.float64)
        # an effective fit (one id >= 0, variance > 0) has the lengthscales the library gets; any other the ones given, else 1
        effective = float(variance) > 0 and bool(np.any(ids >= 0))
        self._check(self._lib.gpx_set_path_groups(self._h, C.c_void_p(ids.ctypes.data), ids.size, float(variance),
                                                  _abi.dptr(lsp), lsp.size, _abi.MEM_HOST))
        self._groups_set = True
        self.path_variance, self.path_lengthscale = float(variance), lsp.copy()
        self._n_path_ls = lsp.size if effective or lengthscale is not None else 1

    @staticmethod
    def _check_basis(basis):
        if basis not in _abi.BASIS_IDS:
            raise ValueError(f"unknown basis {basis!r}; expected None, 'constant', 'linear' or 'quadratic'")
        return basis

    def _set_basis(self, basis):
        """the basis of the fits that follow (``gpx_set_basis``); None clears it"""
        if basis == self._basis_set:
            return  # (a model that never had a basis makes no call at all)
        self._check(self._lib.gpx_set_basis(self._h, _abi.BASIS_IDS[basis]))
        self._basis_set = basis

    def _refusal_keeps_fit(self, basis, prev):
        """-> a handler for the GpxError of a fit made with ``basis``: the library refuses such a fit (GPX_E_ARG,
        GPX_E_UNSUPPORTED) before it touches anything, so the model of the fit before — ``prev``, the Python side of
        it — is still the one the handle holds."""
        def handler(e):
            if basis is not None and e.code in (_abi.E_ARG, _abi.E_UNSUPPORTED):
                (self._fitted, self._N, self._d, self._k, self._y1d, self._alpha) = prev
        return handler

    def _fit_state(self):
        return (self._fitted, getattr(self, "_N", 0), getattr(self, "_d", 0), getattr(self, "_k", 0),
                getattr(self, "_y1d", True), self._alpha)

    def _get_basis(self):
        if not self._fitted:
            raise RuntimeError("no fit")
        b, p = C.c_int32(0), C.c_int32(0)
        self._check(self._lib.gpx_get_basis(self._h, C.byref(b), C.byref(p), None, None))
        beta = np.empty((p.value, self._k), dtype=np.float64)
        cov = np.empty((p.value, p.value), dtype=np.float64)
        if p.value:
            self._check(self._lib.gpx_get_basis(self._h, C.byref(b), C.byref(p), _abi.dptr(beta), _abi.dptr(cov)))
        name = {v: k for k, v in _abi.BASIS_IDS.items()}[b.value]
        return name, (beta[:, 0].copy() if self._y1d else beta), cov

    @property
    def basis_(self):
        """Basis of the fitted model (``fit(..., basis=)``): None, "constant", "linear" or "quadratic"."""
        return self._get_basis()[0]

    @property
    def beta_(self):
        """Generalised-least-squares coefficients of the basis functions, (p, k) — (p,) for a 1-D ``y`` — in the order
        ``[1, x_1..x_d, x_1^2..x_d^2]`` and in the units of the raw inputs; p = 0 for a fit without a basis."""
        return self._get_basis()[1]

    @property
    def beta_cov_(self):
        """Covariance (p, p) of ``beta_`` under the flat prior, ``(H^T K^-1 H)^-1``, shared by the k targets."""
        return self._get_basis()[2]

    @property
    def path_ids_(self):
        """Path id of every observation of the fitted model (N,) int32; all -1 for a fit without path ids (or with
        ``path_variance == 0``, which is the plain model)."""
        if not self._fitted:
            raise RuntimeError("no fit")
        out = np.empty((self._N,), dtype=np.int32)
        self._check(self._lib.gpx_get_path_groups(self._h, C.c_void_p(out.ctypes.data)))
        return out

    def _with_derivatives(self, X, y, derivatives, noise_weights=None):
        """``(X, y, noise_weights, kinds)`` of a fit: without ``derivatives`` the arguments as they are and no kinds;
        with ``derivatives = (Xd, dims, yd)`` the value rows first and the derivative rows last, ``kinds`` (N + Nd,)
        int32 (-1: a value, j: a value of d f / d x_j), and weights of length N extended by ones."""
        if derivatives is None:
            return X, y, noise_weights, None
        try:
            Xd, dims, yd = derivatives
        except (TypeError, ValueError):
            raise ValueError("derivatives must be (Xd, dims, yd)") from None
        if not (_is_torch(X) == _is_torch(Xd) == _is_torch(yd) == _is_torch(y)):
            raise ValueError("Xd and yd must be of the same kind as X and y: all NumPy arrays or all tensors")
        if not _is_torch(X):
            X, y, Xd, yd = (np.asarray(v) for v in (X, y, Xd, yd))
            if noise_weights is not None:
                noise_weights = np.asarray(noise_weights)
        if len(X.shape) != 2 or len(Xd.shape) != 2 or Xd.shape[1] != X.shape[1]:
            raise ValueError("X must be (N, d) and Xd (Nd, d)")
        N, d = int(X.shape[0]), int(X.shape[1])
        Nd = int(Xd.shape[0])
        if len(y.shape) not in (1, 2) or y.shape[0] != N:
            raise ValueError("y must be (N,) or (N, k) with the same N as X")
        if tuple(yd.shape) != (Nd,) + tuple(y.shape[1:]):
            raise ValueError("yd must be (Nd,) or (Nd, k), shaped as y")
        dims = np.asarray(dims)
        if dims.ndim == 0:
            dims = np.full((Nd,), int(dims))
        if dims.shape != (Nd,) or not np.issubdtype(dims.dtype, np.integer) or np.any(dims < 0) or np.any(dims >= d):
            raise ValueError(f"dims must be an int or (Nd,) ints in [0, {d})")
        kinds = np.concatenate([np.full((N,), -1, dtype=np.int32), dims.astype(np.int32)])
        if _is_torch(X):
            import torch
            cat, ones = torch.cat, lambda like: torch.ones((Nd,), dtype=like.dtype, device=like.device)
            Xd, yd = Xd.to(X.device, X.dtype), yd.to(y.device, y.dtype)
        else:
            cat, ones = np.concatenate, lambda like: np.ones((Nd,), dtype=np.asarray(like).dtype)
        w = noise_weights
        if w is not None and tuple(w.shape) == (N,) and Nd > 0:
            w = cat([w, ones(w)])
        return cat([X, Xd]), cat([y, yd]), w, kinds

    @property
    def observation_kinds_(self):
        """Kind of every observation row of the fitted model (N,) int32: -1 a value of f, j a value of d f / d x_j
        (``fit(..., derivatives=)`` puts the value rows first); all -1 for a fit without derivative observations."""
        if not self._fitted:
            raise RuntimeError("no fit")
        out = np.empty((self._N,), dtype=np.int32)
        self._check(self._lib.gpx_get_observation_kinds(self._h, C.c_void_p(out.ctypes.data)))
        return out

    # -- API ----------------------------------------------------------------------------
    def fit(self, X, y, noise_weights=None, derivatives=None, derivative_noise=0.0, path_ids=None, path_variance=0.0,
            path_lengthscale=None, basis=None):
        """Factorise and solve.  ``noise_weights`` (N,), of the same kind as ``X`` (NumPy array or device tensor): the
        diagonal of K gets ``noise * w_i + jitter`` instead of ``noise + jitter``; None (the default) means none — also
        after a weighted fit.

        ``derivatives = (Xd, dims, yd)`` conditions the model on derivative observations as well
        (``gpx_set_observation_kinds``): ``yd[i]`` ((Nd,) or (Nd, k), as ``y``) is a value of d f / d x_dims[i] at
        ``Xd[i]`` — a velocity when that input is time; ``dims`` an int or (Nd,) ints; ``Xd`` and ``yd`` of the same
        kind as ``X``.  Their noise variance is ``derivative_noise`` (>= 0; the attribute of that name keeps it, and
        :meth:`optimize` learns it on request; 0 with a waypoint ``w_i = 0`` at the same point: "pass through here with
        this velocity").  The model then holds the N value rows followed by the Nd
        derivative rows (``alpha_``, ``observation_kinds_``, ``noise_weights_``); ``noise_weights`` may have length N
        (derivative rows get 1) or N + Nd.  RBF, Matern-5/2 and Matern-3/2 on one device, float64 / float32; None (the
        default) means none — also after such a fit.

        ``path_ids`` (N,) ints (NumPy array or tensor) fit the hierarchical model ``y_p(t) = f(t) + g_p(t) + noise``
        (``gpx_set_path_groups``): observations with the same id >= 0 belong to one path and share a deviation ``g_p``,
        a GP of the model's covariance family with variance ``path_variance`` and lengthscale ``path_lengthscale`` (None:
        the model's ``lengthscale``), independent between paths; id -1 is an observation of ``f`` alone.  EVERY
        PREDICTION (:meth:`predict`, ``return_cov``, :meth:`predict_gradient`, :meth:`sample_y`) IS THEN THE POSTERIOR OF
        THE CLUSTER MEAN ``f``; :meth:`score_blocks` scores each block as a new path (``+ path_variance k(., .;
        path_lengthscale)``) and :meth:`forecast_blocks` forecasts one from its first points.  The attributes
        ``path_variance``, ``path_lengthscale`` and ``path_ids_`` keep what the fit used.  ``path_variance=0`` or ids that
        are all -1 are the plain fit bit for bit; None (the default) means none — also after such a fit.  float64 /
        float32 on one device, not with ``derivatives``; :meth:`update` appends to such a fit when it is given the new
        rows' ``path_ids``, and its gradient is ``lml_gradient(path=True)``.

        ``basis`` = "constant", "linear" or "quadratic" gives the model an explicit mean ``h(x)^T beta`` with
        ``h = [1]``, ``[1, x_1..x_d]`` or ``[1, x_1..x_d, x_1^2..x_d^2]`` of the raw inputs and the coefficients
        marginalised under a flat prior (``gpx_set_basis``; Rasmussen & Williams §2.7): away from the data the mean
        reverts to the fitted trend instead of 0, and the uncertainty of ``beta`` is part of every variance,
        covariance, sample, block score and forecast.  ``basis_``, ``beta_`` and ``beta_cov_`` describe the fit;
        ``alpha_`` is ``K^-1 (y - H beta)``; :meth:`log_marginal_likelihood` is then the PROFILE likelihood at
        ``beta_`` and :meth:`lml_gradient` its exact gradient.  k + p <= 64 and N >= p (``GpxError`` otherwise, the
        model as it was).  float64 / float32 on one device, with ``noise_weights`` if wanted, not with
        ``derivatives`` or ``path_ids``; :meth:`update`, :meth:`remove`, :meth:`predict_gradient` and ``path_ids=``
        queries raise ``GpxError`` on such a fit.  None (the default) means none — also after such a fit.
        ``ValueError`` for any other value, before any library call."""
        self._check_basis(basis)
        ids, pvar, plsp = check_path_args(path_ids, path_variance, path_lengthscale, derivatives=derivatives)
        X, y, noise_weights, kinds = self._with_derivatives(X, y, derivatives, noise_weights)
        return self._fit_rows(X, y, noise_weights, kinds, derivative_noise, (ids, pvar, plsp), basis)

    def _not_pd(self, N):
        """the message of a fit whose jitter escalations ran out: a pivot of K, or (info > N) of the basis' H^T K^-1 H"""
        if self.info_ > N:
            return (f"the basis functions are linearly dependent on this data (pivot {self.info_ - N} of H^T K^-1 H is "
                    f"not positive) after {self.max_tries} jitter escalations")
        return (f"kernel matrix not positive definite (first bad pivot {self.info_}) after "
                f"{self.max_tries} jitter escalations")

    def _fit_rows(self, X, y, noise_weights, kinds, derivative_noise, paths=(None, 0.0, None), basis=None):
        """:meth:`fit` of observation rows that are concatenated already, ``kinds`` (None: all values) theirs"""
        px, kx, keepx, devx, sx = self._as_input(X, "X")
        py, ky, keepy, devy, sy = self._as_input(y, "y")
        if len(sx) != 2:
            raise ValueError("X must be (N, d)")
        N, d = sx
        if len(sy) not in (1, 2) or sy[0] != N:
            raise ValueError("y must be (N,) or (N, k) with the same N as X")
        if kx != ky:
            raise ValueError("X and y must both be host arrays or both be device tensors")
        k = 1 if len(sy) == 1 else sy[1]
        if self.lengthscale.size not in (1, d):
            raise ValueError("lengthscale must be scalar or have d entries")
        if paths[0] is not None and paths[0].shape[0] != N:
            raise ValueError(f"path_ids must be ({N},), one id per observation")
        if paths[2] is not None and paths[2].size not in (1, d):
            raise ValueError("path_lengthscale must be scalar or have d entries")
        self._set_noise_weights(noise_weights, N, kx)  # (refused: the model is as it was)
        self._set_observation_kinds(kinds, derivative_noise)
        self._set_path_groups(*paths)
        self._set_basis(basis)
        self.derivative_noise = 0.0 if kinds is None else float(derivative_noise)
        refused = self._refusal_keeps_fit(basis, self._fit_state())
        self._y1d = len(sy) == 1
        self._N, self._d, self._k = N, d, k
        self._alpha = None
        self._fitted = False
        ls = self.lengthscale
        jitter = self.jitter
        info = C.c_int64(0)
        for _ in range(max(1, self.max_tries)):
            rc = self._lib.gpx_fit(self._h, px, py, N, d, k, _abi.dptr(ls), ls.size, self.variance,
                                   self.noise, jitter, kx, C.byref(info))
            try:
                self._check(rc)
            except _abi.GpxError as e:
                refused(e)
                raise
            self.info_ = int(info.value)
            if self.info_ == 0:
                break
            jitter = max(jitter, 1e-12 * self.variance) * 10.0
        else:
            raise np.linalg.LinAlgError(self._not_pd(N))
        self.jitter_used_ = jitter
        self._fitted = True
        self._basis_fit = basis
        ld = C.c_double(0.0)
        self._check(self._lib.gpx_logdet(self._h, C.byref(ld)))
        self.log_det_ = float(ld.value)
        return self

    def _side_input(self, a, kind, dev):
        """(m,) int32 kinds or path ids of appended rows -> pointer and keepalive, where ``kind`` says the rows live"""
        if a is None:
            return None, None
        if kind == _abi.MEM_DEVICE:
            import torch
            t = torch.from_numpy(a).to(dev)
            torch.cuda.current_stream(dev).synchronize()
            return C.c_void_p(t.data_ptr()), t
        return C.c_void_p(a.ctypes.data), a

    def _query_ids(self, path_ids, M, kind, dev):
        """``path_ids`` of M query points -> pointer and keepalive of (M,) int32 ids where the query points live: an int
        names one path for every point, an array or tensor gives one id per point (-1: the cluster mean ``f``)."""
        if _is_torch(path_ids):
            path_ids = path_ids.detach().cpu().numpy()
        a = np.asarray(path_ids)
        if a.dtype.kind not in "iu":
            raise ValueError("path_ids must be integers (-1: the cluster mean, p >= 0: the path p itself)")
        if a.ndim == 0:
            a = np.full((M,), int(a))
        if a.shape != (M,):
            raise ValueError(f"path_ids must be an int or ({M},), one id per query point")
        if a.size and (a.min() < np.iinfo(np.int32).min or a.max() > np.iinfo(np.int32).max):
            raise ValueError("path_ids must fit int32")
        return self._side_input(np.ascontiguousarray(a, dtype=np.int32), kind, dev)

    def update(self, X_new, y_new, noise_weights=None, derivatives=None, path_ids=None):
        """Append observations to the fitted model without factorising the old ones again (``gpx_append``): afterwards
        the model is, to rounding, what ``fit`` of the concatenated data with the same hyper-parameters and the jitter
        the fit needed would be.  Inputs as for :meth:`fit`: NumPy arrays or device tensors, both of the same kind,
        ``y_new`` 1-D or (m, k) as fitted.  Only the rows of the new points and the last, partly filled panel of the
        Cholesky factor are computed (include/gpx.h); :meth:`reserve` keeps the factor from being moved.  Raises
        ``numpy.linalg.LinAlgError`` when the kernel matrix with the new points is not positive definite: the model is
        then unchanged (the previous fit, every call valid).  float64 / float32 models on one device.
        ``noise_weights`` (m,): the new points' noise weights (``gpx_append_weighted``), of the same kind as ``X_new``;
        None appends with weight 1, on a weighted model too.  Returns ``self``.

        On a fit with path ids, ``path_ids`` (m,) ints >= -1 (as :meth:`fit`'s) name the path of every new row — a new
        id is a new path, an id the fit holds already brings more points of that path — and the rows go through
        ``gpx_append_rows``; ``path_ids_`` then has N + m entries.  Without the keyword such a fit stays refused: the
        caller has to say which path the rows belong to.  On a fit made with ``derivatives=`` (an empty one included),
        ``derivatives = (Xd, dims, yd)`` appends the m value rows followed by the Nd derivative rows (``X_new`` may be
        (0, d)); ``noise_weights`` may have length m or m + Nd, as in :meth:`fit`, and ``observation_kinds_``,
        ``alpha_`` and ``noise_weights_`` cover all rows afterwards.  ``ValueError`` before any library call:
        ``path_ids`` on a fit without path ids, ``derivatives`` on a fit made without the keyword, or both at once."""
        if not self._fitted:
            raise RuntimeError("update() before a successful fit()")
        if path_ids is not None and derivatives is not None:
            raise ValueError("path_ids cannot be combined with derivatives=: no builder evaluates both")
        if path_ids is not None and not self._groups_set:
            raise ValueError("path_ids given, but the model was fitted without path ids")
        if derivatives is not None and not self._kinds_set:
            raise ValueError("derivatives given, but the model was fitted without derivatives= (pass an empty "
                             "derivatives=(Xd, dims, yd) to fit() to allow derivative rows later)")
        kinds = None
        if derivatives is not None:
            X_new, y_new, noise_weights, kinds = self._with_derivatives(X_new, y_new, derivatives, noise_weights)
        px, kx, keepx, devx, sx = self._as_input(X_new, "X_new")
        py, ky, keepy, devy, sy = self._as_input(y_new, "y_new")
        if len(sx) != 2 or sx[1] != self._d:
            raise ValueError(f"X_new must be (m, {self._d})")
        m = sx[0]
        if self._y1d:
            ok = len(sy) == 1 or (len(sy) == 2 and sy[1] == 1)
        else:
            ok = len(sy) == 2 and sy[1] == self._k
        if not ok or sy[0] != m:
            raise ValueError("y_new must be (m,)" if self._y1d else f"y_new must be (m, {self._k})")
        if kx != ky:
            raise ValueError("X_new and y_new must both be host arrays or both be device tensors")
        pw, keepw = self._weights_input(noise_weights, m, kx, "noise_weights", "X_new")
        ids = None if path_ids is None else check_path_args(path_ids, 0.0, None, n=m)[0]
        if m == 0:
            return self
        info = C.c_int64(0)
        if kinds is not None or ids is not None:
            pk, keepk = self._side_input(kinds, kx, devx)
            pg, keepg = self._side_input(ids, kx, devx)
            self._check(self._lib.gpx_append_rows(self._h, px, py, pw, pk, pg, m, kx, C.byref(info)))
        elif pw is None:
            self._check(self._lib.gpx_append(self._h, px, py, m, kx, C.byref(info)))
        else:
            self._check(self._lib.gpx_append_weighted(self._h, px, py, pw, m, kx, C.byref(info)))
        if info.value != 0:
            raise np.linalg.LinAlgError(
                f"kernel matrix with the new points not positive definite (first bad pivot {info.value}): the model "
                f"is unchanged (N = {self._N}); refit the concatenated data with a larger jitter")
        self._N += m
        self._alpha = None
        ld = C.c_double(0.0)
        self._check(self._lib.gpx_logdet(self._h, C.byref(ld)))
        self.log_det_ = float(ld.value)
        return self

    def reserve(self, n):
        """Lay the factor out for up to ``n`` points (``gpx_reserve``) at the next :meth:`fit` or :meth:`update`:
        updates within it happen in place, nothing is reallocated or copied.  0 = what the fit itself needs: it takes an
        earlier reservation back for the fits that follow, on a fitted model too (any other ``n`` below the number of
        points the model holds is refused)."""
        self._check(self._lib.gpx_reserve(self._h, int(n)))
        return self

    def remove(self, start=None, stop=None, path_ids=None):
        """Take observations out of the fitted model without factorising the others again (``gpx_remove_rows``):
        afterwards the model is, to rounding, what ``fit`` of the remaining rows (in their order, with their own noise
        weights, kinds and path ids) with the same hyper-parameters and the jitter the fit needed would be.

        ``remove(start, stop)`` takes rows ``[start, stop)``; ``remove(indices)`` any integer index array or sequence
        (sorted, deduplicated and split into runs, which are removed from the highest down); ``remove(path_ids=[3, 7])``,
        on a fit with path ids, every row of those paths.  A removed path id is afterwards an id the fit has never seen.
        No covariance is evaluated, so every kind of fit is served (plain, weighted, with ``derivatives=``, with
        ``path_ids=``); ``noise_weights_``, ``observation_kinds_``, ``path_ids_``, ``alpha_`` and ``log_det_`` follow.
        The factor is compacted inside its buffer (a later :meth:`update` reuses the room).  Rows at the end cost nothing;
        the cost grows with the number of rows BELOW the removed ones, and taking out more than roughly N / 12 rows at
        the front costs as much as a new :meth:`fit`.  float64 / float32 models on one device.  Returns ``self``.

        ``ValueError`` before anything is touched: indices that are not integers or out of range, removing every row,
        ``path_ids=`` on a fit without path ids, both forms at once; ``RuntimeError`` before a fit."""
        if not self._fitted:
            raise RuntimeError("remove() before a successful fit()")
        N = self._N
        if path_ids is not None:
            if start is not None or stop is not None:
                raise ValueError("give rows (start, stop / indices) or path_ids=, not both")
            if not self._groups_set:
                raise ValueError("path_ids given, but the model was fitted without path ids")
            if _is_torch(path_ids):
                path_ids = path_ids.detach().cpu().numpy()
            want = np.atleast_1d(np.asarray(path_ids))
            if want.ndim != 1 or want.dtype.kind not in "iu" or np.any(want < 0):
                raise ValueError("path_ids must be integers >= 0")
            idx = np.flatnonzero(np.isin(self.path_ids_, want))
        elif start is None:
            raise ValueError("remove() needs rows (start, stop / indices) or path_ids=")
        elif stop is not None:
            for v in (start, stop):
                if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                    raise ValueError("start and stop must be integers")
            if not 0 <= start <= stop <= N:
                raise ValueError(f"rows [{start}, {stop}) do not lie inside the {N} fitted rows")
            idx = np.arange(int(start), int(stop))
        else:
            if _is_torch(start):
                start = start.detach().cpu().numpy()
            idx = np.atleast_1d(np.asarray(start))
            if idx.ndim != 1 or (idx.size and idx.dtype.kind not in "iu"):
                raise ValueError("indices must be a 1-D array of integers")
            idx = idx.astype(np.int64)
            if idx.size and (idx.min() < 0 or idx.max() >= N):
                raise ValueError(f"indices must lie in [0, {N})")
            idx = np.unique(idx)
        if idx.size >= N:
            raise ValueError("remove() cannot take out every row: a model keeps at least one observation")
        if idx.size == 0:
            return self
        # runs of consecutive indices, highest first: the rows below a run keep their numbers while it is removed
        cuts = np.flatnonzero(np.diff(idx) != 1) + 1
        runs = [(int(r[0]), int(r.size)) for r in np.split(idx, cuts)]
        for first, count in reversed(runs):
            info = C.c_int64(0)
            self._alpha = None
            try:
                self._check(self._lib.gpx_remove_rows(self._h, first, count, C.byref(info)))
            except _abi.GpxError as e:
                # a refusal comes before anything is touched; any other failure leaves the handle without a fit
                self._fitted = e.code in (_abi.E_ARG, _abi.E_UNSUPPORTED)
                raise
            if info.value != 0:
                self._fitted = False
                raise np.linalg.LinAlgError(
                    f"non-positive pivot {info.value} while removing rows (non-finite numbers in the factor?): the "
                    f"model is left without a fit; fit the remaining data again")
            self._N -= count
        ld = C.c_double(0.0)
        self._check(self._lib.gpx_logdet(self._h, C.byref(ld)))
        self.log_det_ = float(ld.value)
        return self

    def fit_predict(self, X, y, Xs, include_noise=False, noise_weights=None, derivatives=None, derivative_noise=0.0,
                    path_ids=None, path_variance=0.0, path_lengthscale=None, basis=None):
        """``fit(X, y)`` and ``predict(Xs)`` (mean and variance) as ONE factorisation pass: the cross-kernel rows
        of the query points ride through the blocked Cholesky as bordered rows (``gpx_fit_predict``), so the
        variance solve is part of the trailing updates instead of a pass of its own — the small-N schedule
        (N = 8192: the updates' idle CUs take the work).  The model is fitted afterwards as after ``fit``.
        On a shard or a device group every rank's slice of the query points rides through ITS part of the sharded
        factorisation (collective: every rank of a shard makes the call).  ``dtype="mixed"`` takes the two calls.
        ``noise_weights``, ``derivatives``, ``derivative_noise`` and the ``path_*`` keywords as for :meth:`fit` (with
        path ids the prediction is the posterior of the cluster mean ``f``); ``basis`` as for :meth:`fit` too (the
        coefficients are solved between the factorisation and the prediction); ``include_noise`` as for
        :meth:`predict`."""
        self._check_basis(basis)
        paths = check_path_args(path_ids, path_variance, path_lengthscale, derivatives=derivatives)
        X, y, noise_weights, kinds = self._with_derivatives(X, y, derivatives, noise_weights)

        def two_calls():
            return self._fit_rows(X, y, noise_weights, kinds, derivative_noise, paths, basis).predict(
                Xs, include_noise=include_noise)

        fused = self.dtype in ("float64", "float32")
        pq, kq, keepq, devq, sq = self._as_input(Xs, "Xs")
        px, kx, keepx, devx, sx = self._as_input(X, "X")
        py, ky, keepy, devy, sy = self._as_input(y, "y")
        if not fused or len(sq) != 2 or not (kx == ky == kq):
            return two_calls()
        if len(sx) != 2:
            raise ValueError("X must be (N, d)")
        N, d = sx
        if len(sy) not in (1, 2) or sy[0] != N:
            raise ValueError("y must be (N,) or (N, k) with the same N as X")
        if sq[1] != d:
            raise ValueError(f"Xs must be (M, {d})")
        k = 1 if len(sy) == 1 else sy[1]
        if self.lengthscale.size not in (1, d):
            raise ValueError("lengthscale must be scalar or have d entries")
        M = sq[0]
        if paths[0] is not None and paths[0].shape[0] != N:
            raise ValueError(f"path_ids must be ({N},), one id per observation")
        if paths[2] is not None and paths[2].size not in (1, d):
            raise ValueError("path_lengthscale must be scalar or have d entries")
        self._set_noise_weights(noise_weights, N, kx)
        self._set_observation_kinds(kinds, derivative_noise)
        self._set_path_groups(*paths)
        self._set_basis(basis)
        refused = self._refusal_keeps_fit(basis, self._fit_state())
        self._y1d = len(sy) == 1
        self._N, self._d, self._k = N, d, k
        self._alpha = None
        self._fitted = False
        mshape = (M,) if self._y1d else (M, k)
        if devq is not None:
            import torch
            tdt = torch.float32 if self.dtype == "float32" else torch.float64
            mean = torch.empty(mshape, dtype=tdt, device=devq)
            var = torch.empty((M,), dtype=tdt, device=devq)
            pm, pv = C.c_void_p(mean.data_ptr()), C.c_void_p(var.data_ptr())
        else:
            mean = np.empty(mshape, dtype=self._np_dtype)
            var = np.empty((M,), dtype=self._np_dtype)
            pm, pv = C.c_void_p(mean.ctypes.data), C.c_void_p(var.ctypes.data)
        ls = self.lengthscale
        jitter = self.jitter
        info = C.c_int64(0)
        for _ in range(max(1, self.max_tries)):
            rc = self._lib.gpx_fit_predict(self._h, px, py, N, d, k, _abi.dptr(ls), ls.size, self.variance, self.noise,
                                           jitter, pq, M, pm, pv, kx, C.byref(info))
            if rc == _abi.E_NOMEM or (rc == _abi.E_UNSUPPORTED and kinds is None and paths[0] is None
                                      and basis is None):
                # the library's own limits decide (its batch cap honours GPX_PRED_BATCH; M more bordered rows of K and
                # of the panel buffers may not fit beside the factor): the documented fallback is the two calls
                # (with kinds set, GPX_E_UNSUPPORTED is the refusal of the model itself: raised below)
                return two_calls()
            try:
                self._check(rc)
            except _abi.GpxError as e:
                refused(e)
                raise
            self.info_ = int(info.value)
            if self.info_ == 0:
                break
            jitter = max(jitter, 1e-12 * self.variance) * 10.0
        else:
            raise np.linalg.LinAlgError(self._not_pd(N))
        self.jitter_used_ = jitter
        self._fitted = True
        self._basis_fit = basis
        ld = C.c_double(0.0)
        self._check(self._lib.gpx_logdet(self._h, C.byref(ld)))
        self.log_det_ = float(ld.value)
        if include_noise:
            var += self.noise
        return mean, var

    def predict(self, Xs, return_var=True, include_noise=False, return_cov=False, path_ids=None):
        """Posterior at the query points ``Xs`` (M, d): ``mean`` ((M,) for a 1-D ``y``, else (M, k)) and, with
        ``return_var``, the per-point variance (M,).  ``return_cov=True`` returns ``(mean, cov)`` instead, ``cov`` the
        joint (M, M) posterior covariance of the latent function (``gpx_predict_cov``: one SYRK more than the variance;
        the same for every target column), with ``noise`` on its diagonal when ``include_noise``.  ``include_noise``
        adds ``noise`` times 1 also on a model fitted with ``noise_weights``: a query point has no weight of its own
        (scale the latent variance yourself for another one).  NumPy in, NumPy out; a device tensor in, device tensors
        out.

        ``path_ids`` (a model fitted with path ids; ``gpx_predict_paths`` / ``gpx_predict_cov_paths``): an int, or one
        int per query point.  ``-1`` asks for the cluster mean ``f``, as without the argument; ``p >= 0`` asks for the
        path ``p`` itself, ``f + g_p`` — where the path was, is or will be, conditioned on its own observations too.
        An id no observation carries is a path nobody has seen: the mean of ``f``, the variance of ``f`` plus the
        prior ``path_variance``.  Ids may be mixed in one call; the joint covariance couples points of one path
        through ``g_p`` as well."""
        if not self._fitted:
            raise RuntimeError("predict() before a successful fit()")
        pq, kq, keepq, devq, sq = self._as_input(Xs, "Xs")
        if len(sq) != 2 or sq[1] != self._d:
            raise ValueError(f"Xs must be (M, {self._d})")
        M = sq[0]
        mshape = (M,) if self._y1d else (M, self._k)
        pg, keepg = (None, None) if path_ids is None else self._query_ids(path_ids, M, kq, devq)
        if return_cov:
            mean, cov = self._empty(mshape, devq), self._empty((M, M), devq)
            if pg is None:
                self._check(self._lib.gpx_predict_cov(self._h, pq, M, self._ptr(mean), self._ptr(cov), kq))
            else:
                self._check(self._lib.gpx_predict_cov_paths(self._h, pq, pg, M, self._ptr(mean), self._ptr(cov), kq))
            if include_noise:
                if devq is not None:
                    cov.diagonal().add_(self.noise)
                else:
                    cov[np.diag_indices(M)] += self.noise
            return mean, cov
        if devq is not None:
            import torch
            tdt = torch.float32 if self.dtype == "float32" else torch.float64
            mean = torch.empty(mshape, dtype=tdt, device=devq)
            var = torch.empty((M,), dtype=tdt, device=devq) if return_var else None
            pm = C.c_void_p(mean.data_ptr())
            pv = C.c_void_p(var.data_ptr()) if return_var else None
        else:
            mean = np.empty(mshape, dtype=self._np_dtype)
            var = np.empty((M,), dtype=self._np_dtype) if return_var else None
            pm = C.c_void_p(mean.ctypes.data)
            pv = C.c_void_p(var.ctypes.data) if return_var else None
        if pg is None:
            self._check(self._lib.gpx_predict(self._h, pq, M, pm, pv, kq))
        else:
            self._check(self._lib.gpx_predict_paths(self._h, pq, pg, M, pm, pv, kq))
        if not return_var:
            return mean
        if include_noise:
            var += self.noise
        return mean, var

    def predict_gradient(self, Xs, return_var=True, with_value=False, path_ids=None):
        """Gradient of the posterior with respect to the query points ``Xs`` (M, d) (``gpx_predict_grad``): ``dmean``
        ((M, d) for a 1-D ``y``, else (M, d, k)) and, with ``return_var``, ``dvar`` (M, d), the latent variance of each
        partial derivative (no noise term: white noise has no derivative).  ``with_value=True`` returns
        ``(mean, var, dmean, dvar)`` from the same pass (``(mean, dmean)`` without ``return_var``), ``mean`` and ``var``
        shaped as :meth:`predict`'s.  Without variances the device contracts the kernel derivative with the cached
        ``alpha`` matrix-free (no solve).  NumPy in, NumPy out; a device tensor in, device tensors out.  ``path_ids``
        as :meth:`predict`'s (``gpx_predict_grad_paths``): the gradient of ``f + g_p`` for ids ``>= 0``."""
        if not self._fitted:
            raise RuntimeError("predict_gradient() before a successful fit()")
        pq, kq, keepq, devq, sq = self._as_input(Xs, "Xs")
        if len(sq) != 2 or sq[1] != self._d:
            raise ValueError(f"Xs must be (M, {self._d})")
        M, d, k = sq[0], self._d, self._k
        dmean = self._empty((M, d) if self._y1d else (M, d, k), devq)
        dvar = self._empty((M, d), devq) if return_var else None
        mean = self._empty((M,) if self._y1d else (M, k), devq) if with_value else None
        var = self._empty((M,), devq) if with_value and return_var else None
        p = lambda a: None if a is None else self._ptr(a)  # noqa: E731
        if path_ids is None:
            self._check(self._lib.gpx_predict_grad(self._h, pq, M, p(mean), p(var), p(dmean), p(dvar), kq))
        else:
            pg, keepg = self._query_ids(path_ids, M, kq, devq)
            self._check(self._lib.gpx_predict_grad_paths(self._h, pq, pg, M, p(mean), p(var), p(dmean), p(dvar), kq))
        if with_value:
            return (mean, var, dmean, dvar) if return_var else (mean, dmean)
        return (dmean, dvar) if return_var else dmean

    def predict_hessian(self, Xs, return_var=True, path_ids=None, full=False):
        """Second derivatives of the posterior with respect to the query points ``Xs`` (M, d) (``gpx_predict_hess``):
        ``hmean`` ((M, D2) for a 1-D ``y``, else (M, D2, k)) over the ``D2 = d (d + 1) / 2`` pairs ``(i, j)``, ``i <= j``,
        row-major, and, with ``return_var``, ``hvar`` (M, D2), the latent variance of each second derivative (raw, not
        clamped).  ``full=True`` expands both on the host to the symmetric (M, d, d[, k]) and (M, d, d).  Without
        variances the device contracts the kernel's second derivative with the cached ``alpha`` matrix-free (no solve).
        RBF and Matern-5/2 only: Matern-3/2 and Matern-1/2 paths have no second derivative, and ``GpxError`` says so; so
        it does for ``d > 8``, a fit with a basis, ``dtype="mixed"`` and sharded handles.  NumPy in, NumPy out; a device
        tensor in, device tensors out.  ``path_ids`` as :meth:`predict`'s (``gpx_predict_hess_paths``): the second
        derivatives of ``f + g_p`` for ids ``>= 0``."""
        if not self._fitted:
            raise RuntimeError("predict_hessian() before a successful fit()")
        pq, kq, keepq, devq, sq = self._as_input(Xs, "Xs")
        if len(sq) != 2 or sq[1] != self._d:
            raise ValueError(f"Xs must be (M, {self._d})")
        M, d, k = sq[0], self._d, self._k
        d2 = d * (d + 1) // 2
        hmean = self._empty((M, d2) if self._y1d else (M, d2, k), devq)
        hvar = self._empty((M, d2), devq) if return_var else None
        pv = None if hvar is None else self._ptr(hvar)
        if path_ids is None:
            self._check(self._lib.gpx_predict_hess(self._h, pq, M, self._ptr(hmean), pv, kq))
        else:
            pg, keepg = self._query_ids(path_ids, M, kq, devq)
            self._check(self._lib.gpx_predict_hess_paths(self._h, pq, pg, M, self._ptr(hmean), pv, kq))
        if full:
            # pair number of (i, j): the upper triangle row-major, mirrored below the diagonal
            idx = np.zeros((d, d), dtype=np.int64)
            idx[np.triu_indices(d)] = np.arange(d2)
            idx = np.maximum(idx, idx.T).reshape(-1)
            if devq is not None:
                import torch
                idx = torch.from_numpy(idx).to(devq)
            hmean = hmean[:, idx].reshape((M, d, d) + tuple(hmean.shape[2:]))
            hvar = None if hvar is None else hvar[:, idx].reshape(M, d, d)
        return (hmean, hvar) if return_var else hmean

    def score_blocks(self, Xs, ys, block, include_noise=True, return_parts=False, on_bad="raise", noise_weights=None):
        """Joint log predictive density of whole blocks of query points (``gpx_score_blocks``): ``Xs`` (G * block, d)
        holds G blocks of ``block`` consecutive points (a path = a block, 1 <= block <= 64), ``ys`` their observed
        targets ((G * block,) for a 1-D ``y``, else (G * block, k)).  Returns ``logp`` ((G,) for a 1-D fit, else
        (G, k)): the log-density of each block's targets under the joint posterior of its points — of noisy
        observations with ``include_noise`` (``noise`` on the diagonal), else of the latent function.  With
        ``return_parts``: ``(logp, maha, logdet)``, ``maha`` shaped as ``logp`` and ``logdet`` (G,), so that
        ``logp = -maha / 2 - logdet / 2 - block / 2 log 2 pi``.  Only the block-diagonal of the joint covariance is
        ever formed, and a block's numbers do not depend on the other blocks of the call.  A block whose covariance
        is not positive definite (possible without the noise term) raises ``numpy.linalg.LinAlgError`` naming the
        first such block; ``on_bad="nan"`` returns the arrays instead, that block's entries NaN and
        ``score_info_`` its 1-based index.  ``noise_weights`` (G * block,), of the same kind as ``Xs``: query point i
        gets ``noise * w_i`` on the diagonal instead of ``noise`` (``gpx_score_blocks_weighted``; nothing without
        ``include_noise``).  On a model fitted with ``path_ids`` every block is a NEW path of the hierarchical model: its
        covariance is the posterior of ``f`` plus ``path_variance k(., .; path_lengthscale)``, so a path that runs beside
        the cluster mean is one deviation, not ``block`` independent surprises.  NumPy in, NumPy out; device tensors in,
        device tensors out."""
        if not self._fitted:
            raise RuntimeError("score_blocks() before a successful fit()")
        if on_bad not in ("raise", "nan"):
            raise ValueError("on_bad must be 'raise' or 'nan'")
        Lg = int(block)
        if not 1 <= Lg <= 64:
            raise ValueError("block must be between 1 and 64")
        pq, kq, keepq, devq, sq = self._as_input(Xs, "Xs")
        py, ky, keepy, devy, sy = self._as_input(ys, "ys")
        if len(sq) != 2 or sq[1] != self._d:
            raise ValueError(f"Xs must be (G * block, {self._d})")
        M = sq[0]
        if M == 0 or M % Lg:
            raise ValueError(f"Xs must hold whole blocks of {Lg} points, has {M} rows")
        if self._y1d:
            ok = len(sy) == 1 or (len(sy) == 2 and sy[1] == 1)
        else:
            ok = len(sy) == 2 and sy[1] == self._k
        if not ok or sy[0] != M:
            raise ValueError("ys must be (G * block,)" if self._y1d else f"ys must be (G * block, {self._k})")
        if kq != ky:
            raise ValueError("Xs and ys must both be host arrays or both be device tensors")
        G = M // Lg
        oshape = (G,) if self._y1d else (G, self._k)
        logp = self._empty(oshape, devq)
        maha = self._empty(oshape, devq) if return_parts else None
        logdet = self._empty((G,), devq) if return_parts else None
        p = lambda a: None if a is None else self._ptr(a)  # noqa: E731
        pw, keepw = self._weights_input(noise_weights, M, kq, "noise_weights", "Xs")
        info = C.c_int64(0)
        diag_add = self.noise if include_noise else 0.0
        if pw is None:
            self._check(self._lib.gpx_score_blocks(self._h, pq, py, G, Lg, diag_add, p(logp), p(maha), p(logdet), kq,
                                                   C.byref(info)))
        else:
            self._check(self._lib.gpx_score_blocks_weighted(self._h, pq, py, pw, G, Lg, diag_add, p(logp), p(maha),
                                                            p(logdet), kq, C.byref(info)))
        self.score_info_ = int(info.value)
        if self.score_info_ and on_bad == "raise":
            raise np.linalg.LinAlgError(
                f"block {self.score_info_ - 1} (the first of its kind) has a joint posterior covariance that is not "
                f"positive definite; score with include_noise=True or on_bad='nan'")
        return (logp, maha, logdet) if return_parts else logp

    def forecast_blocks(self, Xo, yo, Xp, blocks=None, include_noise=True, return_cov=True, return_logp=False,
                        on_bad="raise"):
        """Forecast of partly observed new paths (``gpx_forecast_blocks``): ``Xo`` (G * Lo, d) holds the Lo observed
        points of each of G paths, ``yo`` their targets ((G * Lo,) for a 1-D ``y``, else (G * Lo, k)), ``Xp`` (G * Lp, d)
        the Lp points to forecast per path; ``blocks`` = G (None: one path), Lo + Lp <= 64.  Each path is a new draw of
        the model — the posterior of ``f`` plus, on a fit with ``path_ids``, its own deviation ``g`` — conditioned on
        its observed points (``noise`` on their diagonal with ``include_noise``).  Returns ``(mean, cov)``: the forecast
        mean ((G * Lp,) or (G * Lp, k)) and the latent joint covariance (G, Lp, Lp), shared by the targets; with
        ``return_cov=False`` ``(mean, var)``, ``var`` (G * Lp,) its diagonal; with ``return_logp`` a third entry, the
        joint log-density of each observed prefix ((G,) or (G, k): :meth:`score_blocks` of those points).  A path whose
        conditioning matrix is not positive definite raises ``numpy.linalg.LinAlgError``; ``on_bad="nan"`` returns NaN
        for it instead and ``forecast_info_`` its 1-based index.  NumPy in, NumPy out; device tensors in, device tensors
        out."""
        if not self._fitted:
            raise RuntimeError("forecast_blocks() before a successful fit()")
        if on_bad not in ("raise", "nan"):
            raise ValueError("on_bad must be 'raise' or 'nan'")
        G = 1 if blocks is None else int(blocks)
        if G < 1:
            raise ValueError("blocks must be >= 1")
        po, ko, keepo, devo, so = self._as_input(Xo, "Xo")
        py, ky, keepy, devy, sy = self._as_input(yo, "yo")
        pp, kp, keepp, devp, sp = self._as_input(Xp, "Xp")
        if len(so) != 2 or so[1] != self._d or len(sp) != 2 or sp[1] != self._d:
            raise ValueError(f"Xo must be (G * Lo, {self._d}) and Xp (G * Lp, {self._d})")
        if so[0] == 0 or sp[0] == 0 or so[0] % G or sp[0] % G:
            raise ValueError(f"Xo and Xp must hold {G} whole blocks each, have {so[0]} and {sp[0]} rows")
        Lo, Lp = so[0] // G, sp[0] // G
        if Lo + Lp > 64:
            raise ValueError(f"a block has Lo + Lp = {Lo} + {Lp} points, at most 64")
        if self._y1d:
            ok = len(sy) == 1 or (len(sy) == 2 and sy[1] == 1)
        else:
            ok = len(sy) == 2 and sy[1] == self._k
        if not ok or sy[0] != G * Lo:
            raise ValueError("yo must be (G * Lo,)" if self._y1d else f"yo must be (G * Lo, {self._k})")
        if not (ko == ky == kp):
            raise ValueError("Xo, yo and Xp must all be host arrays or all be device tensors")
        d = self._d
        if devo is not None:  # each block: its observed points, then its points to forecast
            import torch
            Xb = torch.cat([keepo.reshape(G, Lo, d), keepp.reshape(G, Lp, d)], dim=1).reshape(G * (Lo + Lp), d).contiguous()
            torch.cuda.current_stream(devo).synchronize()
        else:
            Xb = np.ascontiguousarray(np.concatenate([keepo.reshape(G, Lo, d), keepp.reshape(G, Lp, d)], axis=1)
                                      .reshape(G * (Lo + Lp), d))
        mean = self._empty((G * Lp,) if self._y1d else (G * Lp, self._k), devo)
        cov = self._empty((G, Lp, Lp), devo) if return_cov else None
        var = None if return_cov else self._empty((G * Lp,), devo)
        logp = self._empty((G,) if self._y1d else (G, self._k), devo) if return_logp else None
        p = lambda a: None if a is None else self._ptr(a)  # noqa: E731
        info = C.c_int64(0)
        self._check(self._lib.gpx_forecast_blocks(self._h, self._ptr(Xb), py, G, Lo, Lp, self.noise if include_noise else 0.0,
                                                  p(mean), p(cov), p(var), p(logp), ko, C.byref(info)))
        self.forecast_info_ = int(info.value)
        if self.forecast_info_ and on_bad == "raise":
            raise np.linalg.LinAlgError(
                f"block {self.forecast_info_ - 1} (the first of its kind) has a conditioning matrix that is not positive "
                f"definite; forecast with include_noise=True or on_bad='nan'")
        out = (mean, cov if return_cov else var)
        return out + (logp,) if return_logp else out

    def _empty(self, shape, dev):
        """uninitialised output of the model's element type: on the device `dev` (torch), or NumPy when None"""
        if dev is not None:
            import torch
            return torch.empty(shape, dtype=torch.float32 if self.dtype == "float32" else torch.float64, device=dev)
        return np.empty(shape, dtype=self._np_dtype)

    @staticmethod
    def _ptr(a):
        return C.c_void_p(a.data_ptr() if _is_torch(a) else a.ctypes.data)

    def sample_y(self, Xs, n_samples=1, random_state=0, include_noise=False, z=None, jitter=None, max_tries=8,
                 path_ids=None):
        """Joint samples of the posterior at ``Xs`` (M, d), shaped as scikit-learn's ``sample_y``: (M, S) for a 1-D
        ``y``, (M, k, S) otherwise, S = ``n_samples``.  Sample s of target c is ``mean[:, c] + L_S z[s, :, c]`` with
        ``L_S = chol(cov + (diag_add + j) I)`` (``gpx_sample_posterior``), ``diag_add = noise`` when ``include_noise``.
        ``z`` (S, M, k) are the caller's standard normals; without them the device draws them from the Philox stream
        ``random_state`` (an int; include/gpx.h specifies it, so a sample depends only on the seed, its index, M and k).
        ``jitter`` (None: the model's jitter for float64, 1e-6 variance for float32) is multiplied by 10 after a failed
        factorisation, at most ``max_tries`` attempts; the value that worked is ``sample_jitter_``.  Raises
        ``numpy.linalg.LinAlgError`` when none did.  NumPy in, NumPy out; a device tensor in, a device tensor out.
        ``path_ids`` as :meth:`predict`'s (``gpx_sample_posterior_paths``): samples of the paths themselves."""
        if not self._fitted:
            raise RuntimeError("sample_y() before a successful fit()")
        pq, kq, keepq, devq, sq = self._as_input(Xs, "Xs")
        if len(sq) != 2 or sq[1] != self._d:
            raise ValueError(f"Xs must be (M, {self._d})")
        M, k, S = sq[0], self._k, int(n_samples)
        if S < 1:
            raise ValueError("n_samples must be >= 1")
        seed = 0 if random_state is None else int(random_state) & 0xFFFFFFFFFFFFFFFF
        if jitter is None:
            jitter = 1e-6 * self.variance if self.dtype == "float32" else self.jitter
        pz, keepz = None, None
        if z is not None:
            if devq is not None:            # the normals go where the queries are
                import torch
                keepz = torch.as_tensor(z, device=devq).to(torch.float32 if self.dtype == "float32" else torch.float64)
                keepz = keepz.contiguous()
                n = keepz.numel()
                torch.cuda.current_stream(devq).synchronize()
            else:
                if _is_torch(z):
                    z = z.detach().cpu().numpy()
                keepz = np.ascontiguousarray(z, dtype=self._np_dtype)
                n = keepz.size
            if n != S * M * k:
                raise ValueError(f"z must hold (n_samples, M, k) = ({S}, {M}, {k}) standard normals")
            pz = self._ptr(keepz)
        out = self._empty((S, M, k), devq)
        used, info = C.c_double(0.0), C.c_int64(0)
        diag_add = self.noise if include_noise else 0.0
        if path_ids is None:
            self._check(self._lib.gpx_sample_posterior(self._h, pq, M, S, seed, pz, diag_add, float(jitter), int(max_tries),
                                                       self._ptr(out), C.byref(used), C.byref(info), kq))
        else:
            pg, keepg = self._query_ids(path_ids, M, kq, devq)
            self._check(self._lib.gpx_sample_posterior_paths(self._h, pq, pg, M, S, seed, pz, diag_add, float(jitter),
                                                             int(max_tries), self._ptr(out), C.byref(used),
                                                             C.byref(info), kq))
        if info.value != 0:
            raise np.linalg.LinAlgError(
                f"posterior covariance not positive definite (first bad pivot {info.value}) with jitter up to "
                f"{used.value:.3g} after {max_tries} attempts")
        self.sample_jitter_ = float(used.value)
        if self._y1d:
            res = out[:, :, 0].T
        else:
            res = out.permute(1, 2, 0) if devq is not None else out.transpose(1, 2, 0)
        return res.contiguous() if devq is not None else np.ascontiguousarray(res)

    def sample_functions(self, n_samples, n_features=4096, random_state=0, z=None):
        """Draw ``n_samples`` posterior sample FUNCTIONS once; evaluate them anywhere, as often as needed
        (:class:`PosteriorFunctions`; ``gpx_pathwise_draw`` / ``gpx_pathwise_eval``, pathwise conditioning after Wilson
        et al. 2020).  Where :meth:`sample_y` builds and factorises an M x M covariance for every new ``Xs``, the draw here
        costs one solve against the factor the fit already holds, and an evaluation one matrix-free pass over
        ``k(Xs, X)``: M can be millions, and evaluating again elsewhere gives the same functions.

        What is exact and what is not: the conditioning on the data (the update ``k(x, X) K_y^-1 (y - f~(X) - eps)``) is
        exact.  The prior draw ``f~`` is approximate: a sum of ``n_features`` random Fourier features whose covariance
        misses the kernel by O(1 / sqrt(n_features)).  ``profiles/pathwise_bias.json`` tabulates the resulting bias of
        the posterior variance per family for 256, 1024 and 4096 features.

        ``random_state`` (an int) seeds the device's Philox stream; ``z`` instead supplies the call's
        ``F (d + q) + S k (2 F + N)`` standard normals in the layout include/gpx.h specifies.  Sample s depends on
        (seed, s, n_features, N, d, k, kernel) only.  A model that is fitted again, updated or reduced drops the draw:
        the object then raises ``RuntimeError``.  One draw is live per model; a new one replaces it."""
        if not self._fitted:
            raise RuntimeError("sample_functions() before a successful fit()")
        S, F = int(n_samples), int(n_features)
        if S < 1 or F < 1:
            raise ValueError("n_samples and n_features must be >= 1")
        seed = 0 if random_state is None else int(random_state) & 0xFFFFFFFFFFFFFFFF
        pz, kz, keepz = None, _abi.MEM_HOST, None
        if z is not None:
            pz, kz, keepz, _, sz = self._as_input(z, "z")
            q = {"rbf": 0, "matern52": 5, "matern32": 3, "matern12": 1}[self.kernel]
            nn = F * (self._d + q) + S * self._k * (2 * F + self._N)
            if int(np.prod(sz)) != nn:
                raise ValueError(f"z must hold F (d + q) + S k (2 F + N) = {nn} standard normals")
        self._check(self._lib.gpx_pathwise_draw(self._h, S, F, seed, pz, kz))
        self._pw_token = getattr(self, "_pw_token", 0) + 1
        return PosteriorFunctions(self, S, F, self._pw_token)

    # -- checkpoint / resume (optional get_state) ------------------------------
    def get_state(self):
        """Plain-data description of the model (JSON-serialisable): kernel, hyper-parameters,
        dtype, panel width and, once fitted, the jitter that was needed and the log-determinant.
        The training data and the factor are NOT included — the factor is N^2 numbers the GPU
        rebuilds faster than storage returns them, and the path is deterministic:
        ``GP.from_state(s).fit(X, y)`` reproduces alpha, mean and variance bit for bit (tested),
        so a hyper-parameter search is resumed by saving this after every ``optimize`` step.  ``path_variance`` and
        ``path_lengthscale`` of a model fitted with ``path_ids`` are recorded under ``"fitted"``, but they are arguments of
        :meth:`fit`, as the ids are: resume such a model with ``GP.from_state(s).fit(X, y, path_ids=ids,
        path_variance=s["fitted"]["path_variance"], path_lengthscale=s["fitted"]["path_lengthscale"])`` — without them
        the fit is the plain model."""
        st = {"format": 1, "kernel": self.kernel, "lengthscale": [float(v) for v in self.lengthscale],
              "variance": self.variance, "noise": self.noise, "jitter": self.jitter, "dtype": self.dtype,
              "block": self.block, "max_tries": self.max_tries, "refine": self.refine}
        if self._fitted:
            st["fitted"] = {"N": int(self._N), "d": int(self._d), "k": int(self._k),
                            "jitter_used": float(self.jitter_used_), "log_det": float(self.log_det_)}
            if self._basis_fit is not None:
                st["fitted"]["basis"] = self._basis_fit
            if self.path_lengthscale is not None:
                st["fitted"].update(path_variance=float(self.path_variance),
                                    path_lengthscale=[float(v) for v in self.path_lengthscale])
        return st

    @classmethod
    def from_state(cls, state, **overrides):
        """A fresh, unfitted model from :meth:`get_state` output; ``overrides`` are passed to the
        constructor (``device=``, ``devices=``, ``profile=`` ... are not part of the state)."""
        if state.get("format") != 1:
            raise ValueError("not a GP state of this library (format 1)")
        kw = {k: state[k] for k in ("kernel", "variance", "noise", "jitter", "dtype", "block", "max_tries")}
        kw["refine"] = state.get("refine", 0)
        ls = state["lengthscale"]
        kw["lengthscale"] = ls[0] if len(ls) == 1 else ls
        kw.update(overrides)
        return cls(**kw)

    def release_scratch(self):
        """Free the device buffers only the next ``predict`` / ``lml_gradient`` would use (V^T batch,
        L^-T, partial sums); the fit stays valid.  Buffers otherwise stay allocated for reuse."""
        self._check(self._lib.gpx_release_scratch(self._h))

    @property
    def alpha_(self):
        if not self._fitted:
            raise RuntimeError("no fit")
        if self._alpha is None:
            out = np.empty((self._N, self._k), dtype=self._np_dtype)
            self._check(self._lib.gpx_get_alpha(self._h, C.c_void_p(out.ctypes.data)))
            self._alpha = out[:, 0].copy() if self._y1d else out
        return self._alpha

    def set_profile(self, on):
        """Switch the per-launch timing of the Cholesky sub-phases (``profile=``) on an existing model."""
        self._check(self._lib.gpx_set_flags(self._h, _abi.FLAG_PROFILE if on else 0))

    @property
    def timings_(self):
        t = _abi.GpxTimings()
        self._check(self._lib.gpx_get_timings(self._h, C.byref(t)))
        return t.as_dict()

    def log_marginal_likelihood(self, y, derivatives=None, derivative_noise=0.0):
        """-1/2 y^T alpha - 1/2 logdet - N/2 log(2 pi), summed over target columns.  ``derivatives`` as passed to
        :meth:`fit` (their targets follow ``y``; N counts both; ``derivative_noise`` is part of the fit already).
        On a fit with ``basis=`` this is the profile likelihood at ``beta_``: ``alpha_`` is ``K^-1 (y - H beta)`` and
        ``H^T alpha = 0``, so ``y^T alpha = (y - H beta)^T alpha``; :meth:`lml_gradient` is its exact gradient."""
        if _is_torch(y):
            y = y.detach().cpu().numpy()
        if derivatives is not None:
            yd = derivatives[2]
            yd = yd.detach().cpu().numpy() if _is_torch(yd) else np.asarray(yd)
            y = np.concatenate([np.asarray(y, dtype=np.float64).reshape(len(y), -1),
                                np.asarray(yd, dtype=np.float64).reshape(len(yd), -1)])
        Y = np.asarray(y, dtype=np.float64).reshape(self._N, -1)
        A = self.alpha_.reshape(self._N, -1).astype(np.float64)
        n, k = Y.shape
        return float(-0.5 * np.sum(Y * A) - 0.5 * k * self.log_det_
                     - 0.5 * n * k * np.log(2.0 * np.pi))

    def lml_gradient(self, derivative_noise=False, path=False):
        """``(lml, grad)`` of the last ``fit``: the log marginal likelihood and its analytic
        gradient w.r.t. the LOG hyper-parameters, ordered (lengthscale[0..n_ls), variance, noise)
        — R&W eq. 5.9, 1/2 tr((alpha alpha^T - K^-1) dK/dtheta) (with ``noise_weights``: dK/dlog noise =
        noise diag(w)), computed on the GPU by
        ``gpx_lml_grad`` (about two more factorisations' worth of MFMA work: L^-T, then K^-1
        formed and consumed tile by tile, never stored).  fp64 models.  Sharded ones (``devices=`` or
        ``world=``): with the replicated factor L^-T is built in row blocks dealt over the GPUs,
        all-gathered once, and the trace pass is split over the GPUs; when the factor is only held
        distributed (C4-sized problems) L^-T is built distributed, every GPU keeps the columns of its
        own row blocks and contracts the trace over them — either way every rank returns the same
        numbers.

        ``derivative_noise=True`` (``gpx_lml_grad_full``; one device, float64): one more entry at the end, the derivative
        by log ``derivative_noise`` — 0 for a fit without derivative observations or with ``derivative_noise == 0``.
        This is the call for a fit with ``derivatives=``, which the default call refuses (its gradient has no room for
        that entry); on any other fit the leading entries and ``lml`` are the default call's bit for bit.

        ``path=True`` (``gpx_lml_grad_paths``; one device, float64): the gradient of a fit with ``path_ids=``, which the
        other two calls refuse — ``(lengthscale.., variance, noise, path_variance, path_lengthscale..)``, at the default
        call's cost (the path terms are evaluated only in the tiles that can hold a pair of one path).  ``variance`` is the
        derivative of the ``f`` part alone, and the lengthscale entries do not see the path term.  On a fit without
        effective path ids (none, all -1, or ``path_variance == 0``) ``lml`` and the leading entries are the default call's
        bit for bit and the path entries are zeros: one for ``path_variance`` and one per entry of the ``path_lengthscale``
        given to the fit (1 if none was given).  Not together with ``derivative_noise=True`` (``ValueError``): a fit has
        path ids or derivative observations."""
        if path and derivative_noise:
            raise ValueError("path=True and derivative_noise=True exclude each other: a fit has path ids or derivatives")
        if not self._fitted:
            raise RuntimeError("lml_gradient() before a successful fit()")
        lml = C.c_double(0.0)
        if path:
            grad = np.empty(self.lengthscale.size + 3 + self._n_path_ls, dtype=np.float64)
            n_main = self.lengthscale.size + 2
            self._check(self._lib.gpx_lml_grad_paths(self._h, C.byref(lml), _abi.dptr(grad[:n_main]), _abi.dptr(grad[n_main:]),
                                                     grad.size - n_main))
            return float(lml.value), grad
        grad = np.empty(self.lengthscale.size + (3 if derivative_noise else 2), dtype=np.float64)
        call = self._lib.gpx_lml_grad_full if derivative_noise else self._lib.gpx_lml_grad
        self._check(call(self._h, C.byref(lml), _abi.dptr(grad)))
        return float(lml.value), grad

    def _loo(self, want_mean, want_var, want_logp, want_total):
        if not self._fitted:
            raise RuntimeError("loo() before a successful fit()")
        N, k = self._N, self._k
        mean = np.empty((N, k), dtype=np.float64) if want_mean else None
        var = np.empty(N, dtype=np.float64) if want_var else None
        logp = np.empty((N, k), dtype=np.float64) if want_logp else None
        total = np.empty(k, dtype=np.float64) if want_total else None
        self._check(self._lib.gpx_loo(self._h, *(None if a is None else _abi.dptr(a) for a in (mean, var, logp, total))))
        return mean, var, logp, total

    def loo(self, return_var=True, return_logp=False):
        """Leave-one-out predictions of the observations of the current fit, without refitting (``gpx_loo``; R&W §5.4.2):
        ``mean``, then with ``return_var`` ``var`` (N,), then with ``return_logp`` ``logp``.  ``mean`` and ``logp`` are
        shaped as ``alpha_`` is — (N,) for a 1-D ``y``, else (N, k); NumPy float64 arrays.

        Row i is what the model fitted to every OTHER observation predicts for observation i: ``mean[i]``, the variance
        ``var[i]`` of that OBSERVATION — its own noise (times its noise weight) and jitter included, not the latent
        function's variance — and ``logp[i]``, the log-density of the observed ``y[i]`` under it.  ``(y - mean) /
        sqrt(var)`` is the standardised residual: a bad recording is a row where it is large, and :meth:`remove` takes
        such rows out.  On a fit with ``derivatives=`` the rows follow the fit's order (values, then derivative rows;
        ``observation_kinds_``), and a derivative row's entry is the prediction of that derivative observation, with
        ``derivative_noise`` in its variance.  On a fit with ``path_ids=`` the other points of the row's own path count
        among "the others".  On a fit with ``basis=`` the coefficients are marginalised (flat prior), the trend is inside
        ``mean``; a row that the coefficients alone determine (every row when N equals the number of basis functions)
        gets ``var = inf``, ``mean = nan``, ``logp = -inf``.

        Cost: one ``L^-T`` build — about the ``grad_trtri`` phase of a :meth:`lml_gradient` — one pass over it, and
        N^2 * 8 bytes of scratch, which :meth:`release_scratch` frees.  Two calls return the same bits.  float64 models on
        one device; anything else raises ``GpxError`` with the library's message."""
        mean, var, logp, _ = self._loo(True, return_var, return_logp, False)
        out = [mean[:, 0].copy() if self._y1d else mean]
        if return_var:
            out.append(var)
        if return_logp:
            out.append(logp[:, 0].copy() if self._y1d else logp)
        return out[0] if len(out) == 1 else tuple(out)

    def loo_log_likelihood(self):
        """The leave-one-out log predictive density of the current fit, ``sum_i logp[i]`` of :meth:`loo` (R&W eq. 5.11): a
        float, or (k,) for several targets.  The second yardstick beside :meth:`log_marginal_likelihood` for comparing
        kernel families, path terms and trends; ``-inf`` where a row is undetermined (see :meth:`loo`).  Same cost as
        :meth:`loo`."""
        total = self._loo(False, False, False, True)[3]
        return float(total[0]) if self._y1d else total

    def optimize(self, X, y, params=("lengthscale", "variance", "noise"), bounds=(1e-4, 1e4), maxiter=40,
                 rel_step=1e-4, jac="analytic", noise_weights=None, derivatives=None, derivative_noise=0.0,
                 path_ids=None, path_variance=0.0, path_lengthscale=None, basis=None):
        """Fit the hyper-parameters by maximising the log marginal likelihood (SURVEY.md §8f
        rank 1: the natural step after ``fit``; the reference has no counterpart).

        ``params`` chooses what moves ("lengthscale" moves every ARD entry); the search runs in
        log-space with L-BFGS-B.  ``jac="analytic"`` (default): every evaluation is one ``fit()``
        plus one ``lml_gradient()`` on the GPU, about three factorisations' worth of work whatever
        the number of parameters.  Models without the analytic gradient (float32 / mixed) fall back
        to ``jac="3-point"`` central differences: 2 p extra fits per gradient.
        Non-positive-definite trial points count as very bad, they do not raise.  Leaves the
        model fitted at the best point found and returns scipy's result (``.fun`` = minus the
        log marginal likelihood there).  ``noise_weights`` as for :meth:`fit`: every fit of the search, the final one
        included, is made with them; ``noise`` is then the level that is learnt.  ``derivatives`` and
        ``derivative_noise`` as for :meth:`fit` as well: the analytic gradient of such a model is
        ``lml_gradient(derivative_noise=True)``, at the same cost.  ``params`` may then also name ``"derivative_noise"``:
        the noise variance of the derivative observations is learnt with the others, starting from the value passed,
        and the attribute ``derivative_noise`` holds the result (``ValueError`` without ``derivatives`` or when it starts
        at 0: log-space cannot leave 0).  Left out of ``params`` it stays fixed.

        ``path_ids``, ``path_variance`` and ``path_lengthscale`` as for :meth:`fit`.  The analytic gradient of such a
        model is ``lml_gradient(path=True)``, at the same cost (float64 on one device; anything else, and
        ``jac="3-point"``, runs on central differences); ``params`` may name ``"path_variance"`` (which must start above
        0) and ``"path_lengthscale"`` (every entry moves), and the attributes of those names hold the result.

        ``basis`` as for :meth:`fit`: every fit of the search is made with it, the objective is the profile likelihood
        at each point's own ``beta_`` and the analytic gradient is its exact gradient."""
        from scipy.optimize import minimize
        self._check_basis(basis)
        known = ("lengthscale", "variance", "noise", "derivative_noise", "path_variance", "path_lengthscale")
        names = [p for p in known if p in params]
        if not names or len(names) != len(tuple(params)):
            raise ValueError("params must be a non-empty subset of " + " / ".join(known))
        ids, pvar, plsp = check_path_args(path_ids, path_variance, path_lengthscale, derivatives=derivatives)
        if ids is None and ("path_variance" in names or "path_lengthscale" in names):
            raise ValueError("params names path_variance / path_lengthscale, but there are no path_ids")
        if "path_variance" in names and not pvar > 0:
            raise ValueError("path_variance must start above 0 to be learnt (the search runs in log-space)")
        if ids is not None:   # where the search starts; unpack() moves them when they are learnt
            self.path_variance = pvar
            self.path_lengthscale = self.lengthscale.copy() if plsp is None else plsp
        if "derivative_noise" in names:
            if derivatives is None:
                raise ValueError("params names derivative_noise, but there are no derivatives")
            if not float(derivative_noise) > 0:
                raise ValueError("derivative_noise must start above 0 to be learnt (the search runs in log-space)")
        n_ls = self.lengthscale.size
        full_grad = derivatives is not None   # a fit with derivative rows: the gradient with the derivative_noise entry
        if full_grad:
            self.derivative_noise = float(derivative_noise)   # where the search starts; unpack() moves it when it is learnt

        def fit_kw():   # every fit of the search, the final one included, with the current derivative_noise
            kw = dict(noise_weights=noise_weights, derivatives=derivatives, basis=basis,
                      derivative_noise=self.derivative_noise if full_grad else derivative_noise)
            if ids is not None:
                kw.update(path_ids=ids, path_variance=self.path_variance, path_lengthscale=self.path_lengthscale)
            return kw

        def pack():
            v = []
            for p in names:
                v.extend(np.log(getattr(self, p)) if p in ("lengthscale", "path_lengthscale") else
                         [np.log(max(getattr(self, p), bounds[0]))])
            return np.asarray(v, dtype=np.float64)

        def unpack(v):
            i = 0
            for p in names:
                if p == "lengthscale":
                    self.lengthscale = np.exp(v[i:i + n_ls])
                    i += n_ls
                elif p == "path_lengthscale":
                    n = self.path_lengthscale.size
                    self.path_lengthscale = np.exp(v[i:i + n])
                    i += n
                else:
                    setattr(self, p, float(np.exp(v[i])))
                    i += 1

        best = {"f": np.inf, "v": pack()}
        path_grad = ids is not None   # a fit with path ids: the gradient with the path_variance / path_lengthscale entries
        analytic = jac == "analytic" and self.dtype == "float64"
        if analytic and (self.world > 1 or self._is_group or self._host_comm is not None):
            # sharded: the gradient needs the replicated-factor mode, which the library picks from N
            # and the card's memory at fit time — ask it once (every rank gets the same answer)
            try:
                self.fit(X, y, **fit_kw())
                self.lml_gradient()
            except _abi.GpxError:
                analytic = False
            except np.linalg.LinAlgError:
                pass
        # columns of the full gradient that move: (lengthscale.., variance, noise, derivative_noise), or with path ids
        # (lengthscale.., variance, noise, path_variance, path_lengthscale..)
        cols = []
        for p in names:
            if p == "lengthscale":
                cols.extend(range(n_ls))
            elif p == "path_lengthscale":
                cols.extend(range(n_ls + 3, n_ls + 3 + self.path_lengthscale.size))
            else:
                cols.append(n_ls + ("variance", "noise", "path_variance" if path_grad else "derivative_noise").index(p))

        class _NoAnalyticGradient(Exception):
            pass

        def objective(v, analytic):
            unpack(v)
            g = np.zeros(len(cols))
            try:
                self.fit(X, y, **fit_kw())
                if analytic:
                    try:
                        lml, full = (self.lml_gradient(path=True) if path_grad else
                                     self.lml_gradient(derivative_noise=full_grad))
                    except _abi.GpxError as e:
                        # no gradient for this model after all (factor only held distributed, or no
                        # room for the N x N L^-T buffer): free what the attempt allocated and let the
                        # caller restart the search with central differences
                        if e.code not in (_abi.E_UNSUPPORTED, _abi.E_NOMEM):
                            raise
                        self.release_scratch()
                        raise _NoAnalyticGradient() from e
                    f, g = -lml, -full[cols]
                else:
                    f = -self.log_marginal_likelihood(y, derivatives=derivatives)
            except np.linalg.LinAlgError:
                f = 1e300
            if not np.isfinite(f) or not np.all(np.isfinite(g)):
                f, g = 1e300, np.zeros(len(cols))
            if f < best["f"]:
                best["f"], best["v"] = f, np.array(v, copy=True)
            return (f, g) if analytic else f

        v0 = pack()
        lo, hi = np.log(bounds[0]), np.log(bounds[1])

        def search(start, analytic):
            return minimize(objective, start, args=(analytic,), method="L-BFGS-B",
                            jac=True if analytic else "3-point", bounds=[(lo, hi)] * v0.size,
                            options={"maxiter": int(maxiter)} if analytic else
                            {"maxiter": int(maxiter), "eps": float(rel_step)})
        try:
            res = search(v0, analytic)
        except _NoAnalyticGradient:
            res = search(best["v"], False)   # from the best point the analytic steps reached
        unpack(best["v"])
        self.fit(X, y, **fit_kw())
        res.x, res.fun = best["v"], best["f"]
        return res


class PosteriorFunctions:
    """Posterior sample functions of a fitted :class:`GP` (:meth:`GP.sample_functions`): drawn once, evaluated anywhere.

    Calling the object evaluates the SAME functions at whatever points it is given: a coarse grid now, a finer one or
    another consumer's points later.  The conditioning on the data is exact; the prior draw behind it is a sum of
    ``n_features`` random Fourier features, approximate with O(1 / sqrt(n_features)) error in its covariance
    (``profiles/pathwise_bias.json``).  The draw lives in the model's handle: fitting, updating or reducing the model, or
    drawing again, ends it, and the object raises ``RuntimeError`` from then on."""

    def __init__(self, gp, n_samples, n_features, token):
        self._gp, self.n_samples, self.n_features, self._token = gp, int(n_samples), int(n_features), token

    def _live(self):
        gp = self._gp
        if gp is None or getattr(gp, "_h", None) is None or getattr(gp, "_pw_token", None) != self._token:
            return False
        S = C.c_int64(0)
        gp._check(gp._lib.gpx_pathwise_info(gp._h, C.byref(S), None, None))
        return S.value == self.n_samples

    def __call__(self, Xs, samples=None):
        """The functions at ``Xs`` (M, d): (M, S) for a 1-D ``y``, (M, k, S) otherwise, as :meth:`GP.sample_y` shapes its
        result.  ``samples``: None (all), an int count or a ``slice`` with step 1 — the functions to evaluate.  NumPy in,
        NumPy out; a device tensor in, a device tensor out."""
        if not self._live():
            raise RuntimeError("the model changed (or drew again) after sample_functions(): these functions are gone")
        gp = self._gp
        if samples is None:
            s0, s1 = 0, self.n_samples
        elif isinstance(samples, slice):
            s0, s1, step = samples.indices(self.n_samples)
            if step != 1:
                raise ValueError("samples must be a contiguous slice")
        else:
            s0, s1 = 0, int(samples)
        if not 0 <= s0 < s1 <= self.n_samples:
            raise ValueError(f"samples must select at least one of the {self.n_samples} functions")
        pq, kq, keepq, devq, sq = gp._as_input(Xs, "Xs")
        if len(sq) != 2 or sq[1] != gp._d:
            raise ValueError(f"Xs must be (M, {gp._d})")
        M, k, S = sq[0], gp._k, s1 - s0
        out = gp._empty((S, M, k), devq)
        gp._check(gp._lib.gpx_pathwise_eval(gp._h, pq, M, s0, S, gp._ptr(out), kq))
        if gp._y1d:
            res = out[:, :, 0].T
        else:
            res = out.permute(1, 2, 0) if devq is not None else out.transpose(1, 2, 0)
        return res.contiguous() if devq is not None else np.ascontiguousarray(res)

    def close(self):
        """Free the draw's device memory (if it is still this one's)."""
        if self._gp is not None and self._live():
            self._gp._check(self._gp._lib.gpx_pathwise_draw(self._gp._h, 0, 0, 0, None, _abi.MEM_HOST))
        self._gp = None
