"""Path data model, CSV reader and path k-means around the GP engine.

Mirrors the reference's own world so its user can switch over:

=====================================  ==========================================
reference (``GPmap.py``)               here
=====================================  ==========================================
``trajectory`` (``:12-23``)            :class:`Trajectory` (``timestamp, xs, ys``)
``trajectories.pathdict`` (``:30-34``) :class:`Trajectories` (``pathdict``, ``add_trajectory``)
``check_if_valid_trajectory``          :func:`check_if_valid_trajectory` — same *signed* travel
(``:165-175``)                         sum, so inward-moving paths are rejected exactly as there
``readcsvfile`` (``:178-204``)         :func:`read_csv` — same block rules (header row carries the
                                       id in column 1, ``t,_,x,y`` rows with x, y parsed as int,
                                       ``###`` ends a block, keep only valid paths of exactly 33
                                       points, stop after ``numoftrajstoread`` kept paths)
``calc_distance`` (``:114-121``)       :func:`path_distance_matrix` — ONE HIP kernel for all
                                       (path, centroid) pairs (``gpx_path_distance``)
``calc_mean_traj`` (``:95-112``)       :func:`mean_path` (empty cluster = ``ZeroDivisionError``)
``kmeansclustering`` (``:36-93``)      :func:`kmeans` — same Lloyd loop, first-minimum ties, stop
                                       when the centroids moved < 5 in total
=====================================  ==========================================

Deliberate divergences (documented, not reproduced): the reference's "too close" re-draw
loop (``:39-53``) never terminates once a close pair is drawn and compares only
``j in range(i+1, k-1)``; here every pair is checked and re-draws are bounded.  Plotting
(``:125-161``) is out of scope.  The file name is an argument, not the hard-coded
``'testfile.csv'`` (``:181``), and nothing runs at import.

The distance matrix — the reference's hot loop — runs on the GPU through the C ABI; the
O(P*k) bookkeeping around it (arg-min, cluster means) is host NumPy.
"""
from __future__ import annotations

import csv
import ctypes as C
import io
import os
import random as _random
from dataclasses import dataclass, field

import numpy as np

from . import _abi

PATH_LENGTH = 33          # GPmap.py:189
MIN_TRAVEL = 1000         # GPmap.py:36,189
MOVEMENT_STOP = 5.0       # GPmap.py:90


@dataclass
class Trajectory:
    """Growable (timestamp, x, y) path — ``class trajectory`` (GPmap.py:12-23)."""
    xs: np.ndarray = field(default_factory=lambda: np.array([], dtype=float))
    ys: np.ndarray = field(default_factory=lambda: np.array([], dtype=float))
    timestamp: np.ndarray = field(default_factory=lambda: np.array([], dtype=float))

    def add_point(self, time, x, y):
        self.xs = np.append(self.xs, x)
        self.ys = np.append(self.ys, y)
        self.timestamp = np.append(self.timestamp, time)

    def __len__(self):
        return len(self.xs)


class Trajectories:
    """id -> Trajectory — ``class trajectories`` (GPmap.py:28-34)."""

    def __init__(self):
        self.pathdict = {}

    def add_trajectory(self, id, trajectory):
        self.pathdict[id] = trajectory

    def __len__(self):
        return len(self.pathdict)

    def keys(self):
        return list(self.pathdict.keys())

    def as_array(self, keys=None):
        """(P, L, 3) array of (t, x, y) for equal-length paths."""
        keys = self.keys() if keys is None else list(keys)
        return np.stack([np.stack([self.pathdict[k].timestamp, self.pathdict[k].xs, self.pathdict[k].ys], 1)
                         for k in keys]) if keys else np.zeros((0, PATH_LENGTH, 3))

    def kmeansclustering(self, k, treshold=MIN_TRAVEL, **kw):
        """Same name and argument spelling as the reference (GPmap.py:36)."""
        return kmeans(self, k, too_close=treshold, **kw)


def travel_score(traj) -> float:
    """sum_{i<j} (|x_j|-|x_i| + |y_j|-|y_i|), the signed sum of GPmap.py:165-175."""
    a = np.abs(np.asarray(traj.xs, float)) + np.abs(np.asarray(traj.ys, float))
    n = len(a)
    return float(np.sum(a * (2.0 * np.arange(n) - n + 1.0)))


def check_if_valid_trajectory(traj, minimumtraveldistance=1) -> bool:
    return not (travel_score(traj) < minimumtraveldistance)


def read_csv(source, numoftrajstoread=0, minimum_travel=MIN_TRAVEL, length=PATH_LENGTH, into=None):
    """Parse the reference's CSV wire format (GPmap.py:178-204) from a path, file object or
    text; returns a :class:`Trajectories`.  A final block without a closing ``###`` row is
    dropped, as in the reference; a file that starts with ``###`` raises (there: an
    ``UnboundLocalError`` at :189)."""
    trajs = Trajectories() if into is None else into
    if isinstance(source, str) and "\n" not in source and os.path.exists(source):
        fh, close = open(source, newline=""), True
    elif isinstance(source, str):
        fh, close = io.StringIO(source), False          # CSV text
    else:
        fh, close = source, False                       # file object
    try:
        kept = 0
        new = None
        is_new = True
        pid = 0
        for row in csv.reader(fh, delimiter=","):
            if not row:
                continue
            if row[0] == "###":
                if new is None:
                    raise ValueError("CSV starts with a '###' row: no trajectory to close")
                if check_if_valid_trajectory(new, minimum_travel) and len(new.timestamp) == length:
                    trajs.add_trajectory(pid, new)
                    kept += 1
                if numoftrajstoread != 0 and kept >= numoftrajstoread:
                    break
                new = Trajectory()
                is_new = True
            elif not is_new:
                new.add_point(float(row[0]), int(row[2]), int(row[3]))
            else:
                pid = row[1]
                new = Trajectory()
                is_new = False
    finally:
        if close:
            fh.close()
    return trajs


def to_gp_inputs(trajs, keys=None, inputs=("t",), targets=("x", "y"), normalise=True):
    """Flatten paths into GP training data: X (33*P, d) from the chosen input columns, Y
    (33*P, k) from the target columns (k targets share one Cholesky factor).  With
    ``normalise`` every input column is mapped to [0, 1] (returns the (lo, span) used)."""
    col = {"t": 0, "x": 1, "y": 2}
    arr = trajs.as_array(keys).reshape(-1, 3)
    X = arr[:, [col[c] for c in inputs]].astype(np.float64)
    Y = arr[:, [col[c] for c in targets]].astype(np.float64)
    lo, span = np.zeros(X.shape[1]), np.ones(X.shape[1])
    if normalise and len(X):
        lo = X.min(axis=0)
        span = np.where(X.max(axis=0) > lo, X.max(axis=0) - lo, 1.0)
        X = (X - lo) / span
    return np.ascontiguousarray(X), np.ascontiguousarray(Y), (lo, span)


# ---- the hot loop: all path-to-centroid distances in one launch ---------------------------------
def path_distance_matrix(paths_xy, centroids_xy):
    """D[p, c] = sum_i ||paths[p, i] - centroids[c, i]||_2 on the GPU (``gpx_path_distance``).
    paths (P, L, 2), centroids (C, L, 2): NumPy arrays, or torch CUDA tensors (no copies)."""
    lib = _abi.load()
    if type(paths_xy).__module__.split(".")[0] == "torch" and paths_xy.is_cuda:
        import torch
        p = paths_xy.detach().to(torch.float64).contiguous()
        c = centroids_xy.detach().to(device=p.device, dtype=torch.float64).contiguous()
        if p.ndim != 3 or c.ndim != 3 or p.shape[1:] != c.shape[1:] or p.shape[2] != 2:
            raise ValueError("need paths (P, L, 2) and centroids (C, L, 2)")
        D = torch.empty((p.shape[0], c.shape[0]), dtype=torch.float64, device=p.device)
        torch.cuda.current_stream(p.device).synchronize()
        with torch.cuda.device(p.device):
            rc = lib.gpx_path_distance(C.c_void_p(p.data_ptr()), p.shape[0], C.c_void_p(c.data_ptr()),
                                       c.shape[0], p.shape[1], C.c_void_p(D.data_ptr()), _abi.MEM_DEVICE)
        if rc != 0:
            raise _abi.GpxError(rc, lib.gpx_last_error(None).decode())
        return D
    p = np.ascontiguousarray(paths_xy, dtype=np.float64)
    c = np.ascontiguousarray(centroids_xy, dtype=np.float64)
    if p.ndim != 3 or c.ndim != 3 or p.shape[1:] != c.shape[1:] or p.shape[2] != 2:
        raise ValueError("need paths (P, L, 2) and centroids (C, L, 2)")
    D = np.empty((p.shape[0], c.shape[0]), dtype=np.float64)
    rc = lib.gpx_path_distance(C.c_void_p(p.ctypes.data), p.shape[0], C.c_void_p(c.ctypes.data), c.shape[0],
                               p.shape[1], C.c_void_p(D.ctypes.data), _abi.MEM_HOST)
    if rc != 0:
        raise _abi.GpxError(rc, lib.gpx_last_error(None).decode())
    return D


def mean_path(paths_txy):
    """Point-wise mean of (n, L, 3) paths — ``calc_mean_traj`` (GPmap.py:95-112)."""
    paths_txy = np.asarray(paths_txy, dtype=np.float64)
    if paths_txy.shape[0] == 0:
        raise ZeroDivisionError("empty cluster (GPmap.py:111 divides by the cluster size)")
    return paths_txy.sum(axis=0) / paths_txy.shape[0]


def kmeans(trajs, k, too_close=MIN_TRAVEL, init_keys=None, rng=None, movement_stop=MOVEMENT_STOP,
           max_iter=10_000, max_redraws=1000):
    """Lloyd's k-means over whole paths (GPmap.py:36-93) -> {centroid index: [path ids]}.

    Initial centroids: ``init_keys`` or ``rng.sample(keys, k)`` (``rng`` defaults to Python's
    ``random`` module, which is what the reference draws from, so an identical seed draws the
    identical keys).  Each iteration: one GPU launch for all distances, first-minimum
    assignment (the reference's strict ``<`` in dict order), centroid = point-wise mean of its
    cluster, stop when the centroids moved less than ``movement_stop`` in total."""
    keys = trajs.keys()
    if k <= 0 or k > len(keys):
        raise ValueError("need 1 <= k <= number of paths")
    arr = trajs.as_array(keys)                      # (P, L, 3)
    xy = np.ascontiguousarray(arr[:, :, 1:3])
    rng = _random if rng is None else rng
    if init_keys is None:
        init_keys = rng.sample(keys, k)
        for _ in range(max_redraws):                # bounded; every pair checked
            idx = [keys.index(q) for q in init_keys]
            Dc = path_distance_matrix(xy[idx], xy[idx])
            if not np.any(Dc[np.triu_indices(k, 1)] < too_close):
                break
            init_keys = rng.sample(keys, k)
    idx = [keys.index(q) for q in init_keys]
    cents = arr[idx].copy()                         # (k, L, 3): deep copies of the chosen paths
    for _ in range(max_iter):
        D = path_distance_matrix(xy, np.ascontiguousarray(cents[:, :, 1:3]))
        assign = np.argmin(D, axis=1)               # first minimum = the reference's tie rule
        clusters = {c: [keys[p] for p in np.nonzero(assign == c)[0]] for c in range(k)}
        new = np.stack([mean_path(arr[assign == c]) for c in range(k)])
        d = new[:, :, 1:3] - cents[:, :, 1:3]
        moved = float(np.sum(np.sqrt(np.sum(d * d, axis=-1))))
        cents = new
        if moved < movement_stop:
            return clusters
    raise RuntimeError("k-means did not converge")


# ---- one GP per path cluster (independent replicas) ---------------------------------------------
def _dense_only(method):
    """a :class:`PathModel` method that needs the dense factor: on a sparse model it raises, naming itself"""
    import functools

    @functools.wraps(method)
    def guarded(self, *args, **kwargs):
        if self.sparse:
            raise ValueError(f"PathModel.{method.__name__}: the model is sparse (fit_path_models(inducing=)); an "
                             "inducing-point fit serves predict() only")
        return method(self, *args, **kwargs)
    return guarded


class PathModel:
    """GP model of one cluster of paths: inputs (by default the time stamp, mapped to [0, 1]) ->
    (x, y) as two targets sharing ONE Cholesky factor.  Targets are
    standardised per column before the fit (the GP prior has zero mean) and mapped back by
    :meth:`predict`.  ``step_weights`` (L,), or None: the per-step noise weights the model was fitted with
    (``fit_path_models(step_noise=True)``); :meth:`add_paths` and :meth:`log_likelihood` then use them too.
    ``has_velocities``: the model was also conditioned on observed velocities (``fit_path_models(velocities=)``: derivative
    observations along ``"t"``); every prediction works unchanged, and :meth:`append_paths` adds paths with or without
    velocities (:meth:`add_paths`, which takes none, refuses such a model).  ``velocity_noise``: the noise variance of those velocities in the model's normalised units, as given
    or as learnt (``fit_path_models(learn_velocity_noise=True)``); None without velocities.
    ``within_path``: the model is the hierarchical one (``fit_path_models(within_path=True)``): every path is the cluster
    mean plus a deviation of its own.  :meth:`predict`, :meth:`sample`, :meth:`predict_gradient` and :meth:`velocity` are
    then about the cluster mean, or with ``path=key`` about that path of ``keys`` itself (the mean plus its own deviation:
    where it was between, at and beyond its observations); :meth:`log_likelihood` scores a path as a new member of the
    cluster, :meth:`forecast` continues one from its first points; :meth:`append_paths` adds paths under new ids (:meth:`add_paths` refuses such a model).
    Which method adds paths: :meth:`add_paths` on plain and step-noise models, :meth:`append_paths` on every model.
    ``trend``: None, or the basis of the model's explicit mean (``fit_path_models(trend=)``: "constant", "linear",
    "quadratic" in the normalised inputs, coefficients marginalised — ``GP.fit(basis=)``).  :meth:`predict`, :meth:`sample`,
    :meth:`log_likelihood` and :meth:`forecast` include it and its uncertainty; :meth:`add_paths`, :meth:`append_paths`,
    :meth:`remove_paths`, :meth:`predict_gradient`, :meth:`velocity`, :meth:`predict_hessian`, :meth:`acceleration` and
    :meth:`curvature` raise ``GpxError`` with the library's reason.  :meth:`acceleration` and :meth:`curvature` (second
    derivatives) need an "rbf" or "matern52" model.
    ``sparse``: the model is an inducing-point fit (``fit_path_models(inducing=m)``; ``gp`` is a ``SparseGP``), for
    clusters with more observations than a dense factor holds.  :meth:`predict` (mean, variance, ``return_cov``) works as
    on any model; every other method raises ``ValueError`` naming itself."""

    def __init__(self, gp, keys, in_lo, in_span, y_mean, y_std, inputs, targets, step_weights=None, has_velocities=False,
                 within_path=False, row_counts=None, trend=None, sparse=False):
        self.gp, self.keys = gp, list(keys)
        self.trend = trend
        self.sparse = bool(sparse)
        # what remove_paths needs: every key's path id (within_path: its index in keys until a path has been removed, and
        # never reused after) and its number of value rows (row_counts: one per key, in order; None: not recorded)
        self._ids = {q: i for i, q in enumerate(self.keys)}
        self._next_id = len(self.keys)
        self._rows = None if row_counts is None else {q: int(n) for q, n in zip(self.keys, row_counts)}
        self.in_lo, self.in_span, self.y_mean, self.y_std = in_lo, in_span, y_mean, y_std
        self.inputs, self.targets = tuple(inputs), tuple(targets)
        self.step_weights = None if step_weights is None else np.asarray(step_weights, dtype=np.float64)
        self.has_velocities = bool(has_velocities)
        self.within_path = bool(within_path)

    @property
    def velocity_noise(self):
        return float(self.gp.derivative_noise) if self.has_velocities else None

    def _tiled_weights(self, n_rows, what):
        """the step weights repeated for n_rows / L whole paths (None without step weights)"""
        if self.step_weights is None:
            return None
        L = len(self.step_weights)
        if n_rows % L:
            raise ValueError(f"{what}: the model has per-step noise weights for paths of {L} points")
        return np.tile(self.step_weights, n_rows // L)

    def _queries(self, q):
        q = np.asarray(q, dtype=np.float64)
        q = q.reshape(-1, 1) if q.ndim == 1 else q
        if q.ndim != 2 or q.shape[1] != len(self.inputs):
            raise ValueError(f"queries must be (M,) or (M, {len(self.inputs)})")
        return np.ascontiguousarray((q - self.in_lo) / self.in_span)

    def _path_kw(self, path):
        """``path`` (None, or a key of ``self.keys``) -> the ``path_ids`` keyword of the GP's methods: a path's id is its
        index in ``keys`` (``fit_path_models`` and :meth:`append_paths` number them so) until :meth:`remove_paths` has
        taken a path out; from then on new paths get ids no path has had"""
        if path is None:
            return {}
        if not self.within_path:
            raise ValueError("path= needs a within_path model (fit_path_models(within_path=True)): only there has a path a "
                             "deviation of its own")
        if path not in self._ids:
            raise KeyError(path)
        return {"path_ids": self._ids[path]}

    def predict(self, q, return_var=True, include_noise=False, return_cov=False, path=None):
        """Posterior at raw (un-normalised) inputs ``q`` (M,) or (M, d): mean (M, k) in the
        targets' own units and, with ``return_var``, the variance (M, k) per target.  ``return_cov=True``
        returns ``(mean (M, k), cov (k, M, M))``: the joint covariance of each target over the queries.
        ``path`` (a key of ``keys``; ``within_path`` models): the posterior of that path itself instead of the cluster
        mean.  ``ValueError`` on a model that is not ``within_path``, ``KeyError`` for a key the model does not hold."""
        kw = self._path_kw(path)
        qn = self._queries(q)
        if return_cov:
            mean, cov = self.gp.predict(qn, include_noise=include_noise, return_cov=True, **kw)
            mean = mean.reshape(len(qn), -1) * self.y_std + self.y_mean
            return mean, cov[None, :, :] * (self.y_std ** 2)[:, None, None]
        out = self.gp.predict(qn, return_var=return_var, include_noise=include_noise, **kw)
        mean = (out[0] if return_var else out).reshape(len(qn), -1) * self.y_std + self.y_mean
        if not return_var:
            return mean
        return mean, out[1][:, None] * (self.y_std ** 2)[None, :]

    @_dense_only
    def sample(self, q, n_samples, seed=0, include_noise=False, path=None):
        """``n_samples`` plausible paths of this cluster: joint posterior samples over the raw inputs ``q`` (M,) or
        (M, d), (n_samples, M, k) in the targets' own units (``GP.sample_y`` on the device, Philox stream ``seed``).
        ``path`` as :meth:`predict`'s: samples of that path itself, which pass near its observations."""
        kw = self._path_kw(path)
        qn = self._queries(q)
        s = self.gp.sample_y(qn, n_samples, random_state=seed, include_noise=include_noise, **kw)
        s = s.reshape(len(qn), -1, int(n_samples))                     # (M, k, n)
        return np.ascontiguousarray(s.transpose(2, 0, 1)) * self.y_std + self.y_mean

    @_dense_only
    def sample_functions(self, n_samples, n_features=4096, seed=0):
        """``n_samples`` plausible paths of this cluster as FUNCTIONS (``GP.sample_functions``: drawn once, evaluated
        anywhere).  Returns a callable: ``paths(q)`` takes raw inputs ``q`` (M,) or (M, d) and returns (n_samples, M, k) in
        the targets' own units, like :meth:`sample` — the same paths on any grid, as fine as needed, at no cost in M^2.
        The prior behind the draw is approximate (``n_features`` random features; see ``GP.sample_functions``).  Raises
        ``ValueError`` on models that are ``within_path``, have a trend or have velocities.  The callable raises
        ``RuntimeError`` once the model has changed."""
        for flag, why in ((self.within_path, "the model is within_path (path ids)"),
                          (self.trend is not None, "the model has a trend (basis functions)"),
                          (self.has_velocities, "the model has velocities (derivative observations)")):
            if flag:
                raise ValueError(f"sample_functions: {why}: pathwise sampling does not cover it")
        fs = self.gp.sample_functions(n_samples, n_features=n_features, random_state=seed)
        n = int(n_samples)

        def paths(q):
            qn = self._queries(q)
            s = fs(qn).reshape(len(qn), -1, n)                             # (M, k, n)
            return np.ascontiguousarray(s.transpose(2, 0, 1)) * self.y_std + self.y_mean

        paths.functions = fs
        return paths

    @_dense_only
    def predict_gradient(self, q, return_var=True, path=None):
        """Gradient of the posterior with respect to the raw (un-normalised) inputs ``q`` (M,) or (M, d), in target units
        per input unit: ``dmean`` (M, d, k) and, with ``return_var``, ``dvar`` (M, d, k), the latent variance of each
        partial derivative per target (``GP.predict_gradient`` on the device, rescaled by ``y_std[c] / in_span[j]``).
        ``path`` as :meth:`predict`'s: the gradient of that path itself."""
        kw = self._path_kw(path)
        qn = self._queries(q)
        M, d = qn.shape
        out = self.gp.predict_gradient(qn, return_var=return_var, **kw)
        scale = self.y_std[None, None, :] / np.asarray(self.in_span, dtype=np.float64)[None, :, None]   # (1, d, k)
        dmean = (out[0] if return_var else out).reshape(M, d, -1) * scale
        if not return_var:
            return dmean
        return dmean, out[1][:, :, None] * scale ** 2

    @_dense_only
    def velocity(self, q, return_var=True, path=None):
        """Velocity of the modelled path at the raw time stamps ``q``: the ``"t"`` column of :meth:`predict_gradient`,
        (M, k) arrays, e.g. (dx/dt, dy/dt), and with ``return_var`` their latent variances (M, k).  ``q`` is (M,) when
        ``t`` is the only input, else (M, d) as for :meth:`predict`.  ``path`` as :meth:`predict`'s: that path's own
        velocity."""
        if "t" not in self.inputs:
            raise ValueError(f"velocity() needs 't' among the model's inputs, have {self.inputs}")
        jt = self.inputs.index("t")
        out = self.predict_gradient(q, return_var=return_var, path=path)
        if not return_var:
            return out[:, jt, :]
        return out[0][:, jt, :], out[1][:, jt, :]

    @_dense_only
    def predict_hessian(self, q, return_var=True, path=None):
        """Second derivatives of the posterior with respect to the raw (un-normalised) inputs ``q`` (M,) or (M, d), in
        target units per input unit squared: ``hmean`` (M, D2, k) over the pairs ``(i, j)``, ``i <= j``, of the inputs,
        row-major (``D2 = d (d + 1) / 2``), and, with ``return_var``, ``hvar`` (M, D2, k), the latent variance of each
        (``GP.predict_hessian`` on the device, rescaled by ``y_std[c] / (in_span[i] in_span[j])``, variances by its
        square).  RBF and Matern-5/2 models only.  ``path`` as :meth:`predict`'s: that path itself."""
        kw = self._path_kw(path)
        qn = self._queries(q)
        M, d = qn.shape
        out = self.gp.predict_hessian(qn, return_var=return_var, **kw)
        span = np.asarray(self.in_span, dtype=np.float64).reshape(-1)
        i, j = np.triu_indices(d)
        scale = self.y_std[None, None, :] / (span[i] * span[j])[None, :, None]   # (1, D2, k)
        hmean = (out[0] if return_var else out).reshape(M, len(i), -1) * scale
        if not return_var:
            return hmean
        return hmean, out[1][:, :, None] * scale ** 2

    @_dense_only
    def acceleration(self, q, return_var=True, path=None):
        """Acceleration of the modelled path at the raw time stamps ``q``: the ``("t", "t")`` entry of
        :meth:`predict_hessian`, (M, k) arrays, e.g. (d2x/dt2, d2y/dt2), and with ``return_var`` their latent variances
        (M, k).  ``q`` and ``path`` as :meth:`velocity`'s."""
        if "t" not in self.inputs:
            raise ValueError(f"acceleration() needs 't' among the model's inputs, have {self.inputs}")
        jt, d = self.inputs.index("t"), len(self.inputs)
        b = jt * d - jt * (jt - 1) // 2   # the pair (jt, jt) in the row-major upper triangle
        out = self.predict_hessian(q, return_var=return_var, path=path)
        if not return_var:
            return out[:, b, :]
        return out[0][:, b, :], out[1][:, b, :]

    @_dense_only
    def curvature(self, q, path=None):
        """Signed curvature of the posterior MEAN path of a model with exactly two targets (x, y) at the raw time stamps
        ``q``, (M,), in raw units (1 / length): ``(x' y'' - y' x'') / (x'^2 + y'^2)^(3/2)`` from the means of
        :meth:`velocity` and :meth:`acceleration`; counter-clockwise is positive, NaN where the mean speed is 0.  It is a
        plug-in value: the curvature of the mean path, not the mean of the curvature, and it comes with no uncertainty
        (the joint covariance of velocity and acceleration is not computed)."""
        if len(self.targets) != 2:
            raise ValueError(f"curvature() needs a model with exactly two targets, have {self.targets}")
        v = self.velocity(q, return_var=False, path=path)
        a = self.acceleration(q, return_var=False, path=path)
        speed2 = v[:, 0] ** 2 + v[:, 1] ** 2
        with np.errstate(divide="ignore", invalid="ignore"):
            kappa = (v[:, 0] * a[:, 1] - v[:, 1] * a[:, 0]) / speed2 ** 1.5
        return np.where(speed2 > 0.0, kappa, np.nan)

    @_dense_only
    def add_paths(self, trajs, keys):
        """Append the paths ``keys`` of ``trajs`` to this cluster's model (``GP.update``: the factor of the paths already
        modelled is kept).  Inputs and targets go through the normalisation fixed at the first fit (``in_lo``,
        ``in_span``, ``y_mean``, ``y_std``), so the result is the GP of all the cluster's paths under that normalisation.
        A model with ``step_weights`` appends with them, tiled over the new paths (which must have its path length).
        Extends ``keys``; returns ``self``."""
        if self.has_velocities:
            raise ValueError("add_paths: the model is conditioned on velocities (derivative observations), and the new paths "
                             "may bring velocities of their own: call append_paths(trajs, keys, velocities=)")
        if self.within_path:
            raise ValueError("add_paths: the model has within-path deviations (path ids), and the new paths need ids of "
                             "their own: call append_paths(trajs, keys), which numbers them")
        return self.append_paths(trajs, keys)

    @_dense_only
    def append_paths(self, trajs, keys, velocities=None):
        """:meth:`add_paths` for every model (``GP.update`` with the rows' path ids or derivative rows where the model has
        them).  On a ``within_path`` model path i of ``keys`` gets the id ``len(self.keys) + i``, which continues the
        numbering of :func:`fit_path_models` (after a :meth:`remove_paths`: the next id no path has had).  On a model with velocities, ``velocities`` = {key: (L, k)} in raw units
        (target per unit of ``"t"``) become derivative rows under the model's normalisation, as at the fit; a key without
        an entry appends its values only.  ``velocities`` on a model without them: ``ValueError``.  Extends ``keys``;
        returns ``self``."""
        keys = list(keys)
        if velocities is not None and not self.has_velocities:
            raise ValueError("append_paths: velocities given, but the model was fitted without velocities")
        if not keys:
            return self
        if self.step_weights is not None and any(len(trajs.pathdict[q]) != len(self.step_weights) for q in keys):
            raise ValueError(f"append_paths: the model has per-step noise weights for paths of {len(self.step_weights)} points")
        X, Y, _ = to_gp_inputs(trajs, keys, inputs=self.inputs, targets=self.targets, normalise=False)
        Xn = np.ascontiguousarray((X - self.in_lo) / self.in_span)
        Yn = np.ascontiguousarray((Y - self.y_mean) / self.y_std)
        kw = {}
        if self.within_path:
            first = self._next_id
            kw["path_ids"] = np.concatenate([np.full(len(trajs.pathdict[q]), first + i, dtype=np.int32)
                                             for i, q in enumerate(keys)])
        if self.has_velocities:
            jt = self.inputs.index("t")
            rows, vals, at = [], [], 0
            for q in keys:
                L = len(trajs.pathdict[q])
                if velocities is not None and q in velocities:
                    v = np.asarray(velocities[q], dtype=np.float64)
                    if v.shape != (L, len(self.targets)):
                        raise ValueError(f"velocities[{q!r}] must be ({L}, {len(self.targets)}): one row per path point, "
                                         f"one column per target")
                    rows.append(np.arange(at, at + L))
                    vals.append(v * self.in_span[jt] / self.y_std[None, :])
                at += L
            at_rows = np.concatenate(rows) if rows else np.zeros(0, dtype=int)
            yd = np.concatenate(vals) if vals else np.zeros((0, len(self.targets)))
            kw["derivatives"] = (np.ascontiguousarray(Xn[at_rows]), jt, np.ascontiguousarray(yd))
        self.gp.update(Xn, Yn, noise_weights=self._tiled_weights(len(Xn), "append_paths"), **kw)
        for i, q in enumerate(keys):
            self._ids[q] = self._next_id + i
            if self._rows is not None:
                self._rows[q] = len(trajs.pathdict[q])
        self._next_id += len(keys)
        self.keys.extend(keys)
        return self

    @_dense_only
    def remove_paths(self, keys):
        """Take the paths ``keys`` out of this cluster's model (``GP.remove``: the factor of the other paths is updated, not
        computed again) — a path that went stale, was assigned to another cluster, or was a bad recording.  The result is
        the GP of the remaining paths under the normalisation fixed at the first fit.  A ``within_path`` model finds the
        rows by the path's id, and that id is never given to a later path; other models by the row counts recorded at the
        fit and at every append.  ``KeyError`` for a key the model does not hold (nothing is removed then);
        ``ValueError`` on a model with velocities, whose derivative rows are interleaved by :meth:`append_paths` and not
        recorded per key (``gp.remove(indices)`` remains available there), and when no path would be left.  Shortens
        ``keys``; returns ``self``."""
        keys = list(dict.fromkeys(keys))
        if self.has_velocities:
            raise ValueError("remove_paths: the model is conditioned on velocities, whose derivative rows are interleaved "
                             "with the value rows by append_paths and are not recorded per key: remove rows with "
                             "gp.remove(indices)")
        for q in keys:
            if q not in self._ids:
                raise KeyError(q)
        if not keys:
            return self
        if len(keys) >= len(self.keys):
            raise ValueError("remove_paths: a model keeps at least one path")
        if self.within_path:
            self.gp.remove(path_ids=[self._ids[q] for q in keys])
        else:
            if self._rows is None:
                raise ValueError("remove_paths: the model does not know its paths' row counts (it was not built by "
                                 "fit_path_models)")
            gone, at, idx = set(keys), 0, []
            for q in self.keys:
                n = self._rows[q]
                if q in gone:
                    idx.append(np.arange(at, at + n))
                at += n
            self.gp.remove(np.concatenate(idx))
        for q in keys:
            del self._ids[q]
            if self._rows is not None:
                del self._rows[q]
        gone = set(keys)
        self.keys = [q for q in self.keys if q not in gone]
        return self

    def _value_rows(self):
        """{key: indices of the key's value rows among the fit's rows}: by path id on a ``within_path`` model, else by the
        recorded row counts in ``keys`` order (value rows only: a model with velocities skips its derivative rows)"""
        if self.within_path:
            ids = np.asarray(self.gp.path_ids_)
            return {q: np.flatnonzero(ids == self._ids[q]) for q in self.keys}
        if self._rows is None:
            raise ValueError("loo: the model does not know its paths' row counts (it was not built by fit_path_models)")
        if self.has_velocities:
            values = np.flatnonzero(np.asarray(self.gp.observation_kinds_) == -1)
        else:
            values = np.arange(self.gp._N)
        if sum(self._rows[q] for q in self.keys) != len(values):
            raise ValueError("loo: the recorded row counts do not add up to the fit's value rows (rows were removed or "
                             "appended through the GP itself)")
        out, at = {}, 0
        for q in self.keys:
            out[q] = values[at:at + self._rows[q]]
            at += self._rows[q]
        return out

    @_dense_only
    def loo(self, keys=None):
        """Leave-one-out check of the model against its own paths (``GP.loo``; no refit): {key: (mean (L_key, k), std
        (L_key, k), z (L_key, k))} for ``keys`` (default: every path of the model), in the targets' own units.  Row s of a
        key is what the model fitted to every other observation — the other points of the same path included — predicts
        for point s of that path: ``mean``, the standard deviation ``std`` of that observation (its own noise included),
        and the standardised residual ``z = (y - mean) / std``.  A glitch in a recording is the (key, step) with the
        largest ``|z|``.  Only value rows are reported (a model with velocities leaves its derivative rows out).  Works on
        every model, also after :meth:`append_paths` / :meth:`remove_paths`; ``KeyError`` for a key the model does not
        hold, ``ValueError`` when the paths' row counts are not recorded (a model not built by
        :func:`fit_path_models`, unless it is ``within_path``)."""
        keys = self.keys if keys is None else list(keys)
        for q in keys:
            if q not in self._ids:
                raise KeyError(q)
        rows = self._value_rows()
        mean, var = self.gp.loo(return_var=True)
        mean = np.asarray(mean, dtype=np.float64).reshape(len(var), -1)
        alpha = np.asarray(self.gp.alpha_, dtype=np.float64).reshape(len(var), -1)
        resid = alpha * var[:, None]  # y - mean = alpha / Q_ii, in the model's normalised units
        std = np.sqrt(var)[:, None]
        out = {}
        for q in keys:
            r = rows[q]
            out[q] = (mean[r] * self.y_std + self.y_mean, std[r] * self.y_std[None, :], resid[r] / std[r])
        return out

    @_dense_only
    def log_likelihood(self, paths_txy, include_noise=True):
        """How likely whole paths are under this cluster's model: ``paths_txy`` (P, L, 3) raw (t, x, y) paths of one
        length L <= 64 -> (P, k) log-densities of each path's targets, in the targets' own units, under the joint
        posterior of its L points (``GP.score_blocks`` on the device: the points of a path are strongly correlated, so
        this is not the sum of the per-point densities).  Inputs and targets go through the model's normalisation; the
        Jacobian of the standardisation, ``-L log y_std[c]``, is included, so models with different standardisations
        are comparable.  A model with ``step_weights`` scores with them (point s of a path gets ``noise * w_s``); paths
        of another length than its own then raise ``ValueError``."""
        arr = np.asarray(paths_txy, dtype=np.float64)
        if arr.ndim != 3 or arr.shape[2] != 3 or arr.shape[0] == 0:
            raise ValueError("paths must be a non-empty (P, L, 3) array of (t, x, y)")
        P, L = arr.shape[:2]
        if self.step_weights is not None and L != len(self.step_weights):
            raise ValueError(f"log_likelihood: the model has per-step noise weights for paths of {len(self.step_weights)} "
                             f"points, these have {L}")
        col = {"t": 0, "x": 1, "y": 2}
        flat = arr.reshape(-1, 3)
        Xn = np.ascontiguousarray((flat[:, [col[c] for c in self.inputs]] - self.in_lo) / self.in_span)
        Yn = np.ascontiguousarray((flat[:, [col[c] for c in self.targets]] - self.y_mean) / self.y_std)
        logp = self.gp.score_blocks(Xn, Yn, L, include_noise=include_noise,
                                    noise_weights=self._tiled_weights(P * L, "log_likelihood"))
        return np.asarray(logp, dtype=np.float64).reshape(P, -1) - L * np.log(self.y_std)[None, :]

    @_dense_only
    def forecast(self, prefix_txy, t_future, include_noise=True, return_logp=False):
        """Where partly observed paths of this cluster go: ``prefix_txy`` (P, Lo, 3) raw (t, x, y), the first Lo points
        of P new paths, ``t_future`` (Lp,) raw time stamps shared by the paths or (P, Lp) (``t`` must be the model's only
        input; Lo + Lp <= 64) -> ``(mean (P, Lp, k), cov (P, k, Lp, Lp))`` in the targets' own units: each path is a new
        member of the cluster conditioned on its prefix (``GP.forecast_blocks``).  On a ``within_path`` model the prefix
        pins the path's own deviation down; on any other model it barely moves the cluster mean.  ``return_logp``: a
        third entry (P, k), the joint log-density of each prefix in the targets' own units (``-Lo log y_std`` included,
        as :meth:`log_likelihood`), from the same call.  The observed points get the model's ``noise`` as it is, also on
        a model with ``step_weights``."""
        arr = np.asarray(prefix_txy, dtype=np.float64)
        if arr.ndim != 3 or arr.shape[2] != 3 or arr.shape[0] == 0 or arr.shape[1] == 0:
            raise ValueError("prefixes must be a non-empty (P, Lo, 3) array of (t, x, y)")
        if self.inputs != ("t",):
            raise ValueError(f"forecast() needs 't' as the model's only input, have {self.inputs}")
        P, Lo = arr.shape[:2]
        tf = np.asarray(t_future, dtype=np.float64)
        if tf.ndim == 1:
            tf = np.broadcast_to(tf, (P, tf.shape[0]))
        if tf.ndim != 2 or tf.shape[0] != P or tf.shape[1] == 0:
            raise ValueError(f"t_future must be (Lp,) or ({P}, Lp)")
        Lp = tf.shape[1]
        col = {"t": 0, "x": 1, "y": 2}
        flat = arr.reshape(-1, 3)
        Xo = np.ascontiguousarray((flat[:, [0]] - self.in_lo) / self.in_span)
        Yo = np.ascontiguousarray((flat[:, [col[c] for c in self.targets]] - self.y_mean) / self.y_std)
        Xp = np.ascontiguousarray((tf.reshape(-1, 1) - self.in_lo) / self.in_span)
        mean, cov, logp = self.gp.forecast_blocks(Xo, Yo, Xp, blocks=P, include_noise=include_noise, return_logp=True)
        mean = np.asarray(mean, dtype=np.float64).reshape(P, Lp, -1) * self.y_std + self.y_mean
        cov = np.asarray(cov, dtype=np.float64)[:, None, :, :] * (self.y_std ** 2)[None, :, None, None]
        if not return_logp:
            return mean, cov
        return mean, cov, np.asarray(logp, dtype=np.float64).reshape(P, -1) - Lo * np.log(self.y_std)[None, :]

    def close(self):
        self.gp.close()


STEP_WEIGHT_FLOOR = 1e-3


def step_noise_weights(Yn, n_paths):
    """Per-step noise weights of one cluster: ``Yn`` (n_paths * L, k) standardised targets, path after path.  The
    weight of step s is the variance over the paths of the targets at step s (about their mean path), averaged over
    the targets, divided by its mean over the steps and floored at 1e-3 — the spread of the cluster along the path,
    relative to its average.  (L,); all ones for a single path (or paths without any spread)."""
    Y3 = np.asarray(Yn, dtype=np.float64).reshape(n_paths, -1, Yn.shape[-1] if np.ndim(Yn) > 1 else 1)
    v = Y3.var(axis=0).mean(axis=1)
    if n_paths < 2 or not v.mean() > 0:
        return np.ones(Y3.shape[1])
    return np.maximum(v / v.mean(), STEP_WEIGHT_FLOOR)


def fit_path_models(trajs, clusters, inputs=("t",), targets=("x", "y"), devices=None, optimize=False,
                    lengthscale=0.25, variance=1.0, noise=0.05, step_noise=False, velocities=None, velocity_noise=0.05,
                    learn_velocity_noise=False, within_path=False, path_variance=0.25, path_lengthscale=None,
                    learn_path_parameters=False, trend=None, inducing=None, **gp_kwargs):
    """One exact GP per cluster of ``clusters`` = {cluster id: [path ids]} — what
    :func:`kmeans` (``kmeansclustering``, GPmap.py:36-93) returns — modelling the cluster's paths
    as (x(t), y(t)); the modelling step the reference's title names and its clustering prepares
    (the reference itself stops after the clustering, GPmap.py:220).

    The clusters are independent problems, so they run as REPLICAS (SURVEY.md §8e "Replicas-only
    parts"): cluster i is fitted on ``devices[i % len(devices)]`` (an int n = devices 0..n-1;
    default: the current device), one host thread per device, no data-path collective.  With
    ``optimize`` the hyper-parameters of each model are fitted by :meth:`GP.optimize` (analytic
    gradient, with ``velocities`` as well) first.  ``step_noise``: the paths of a cluster are tight in some places and spread out in others, so each
    cluster's observations get per-step noise weights (:func:`step_noise_weights`, tiled over its paths; the paths
    of a cluster have one length); ``noise`` stays the level, and the model keeps them as ``step_weights``.
    ``velocities`` = {path id: (L, k)}: observed velocities of (some of) the paths — tracker or odometry output — one row
    per path point and one column per target, in raw target units per raw time unit.  Needs ``"t"`` among the inputs.
    They condition the cluster's GP as derivative observations along ``"t"`` at the path's own points
    (``GP.fit(derivatives=)``), normalised by the chain rule ``v * in_span[t] / y_std[c]``; ``velocity_noise`` is their
    noise variance in those normalised units (as ``noise`` is for the positions).  ``optimize`` keeps it fixed unless
    ``learn_velocity_noise`` is set: then each cluster that has velocities learns its own, starting from ``velocity_noise``
    (which must be > 0), and :attr:`PathModel.velocity_noise` reports it.
    ``within_path``: fit the hierarchical model — every path is the cluster mean plus a deviation of its own, a GP with
    variance ``path_variance`` (normalised target units) and lengthscale ``path_lengthscale`` (None: ``lengthscale``):
    ``GP.fit(path_ids=repeat(arange(P), L))`` per cluster.  Whole-path likelihoods then stay calibrated however many paths
    a cluster has, and :meth:`PathModel.forecast` / :func:`forecast_paths` continue a partly observed path.  Not with
    ``velocities``.  ``optimize`` keeps the two fixed unless ``learn_path_parameters`` is set: then each cluster learns its
    own with the others (analytic gradient, ``GP.lml_gradient(path=True)``), starting from the values passed, and the
    model's ``gp.path_variance`` and ``gp.path_lengthscale`` report them (``ValueError`` without ``within_path`` or without
    ``optimize``).
    ``trend`` = "constant", "linear" or "quadratic": every cluster's GP gets an explicit mean in its normalised inputs
    with marginalised coefficients (``GP.fit(basis=)``), so the plug-in standardisation no longer has to carry the trend
    and its uncertainty reaches the variances; stored on the model as ``trend``.  Not with ``velocities`` or
    ``within_path``.  None (the default) changes nothing.
    ``inducing`` = m (an int): every cluster gets an inducing-point fit (``SparseGP``: m points, equally spaced over the
    cluster's normalised inputs when there is one input, else a seeded subset of its distinct rows) instead of a dense
    one — for clusters of tens of thousands of paths, whose observations no dense factor holds.  The models are
    ``sparse`` (:class:`PathModel`): ``predict`` only.  Of ``gp_kwargs`` only ``kernel``, ``jitter`` (None: 1e-8 *
    ``variance``, on K_uu — a change of model, not of noise) and ``chunk`` apply.  Not with ``velocities``,
    ``within_path``, ``trend`` or ``optimize`` (``ValueError``).  None (the default) changes nothing.
    Returns {cluster id: :class:`PathModel`}; empty clusters are skipped."""
    import threading
    from concurrent.futures import ThreadPoolExecutor
    from .gp import GP
    if inducing is not None:
        if isinstance(inducing, bool) or not isinstance(inducing, (int, np.integer)) or inducing < 1:
            raise ValueError("inducing must be None or an int >= 1 (the number of inducing points per cluster)")
        for name, on in (("velocities", bool(velocities)), ("within_path", within_path), ("trend", trend is not None),
                         ("optimize", optimize)):
            if on:
                raise ValueError(f"inducing cannot be combined with {name}: an inducing-point fit takes plain value "
                                 "observations and fixed hyper-parameters")
        extra = sorted(set(gp_kwargs) - {"kernel", "jitter", "chunk"})
        if extra:
            raise ValueError(f"inducing: a sparse model takes kernel, jitter and chunk, not {extra}")
    if devices is None:
        devs = [None]
    elif isinstance(devices, (int, np.integer)):
        if devices < 1:
            raise ValueError("devices must be >= 1")
        devs = list(range(int(devices)))
    else:
        devs = [int(v) for v in devices]
        if not devs:
            raise ValueError("devices must not be empty")
    known = set(trajs.keys())
    velocities = dict(velocities) if velocities else {}
    if velocities and "t" not in inputs:
        raise ValueError(f"velocities need 't' among the inputs, have {tuple(inputs)}")
    if within_path and velocities:
        raise ValueError("within_path cannot be combined with velocities (path ids and derivative observations)")
    GP._check_basis(trend)
    if trend is not None and (velocities or within_path):
        raise ValueError("trend cannot be combined with velocities or within_path (basis functions with derivative "
                         "observations or path ids)")
    if learn_path_parameters and not (within_path and optimize):
        raise ValueError("learn_path_parameters needs within_path=True and optimize=True")
    jobs = []
    for cid, keys in clusters.items():
        keys = list(keys)
        if not keys:
            continue
        missing = [q for q in keys if q not in known]
        if missing:
            raise KeyError(f"cluster {cid!r} names unknown paths {missing[:3]}")
        jobs.append((cid, keys))

    def cluster_velocities(keys, X, span, sd):
        """(Xd, dims, yd) of the cluster's paths that have velocities (None: none has): derivative observations along "t"
        at the normalised inputs of those paths' own points, d target / d t_normalised = v * span[t] / y_std"""
        jt = tuple(inputs).index("t") if velocities else 0
        rows, vals, at = [], [], 0
        for q in keys:
            L = len(trajs.pathdict[q])
            if q in velocities:
                v = np.asarray(velocities[q], dtype=np.float64)
                if v.shape != (L, len(targets)):
                    raise ValueError(f"velocities[{q!r}] must be ({L}, {len(targets)}): one row per path point, one column "
                                     f"per target")
                rows.append(np.arange(at, at + L))
                vals.append(v * span[jt] / sd[None, :])
            at += L
        if not rows:
            return None
        return np.ascontiguousarray(X[np.concatenate(rows)]), jt, np.ascontiguousarray(np.concatenate(vals))

    def fit_one(slot, cid, keys):
        X, Y, (lo, span) = to_gp_inputs(trajs, keys, inputs=inputs, targets=targets, normalise=True)
        mu = Y.mean(axis=0)
        sd = Y.std(axis=0)
        sd = np.where(sd > 0, sd, 1.0)
        Yn = np.ascontiguousarray((Y - mu) / sd)
        if inducing is not None:
            from .sparse import SparseGP
            sw = step_noise_weights(Yn, len(keys)) if step_noise else None
            gp = SparseGP(lengthscale=lengthscale, variance=variance, noise=noise, device=devs[slot % len(devs)], **gp_kwargs)
            try:
                gp.fit(X, Yn, inducing=int(inducing), noise_weights=None if sw is None else np.tile(sw, len(keys)))
            except Exception:
                gp.close()
                raise
            return cid, PathModel(gp, keys, lo, span, mu, sd, inputs, targets, step_weights=sw,
                                  row_counts=[len(trajs.pathdict[q]) for q in keys], sparse=True)
        der = cluster_velocities(keys, X, span, sd)
        gp = GP(lengthscale=lengthscale, variance=variance, noise=noise, device=devs[slot % len(devs)],
                **gp_kwargs)
        sw = step_noise_weights(Yn, len(keys)) if step_noise else None
        w = None if sw is None else np.tile(sw, len(keys))
        kw = {} if der is None else dict(derivatives=der, derivative_noise=velocity_noise)
        if trend is not None:
            kw["basis"] = trend
        if within_path:
            kw.update(path_ids=np.concatenate([np.full(len(trajs.pathdict[q]), p, dtype=np.int32) for p, q in enumerate(keys)]),
                      path_variance=path_variance, path_lengthscale=path_lengthscale)
        try:
            if optimize:
                if learn_velocity_noise and der is not None:
                    kw["params"] = ("lengthscale", "variance", "noise", "derivative_noise")
                if learn_path_parameters:
                    kw["params"] = ("lengthscale", "variance", "noise", "path_variance", "path_lengthscale")
                gp.optimize(X, Yn, noise_weights=w, **kw)  # leaves the model fitted at the best point
            else:
                gp.fit(X, Yn, noise_weights=w, **kw)
        except Exception:
            gp.close()
            raise
        return cid, PathModel(gp, keys, lo, span, mu, sd, inputs, targets, step_weights=sw, has_velocities=der is not None,
                              within_path=within_path, row_counts=[len(trajs.pathdict[q]) for q in keys], trend=trend)

    by_dev = [[] for _ in devs]                    # one worker per device, its clusters in order
    for i, (cid, keys) in enumerate(jobs):
        by_dev[i % len(devs)].append((i, cid, keys))
    models = {}
    lock = threading.Lock()

    def worker(lst):
        # every model is filed the moment it exists: if a later cluster of this device raises, the
        # ones already built are still in `models` and get closed below (their factors live on the GPU)
        for i, c, k in lst:
            cid, m = fit_one(i, c, k)
            with lock:
                models[cid] = m

    with ThreadPoolExecutor(max_workers=len(devs)) as pool:
        futs = [pool.submit(worker, lst) for lst in by_dev if lst]
        err = None
        for f in futs:
            try:
                f.result()
            except Exception as e:                  # keep collecting so every handle gets closed
                err = err or e
        if err is not None:
            for m in models.values():
                m.close()
            raise err
    return {cid: models[cid] for cid, _ in jobs}


# ---- which cluster does a path belong to: whole-path likelihood under every cluster's GP ----------
def path_log_likelihood_matrix(trajs, models, keys=None):
    """``(keys, LL)``: LL[p, c] = log-density of path ``keys[p]`` of ``trajs`` under model c of ``models`` =
    {cluster id: :class:`PathModel`} (column order = ``models``' order), summed over the targets
    (:meth:`PathModel.log_likelihood`).  The GP counterpart of :func:`path_distance_matrix`: it weighs a deviation
    by what the cluster's own paths do at that point of the path, and it is a density, so an anomalous path shows
    as a low maximum over the clusters."""
    keys = trajs.keys() if keys is None else list(keys)
    arr = trajs.as_array(keys)
    LL = np.empty((len(keys), len(models)), dtype=np.float64)
    if keys:
        for c, m in enumerate(models.values()):
            LL[:, c] = m.log_likelihood(arr).sum(axis=1)
    return keys, LL


def assign_paths(trajs, models, keys=None):
    """{cluster id: [path ids]} by the largest whole-path log-likelihood (first maximum on ties) — the shape
    :func:`kmeans` returns, so each list can go straight to that cluster's :meth:`PathModel.append_paths` (every model;
    :meth:`PathModel.add_paths` serves plain and step-noise models only)."""
    keys, LL = path_log_likelihood_matrix(trajs, models, keys)
    cids = list(models.keys())
    best = np.argmax(LL, axis=1) if keys else np.zeros(0, dtype=int)
    return {cid: [keys[p] for p in np.nonzero(best == c)[0]] for c, cid in enumerate(cids)}


def forecast_paths(prefixes, t_future, models, include_noise=True):
    """Continue partly observed paths under every cluster's model: ``prefixes`` (P, Lo, 3) raw (t, x, y), ``t_future`` (Lp,)
    or (P, Lp), ``models`` = {cluster id: :class:`PathModel`} -> ``(weights (P, C), means, covs)``: ``weights[p, c]`` the
    posterior probability (equal priors) that path p belongs to cluster c — the softmax over the clusters of the prefix
    log-likelihoods summed over the targets, which come from the same call as the forecasts — and ``means`` / ``covs`` =
    {cluster id: (P, Lp, k) / (P, k, Lp, Lp)}, :meth:`PathModel.forecast` under each cluster (column order = ``models``'
    order).  The mixture over the clusters with these weights is the forecast of a path whose cluster is not known."""
    P = np.asarray(prefixes).shape[0]
    LL = np.empty((P, len(models)), dtype=np.float64)
    means, covs = {}, {}
    for c, (cid, m) in enumerate(models.items()):
        means[cid], covs[cid], logp = m.forecast(prefixes, t_future, include_noise=include_noise, return_logp=True)
        LL[:, c] = logp.sum(axis=1)
    w = np.exp(LL - LL.max(axis=1, keepdims=True))
    return w / w.sum(axis=1, keepdims=True), means, covs
