"""Helpers of tests/test_handle_history_gpu.py: the model specs, the walks over them, ``observe`` (every call a fitted
model answers, every output), the table of the calls a model kind refuses, and the CPU anchors of every spec.

Nothing here touches a device at import: the sequence checks and the refusal table are plain Python and are tested
without a GPU.  Inputs are drawn once from fixed seeds, cached and write-protected."""
import contextlib
import functools
import os
import sys
from collections import namedtuple

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

# ---- handles ---------------------------------------------------------------------------------------------------------------
HANDLES = {
    "matern32_f64": dict(kernel="matern32", dtype="float64", block=128),   # several panels from N = 300 on
    "rbf_f32": dict(kernel="rbf", dtype="float32"),                        # the library's panel width: S2 has two panels
    "matern12_f64": dict(kernel="matern12", dtype="float64"),              # no derivatives of any kind
}

# ---- model specs -----------------------------------------------------------------------------------------------------------
# kind: what the fit is made with; (N, d, k): the rows, inputs and targets of the model the spec leaves behind.  Every spec
# has its own lengthscale, variance and noise: a stale value of any of them on the device changes every output.
Spec = namedtuple("Spec", "name kind N d k ls sf2 sn2")
SPECS = {s.name: s for s in (
    Spec("S1", "plain", 300, 3, 2, (0.35, 0.25, 0.3), 1.5, 0.05),
    Spec("S2", "plain", 1100, 2, 9, 0.3, 2.0, 0.1),
    Spec("S3", "plain", 70, 1, 1, 0.2, 0.8, 0.08),
    Spec("S4", "weights", 129, 1, 1, 0.15, 1.2, 0.06),
    Spec("S5", "derivatives", 260, 3, 1, (0.4, 0.3, 0.35), 0.9, 0.07),
    Spec("S6", "paths", 106, 2, 2, (0.28, 0.4), 1.3, 0.09),
    Spec("S7", "basis", 200, 3, 1, (0.32, 0.36, 0.42), 1.1, 0.04),
    Spec("S8", "fused", 300, 3, 2, (0.35, 0.25, 0.3), 1.5, 0.05),
    Spec("S9", "resized", 307, 3, 2, (0.35, 0.25, 0.3), 1.5, 0.05),
    Spec("S10", "paths_resized", 110, 2, 2, (0.28, 0.4), 1.3, 0.09),
    # not part of a walk: the model of tests/test_append_gpu.py's failed append (K of the fitted points is the identity to
    # the last bit, no noise, no jitter: a point appended twice has a second pivot of exactly 0)
    Spec("T1", "plain", 300, 1, 1, 1.0, 1.0, 0.0),
)}
WALK_SPECS = tuple(n for n in SPECS if n != "T1")
JITTER = 1e-10                                                   # every spec's, but T1's 0
PLAIN = ("S1", "S3")
FEATURES = ("S4", "S5", "S6", "S7", "S9", "S10")
NO_DERIVATIVES = ("S1", "S2", "S3", "S4", "S6", "S7", "S10")     # what a Matern-1/2 handle can fit
S5_VALUES, S5_DERIVS, S5_DERIV_NOISE = 200, 60, 1e-3
S6_PATHS, S6_ROWS, S6_LOOSE, S6_SG2, S6_LSP = 6, 16, 10, 0.4, (0.12, 0.2)
S9_RESERVE, S9_NEW, S9_CUT = 600, 77, (40, 110)
S10_NEW_OLD, S10_NEW_PATH, S10_GONE = 8, 12, 2                   # 8 rows more of path 4, 12 rows of the new path 7; path 2 leaves
ANCHORS = 8                                                      # rows 0..7 of every training set with d inputs are the same points

# The walks.  check_sequence() holds them to the rules of the test's docstring, so an edit cannot thin them out.
FULL_WALK = ("S3", "S1", "S9", "S2", "S8", "S5", "S7", "S5", "S3", "S7", "S3", "S4", "S6", "S4", "S3", "S6", "S3", "S10",
             "S9", "S6", "S2", "S10", "S3", "S8", "S4", "S9", "S1", "S9", "S8")
MATERN12_WALK = ("S3", "S4", "S6", "S3", "S7", "S4", "S3", "S10", "S7", "S3", "S1", "S7", "S2", "S6", "S10", "S3", "S2",
                 "S10", "S1", "S3", "S6")
WALKS = {"matern32_f64": FULL_WALK, "rbf_f32": FULL_WALK, "matern12_f64": MATERN12_WALK}


def dominates(a, b):
    """spec a is the larger model: no fewer inputs and targets, and more rows"""
    return a.N > b.N and a.d >= b.d and a.k >= b.k


def check_sequence(walk, allowed):
    """-> list of the rules the walk breaks (empty: none).  ``allowed``: the specs the handle can fit; every one occurs."""
    specs = [SPECS[n] for n in allowed]
    pairs = list(zip(walk[:-1], walk[1:]))
    preds = {n: {a for a, b in pairs if b == n} for n in allowed}
    succs = {n: {b for a, b in pairs if a == n} for n in allowed}
    bad = [f"{n} is not a spec of this handle" for n in walk if n not in allowed]
    bad += [f"{a} follows itself" for a, b in pairs if a == b]
    for s in specs:
        n = s.name
        if walk.count(n) < 2 or len(preds[n] | ({None} if walk[0] == n else set())) < 2:
            bad.append(f"{n} does not occur twice with different predecessors")
        if any(dominates(o, s) for o in specs) and not any(dominates(SPECS[p], s) for p in preds[n]):
            bad.append(f"{n} never follows a larger model")
        if any(dominates(s, o) for o in specs) and not any(dominates(s, SPECS[p]) for p in preds[n]):
            bad.append(f"{n} never follows a smaller model")
        if n in FEATURES:
            if not any(b in PLAIN and SPECS[b].N < s.N for b in succs[n]):
                bad.append(f"{n} is never followed directly by a plain spec of smaller N")
            if not any(b in FEATURES and SPECS[b].kind != s.kind for b in succs[n]):
                bad.append(f"{n} is never followed directly by a different feature spec")
    if "S8" in allowed and ("S2", "S8") not in pairs:   # (the walk makes S2's large queries: more scratch than S8's 70 points)
        bad.append("S8 never follows S2 and its large queries")
    if "S9" in allowed and not any(a == "S9" and SPECS[b].N > S9_RESERVE for a, b in pairs):
        bad.append("S9 is never followed by a model larger than its reserve")
    return bad


# ---- inputs ----------------------------------------------------------------------------------------------------------------
def _frozen(*arrays):
    for a in arrays:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def anchors(d):
    """the eight training points every spec with d inputs shares: the queries repeat them"""
    return _frozen(np.random.default_rng(900 + d).uniform(0.05, 0.95, (ANCHORS, d)))[0]


def _truth(d, k):
    a = np.random.default_rng(700 + 10 * d + k).uniform(2.0, 5.0, (d, k))

    def f(A):
        return np.sin(A @ a) + 0.3 * np.cos(2.0 * A.sum(axis=1, keepdims=True))

    def df(A, dims):
        return np.cos(A @ a) * a[dims, :] - 0.6 * np.sin(2.0 * A.sum(axis=1, keepdims=True))
    return f, df


def _targets(Y, k):
    return np.ascontiguousarray(Y[:, 0] if k == 1 else Y)      # a 1-D y for one target: the other output shapes


def _points(rng, n, d):
    X = rng.uniform(0.0, 1.0, (n, d))
    X[:ANCHORS] = anchors(d)
    return X


@functools.lru_cache(maxsize=None)
def data(name):
    """the arguments of spec `name`, as a dict of read-only arrays"""
    if name == "T1":
        return dict(zip(("X", "Y"), _frozen(100.0 * np.arange(300, dtype=np.float64)[:, None],
                                            np.sin(np.arange(300, dtype=np.float64)))))
    s = SPECS["S1" if name in ("S8", "S9") else "S6" if name == "S10" else name]
    rng = np.random.default_rng(100 + int(s.name[1:]))
    f, df = _truth(s.d, s.k)
    n = S5_VALUES if s.kind == "derivatives" else s.N
    X = _points(rng, n, s.d)
    Y = f(X) + np.sqrt(s.sn2) * rng.standard_normal((n, s.k))
    out = {}
    if s.kind == "weights":
        w = np.exp(rng.uniform(np.log(0.2), np.log(5.0), n))
        w[::43] = 0.0                                          # exact observations, the anchor row 0 among them
        out["w"] = w
    if s.kind == "derivatives":
        out["Xd"] = rng.uniform(0.0, 1.0, (S5_DERIVS, s.d))
        out["dims"] = rng.integers(0, s.d, S5_DERIVS)
        out["yd"] = _targets(df(out["Xd"], out["dims"]) + 0.03 * rng.standard_normal((S5_DERIVS, s.k)), s.k)
    if s.kind == "paths":
        ids = np.concatenate([np.repeat(np.arange(S6_PATHS), S6_ROWS), np.full(S6_LOOSE, -1)]).astype(np.int64)
        Y = Y + np.where(ids >= 0, 0.4 * np.sin(6.0 * X[:, 0] + ids), 0.0)[:, None]
        out["ids"] = ids
    if s.kind == "basis":
        Y = Y + 1.0 + X @ np.array([[2.0], [-1.0], [0.5]])
        out["w"] = np.exp(rng.uniform(np.log(0.2), np.log(5.0), n))
    out["X"], out["Y"] = X, _targets(Y, s.k)
    if name == "S9":
        r9 = np.random.default_rng(109)
        Xn = r9.uniform(0.0, 1.0, (S9_NEW, s.d))
        out["Xn"], out["Yn"] = Xn, f(Xn) + np.sqrt(s.sn2) * r9.standard_normal((S9_NEW, s.k))
    if name == "S10":
        r10 = np.random.default_rng(110)
        m = S10_NEW_OLD + S10_NEW_PATH
        Xn = r10.uniform(0.0, 1.0, (m, s.d))
        idn = np.concatenate([np.full(S10_NEW_OLD, 4), np.full(S10_NEW_PATH, 7)]).astype(np.int64)
        out["Xn"], out["idn"] = Xn, idn
        out["Yn"] = f(Xn) + 0.4 * np.sin(6.0 * Xn[:, :1] + idn[:, None]) + np.sqrt(s.sn2) * r10.standard_normal((m, s.k))
    _frozen(*out.values())
    return out


def final_rows(name):
    """-> dict(X, Y, ids | None): the rows the model of spec `name` holds at the end (S9, S10: after update and remove)"""
    c = data(name)
    X, Y, ids = c["X"], c["Y"], c.get("ids")
    if name == "S9":
        keep = np.ones(SPECS["S1"].N + S9_NEW, dtype=bool)
        keep[S9_CUT[0]:S9_CUT[1]] = False
        X, Y = np.concatenate([X, c["Xn"]])[keep], np.concatenate([Y, c["Yn"]])[keep]
    if name == "S10":
        ids = np.concatenate([ids, c["idn"]])
        keep = ids != S10_GONE
        X, Y, ids = np.concatenate([X, c["Xn"]])[keep], np.concatenate([Y, c["Yn"]])[keep], ids[keep]
    assert len(X) == SPECS[name].N or SPECS[name].kind == "derivatives"
    return dict(X=X, Y=Y, ids=ids)


@functools.lru_cache(maxsize=None)
def queries(d, k):
    """the query inputs of every model with d inputs and k targets, drawn once: dict of read-only arrays"""
    rng = np.random.default_rng(1000 * d + k)
    f, _ = _truth(d, k)
    Xq = rng.uniform(-0.05, 1.05, (70, d))
    Xq[:ANCHORS] = anchors(d)                                    # points of the training set itself
    Xq[ANCHORS:ANCHORS + 3] = rng.uniform(2.0, 3.0, (3, d))      # and points well outside the data
    Xq[ANCHORS + 3:ANCHORS + 6] = rng.uniform(-2.0, -1.0, (3, d))
    q = dict(Xq=Xq, Xq5=np.ascontiguousarray(Xq[[0, 9, 20, 40, 69]]), z=rng.standard_normal((3, 70, k)))
    q["gq"] = np.where(np.arange(70) % 4 == 0, -1, np.arange(70) % S6_PATHS).astype(np.int64)
    q["gq"][5::17] = 99                                          # a path no fit here has seen
    t = np.linspace(0.0, 1.0, 17)[None, :, None]
    p0, p1 = rng.uniform(0.0, 1.0, (3, 1, d)), rng.uniform(0.0, 1.0, (3, 1, d))
    q["Xb"] = (p0 + t * (p1 - p0)).reshape(-1, d)                # 3 blocks of 17: straight paths through the box
    q["Xb"][0] = anchors(d)[0]
    q["Yb"] = _targets(f(q["Xb"]) + 0.2 * rng.standard_normal((51, k)), k)
    t = np.linspace(0.0, 1.0, 9)[None, :, None]
    p0, p1 = rng.uniform(0.0, 1.0, (3, 1, d)), rng.uniform(0.0, 1.0, (3, 1, d))
    Xf = p0 + t * (p1 - p0)                                      # G = 3 paths of Lo + Lp = 5 + 4 points
    q["Xo"], q["Xp"] = np.ascontiguousarray(Xf[:, :5].reshape(-1, d)), np.ascontiguousarray(Xf[:, 5:].reshape(-1, d))
    q["Yo"] = _targets(f(q["Xo"]) + 0.2 * rng.standard_normal((15, k)), k)
    # the decoys: the same calls at larger sizes
    q["Xq700"] = rng.uniform(-0.1, 1.1, (700, d))
    q["Xq200"], q["z200"] = np.ascontiguousarray(q["Xq700"][:200]), rng.standard_normal((8, 200, k))
    t = np.linspace(0.0, 1.0, 33)[None, :, None]
    p0, p1 = rng.uniform(0.0, 1.0, (40, 1, d)), rng.uniform(0.0, 1.0, (40, 1, d))
    q["Xb40"] = (p0 + t * (p1 - p0)).reshape(-1, d)
    q["Yb40"] = _targets(f(q["Xb40"]) + 0.2 * rng.standard_normal((40 * 33, k)), k)
    t = np.linspace(0.0, 1.0, 64)[None, :, None]
    p0, p1 = rng.uniform(0.0, 1.0, (3, 1, d)), rng.uniform(0.0, 1.0, (3, 1, d))
    Xf = p0 + t * (p1 - p0)
    q["Xo64"], q["Xp64"] = np.ascontiguousarray(Xf[:, :40].reshape(-1, d)), np.ascontiguousarray(Xf[:, 40:].reshape(-1, d))
    q["Yo64"] = _targets(f(q["Xo64"]) + 0.2 * rng.standard_normal((120, k)), k)
    _frozen(*q.values())
    return q


# ---- making the model of a spec ---------------------------------------------------------------------------------------------
def make(handle):
    from gaussianprocesspathmodelling_amd import GP
    return GP(**HANDLES[handle])


def apply(gp, name, pause=None):
    """give the handle the model of spec `name`: its hyper-parameters, its reserve and its fit / update / remove calls.
    -> dict of what the fitting calls themselves returned (S8: the fused pass's prediction).  ``pause()`` runs between
    the fit, the update and the remove of S9 and S10."""
    s, c = SPECS[name], data(name)
    pause = pause or (lambda: None)
    gp.lengthscale = np.atleast_1d(np.asarray(s.ls, dtype=np.float64)).copy()
    gp.variance, gp.noise, gp.jitter = s.sf2, s.sn2, (0.0 if name == "T1" else JITTER)
    want = S9_RESERVE if name == "S9" else 0
    if getattr(gp, "_history_reserve", 0) != want:               # (a handle that never reserved makes no call at all)
        gp.reserve(want)
        gp._history_reserve = want
    out = {}
    if s.kind in ("plain", "resized"):
        gp.fit(c["X"], c["Y"])
    elif s.kind == "weights":
        gp.fit(c["X"], c["Y"], noise_weights=c["w"])
    elif s.kind == "derivatives":
        gp.fit(c["X"], c["Y"], derivatives=(c["Xd"], c["dims"], c["yd"]), derivative_noise=S5_DERIV_NOISE)
    elif s.kind in ("paths", "paths_resized"):
        gp.fit(c["X"], c["Y"], path_ids=c["ids"], path_variance=S6_SG2, path_lengthscale=S6_LSP)
    elif s.kind == "basis":
        gp.fit(c["X"], c["Y"], basis="linear", noise_weights=c["w"])
    elif s.kind == "fused":
        mean, var = gp.fit_predict(c["X"], c["Y"], queries(s.d, s.k)["Xq"])
        out = {"fit_predict.mean": mean, "fit_predict.var": var}
    if s.kind == "resized":
        pause()
        gp.update(c["Xn"], c["Yn"])
        pause()
        gp.remove(*S9_CUT)
    if s.kind == "paths_resized":
        pause()
        gp.update(c["Xn"], c["Yn"], path_ids=c["idn"])
        pause()
        gp.remove(path_ids=[S10_GONE])
    return out


# ---- the decoys: the calls of observe() at larger sizes, results thrown away -------------------------------------------------
def _on_device(gp, *arrays):
    import torch
    dt = torch.float32 if gp.dtype == "float32" else torch.float64
    return [torch.from_numpy(np.array(a)).to(device=f"cuda:{gp.device}", dtype=dt) for a in arrays]


def _decoy_device(gp, s, q):
    Xq, Xb, Yb = _on_device(gp, q["Xq200"], q["Xb40"], q["Yb40"])
    mean, var = gp.predict(Xq)
    assert mean.is_cuda and var.is_cuda
    gp.predict(Xq, return_cov=True)
    gp.score_blocks(Xb, Yb, 33)


DECOYS = {
    "predict700": lambda gp, s, q: (gp.predict(q["Xq700"]), gp.predict(q["Xq700"], return_var=False)),
    "cov200": lambda gp, s, q: (gp.predict(q["Xq200"], return_cov=True), gp.sample_y(q["Xq200"], 8, z=q["z200"]),
                               gp.sample_y(q["Xq200"], 8, random_state=11)),
    "gradient700": lambda gp, s, q: gp.predict_gradient(q["Xq700"], with_value=True),
    "score40x33": lambda gp, s, q: gp.score_blocks(q["Xb40"], q["Yb40"], 33, return_parts=True),
    "forecast64": lambda gp, s, q: gp.forecast_blocks(q["Xo64"], q["Yo64"], q["Xp64"], blocks=3, return_logp=True),
    "device": _decoy_device,
}


def decoy(gp, name, which):
    s = SPECS[name]
    DECOYS[which](gp, s, queries(s.d, s.k))


# ---- the calls a model kind refuses by its documentation -------------------------------------------------------------------
# (what: the handle's kernel or element type, or the spec's kind) x (the call of CALLS) -> the exception the documentation
# names.  observe() asserts each of them; no other call may be left out.
REFUSALS = (
    ("matern12", "predict_gradient", "GpxError"),        # GP: "Matern-1/2 ... has no derivative, so predict_gradient raises"
    ("matern12", "paths.predict_gradient", "GpxError"),
    ("basis", "predict_gradient", "GpxError"),           # GP.fit: "predict_gradient and path_ids= queries raise GpxError"
    ("basis", "paths.predict", "GpxError"),
    ("basis", "paths.cov", "GpxError"),
    ("basis", "paths.sample_z", "GpxError"),
    ("basis", "paths.predict_gradient", "GpxError"),
    ("float32", "lml_gradient", "GpxError"),             # GP.lml_gradient: "fp64 models"
)
PATH_KINDS = ("paths", "paths_resized")


def refused(handle, name, call):
    """-> the name of the exception `call` raises on this handle with the model of spec `name`, or None"""
    tags = (HANDLES[handle]["kernel"], HANDLES[handle]["dtype"], SPECS[name].kind)
    hits = [exc for what, c, exc in REFUSALS if what in tags and c == call]
    return hits[0] if hits else None


def applicable(handle, name):
    """the calls observe() makes, in order: every call of CALLS; the ``paths.*`` ones on fits with path ids, and on a basis
    fit, where they are refusals"""
    kind = SPECS[name].kind
    return [c for c in CALLS if not c.startswith("paths.") or kind in PATH_KINDS or kind == "basis"]


# ---- observe ---------------------------------------------------------------------------------------------------------------
class _SentinelNumpy:
    """numpy, but ``empty`` hands out arrays filled with a sentinel (NaN; the most negative integer): an output the library
    did not write is then not finite / not a valid id"""

    def __getattr__(self, name):
        return getattr(np, name)

    @staticmethod
    def empty(shape, dtype=float, **kw):
        dt = np.dtype(dtype)
        return np.full(shape, np.nan if dt.kind == "f" else np.iinfo(dt).min, dtype=dt)


@contextlib.contextmanager
def sentinel_outputs():
    """inside, every host output GP allocates starts out as the sentinel"""
    import gaussianprocesspathmodelling_amd.gp as gpmod
    saved, gpmod.np = gpmod.np, _SentinelNumpy()
    try:
        yield
    finally:
        gpmod.np = saved


def _host(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def _named(prefix, names, values):
    return {f"{prefix}.{n}": v for n, v in zip(names, values)}


def _lml_gradient(gp, s, q, ids):
    kw = {"derivatives": dict(derivative_noise=True), "paths": dict(path=True), "paths_resized": dict(path=True)}.get(s.kind, {})
    lml, grad = gp.lml_gradient(**kw)
    return {"lml_gradient.lml": np.float64(lml), "lml_gradient.grad": grad}


def _with_ids(call):
    return lambda gp, s, q, ids: call(gp, s, q, q["gq"])


def _predict(gp, s, q, ids):
    return _named("predict", ("mean", "var"), gp.predict(q["Xq"], path_ids=ids))


def _predict5(gp, s, q, ids):
    return {"predict5.mean": gp.predict(q["Xq5"], return_var=False)}


def _cov(gp, s, q, ids):
    return _named("cov", ("mean", "cov"), gp.predict(q["Xq"], return_cov=True, path_ids=ids))


def _sample_z(gp, s, q, ids):
    return {"sample_z": gp.sample_y(q["Xq"], 3, z=q["z"], path_ids=ids)}


def _sample_seed(gp, s, q, ids):
    return {"sample_seed": gp.sample_y(q["Xq"], 3, random_state=5)}


def _predict_gradient(gp, s, q, ids):
    return _named("predict_gradient", ("mean", "var", "dmean", "dvar"),
                  gp.predict_gradient(q["Xq"], with_value=True, path_ids=ids))


def _score(gp, s, q, ids):
    return _named("score", ("logp", "maha", "logdet"), gp.score_blocks(q["Xb"], q["Yb"], 17, return_parts=True))


def _forecast(gp, s, q, ids):
    return _named("forecast", ("mean", "cov", "logp"), gp.forecast_blocks(q["Xo"], q["Yo"], q["Xp"], blocks=3, return_logp=True))


def _prefixed(call):
    return lambda gp, s, q, ids: {"paths." + n: v for n, v in _with_ids(call)(gp, s, q, ids).items()}


CALLS = {
    "predict": _predict, "predict5": _predict5, "cov": _cov, "sample_z": _sample_z, "sample_seed": _sample_seed,
    "predict_gradient": _predict_gradient, "score": _score, "forecast": _forecast, "lml_gradient": _lml_gradient,
    "paths.predict": _prefixed(_predict), "paths.cov": _prefixed(_cov), "paths.sample_z": _prefixed(_sample_z),
    "paths.predict_gradient": _prefixed(_predict_gradient),
}


def attributes(gp):
    basis = gp.basis_
    return {"alpha_": gp.alpha_.copy(), "log_det_": np.float64(gp.log_det_), "jitter_used_": np.float64(gp.jitter_used_),
            "noise_weights_": gp.noise_weights_, "observation_kinds_": gp.observation_kinds_, "path_ids_": gp.path_ids_,
            "basis_": np.array(str(basis)), "beta_": gp.beta_, "beta_cov_": gp.beta_cov_}


def one_call(gp, handle, name, call):
    """make one call of CALLS on the model of spec `name` -> its outputs as host arrays ({} for a documented refusal, which
    is asserted to raise)"""
    import pytest
    from gaussianprocesspathmodelling_amd import GpxError
    s = SPECS[name]
    q = queries(s.d, s.k)
    exc = refused(handle, name, call)
    with sentinel_outputs():
        if exc is not None:
            with pytest.raises({"GpxError": GpxError}[exc]):
                CALLS[call](gp, s, q, None)
            return {}
        out = {n: _host(v) for n, v in CALLS[call](gp, s, q, None).items()}
    for n, v in out.items():
        assert np.all(np.isfinite(v)), f"{handle} {name} {n}: not finite (or never written)"
    return out


def observe(gp, handle, name, order=None, between=None):
    """every attribute of the fitted model and every call it answers -> {output name: host array}.  ``order``: the calls in
    another order (default: applicable()); ``between(i)`` runs before call i (the decoys of the query-history test)."""
    with sentinel_outputs():
        out = attributes(gp)
    for n, v in out.items():
        if v.dtype.kind == "f":
            assert np.all(np.isfinite(v)), f"{handle} {name} {n}: not finite (or never written)"
        elif v.dtype.kind == "i":
            assert v.size == 0 or v.min() >= -1, f"{handle} {name} {n}: never written"
    calls = applicable(handle, name) if order is None else list(order)
    assert sorted(calls) == sorted(applicable(handle, name))
    for i, call in enumerate(calls):
        if between is not None:
            between(i)
        got = one_call(gp, handle, name, call)
        assert not set(got) & set(out)
        out.update(got)
    return out


def differences(got, want):
    """-> the names of the outputs of `want` that `got` lacks or holds with other bits (and those `got` has on top)"""
    bad = [n for n in want if n not in got or got[n].shape != want[n].shape or got[n].dtype != want[n].dtype
           or not np.array_equal(got[n], want[n])]
    return bad + [n for n in got if n not in want]


def describe(got, want, names):
    """one line per differing output: the largest difference and where"""
    lines = []
    for n in names:
        if n not in got or n not in want:
            lines.append(f"{n}: only in one of the two")
        elif got[n].shape != want[n].shape or got[n].dtype.kind not in "fi":
            lines.append(f"{n}: {got[n].shape} {got[n]!r:.40} against {want[n].shape} {want[n]!r:.40}")
        else:
            diff = np.abs(got[n].astype(np.float64) - want[n].astype(np.float64))
            at = tuple(int(i) for i in np.unravel_index(int(np.argmax(diff)), diff.shape)) if diff.ndim else ()
            lines.append(f"{n}: {int(np.count_nonzero(got[n] != want[n]))} of {diff.size} entries differ, largest "
                         f"{float(diff.max()):.3e} at {at} (reference {float(np.abs(want[n]).max()):.3e} at most)")
    return lines


_FRESH = {}


def fresh(handle, name):
    """the observation of a fresh handle that was given spec `name` and nothing else; computed once, closed at once"""
    key = (handle, name)
    if key not in _FRESH:
        with make(handle) as gp:
            first = apply(gp, name)
            obs = observe(gp, handle, name)
        obs.update({n: _host(v) for n, v in first.items()})
        _frozen(*obs.values())
        _FRESH[key] = obs
    return _FRESH[key]


def fresh_after_fit(handle, name, call):
    """the outputs of `call` as the FIRST call after the fit of spec `name` on a fresh handle"""
    key = (handle, name, call)
    if key not in _FRESH:
        with make(handle) as gp:
            apply(gp, name)
            _FRESH[key] = one_call(gp, handle, name, call)
        _frozen(*_FRESH[key].values())
    return _FRESH[key]


# ---- the CPU anchors -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def anchor(kernel, name):
    """-> dict(mean, var, logdet, family) of the model of spec `name` from the reference its feature's suite uses, at the
    70 query points"""
    import basis_ref
    import dobs_ref
    import hetero_ref
    import within_ref
    from oracle.gp_oracle import OracleGP
    s, c, rows = SPECS[name], data(name), final_rows(name)
    Xq, jitter = queries(s.d, s.k)["Xq"], JITTER
    ls = np.asarray(s.ls, dtype=np.float64) if np.ndim(s.ls) else float(s.ls)
    if s.kind in ("plain", "fused", "resized"):
        if kernel == "rbf":
            ref = OracleGP(kernel, ls, s.sf2, s.sn2, jitter=jitter).fit(rows["X"], rows["Y"])
            mean, var = ref.predict(Xq)
            return dict(mean=mean, var=var, logdet=ref.log_det_, family="plain")
        # (the oracle knows neither Matern-3/2 nor Matern-1/2: the weighted reference without weights)
        ref = hetero_ref.HeteroGP(kernel, ls, s.sf2, s.sn2, jitter).fit(rows["X"], rows["Y"])
        mean, var = ref.predict(Xq)
        return dict(mean=mean, var=var, logdet=ref.logdet, family="plain")
    if s.kind == "weights":
        ref = hetero_ref.HeteroGP(kernel, ls, s.sf2, s.sn2, jitter).fit(c["X"], c["Y"], c["w"])
        mean, var = ref.predict(Xq)
        return dict(mean=mean, var=var, logdet=ref.logdet, family="plain")
    if s.kind == "derivatives":
        kinds = np.concatenate([np.full(S5_VALUES, -1), c["dims"]])
        ref = dobs_ref.DobsGP(kernel, ls, s.sf2, s.sn2, S5_DERIV_NOISE, jitter)
        ref.fit(np.concatenate([c["X"], c["Xd"]]), kinds, np.concatenate([c["Y"], c["yd"]]))
        mean, var = ref.predict(Xq)
        return dict(mean=mean, var=var, logdet=ref.logdet, family="largest")
    if s.kind in PATH_KINDS:
        fit = within_ref.fit_ref(rows["X"], rows["ids"], rows["Y"], kernel, ls, s.sf2, s.sn2, np.asarray(S6_LSP), S6_SG2,
                                 jitter=jitter)
        mean, cov, _ = within_ref.predict_f(fit, Xq)
        return dict(mean=mean, var=np.diag(cov).copy(), logdet=fit["logdet"], family="largest")
    assert s.kind == "basis"
    ref = basis_ref.BasisGP(kernel, ls, s.sf2, s.sn2, "linear", jitter).fit(c["X"], c["Y"], c["w"])
    mean, var = ref.predict(Xq)
    return dict(mean=mean, var=var, logdet=ref.logdet, family="plain")


def anchor_ratios(dtype, sf2, ref, mean, var, logdet):
    """error / bound of a fresh handle's mean, variance and log-determinant, with the bound of the suite of the spec's
    feature for the handle's element type:

    float64, family "plain" (tests/test_gp_parity_gpu.py, test_hetero_gpu.py, test_basis_gpu.py, test_remove_gpu.py):
        |d mean| <= 1e-6 max(|ref|, 1e-6), |d var| <= 1e-6 max(ref, 1e-6 sf2), log-determinant 1e-9 relative;
    float64, family "largest" (tests/test_dobs_gpu.py, test_within_gpu.py): mean 1e-6 of its largest entry, variance as
        above, log-determinant 1e-6 of max(|ref|, 1);
    float32 (tests/test_fp32_gpu.py, and every feature suite after it): mean 2e-3 of its largest entry, variance 2e-3 sf2,
        log-determinant 1e-3 relative."""
    mr = np.asarray(ref["mean"], dtype=np.float64)
    dm = np.abs(np.asarray(mean, dtype=np.float64).reshape(mr.shape) - mr)
    dv = np.abs(np.asarray(var, dtype=np.float64) - ref["var"])
    dl = abs(float(logdet) - ref["logdet"])
    if dtype == "float32":
        return {"mean": float(dm.max() / np.abs(mr).max() / 2e-3), "var": float(dv.max() / sf2 / 2e-3),
                "logdet": dl / abs(ref["logdet"]) / 1e-3}
    rv = float(np.max(dv / np.maximum(np.abs(ref["var"]), 1e-6 * sf2)) / 1e-6)
    if ref["family"] == "plain":
        return {"mean": float(np.max(dm / np.maximum(np.abs(mr), 1e-6)) / 1e-6), "var": rv,
                "logdet": dl / abs(ref["logdet"]) / 1e-9}
    return {"mean": float(dm.max() / np.abs(mr).max() / 1e-6), "var": rv, "logdet": dl / max(abs(ref["logdet"]), 1.0) / 1e-6}
