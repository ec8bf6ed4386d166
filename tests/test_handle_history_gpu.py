"""GPU: what a handle computes does not depend on what it computed before ("What a handle remembers").

The contract: the result of any call depends only on (a) the handle's constructor arguments, (b) the arguments of its last
successful fit / fit_predict and the reserve in force at it, (c) the update / remove calls made since, and (d) the call's
own arguments — not on an earlier fit, an earlier query, a failed or refused call, or another handle of the process.

The instrument is comparison BIT FOR BIT (np.array_equal) with a fresh handle that was given (a)-(d) and nothing else:
no kernel here accumulates in an order that can vary, split counts depend on the padded sizes only and batching does not
change bits, so a reused handle has no excuse for another last bit.  tests/history_util.py holds the model specs S1-S10
(the smallest shapes at which padding to 64 / 128, the panel count and the host-side flags change), ``observe`` — every
attribute and every call a fitted model answers, outputs allocated as NaN so that one the library did not write counts as
not finite — the table of the calls a model kind refuses by its documentation (asserted to raise; nothing else is left out)
and the walks, whose rules test_the_walks_and_the_refusal_table_are_whole checks without a GPU.

Two handles agreeing could be two handles equally wrong, so test_fresh_handles_agree_with_the_cpu_references anchors every
fresh observation to the CPU reference of the spec's feature, with that feature's own bound."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import history_util as hu  # noqa: E402

gpu = pytest.mark.gpu
ALLOWED = {"matern32_f64": hu.WALK_SPECS, "rbf_f32": hu.WALK_SPECS, "matern12_f64": hu.NO_DERIVATIVES}
LARGE_QUERIES = ("predict700", "cov200", "score40x33")           # made after every S2 of a walk: more scratch than S8 needs


# ---- without a GPU -----------------------------------------------------------------------------------------------------------
def test_the_walks_and_the_refusal_table_are_whole():
    """The rules of the fit-history walks, on the walks themselves:
    every spec occurs at least twice, with different predecessors; every spec follows once a larger model (no fewer inputs
    and targets, more rows) and once a smaller one, where the handle has such a spec; each of S4, S5, S6, S7, S9, S10 is
    once followed directly by a plain spec (S1, S3) of smaller N and once by a different feature spec; S8 follows S2 (and
    the large queries the walk makes there); S9 is once followed by a model larger than its reserve."""
    for handle, walk in hu.WALKS.items():
        assert hu.check_sequence(walk, ALLOWED[handle]) == [], handle
        assert set(walk) == set(ALLOWED[handle])
    # the check itself notices a thinned walk
    assert hu.check_sequence(hu.FULL_WALK[:-1], hu.WALK_SPECS) != []
    assert hu.check_sequence(tuple(n for n in hu.FULL_WALK if n != "S2"), hu.WALK_SPECS) != []
    assert hu.check_sequence(hu.MATERN12_WALK + ("S5",), hu.NO_DERIVATIVES) != []
    # the specs are the ones the padding and the flags change at
    shapes = {n: (s.N, s.d, s.k) for n, s in hu.SPECS.items()}
    assert shapes == {"S1": (300, 3, 2), "S2": (1100, 2, 9), "S3": (70, 1, 1), "S4": (129, 1, 1), "S5": (260, 3, 1),
                      "S6": (106, 2, 2), "S7": (200, 3, 1), "S8": (300, 3, 2), "S9": (307, 3, 2), "S10": (110, 2, 2),
                      "T1": (300, 1, 1)}
    hyper = [(np.atleast_1d(s.ls)[0], s.sf2, s.sn2) for n, s in hu.SPECS.items() if n not in ("S8", "S9", "S10")]
    for column in zip(*hyper):
        assert len(set(column)) == len(column)                  # no two specs share a lengthscale, a variance or a noise
    for name in hu.WALK_SPECS:
        rows = hu.final_rows(name)
        assert len(rows["X"]) == (hu.S5_VALUES if name == "S5" else hu.SPECS[name].N)
        assert np.array_equal(rows["X"][:hu.ANCHORS], hu.anchors(hu.SPECS[name].d))
    assert np.count_nonzero(hu.data("S4")["w"] == 0.0) == 3
    q = hu.queries(2, 2)
    assert set(np.unique(q["gq"])) == {-1, 0, 1, 2, 3, 4, 5, 99} and np.abs(q["Xq"]).max() > 2.0
    # the refusal table: calls that exist, exceptions that are named, and the cases the documentation lists
    assert all(call in hu.CALLS and exc == "GpxError" for _, call, exc in hu.REFUSALS)
    assert hu.refused("matern12_f64", "S1", "predict_gradient") == "GpxError"
    assert hu.refused("matern12_f64", "S6", "paths.predict_gradient") == "GpxError"
    assert hu.refused("matern32_f64", "S7", "predict_gradient") == "GpxError"
    assert all(hu.refused("rbf_f32", "S7", c) == "GpxError" for c in hu.CALLS if c.startswith("paths."))
    assert all(hu.refused("rbf_f32", n, "lml_gradient") == "GpxError" for n in hu.WALK_SPECS)
    assert all(hu.refused("matern32_f64", n, c) is None for n in hu.WALK_SPECS if n != "S7" for c in hu.CALLS)
    # nothing is left out silently: a model answers or refuses every call; the path queries go to fits with path ids (and,
    # as refusals, to the basis fit)
    for handle, allowed in ALLOWED.items():
        for name in allowed:
            made = hu.applicable(handle, name)
            plain = [c for c in hu.CALLS if not c.startswith("paths.")]
            assert made[:len(plain)] == plain
            assert (len(made) == len(hu.CALLS)) == (name in ("S6", "S7", "S10"))


# ---- helpers -----------------------------------------------------------------------------------------------------------------
def _step(gp, handle, name, pause=None):
    first = hu.apply(gp, name, pause)
    obs = hu.observe(gp, handle, name)
    obs.update({n: hu._host(v) for n, v in first.items()})
    return obs


def _same_as(got, want, where):
    """every output of `want` is in `got` with the same bits, and nothing else is -> how many were compared"""
    bad = hu.differences(got, want)
    if bad:
        lines = hu.describe(got, want, bad)
        print(f"{where}: {len(bad)} of {len(want)} outputs differ\n  " + "\n  ".join(lines))
    assert not bad, (where, bad)
    assert not set(want) - set(got)
    return len(want)


def _large_queries(gp, handle, name):
    for which in LARGE_QUERIES + (("gradient700",) if hu.HANDLES[handle]["kernel"] != "matern12" else ()):
        hu.decoy(gp, name, which)


# ---- 3. fit history -----------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("handle", list(hu.HANDLES))
def test_a_fit_forgets_the_fits_before_it(handle):
    """One handle walks through hu.WALKS[handle] (rules: test_the_walks_and_the_refusal_table_are_whole); after every step
    every output of observe() has the bits of a fresh handle that was given that one spec."""
    walk = hu.WALKS[handle]
    assert hu.check_sequence(walk, ALLOWED[handle]) == []
    want = {name: hu.fresh(handle, name) for name in dict.fromkeys(walk)}      # (each fresh handle is closed again)
    compared = 0
    with hu.make(handle) as gp:
        for i, name in enumerate(walk):
            got = _step(gp, handle, name)
            compared += _same_as(got, want[name], f"{handle} step {i} ({name} after {walk[i - 1] if i else 'nothing'})")
            if name == "S2":
                _large_queries(gp, handle, name)
    assert compared == sum(len(want[name]) for name in walk)
    print(f"{handle}: {len(walk)} steps, {compared} outputs compared bit for bit")


@gpu
def test_a_reservation_can_be_taken_back():
    """``reserve(0)`` is "what the fit itself needs", on a fitted handle too (the walks rely on it after every S9; the
    library used to refuse it there, so a handle that had reserved once laid out every later fit for that capacity).  The
    model it is made on does not change, the next fit is laid out for its own size, and a capacity between 0 and N is still
    refused."""
    import ctypes as C
    from gaussianprocesspathmodelling_amd import GpxError, _abi

    def capacity(gp):
        cap = C.c_int64(0)
        gp._check(gp._lib.gpx_factor_info(gp._h, None, None, C.byref(cap)))
        return cap.value

    handle = "matern32_f64"
    s9, s3 = hu.fresh(handle, "S9"), hu.fresh(handle, "S3")
    with hu.make(handle) as gp, hu.make(handle) as never:
        hu.apply(gp, "S9")
        assert capacity(gp) >= hu.S9_RESERVE
        with pytest.raises(GpxError) as e:
            gp.reserve(100)
        assert e.value.code == _abi.E_ARG
        gp.reserve(0)
        gp._history_reserve = 0
        _same_as(hu.observe(gp, handle, "S9"), s9, "S9 after reserve(0)")
        assert capacity(gp) >= hu.S9_RESERVE                     # (the current layout stays)
        _same_as(_step(gp, handle, "S3"), s3, "S3 after S9 and reserve(0)")
        hu.apply(never, "S3")
        assert capacity(gp) == capacity(never) < hu.S9_RESERVE


# ---- 4. query history ---------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("handle,name", [("matern32_f64", "S1"), ("matern32_f64", "S6"), ("rbf_f32", "S1")])
def test_a_call_forgets_the_calls_before_it(handle, name, monkeypatch):
    """The calls of observe() forward, reversed and in a seeded shuffle, a decoy (the same kind of call at a larger size:
    700 query points, covariance and samples at M = 200 and S = 8, 40 blocks of 33, forecasts with Lo + Lp = 64, device
    tensors) before every call and one release_scratch() in the middle of each pass; the shuffled pass runs with
    GPX_PRED_BATCH=128 (read per call).  Every output has the bits it has as the FIRST call after the fit on a fresh handle."""
    calls = hu.applicable(handle, name)
    want = {call: hu.fresh_after_fit(handle, name, call) for call in calls}
    shuffled = list(np.random.default_rng(4).permutation(calls))
    decoys = list(hu.DECOYS)
    compared = 0
    with hu.make(handle) as gp:
        hu.apply(gp, name)
        for p, order in enumerate((calls, calls[::-1], shuffled)):
            if p == 2:
                monkeypatch.setenv("GPX_PRED_BATCH", "128")

            def between(i, p=p):
                if i == len(calls) // 2:
                    gp.release_scratch()
                hu.decoy(gp, name, decoys[(i + p) % len(decoys)])

            got = hu.observe(gp, handle, name, order=order, between=between)
            for call in calls:
                outs = {n: got[n] for n in want[call]}
                compared += _same_as(outs, want[call], f"{handle} {name} pass {p}: {call}")
            compared += _same_as({n: got[n] for n in hu.fresh(handle, name) if n in got}, hu.fresh(handle, name),
                                 f"{handle} {name} pass {p}: the whole observation")
    assert compared == 3 * (sum(len(w) for w in want.values()) + len(hu.fresh(handle, name)))


# ---- 5. failed and refused calls ------------------------------------------------------------------------------------------------
@gpu
def test_a_failed_call_leaves_no_trace():
    from gaussianprocesspathmodelling_amd import GpxError, _abi
    handle = "matern32_f64"
    s1, s3, t1 = hu.fresh(handle, "S1"), hu.fresh(handle, "S3"), hu.fresh(handle, "T1")
    c, q = hu.data("S1"), hu.queries(3, 2)
    with hu.make(handle) as gp:
        _same_as(_step(gp, handle, "S1"), s1, "S1")
        # a refused fit: quadratic basis, d = 3: p = 7, k = 60 targets: k + p > 64.  "The model as it was."
        with pytest.raises(GpxError) as e:
            gp.fit(c["X"], np.tile(c["Y"], (1, 30)), basis="quadratic")
        assert e.value.code == _abi.E_ARG
        _same_as(hu.observe(gp, handle, "S1"), s1, "S1 after a refused fit")
        # a singular block (17 times one point, no noise term) and a sample of 40 times one point without jitter
        Xb = np.array(q["Xb"])
        Xb[17:34] = Xb[17]
        got = gp.score_blocks(Xb, q["Yb"], 17, include_noise=False, return_parts=True, on_bad="nan")
        assert gp.score_info_ in (0, 2)
        assert all(np.all(np.isnan(a[1])) == bool(gp.score_info_) for a in got)
        with pytest.raises(np.linalg.LinAlgError):
            gp.sample_y(np.repeat(q["Xq"][20:21], 40, axis=0), 2, jitter=0.0, max_tries=1)
        _same_as(hu.observe(gp, handle, "S1"), s1, "S1 after a singular block and a failed sample")
        # an update that is not positive definite (tests/test_append_gpu.py: the point -100 twice): the model is unchanged
        _same_as(_step(gp, handle, "T1"), t1, "T1")
        with pytest.raises(np.linalg.LinAlgError, match="unchanged"):
            gp.update(np.array([[-100.0], [-100.0]]), np.array([0.5, -0.25]))
        _same_as(hu.observe(gp, handle, "T1"), t1, "T1 after a failed update")
        # a fit that fails (duplicated points, no noise, no jitter, one try) on a handle that held S5
        hu.apply(gp, "S5")
        X = np.zeros((200, 3))
        X[:, 0] = np.repeat(np.linspace(0.0, 1.0, 100), 2)
        gp.noise, gp.jitter, gp.max_tries = 0.0, 0.0, 1
        with pytest.raises(np.linalg.LinAlgError):
            gp.fit(X, np.sin(X[:, 0]))
        assert gp.info_ > 0
        with pytest.raises(RuntimeError):
            gp.predict(X[:3])
        gp.max_tries = 3
        _same_as(_step(gp, handle, "S3"), s3, "S3 after a failed fit after S5")


# ---- 6. two handles --------------------------------------------------------------------------------------------------
@gpu
def test_two_handles_do_not_see_each_other():
    """The fp64 Matern-3/2 handle (S1, S6, S9) and the fp32 RBF handle (S2, S4, S7) take turns: a fit on one, a query on the
    other, the update of S9 with queries of the other handle around it, then their observations call by call in turn.  The
    launchers' thread-local modes and error flag are left as they were found: every output has the fresh handle's bits."""
    ha, hb = "matern32_f64", "rbf_f32"
    turns = (("S1", "S2"), ("S6", "S4"), ("S9", "S7"))
    want = {(h, n): hu.fresh(h, n) for pair in turns for h, n in zip((ha, hb), pair)}
    compared = 0
    with hu.make(ha) as a, hu.make(hb) as b:
        held = None
        for na, nb in turns:
            first_a = hu.apply(a, na, pause=None if held is None else (lambda: hu.one_call(b, hb, held, "predict")))
            hu.one_call(a, ha, na, "cov")
            hu.apply(b, nb, pause=lambda: hu.one_call(a, ha, na, "predict"))
            held = nb
            hu.one_call(a, ha, na, "score")
            hu.one_call(b, hb, nb, "sample_seed")
            calls_a, calls_b = hu.applicable(ha, na), hu.applicable(hb, nb)
            got_b = {}

            def other(i):
                if i < len(calls_b):
                    got_b.update(hu.one_call(b, hb, nb, calls_b[i]))

            got_a = hu.observe(a, ha, na, between=other)
            got_a.update({n: hu._host(v) for n, v in first_a.items()})
            for i in range(len(calls_a), len(calls_b)):
                other(i)
            with hu.sentinel_outputs():
                got_b.update(hu.attributes(b))
            compared += _same_as(got_a, want[ha, na], f"{ha} {na} beside {hb} {nb}")
            compared += _same_as(got_b, want[hb, nb], f"{hb} {nb} beside {ha} {na}")
    assert compared == sum(len(w) for w in want.values())


# ---- 7. the CPU anchors -------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("handle", list(hu.HANDLES))
def test_fresh_handles_agree_with_the_cpu_references(handle):
    """predict's mean and variance at the 70 query points and the log-determinant of every fresh handle against the
    reference of the spec's feature (oracle.gp_oracle.OracleGP for the plain RBF fits, tests/hetero_ref.py for the plain
    Matern fits — the oracle knows neither family — and for weights, dobs_ref, within_ref and basis_ref for the others; S9
    and S10 against a reference fit of the rows that are left), with the bound that feature's suite states for the
    handle's element type (hu.anchor_ratios).  Printed: error / bound."""
    kernel, dtype = hu.HANDLES[handle]["kernel"], hu.HANDLES[handle]["dtype"]
    worst = {}
    for name in ALLOWED[handle]:
        obs, ref = hu.fresh(handle, name), hu.anchor(kernel, name)
        r = hu.anchor_ratios(dtype, hu.SPECS[name].sf2, ref, obs["predict.mean"], obs["predict.var"], obs["log_det_"])
        print(f"anchor {handle} {name}: error / bound " + " ".join(f"{k} {v:.3g}" for k, v in r.items()))
        worst[name] = max(r.values())
        if name == "S8":                                       # the fused pass's own prediction too
            r8 = hu.anchor_ratios(dtype, hu.SPECS[name].sf2, ref, obs["fit_predict.mean"], obs["fit_predict.var"], obs["log_det_"])
            print(f"anchor {handle} {name} (fit_predict): error / bound " + " ".join(f"{k} {v:.3g}" for k, v in r8.items()))
            worst[name] = max(worst[name], max(r8.values()))
    print(f"anchor {handle}: largest error / bound {max(worst.values()):.3g} ({max(worst, key=worst.get)})")
    assert all(v <= 1.0 for v in worst.values()), worst
