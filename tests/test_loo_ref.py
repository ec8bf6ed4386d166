"""CPU: the reference of the leave-one-out tests checks itself — the closed form of tests/loo_ref.py (what the library
computes, R&W eqs. 5.10-5.12) against deleting each row and refitting, which shares no step with it, for each of the five
kinds of fit a handle can hold.  Bars 1e-9 with the floors of the GPU tests (mean 1e-6, var purely relative, logp 1)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import basis_ref  # noqa: E402
import dobs_ref  # noqa: E402
import loo_ref  # noqa: E402
import within_ref  # noqa: E402
from oracle.gp_oracle import synthetic_problem  # noqa: E402

SF2, SN2 = 1.5, 1e-2
BAR = 1e-9


def _plain():
    X, y, _ = synthetic_problem(60, 3, 1, seed=60)
    return loo_ref.plain_gram(X, "rbf", 0.5, SF2, SN2), y, None


def _weighted():
    X, y, _ = synthetic_problem(61, 3, 1, seed=61)
    w = np.random.default_rng(3).uniform(0.25, 4.0, len(X))
    Y = np.stack([y, np.cos(3.0 * X[:, 0])], axis=1)
    return loo_ref.plain_gram(X, "matern12", (0.5, 0.4, 0.6), SF2, SN2, w), Y, None


def _derivative():
    c = dobs_ref.problem("matern52", 3, "last", 7)
    rows = np.concatenate([np.arange(40), dobs_ref.N_VAL + np.arange(20)])      # 40 value and 20 derivative rows
    c = dict(c, Xall=c["Xall"][rows], kinds=c["kinds"][rows], yall=c["yall"][rows])
    return loo_ref.dobs_gram(c), c["yall"], None


def _paths():
    p = within_ref.problem(P=5, L=12, G=1)
    return loo_ref.within_gram(p["X"], p["ids"], "matern32", 0.25, SF2, SN2, 0.1, 0.4), p["Y"], None


def _basis():
    X, Y, _ = basis_ref.trend_problem(60, 3, 2, 1, seed=63)
    return loo_ref.plain_gram(X, "rbf", (0.3, 0.2, 0.25), SF2, SN2), Y, basis_ref.basis_matrix(X, "quadratic")


CASES = {"plain": _plain, "weighted": _weighted, "derivative": _derivative, "paths": _paths, "basis": _basis}


@pytest.mark.parametrize("kind", sorted(CASES))
def test_closed_form_is_the_refit(kind):
    K, Y, H = CASES[kind]()
    closed, refit = loo_ref.loo_closed(K, Y, H), loo_ref.loo_refit(K, Y, H)
    fig = loo_ref.errors(closed, refit)
    print(f"{kind}: N = {len(K)}, cond(K) = {np.linalg.cond(K):.3g}, closed form against the refit: {fig}")
    assert np.all(np.isfinite(refit["var"])) and closed["mean"].shape == refit["mean"].shape
    assert max(fig.values()) < BAR, fig


def test_rows_that_the_basis_alone_determines():
    """N = p = 3 (linear basis, d = 2): the three coefficients reproduce the three observations, nothing is left to predict"""
    X = np.random.default_rng(0).uniform(0.0, 1.0, (3, 2))
    Y = np.array([[0.3], [-1.0], [2.0]])
    K, H = loo_ref.plain_gram(X, "rbf", 0.5, SF2, SN2), basis_ref.basis_matrix(X, "linear")
    for r in (loo_ref.loo_closed(K, Y, H), loo_ref.loo_refit(K, Y, H)):
        assert np.all(r["var"] == np.inf) and np.all(np.isnan(r["mean"])) and np.all(r["logp"] == -np.inf)
        assert np.all(r["total"] == -np.inf)
    assert loo_ref.errors(loo_ref.loo_closed(K, Y, H), loo_ref.loo_refit(K, Y, H))["total"] == 0.0
