"""CPU: the NumPy definition of the bound's gradient (tests/sparse_grad_ref.py) against five-point central differences of
the bound itself on the eight parity cases, and against the exact GP's LML gradient where the bound IS the LML."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sparse_grad_ref  # noqa: E402
import sparse_ref  # noqa: E402

SF2, SN2 = sparse_ref.SF2, sparse_ref.SN2
FD_BAR = 1e-7  # measured: worst 5.1e-9 ("rbf-d1-N700-m130"), every other case <= 2.3e-9


@pytest.mark.parametrize("case", sparse_ref.CASES, ids=[c["id"] for c in sparse_ref.CASES])
def test_analytic_gradient_against_central_differences(case):
    D = sparse_ref.case_data(case)
    args = (case["kernel"], D["ls"], SF2, SN2, case["jitter"], D["X"], D["y"], D["Z"], D["w"])
    F, g = sparse_grad_ref.gradient(*args)
    assert g.shape == (np.size(D["ls"]) + 2,) and np.all(np.isfinite(g))
    assert F == float(sparse_ref.SparseRef(*args[:5]).fit(D["X"], D["y"], D["Z"], D["w"]).elbo.sum())
    figs = {h: sparse_grad_ref.metric(g, sparse_grad_ref.fd_gradient(*args, h=h)) for h in sparse_grad_ref.FD_STEPS}
    print(case["id"], {h: f"{v:.2e}" for h, v in figs.items()})
    assert min(figs.values()) < FD_BAR, figs


@pytest.mark.parametrize("kernel", ["matern32", "matern12"])
def test_with_z_the_distinct_inputs_the_gradient_is_the_exact_gps(kernel):
    """Z = the shared grid, jitter = 0: the bound equals the LML for every theta, so the gradients agree"""
    X, y, grid = sparse_ref.path_grid_problem(40, 33, 5)
    F, g = sparse_grad_ref.gradient(kernel, 0.25, SF2, SN2, 0.0, X, y, grid)
    e = sparse_grad_ref.exact_lml_gradient(kernel, 0.25, SF2, SN2, X, y)
    fig = sparse_grad_ref.metric(g, e)
    print(kernel, f"{fig:.2e}", g, e)
    assert fig < 1e-6
