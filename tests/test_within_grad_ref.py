"""CPU: the reference of the LML gradient with path ids (tests/within_grad_ref.py) against what it does not share code
with — central differences of ``within_ref.path_cov`` for the element matrices and of ``within_ref.fit_ref``'s LML for the
gradient — the agreement of its two analytic forms, and the conditioning of every case the GPU tests compare against it.

Bounds: those of tests/test_dobs_grad_ref.py, for its reasons.  Central differences at step h carry h^2 f''' / 6 of
truncation and eps |f| / h of rounding: for the covariance entries (h = 1e-5) 1e-7 of the largest entry; for the LML
(h = 1e-4; the LML is rounded at ~1e-13 |lml|, i.e. 1e-9 |lml| in the quotient, against gradients of 1e-3 .. 1 |lml|) 1e-5
of the largest entry.  Every figure is printed."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import within_ref as wr  # noqa: E402
import within_grad_ref as gr  # noqa: E402

COND_MAX = 1e7   # the conditioning the GPU tolerances (1e-9 / 1e-8) assume: eps cond(K) = 1e-9
FD_PAIRS = [("sorted_d1", k) for k in gr.KERNELS] + [("shuffled_d3", k) for k in gr.KERNELS] + \
           [("ls_d_path_1", "matern32"), ("ls_1_path_d", "matern32"), ("weighted", "matern32"), ("sorted_d4", "matern32")]


def matrix_case(d, order, seed=0):
    """tests/test_within_gpu.py's ``_matrix_case``: 130 rows against 200 columns, 12 paths and some -1, close pairs"""
    rng = np.random.default_rng(1000 * d + seed)
    A, B = rng.uniform(0.0, 1.0, (130, d)), rng.uniform(0.0, 1.0, (200, d))
    B[:40] = A[:40] + 0.01 * rng.standard_normal((40, d))
    ga, gb = rng.integers(-1, 12, 130), rng.integers(-1, 12, 200)
    gb[:40] = ga[:40]
    if order == "sorted":
        ga, gb = np.sort(ga), np.sort(gb)[::-1].copy()
    lsp = np.linspace(0.2, 0.1, d) if d > 1 else np.array([0.1])
    return A, ga.astype(np.int32), B, gb.astype(np.int32), lsp


@pytest.mark.parametrize("kernel", gr.KERNELS)
@pytest.mark.parametrize("d", [1, 3, 5])
def test_element_matrices_against_central_differences_of_the_covariance(kernel, d):
    A, ga, B, gb, lsp = matrix_case(d, "shuffled")
    B[:5] = A[:5]                                                         # coincident same-path pairs (Matern-1/2: 0 there)
    ls, h = np.full(d, 0.7), 1e-5
    plain = wr.path_cov(A, None, B, None, kernel, ls, gr.SF2, lsp, gr.SG2)
    for lp in (lsp, lsp[:1]):
        got = gr.path_dtheta_ref(A, ga, B, gb, kernel, lp, gr.SG2)
        assert got.shape == (1 + lp.size, 130, 200)
        term = wr.path_cov(A, ga, B, gb, kernel, ls, gr.SF2, lp, gr.SG2) - plain
        e0 = float(np.max(np.abs(got[0] - term)) / gr.SG2)
        worst = 0.0
        for c in range(lp.size):
            f = []
            for sgn in (+1, -1):
                l = lp.copy()
                l[c] *= np.exp(sgn * h)
                f.append(wr.path_cov(A, ga, B, gb, kernel, ls, gr.SF2, l, gr.SG2))
            fd = (f[0] - f[1]) / (2 * h)
            worst = max(worst, float(np.max(np.abs(got[1 + c] - fd)) / np.max(np.abs(got[1 + c]))))
        print(f"{kernel} d={d} n_ls_path={lp.size}: |term - path_cov's| / sg2 {e0:.2e}, worst |d / d log l_path - difference| "
              f"/ largest entry {worst:.2e}")
        assert e0 <= 1e-14
        assert worst <= 1e-7
        assert np.all(got[:, ~((ga[:, None] == gb[None, :]) & (ga[:, None] >= 0))] == 0.0)
    if kernel == "matern12":
        assert np.all(got[1:, :5, :5][:, np.arange(5), np.arange(5)] == 0.0)


def test_swapping_the_sides_transposes_the_matrices():
    A, ga, B, gb, lsp = matrix_case(3, "sorted")
    for kernel in gr.KERNELS:
        G = gr.path_dtheta_ref(A, ga, B, gb, kernel, lsp, gr.SG2)
        H = gr.path_dtheta_ref(B, gb, A, ga, kernel, lsp, gr.SG2)
        assert np.array_equal(G, H.transpose(0, 2, 1))


def _theta(p):
    return np.log(np.concatenate([p["ls"], [gr.SF2, gr.SN2, gr.SG2], p["lsp"]]))


def _lml_at(p, kernel, v):
    e, n_ls = np.exp(v), p["ls"].size
    fit = gr.fit_case(p, kernel, ls=e[:n_ls], sf2=e[n_ls], sn2=e[n_ls + 1], sg2=e[n_ls + 2], lsp=e[n_ls + 3:])
    return float(np.sum(fit["lml"]))


@pytest.mark.parametrize("name,kernel", FD_PAIRS)
def test_gradient_against_central_differences_of_the_lml(name, kernel):
    p, fit, lml, grad = gr.case(name, kernel)
    assert grad.shape == (p["ls"].size + 3 + p["lsp"].size,)
    v0, h = _theta(p), 1e-4
    fd = np.zeros(len(v0))
    for i in range(len(v0)):
        f = []
        for sgn in (+1, -1):
            v = v0.copy()
            v[i] += sgn * h
            f.append(_lml_at(p, kernel, v))
        fd[i] = (f[0] - f[1]) / (2 * h)
    err = float(np.max(np.abs(fd - grad)) / np.max(np.abs(grad)))
    small = float(np.min(np.abs(grad[p["ls"].size + 2:])) / np.max(np.abs(grad)))
    print(f"{name} {kernel}: lml {lml:.6f} gradient {np.array2string(grad, precision=5)} |gradient - difference| / largest "
          f"{err:.2e}; smallest path entry / largest entry {small:.2e}")
    assert err <= 1e-5


@pytest.mark.parametrize("name,kernel", gr.PAIRS)
def test_two_analytic_forms_agree_and_the_case_is_well_conditioned(name, kernel):
    p, fit, lml, grad = gr.case(name, kernel)
    other = gr.lml_grad_inverse(p, kernel, fit)
    err = float(np.max(np.abs(other - grad)) / np.max(np.abs(grad)))
    ev = np.linalg.eigvalsh(gr.full_K(fit))
    cond = float(ev[-1] / ev[0])
    n_ls = p["ls"].size
    wrong = gr.wrong_variance_entry(p, kernel, fit)
    print(f"{name} {kernel}: N {len(p['X'])} cond(K) {cond:.3g} inverse against solves {err:.2e}; variance entry "
          f"{grad[n_ls]:.6g}, the whole-K contraction would be {wrong:.6g}")
    assert err <= 1e-10
    assert cond <= COND_MAX
    assert np.isfinite(lml) and np.all(np.isfinite(grad))
    # the whole-K contraction is the variance entry plus the path_variance entry: far from the right one
    assert abs(wrong - (grad[n_ls] + grad[n_ls + 2])) <= 1e-9 * np.max(np.abs(grad))
    assert abs(wrong - grad[n_ls]) > 1e-3 * np.max(np.abs(grad))


def test_the_cases_are_what_the_gpu_tests_say_they_are():
    p = gr.problem("sorted_d1")
    assert len(p["X"]) == 396 and np.array_equal(p["ids"], np.repeat(np.arange(12), 33)) and p["Y"].shape == (396, 2)
    ids = p["ids"]
    for ti in range(4):                                                   # no off-diagonal 128-tile holds a same-path pair
        for tj in range(ti):
            a, b = ids[ti * 128:(ti + 1) * 128], ids[tj * 128:(tj + 1) * 128]
            assert not np.any(a[:, None] == b[None, :]) or abs(ti - tj) == 1
    p = gr.problem("shuffled_d3")
    ids = p["ids"]
    assert p["X"].shape == (396, 3) and np.sum(ids < 0) >= 396 // 17 and np.any(np.diff(ids[ids >= 0]) < 0)
    for ti in range(4):                                                   # every tile does
        for tj in range(ti + 1):
            a, b = ids[ti * 128:(ti + 1) * 128], ids[tj * 128:(tj + 1) * 128]
            assert np.any((a[:, None] == b[None, :]) & (a[:, None] >= 0))
    assert len(gr.problem("nine_tiles_d2")["X"]) == 1122 and gr.problem("nine_tiles_d2")["X"].shape[1] == 2
    assert gr.problem("ls_d_path_1")["ls"].size == 2 and gr.problem("ls_d_path_1")["lsp"].size == 1
    assert gr.problem("ls_1_path_d")["ls"].size == 1 and gr.problem("ls_1_path_d")["lsp"].size == 2
    w = gr.problem("weighted")["w"]
    assert w.min() == 0.0 and np.sum(w == 0.0) == 1 and w.max() <= 2.0 and np.sort(w)[1] >= 0.5
