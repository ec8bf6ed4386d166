"""CPU: the kernel unit-test entry points with the four kernel ids (no compute call is made: every case below is
refused before any device work).  gpx_kernel_deriv_matrix takes every family and refuses Matern-1/2;
gpx_kernel_grad_matrix keeps its original kernel set."""
import numpy as np

from gaussianprocesspathmodelling_amd import _abi


def test_deriv_matrix_declared_bound_and_exported(gpx):
    assert len(_abi.SIGNATURES["gpx_kernel_deriv_matrix"][1]) == 10 and hasattr(gpx, "gpx_kernel_deriv_matrix")


def test_kernel_deriv_matrix_bad_arguments(gpx):
    a, ls, g = np.zeros((4, 2)), np.ones(2), np.zeros((2, 4, 4))
    pd = _abi.dptr

    def call(kernel=2, A=pd(a), na=4, B=pd(a), nb=4, d=2, L=pd(ls), n_ls=1, G=pd(g)):
        return gpx.gpx_kernel_deriv_matrix(kernel, A, na, B, nb, d, L, n_ls, 1.0, G)

    assert call(kernel=4) == _abi.E_ARG and call(kernel=-1) == _abi.E_ARG
    assert call(A=None) == _abi.E_ARG and call(B=None) == _abi.E_ARG and call(G=None) == _abi.E_ARG
    assert call(L=None) == _abi.E_ARG
    assert call(na=0) == _abi.E_ARG and call(nb=-1) == _abi.E_ARG
    assert call(d=0) == _abi.E_ARG and call(d=33) == _abi.E_ARG
    assert call(n_ls=3) == _abi.E_ARG


def test_kernel_deriv_matrix_refuses_matern12(gpx):
    a, ls, g = np.zeros((4, 2)), np.ones(2), np.full((2, 4, 4), 7.0)
    pd = _abi.dptr
    rc = gpx.gpx_kernel_deriv_matrix(_abi.KERNEL_IDS["matern12"], pd(a), 4, pd(a), 4, 2, pd(ls), 1, 1.0, pd(g))
    assert rc == _abi.E_UNSUPPORTED
    assert b"not differentiable" in gpx.gpx_last_error(None)
    assert np.all(g == 7.0)


def test_kernel_grad_matrix_keeps_its_kernel_set(gpx):
    a, ls, g = np.zeros((4, 2)), np.ones(2), np.full((2, 4, 4), 7.0)
    pd = _abi.dptr
    for kid in (_abi.KERNEL_IDS["matern32"], _abi.KERNEL_IDS["matern12"], 4):
        assert gpx.gpx_kernel_grad_matrix(kid, pd(a), 4, pd(a), 4, 2, pd(ls), 1, 1.0, pd(g)) == _abi.E_ARG
    assert np.all(g == 7.0)


def test_kernel_matrix_rejects_unknown_ids(gpx):
    a, ls, k = np.zeros((4, 2)), np.ones(1), np.zeros((4, 4))
    pd = _abi.dptr
    for kid in (4, -1, 99):
        assert gpx.gpx_kernel_matrix(kid, pd(a), 4, None, 0, 2, pd(ls), 1, 1.0, 0.0, pd(k)) == _abi.E_ARG
