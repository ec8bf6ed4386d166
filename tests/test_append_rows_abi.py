"""CPU: gpx_append_rows (appends to fits with kinds or path ids) and the unit-test entry point gpx_kernel_mixed_matrix
(both additive to ABI v6) are declared in the header, bound in _abi and exported by the library, and refuse bad arguments
without a GPU."""
import ctypes as C
import os
import re

import numpy as np

from gaussianprocesspathmodelling_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_declared_bound_and_exported(gpx):
    raw = open(os.path.join(ROOT, "include", "gpx.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    assert re.search(r"#define GPX_ABI_VERSION 6\b", raw) and gpx.gpx_abi_version() == 6
    for name, arity in (("gpx_append_rows", 9), ("gpx_kernel_mixed_matrix", 13)):
        decl = re.search(rf"\b{name}\s*\(([^)]*)\)", text)
        assert decl and len(decl.group(1).split(",")) == arity
        assert len(_abi.SIGNATURES[name][1]) == arity and hasattr(gpx, name)
    # the calls it extends keep their arities
    assert len(_abi.SIGNATURES["gpx_append"][1]) == 6 and len(_abi.SIGNATURES["gpx_append_weighted"][1]) == 7


def test_append_rows_null_and_bad_arguments(gpx):
    x, y, info = np.zeros((4, 1)), np.zeros((4, 1)), C.c_int64(7)
    kinds = np.zeros(4, dtype=np.int32)
    p = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731

    def call(h=None, X=p(x), Y=p(y), w=None, kind=None, group=None, m=4, mem=_abi.MEM_HOST, inf=C.byref(info)):
        return gpx.gpx_append_rows(h, X, Y, w, kind, group, m, mem, inf)

    assert call() == _abi.E_ARG                      # null handle
    assert call(h=C.c_void_p(0)) == _abi.E_ARG
    assert call(kind=p(kinds), group=p(kinds), w=p(y)) == _abi.E_ARG
    assert call(X=None) == _abi.E_ARG and call(Y=None) == _abi.E_ARG and call(inf=None) == _abi.E_ARG
    assert call(m=0) == _abi.E_ARG and call(m=-5) == _abi.E_ARG
    assert call(mem=9) == _abi.E_ARG
    assert info.value == 7                           # nothing was written


def test_kernel_mixed_matrix_bad_arguments(gpx):
    A, B, ls, K = np.zeros((4, 2)), np.zeros((3, 2)), np.ones(2), np.full((4, 3), 7.0)
    ka, kb = np.array([-1, 0, 1, -1], dtype=np.int32), np.array([1, -1, 0], dtype=np.int32)
    ip = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_int32))  # noqa: E731
    RBF, M12, F64 = _abi.KERNEL_IDS["rbf"], _abi.KERNEL_IDS["matern12"], _abi.DTYPE_IDS["float64"]

    def call(kernel=RBF, dtype=F64, a=A, ka=ka, na=4, b=B, kb=kb, nb=3, d=2, l=ls, n_ls=2, out=K):
        dp = lambda v: None if v is None else _abi.dptr(v)  # noqa: E731
        return gpx.gpx_kernel_mixed_matrix(kernel, dtype, dp(a), ip(ka), na, dp(b), ip(kb), nb, d, dp(l), n_ls, 1.5, dp(out))

    assert call(a=None) == _abi.E_ARG and call(b=None) == _abi.E_ARG and call(out=None) == _abi.E_ARG
    assert call(l=None) == _abi.E_ARG and call(na=0) == _abi.E_ARG and call(nb=-1) == _abi.E_ARG
    assert call(d=0) == _abi.E_ARG and call(d=33) == _abi.E_ARG and call(n_ls=3) == _abi.E_ARG
    assert call(kernel=99) == _abi.E_ARG and call(dtype=_abi.DTYPE_IDS["mixed"]) == _abi.E_ARG
    assert call(ka=np.array([-1, 0, 2, -1], dtype=np.int32)) == _abi.E_ARG       # a kind >= d
    assert call(kb=np.array([1, -2, 0], dtype=np.int32)) == _abi.E_ARG           # a kind below -1
    assert call(kernel=M12) == _abi.E_UNSUPPORTED                                # Matern-1/2 has no derivative
    assert b"not differentiable" in gpx.gpx_last_error(None)
    assert np.all(K == 7.0)                                                      # nothing was written
