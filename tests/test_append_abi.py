"""CPU: the append entry points (gpx_append, gpx_reserve and the layout query gpx_factor_info; additive to ABI v6) are
declared in the header, bound in _abi and exported by the library, and refuse bad arguments without a GPU."""
import ctypes as C
import os
import re

import numpy as np

from gaussianprocesspathmodelling_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gpx_append", "gpx_reserve", "gpx_factor_info")


def test_declared_bound_and_exported(gpx):
    raw = open(os.path.join(ROOT, "include", "gpx.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    assert re.search(r"#define GPX_ABI_VERSION 6\b", raw) and _abi.ABI_VERSION == 6
    assert gpx.gpx_abi_version() == 6
    for name in NEW:
        assert re.search(rf"\b{name}\s*\(", text) and name in _abi.SIGNATURES and hasattr(gpx, name)
    assert len(_abi.SIGNATURES["gpx_append"][1]) == 6
    assert len(_abi.SIGNATURES["gpx_reserve"][1]) == 2
    # the timings struct keeps its layout: the append books into the fit's fields
    assert C.sizeof(_abi.GpxTimings) == 29 * 8


def test_append_null_and_bad_arguments(gpx):
    x, y, info = np.zeros((4, 1)), np.zeros((4, 1)), C.c_int64(7)
    p = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731

    def call(h=None, X=p(x), Y=p(y), m=4, mem=_abi.MEM_HOST, inf=C.byref(info)):
        return gpx.gpx_append(h, X, Y, m, mem, inf)

    assert call() == _abi.E_ARG                      # null handle
    assert call(h=C.c_void_p(0)) == _abi.E_ARG
    assert call(X=None) == _abi.E_ARG and call(Y=None) == _abi.E_ARG and call(inf=None) == _abi.E_ARG
    assert call(m=0) == _abi.E_ARG and call(m=-5) == _abi.E_ARG
    assert call(mem=9) == _abi.E_ARG
    assert info.value == 7                           # nothing was written


def test_reserve_and_factor_info_null_handle(gpx):
    assert gpx.gpx_reserve(None, 4096) == _abi.E_ARG
    assert gpx.gpx_reserve(None, -1) == _abi.E_ARG
    ptr, ld, cap = C.c_void_p(0), C.c_int64(0), C.c_int64(0)
    assert gpx.gpx_factor_info(None, C.byref(ptr), C.byref(ld), C.byref(cap)) == _abi.E_ARG
