"""CPU: the pathwise calls are declared, bound, built and exported; they are additive to ABI 6 (no struct grows); their
null refusals need no device and write nothing."""
import ctypes as C
import os
import re

import numpy as np

from gaussianprocesspathmodelling_amd import _abi, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DECLARED = {
    "gpx_pathwise_draw": ["gpx_handle*", "int64_t", "int64_t", "uint64_t", "const", "int32_t"],
    "gpx_pathwise_eval": ["gpx_handle*", "const", "int64_t", "int64_t", "int64_t", "void*", "int32_t"],
    "gpx_pathwise_info": ["gpx_handle*", "int64_t*", "int64_t*", "int64_t*"],
    "gpx_pathwise_eval_raw": ["int32_t", "int32_t", "const", "int64_t", "const", "int64_t", "int32_t", "const", "int32_t",
                              "double", "const", "int64_t", "const", "const", "int64_t", "double*"],
}


def test_header_binding_and_sources_carry_the_pathwise_calls():
    text = open(os.path.join(ROOT, "include", "gpx.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name, first_words in DECLARED.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", code)
        assert m, name
        assert [a.split()[0] for a in m.group(1).split(",")] == first_words, name
        res, args = _abi.SIGNATURES[name]
        assert res is C.c_int and len(args) == len(first_words), name
    _P, _PD, _PI = C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int64)
    assert _abi.SIGNATURES["gpx_pathwise_draw"][1] == [_P, C.c_int64, C.c_int64, C.c_uint64, _P, C.c_int32]
    assert _abi.SIGNATURES["gpx_pathwise_eval"][1] == [_P, _P, C.c_int64, C.c_int64, C.c_int64, _P, C.c_int32]
    assert _abi.SIGNATURES["gpx_pathwise_info"][1] == [_P, _PI, _PI, _PI]
    assert _abi.SIGNATURES["gpx_pathwise_eval_raw"][1] == [C.c_int32, C.c_int32, _PD, C.c_int64, _PD, C.c_int64, C.c_int32,
                                                           _PD, C.c_int32, C.c_double, _PD, C.c_int64, _PD, _PD, C.c_int64,
                                                           _PD]
    assert "gpx_pathwise.hip" in build.SOURCES
    assert os.path.exists(os.path.join(build.CSRC, "gpx_pathwise.hip"))


def test_abi_version_and_struct_sizes_are_unchanged():
    text = open(os.path.join(ROOT, "include", "gpx.h")).read()
    assert re.search(r"#define\s+GPX_ABI_VERSION\s+6\b", text) and _abi.ABI_VERSION == 6
    assert C.sizeof(_abi.GpxConfig) == 80
    assert C.sizeof(_abi.GpxTimings) == 8 * 29


def test_null_refusals_without_a_device(gpx):
    for name in DECLARED:
        assert hasattr(gpx, name), name
    assert gpx.gpx_abi_version() == 6
    out = np.full(8, 7.0)
    p = out.ctypes.data_as(C.c_void_p)
    assert gpx.gpx_pathwise_draw(None, 4, 16, 0, None, _abi.MEM_HOST) == _abi.E_ARG
    assert gpx.gpx_pathwise_eval(None, p, 2, 0, 1, p, _abi.MEM_HOST) == _abi.E_ARG
    n = (C.c_int64 * 3)(5, 5, 5)
    pn = [C.cast(C.byref(n, 8 * i), C.POINTER(C.c_int64)) for i in range(3)]
    assert gpx.gpx_pathwise_info(None, *pn) == _abi.E_ARG
    assert list(n) == [5, 5, 5]
    # the stateless primitive: every NULL pointer and every bad size is refused before any device call
    x = np.zeros((4, 1))
    ls = np.array([0.5])
    om, w, v, o = np.zeros((2, 1)), np.zeros((1, 4)), np.zeros((1, 4)), np.full((1, 4), 7.0)
    d = _abi.dptr
    good = [0, 0, d(x), 4, d(x), 4, 1, d(ls), 1, 1.0, d(om), 2, d(w), d(v), 1, d(o)]
    for i in (2, 4, 7, 10, 12, 13, 15):                                # each pointer in turn
        args = list(good)
        args[i] = None
        assert gpx.gpx_pathwise_eval_raw(*args) == _abi.E_ARG
    for i, bad in ((0, 9), (1, 2), (3, 0), (5, 0), (6, 0), (6, 33), (8, 2), (11, 0), (14, 0)):
        args = list(good)
        args[i] = bad
        assert gpx.gpx_pathwise_eval_raw(*args) == _abi.E_ARG
    assert np.all(out == 7.0) and np.all(o == 7.0)                     # nothing written
