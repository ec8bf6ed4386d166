"""CPU: the calls of the bound's gradient are declared, bound, built and exported; they are additive to ABI 6 (no struct
grows); their null refusals need no device."""
import ctypes as C
import os
import re

from gaussianprocesspathmodelling_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_P, _PD, _I64, _I32, _D = C.c_void_p, C.POINTER(C.c_double), C.c_int64, C.c_int32, C.c_double
_CTYPE = {"gpx_handle*": _P, "const void*": _P, "int64_t": _I64, "int32_t": _I32, "double": _D, "const double*": _PD, "double*": _PD}

DECLARED = {
    "gpx_sparse_elbo_grad": ["gpx_handle*", "const void*", "const void*", "const void*", "int64_t", "int32_t", "double*", "double*"],
    "gpx_cross_dtheta_contract": ["int32_t", "const double*", "int64_t", "const double*", "int64_t", "int32_t", "const double*",
                                  "const double*", "int32_t", "double", "double*"],
    "gpx_debug_cross_dtheta_bench": ["int32_t", "int64_t", "int64_t", "int32_t", "int32_t", "int32_t", "double*"],
}


def _arg_type(arg):
    words = arg.split()
    return " ".join(words[:-1])  # the declaration names every argument: drop the name


def test_header_and_binding_carry_the_calls():
    text = open(os.path.join(ROOT, "include", "gpx.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name, types in DECLARED.items():
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, code)
        assert m, name
        assert [_arg_type(a) for a in m.group(1).split(",")] == types, name
        res, args = _abi.SIGNATURES[name]
        assert res is C.c_int and args == [_CTYPE[t] for t in types], name
    assert "gradient of the\n * bound with respect to Z" in text      # what is still not available is said where it was said


def test_abi_version_and_struct_sizes_are_unchanged():
    text = open(os.path.join(ROOT, "include", "gpx.h")).read()
    assert re.search(r"#define\s+GPX_ABI_VERSION\s+6\b", text) and _abi.ABI_VERSION == 6
    assert C.sizeof(_abi.GpxConfig) == 80
    assert C.sizeof(_abi.GpxTimings) == 8 * 29


def test_null_refusals_without_a_device(gpx):
    for name in DECLARED:
        assert hasattr(gpx, name), name
    out = (C.c_double * 8)()
    p = C.cast(out, _PD)
    buf = C.cast(out, _P)
    assert gpx.gpx_sparse_elbo_grad(None, buf, buf, None, 1, 0, p, p) == _abi.E_ARG
    assert gpx.gpx_cross_dtheta_contract(0, None, 1, p, 1, 1, p, p, 1, 1.0, p) == _abi.E_ARG
    assert gpx.gpx_cross_dtheta_contract(0, p, 1, p, 1, 1, None, p, 1, 1.0, p) == _abi.E_ARG
    assert gpx.gpx_cross_dtheta_contract(0, p, 1, p, 1, 1, p, p, 1, 1.0, None) == _abi.E_ARG
    assert gpx.gpx_cross_dtheta_contract(0, p, 1, p, 0, 1, p, p, 1, 1.0, p) == _abi.E_ARG
    assert gpx.gpx_cross_dtheta_contract(0, p, 1, p, 1, 33, p, p, 1, 1.0, p) == _abi.E_ARG
    assert gpx.gpx_debug_cross_dtheta_bench(0, 64, 64, 1, 1, 1, None) == _abi.E_ARG
    assert gpx.gpx_debug_cross_dtheta_bench(0, 63, 64, 1, 1, 1, p) == _abi.E_ARG
    assert list(out) == [0.0] * 8                       # nothing written
