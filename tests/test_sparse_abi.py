"""CPU: the six calls of the inducing-point GP are declared, bound, built and exported; they are additive to ABI 6 (no
struct grows); their null refusals need no device."""
import ctypes as C
import os
import re

from gaussianprocesspathmodelling_amd import _abi, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_P, _PD, _I64, _I32, _D = C.c_void_p, C.POINTER(C.c_double), C.c_int64, C.c_int32, C.c_double
_CTYPE = {"gpx_handle*": _P, "const void*": _P, "void*": _P, "int64_t": _I64, "int32_t": _I32, "double": _D,
          "const double*": _PD, "double*": _PD, "int64_t*": C.POINTER(_I64)}

DECLARED = {
    "gpx_sparse_fit": ["gpx_handle*", "const void*", "const void*", "const void*", "int64_t", "int32_t", "int32_t", "const void*",
                       "int64_t", "const double*", "int32_t", "double", "double", "double", "int64_t", "int32_t", "int64_t*"],
    "gpx_sparse_predict": ["gpx_handle*", "const void*", "int64_t", "void*", "void*", "int32_t"],
    "gpx_sparse_predict_cov": ["gpx_handle*", "const void*", "int64_t", "void*", "void*", "int32_t"],
    "gpx_sparse_elbo": ["gpx_handle*", "double*"],
    "gpx_sparse_info": ["gpx_handle*", "int64_t*", "int64_t*", "int64_t*", "int64_t*"],
    "gpx_syrk_tn": ["double*", "int64_t", "const double*", "int64_t", "int32_t"],
}


def _arg_type(arg):
    words = arg.split()
    return " ".join(words[:-1])  # the declaration names every argument: drop the name


def test_header_binding_and_sources_carry_the_six_calls():
    text = open(os.path.join(ROOT, "include", "gpx.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name, types in DECLARED.items():
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, code)
        assert m, name
        assert [_arg_type(a) for a in m.group(1).split(",")] == types, name
        res, args = _abi.SIGNATURES[name]
        assert res is C.c_int and args == [_CTYPE[t] for t in types], name
    assert "gpx_sparse.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "gpx_sparse.hip"))
    assert "gpx_sparse.inc" in build.HEADERS and os.path.exists(os.path.join(build.CSRC, "gpx_sparse.inc"))


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
    info = _I64(7)
    buf = C.cast(out, _P)
    assert gpx.gpx_sparse_fit(None, buf, buf, None, 1, 1, 1, buf, 1, p, 1, 1.0, 1.0, 0.0, 0, 0, C.byref(info)) == _abi.E_ARG
    assert info.value == 7
    assert gpx.gpx_sparse_predict(None, buf, 1, buf, buf, 0) == _abi.E_ARG
    assert gpx.gpx_sparse_predict_cov(None, buf, 1, buf, buf, 0) == _abi.E_ARG
    assert gpx.gpx_sparse_elbo(None, p) == _abi.E_ARG
    n = _I64(5)
    assert gpx.gpx_sparse_info(None, C.byref(n), None, None, None) == _abi.E_ARG and n.value == 5
    assert gpx.gpx_syrk_tn(None, 64, p, 1, 0) == _abi.E_ARG
    assert gpx.gpx_syrk_tn(p, 64, None, 1, 0) == _abi.E_ARG
    assert gpx.gpx_syrk_tn(p, 65, p, 1, 0) == _abi.E_ARG and gpx.gpx_syrk_tn(p, 64, p, 0, 0) == _abi.E_ARG
    assert list(out) == [0.0] * 8                       # nothing written
