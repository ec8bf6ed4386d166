"""CPU: the basis-function entry points (gpx_set_basis, gpx_get_basis; additive to ABI v6) are declared in the header,
bound in _abi and exported by the library, leave the ABI version and the two structs as they were, and refuse bad arguments
without a GPU; the Python host refuses an unknown basis before any library call.  (The refusal of a bad VALUE on a live
handle needs a device to create the handle: tests/test_basis_gpu.py.)"""
import ctypes as C
import os
import re

import numpy as np
import pytest

from gaussianprocesspathmodelling_amd import GP, _abi, build
from gaussianprocesspathmodelling_amd import paths as gpaths

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"gpx_set_basis": 2, "gpx_get_basis": 5}


def test_declared_bound_and_exported(gpx):
    raw = open(os.path.join(ROOT, "include", "gpx.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    for name, nargs in NEW.items():
        m = re.search(rf"\bint\s+{name}\s*\(([^;]*)\)\s*;", text, flags=re.S)
        assert m and len([a for a in m.group(1).split(",") if a.strip()]) == nargs, name
        res, args = _abi.SIGNATURES[name]
        assert res is C.c_int and len(args) == nargs and hasattr(gpx, name)
    assert _abi.SIGNATURES["gpx_set_basis"][1][1] is C.c_int32
    for name, value in (("NONE", 0), ("CONSTANT", 1), ("LINEAR", 2), ("QUADRATIC", 3)):
        assert re.search(rf"#define GPX_BASIS_{name} {value}\b", raw)
    assert _abi.BASIS_IDS == {None: 0, "constant": 1, "linear": 2, "quadratic": 3}
    assert "gpx_basis.hip" in build.SOURCES


def test_abi_version_and_struct_sizes_are_unchanged(gpx):
    raw = open(os.path.join(ROOT, "include", "gpx.h")).read()
    assert re.search(r"#define GPX_ABI_VERSION 6\b", raw)
    assert _abi.ABI_VERSION == 6 and gpx.gpx_abi_version() == 6
    assert C.sizeof(_abi.GpxTimings) == 29 * 8
    assert C.sizeof(_abi.GpxConfig) == (10 + _abi.MAX_GROUP + 2) * 4


def test_null_handle_is_refused(gpx):
    b, p = C.c_int32(-7), C.c_int32(-7)
    beta = np.full(4, 9.0)
    for basis in (0, 1, 2, 3, 4, -1):
        assert gpx.gpx_set_basis(None, basis) == _abi.E_ARG
        assert gpx.gpx_set_basis(C.c_void_p(0), basis) == _abi.E_ARG
    assert gpx.gpx_get_basis(None, C.byref(b), C.byref(p), _abi.dptr(beta), None) == _abi.E_ARG
    assert b.value == -7 and p.value == -7 and np.array_equal(beta, np.full(4, 9.0))   # nothing was written


def test_an_unknown_basis_is_a_value_error_before_any_library_call():
    gp = GP.__new__(GP)          # no handle, no library: the check has to come first
    X, y = np.zeros((4, 1)), np.zeros(4)
    for bad in ("cubic", "Linear", 2, ""):
        with pytest.raises(ValueError, match="basis"):
            gp.fit(X, y, basis=bad)
        with pytest.raises(ValueError, match="basis"):
            gp.fit_predict(X, y, X, basis=bad)
        with pytest.raises(ValueError, match="basis"):
            gp.optimize(X, y, basis=bad)
    with pytest.raises(ValueError, match="basis"):
        gpaths.fit_path_models(gpaths.Trajectories(), {}, trend="cubic")
    gp._h = None                 # (what close() expects of an object that never had a handle)
