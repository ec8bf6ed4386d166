"""CPU: gpx_remove_rows (additive to ABI v6) is declared in the header, bound in _abi and exported by the library, refuses
bad arguments without a GPU, and GP.remove / PathModel.remove_paths validate their arguments before any library call."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from gaussianprocesspathmodelling_amd import GP, _abi
from gaussianprocesspathmodelling_amd.paths import PathModel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_declared_bound_and_exported(gpx):
    raw = open(os.path.join(ROOT, "include", "gpx.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    assert re.search(r"#define GPX_ABI_VERSION 6\b", raw) and _abi.ABI_VERSION == 6
    assert gpx.gpx_abi_version() == 6
    assert re.search(r"\bint\s+gpx_remove_rows\s*\(\s*gpx_handle\*\s*h,\s*int64_t\s+start,\s*int64_t\s+count,\s*int64_t\*\s*info\)",
                     text)
    assert "gpx_remove_rows" in _abi.SIGNATURES and hasattr(gpx, "gpx_remove_rows")
    assert len(_abi.SIGNATURES["gpx_remove_rows"][1]) == 4
    # additive: the structs keep their layout, the removal books into the fit's timing fields
    assert C.sizeof(_abi.GpxTimings) == 29 * 8 and C.sizeof(_abi.GpxConfig) == 80


def test_null_handle(gpx):
    info = C.c_int64(7)
    assert gpx.gpx_remove_rows(None, 0, 1, C.byref(info)) == _abi.E_ARG
    assert gpx.gpx_remove_rows(C.c_void_p(0), 0, 0, C.byref(info)) == _abi.E_ARG
    assert info.value == 7                           # nothing was written


class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"{name} called: the arguments must be refused before any library call")


def _model(N=100, fitted=True, groups=False):
    gp = object.__new__(GP)                          # no handle: GP.__del__ / close() find nothing to destroy
    gp._h, gp._lib = None, _NoLibrary()
    gp._fitted, gp._N, gp._groups_set, gp._alpha = fitted, N, groups, None
    return gp


def test_gp_remove_validates_before_touching_the_handle():
    with pytest.raises(RuntimeError):
        _model(fitted=False).remove(0, 5)
    gp = _model()
    for args, kw in (((-1, 5), {}), ((5, 101), {}), ((7, 3), {}), ((0.0, 5), {}), ((0, 100), {}), (([3, 100],), {}),
                     (([-1],), {}), ((np.array([1.0, 2.0]),), {}), ((np.arange(100),), {}), ((np.zeros((2, 2), dtype=int),), {}),
                     ((), {}), ((), {"path_ids": [3]}), ((0, 5), {"path_ids": [3]}), (([1],), {"path_ids": [3]})):
        with pytest.raises(ValueError):
            gp.remove(*args, **kw)
    assert gp.remove(5, 5) is gp and gp.remove([]) is gp and gp.remove(np.zeros(0, dtype=np.int64)) is gp
    assert gp._N == 100 and gp._fitted
    with pytest.raises(ValueError):
        _model(groups=True).remove(path_ids=[-1])
    with pytest.raises(ValueError):
        _model(groups=True).remove(path_ids=[0.5])


def _path_model(**kw):
    one = np.ones(1)
    return PathModel(_model(), ["a", "b", "c"], one * 0, one, one * 0, one, ("t",), ("x", "y"), **kw)


def test_remove_paths_validates_before_touching_the_model():
    pm = _path_model(row_counts=[33, 33, 33])
    with pytest.raises(KeyError):
        pm.remove_paths(["b", "nope"])
    with pytest.raises(ValueError):
        pm.remove_paths(["a", "b", "c"])             # a model keeps one path
    assert pm.remove_paths([]) is pm and pm.keys == ["a", "b", "c"]
    with pytest.raises(ValueError, match="velocities"):
        _path_model(has_velocities=True, row_counts=[33, 33, 33]).remove_paths(["a"])
    with pytest.raises(ValueError, match="row counts"):
        _path_model().remove_paths(["a"])
    # the numbering of a model nothing was removed from is the index in keys
    assert _path_model(within_path=True)._path_kw("c") == {"path_ids": 2}
