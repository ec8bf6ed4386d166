"""CPU: the derivative-observation entry points (gpx_set_observation_kinds, gpx_get_observation_kinds; additive to ABI v6)
are declared in the header, bound in _abi and exported by the library, leave the ABI version, gpx_timings and gpx_config as
they were, and refuse a NULL handle and bad arguments without a GPU: GPX_E_ARG, nothing written."""
import ctypes as C
import os
import re

import numpy as np

from gaussianprocesspathmodelling_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"gpx_set_observation_kinds": 5, "gpx_get_observation_kinds": 2}


def test_declared_bound_and_exported(gpx):
    raw = open(os.path.join(ROOT, "include", "gpx.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    for name, nargs in NEW.items():
        m = re.search(rf"\bint\s+{name}\s*\(([^;]*)\)\s*;", text, flags=re.S)
        assert m, f"{name} is not declared in include/gpx.h"
        assert len([a for a in m.group(1).split(",") if a.strip()]) == nargs, name
        assert name in _abi.SIGNATURES and hasattr(gpx, name)
        res, args = _abi.SIGNATURES[name]
        assert res is C.c_int and len(args) == nargs, name
    a = _abi.SIGNATURES["gpx_set_observation_kinds"][1]
    assert a[2] is C.c_int64 and a[3] is C.c_double and a[4] is C.c_int32


def test_abi_version_and_struct_sizes_are_unchanged(gpx):
    raw = open(os.path.join(ROOT, "include", "gpx.h")).read()
    assert re.search(r"#define GPX_ABI_VERSION 6\b", raw)
    assert _abi.ABI_VERSION == 6 and gpx.gpx_abi_version() == 6
    assert C.sizeof(_abi.GpxTimings) == 29 * 8
    assert C.sizeof(_abi.GpxConfig) == (10 + _abi.MAX_GROUP + 2) * 4


def test_null_handle_and_bad_arguments_write_nothing(gpx):
    kinds, out = np.array([-1, 0, -1, 0], dtype=np.int32), np.full(4, 7, dtype=np.int32)
    p = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731

    def call(h=None, k=p(kinds), n=4, s=0.0, mem=_abi.MEM_HOST):
        return gpx.gpx_set_observation_kinds(h, k, n, s, mem)

    assert call() == _abi.E_ARG                      # null handle, everything else fine
    assert call(h=C.c_void_p(0)) == _abi.E_ARG
    assert call(k=None, n=0) == _abi.E_ARG           # (clearing is allowed; the handle is still null)
    assert call(n=-1) == _abi.E_ARG and call(k=None) == _abi.E_ARG and call(s=-1.0) == _abi.E_ARG
    assert call(s=float("nan")) == _abi.E_ARG and call(mem=9) == _abi.E_ARG
    assert gpx.gpx_get_observation_kinds(None, p(out)) == _abi.E_ARG
    assert gpx.gpx_get_observation_kinds(C.c_void_p(0), p(out)) == _abi.E_ARG
    assert np.array_equal(out, np.full(4, 7)) and np.array_equal(kinds, [-1, 0, -1, 0])
