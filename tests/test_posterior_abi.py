"""CPU: the joint-posterior entry points of ABI v6 (gpx_predict_cov, gpx_sample_posterior) exist, are bound, refuse bad
arguments without a GPU, and the NumPy reference of their device normals reproduces the Philox known answers."""
import ctypes as C
import os
import re
import sys

import numpy as np

from gaussianprocesspathmodelling_amd import _abi

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from philox_ref import normals, philox4x32_10, philox_ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gpx_predict_cov", "gpx_sample_posterior")


def test_abi_v6_declares_and_binds_the_posterior_calls(gpx):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gpx.h")).read(), flags=re.S)
    assert re.search(r"#define GPX_ABI_VERSION 6\b", open(os.path.join(ROOT, "include", "gpx.h")).read())
    assert _abi.ABI_VERSION == 6 and gpx.gpx_abi_version() == 6
    for name in NEW:
        assert re.search(rf"\b{name}\s*\(", text) and name in _abi.SIGNATURES and hasattr(gpx, name)
    assert len(_abi.SIGNATURES["gpx_predict_cov"][1]) == 6
    assert len(_abi.SIGNATURES["gpx_sample_posterior"][1]) == 13


def test_predict_cov_null_and_bad_arguments(gpx):
    xs, mean, cov = np.zeros((4, 1)), np.zeros(4), np.zeros((4, 4))
    p = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    fake = C.c_void_p(0)
    assert gpx.gpx_predict_cov(None, p(xs), 4, p(mean), p(cov), _abi.MEM_HOST) == _abi.E_ARG
    assert gpx.gpx_predict_cov(fake, p(xs), 4, p(mean), None, _abi.MEM_HOST) == _abi.E_ARG
    assert gpx.gpx_predict_cov(None, None, 4, None, p(cov), _abi.MEM_HOST) == _abi.E_ARG
    assert gpx.gpx_predict_cov(None, p(xs), 0, p(mean), p(cov), _abi.MEM_HOST) == _abi.E_ARG
    assert gpx.gpx_predict_cov(None, p(xs), -3, p(mean), p(cov), _abi.MEM_HOST) == _abi.E_ARG


def test_sample_posterior_null_and_bad_arguments(gpx):
    xs, out = np.zeros((4, 1)), np.zeros((2, 4, 1))
    p = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    used, info = C.c_double(0.0), C.c_int64(0)

    def call(h=None, x=p(xs), M=4, S=2, o=p(out), u=C.byref(used), i=C.byref(info)):
        return gpx.gpx_sample_posterior(h, x, M, S, 7, None, 0.0, 0.0, 3, o, u, i, _abi.MEM_HOST)

    assert call() == _abi.E_ARG                       # null handle
    assert call(o=None) == _abi.E_ARG                 # null out
    assert call(i=None) == _abi.E_ARG                 # null info
    assert call(u=None) == _abi.E_ARG                 # null jitter_used
    assert call(x=None) == _abi.E_ARG
    assert call(M=0) == _abi.E_ARG and call(M=-1) == _abi.E_ARG
    assert call(S=0) == _abi.E_ARG and call(S=-5) == _abi.E_ARG


def _hex(words):
    return " ".join(f"{int(w):08x}" for w in words)


def test_philox_reference_known_answers():
    assert _hex(philox4x32_10((0, 0, 0, 0), (0, 0))) == "6627e8d5 e169c58d bc57ac4c 9b00dbd8"
    m = 0xFFFFFFFF
    assert _hex(philox4x32_10((m, m, m, m), (m, m))) == "408f276d 41c83b0e a20bc7c6 6d5451fd"


def test_philox_reference_stream_layout():
    # element (s, m, c) is normal number (s M + m) k + c; a pair of normals shares one Philox block
    z = philox_ref(5, 3, 7, 2)
    assert z.shape == (3, 7, 2)
    assert np.array_equal(z.reshape(-1), normals(5, np.arange(42)))
    # the first samples of a longer call are the samples of a shorter one
    assert np.array_equal(philox_ref(5, 8, 7, 2), philox_ref(5, 64, 7, 2)[:8])
    # block 0 of seed 0 is the known answer: u1, u2 from its words, Box-Muller in float64
    w0, w1, w2, w3 = (int(w) for w in philox4x32_10((0, 0, 0, 0), (0, 0)))
    u1 = (((w0 << 32 | w1) >> 11) + 1) * 2.0 ** -53
    u2 = ((w2 << 32 | w3) >> 11) * 2.0 ** -53
    r = np.sqrt(-2.0 * np.log(u1))
    assert normals(0, [0, 1]).tolist() == [r * np.cos(2 * np.pi * u2), r * np.sin(2 * np.pi * u2)]
    assert not np.array_equal(philox_ref(1, 4, 7, 2), philox_ref(2, 4, 7, 2))
    big = philox_ref(11, 4000, 25, 1).reshape(-1)
    assert abs(big.mean()) < 5 / np.sqrt(big.size) and abs(big.var() - 1) < 5 * np.sqrt(2 / big.size)


def test_seed_is_taken_modulo_two_to_the_64():
    assert np.array_equal(normals(2 ** 64 + 3, np.arange(10)), normals(3, np.arange(10)))
    # both halves of the key matter
    assert not np.array_equal(normals(1 << 32, np.arange(10)), normals(0, np.arange(10)))
