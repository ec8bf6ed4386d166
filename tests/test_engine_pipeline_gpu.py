"""GPU: the software-pipelined k-loop of the MFMA tile engine (gemm_tile_g) at the shapes where a
peeled, rotated and twice-unrolled loop can go wrong.

The engine carries the last MFMAs of every k-step across the step's barrier, peels the first step, walks the rest two
steps per loop trip (one per LDS buffer) with an odd step left over, and drains the carried MFMAs after the last step.
So the cases are the step counts 1 (nothing carried, no loop), 2 (the left-over step alone), 3 (one loop trip), 4 (one
trip and the left-over step) and 5, for the 128-tile and the 64-tile engine, through `gpx_gemm_nt` with the reference and
the bound of tests/test_kernels_gpu.py::test_gemm_nt.

`gpx_gemm_nt` launches outside the library's latency mode, where `launch_gemm_nt_t` picks ONE k-step per barrier for
64-tiles too (KSUB = 1: a barrier per 16 doubles of K, so K = 16, 32, 48 give one, two and three barriers).  The
instantiations with two and four k-steps per barrier only go out from inside a fit; the fits below (N = 384: one panel,
N = 1100: several, with 64-tile strips and block solves in latency mode) and the fp64 handle they are compared with run
them in both element types."""
import numpy as np
import pytest

from gaussianprocesspathmodelling_amd import GP, _abi
from oracle.gp_oracle import synthetic_problem

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps


def _gemm_nt(gpx, A, B, C0, lower):
    m, k = A.shape
    n = B.shape[0]
    Cg = C0.copy()
    assert gpx.gpx_gemm_nt(_abi.dptr(Cg), m, n, _abi.dptr(A), _abi.dptr(B), k, lower) == 0
    return Cg


def _check(gpx, m, n, k, lower):
    rng = np.random.default_rng(m * 7 + n * 3 + k)
    A = rng.standard_normal((m, k))
    B = A if lower else rng.standard_normal((n, k))
    C0 = rng.standard_normal((m, n))
    Cg = _gemm_nt(gpx, A, B, C0, lower)
    ref = C0 - A @ B.T
    tile = 128 if (m % 128 == 0 and n % 128 == 0) else 64
    scale = np.abs(A) @ np.abs(B.T) + np.abs(C0)
    err = np.abs(Cg - ref) / scale
    if lower:
        ti = np.arange(m)[:, None] // tile
        tj = np.arange(n)[None, :] // tile
        done = tj <= ti
        print(f"gemm_nt {m}x{n} k={k} lower: max err {err[done].max():.3e} of bound {4 * k * EPS:.3e}")
        assert err[done].max() <= 4 * k * EPS
        assert np.array_equal(Cg[~done], C0[~done]), "tiles above the diagonal must be untouched"
    else:
        print(f"gemm_nt {m}x{n} k={k}: max err {err.max():.3e} of bound {4 * k * EPS:.3e}")
        assert err.max() <= 4 * k * EPS


# K = 16: one step, nothing carried; 32: the odd left-over step alone; 48: one loop trip, the last step lands in
# buffer 0; 64: a trip and the left-over step; 80: five steps
@pytest.mark.parametrize("k", [16, 32, 48, 64, 80])
@pytest.mark.parametrize("m,n,lower", [(128, 128, 0), (128, 256, 0), (256, 128, 0), (256, 256, 0),
                                       (128, 128, 1), (256, 256, 1)])
def test_gemm_nt_128_tiles_short_walks(gpx, m, n, k, lower):
    _check(gpx, m, n, k, lower)


# 64-tiles (m or n no multiple of 128): one, two and three barriers (K = 16, 32, 48 at one k-step per barrier), 64,
# and 80 — a multiple of 16 but not of 64
@pytest.mark.parametrize("k", [16, 32, 48, 64, 80])
@pytest.mark.parametrize("m,n,lower", [(64, 192, 0), (192, 64, 0), (192, 192, 1), (320, 320, 1)])
def test_gemm_nt_64_tiles_short_walks(gpx, m, n, k, lower):
    _check(gpx, m, n, k, lower)


@pytest.mark.parametrize("k", [16, 48, 112, 2048])
def test_128_and_64_tile_engines_agree_bit_for_bit(gpx, k):
    """Both engines give every accumulator the same MFMAs in the same order (k-steps in order; inside a step the first
    slot's s = 0.., then the second's), so the 128-tile product of a 256 x 256 problem and the 64-tile product of its
    leading 192 x 192 block are the same bits on the shared entries."""
    rng = np.random.default_rng(k)
    A = rng.standard_normal((256, k))
    B = rng.standard_normal((256, k))
    big = _gemm_nt(gpx, A, B, np.zeros((256, 256)), 0)                                      # 128-tiles
    small = _gemm_nt(gpx, np.ascontiguousarray(A[:192]), np.ascontiguousarray(B[:192]), np.zeros((192, 192)), 0)  # 64-tiles
    assert np.array_equal(big[:192, :192], small)


@pytest.fixture(scope="module")
def fits():
    """(fp64 handle's, fp32 handle's) mean, variance and log-determinant per N: computed once, never modified."""
    out = {}
    for N, M in ((384, 64), (1100, 130)):
        X, y, Xs = synthetic_problem(N, 3, M, seed=N)
        res = []
        for dtype in ("float64", "float32"):
            with GP("rbf", (0.3, 0.2, 0.25), 1.5, 1e-1, jitter=0.0, dtype=dtype) as gp:
                mean, var = gp.fit(X, y).predict(Xs)
                assert gp.info_ == 0
                res.append((mean, var, gp.log_det_))
        out[N] = res
    return out


@pytest.mark.parametrize("N", [384, 1100])
def test_fp32_engine_tracks_the_fp64_handle(fits, N):
    """The fp32 instantiation of the engine (128 MFMAs per k-step, 32 floats per line) through a whole fit + predict,
    against the fp64 handle at the tolerance of tests/test_fp32_gpu.py."""
    (m64, v64, l64), (m32, v32, l32) = fits[N]
    assert m32.dtype == np.float32 and v32.dtype == np.float32
    em = np.max(np.abs(m32 - m64)) / np.max(np.abs(m64))
    ev = np.max(np.abs(v32 - v64)) / 1.5
    el = abs(l32 - l64) / abs(l64)
    print(f"fp32 vs fp64 handle N={N}: mean err {em:.2e} (of max|mean|), var err {ev:.2e} (of sf2), logdet rel {el:.2e}")
    assert em <= 2e-3 and ev <= 2e-3 and el <= 1e-3
