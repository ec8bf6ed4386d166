"""NumPy reference of the device normals of ``gpx_sample_posterior`` (the stream include/gpx.h specifies):
Philox4x32-10 with the Random123 constants, counter (n & 0xffffffff, n >> 32, 0, 0), key (seed & 0xffffffff,
seed >> 32), two 53-bit uniforms per block and Box-Muller in float64."""
import numpy as np

_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_LO = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter, key):
    """counter: 4 uint32 arrays (broadcastable), key: 2 ints -> the 4 output words as uint64 arrays (< 2**32)."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & _LO for c in counter)
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = _M0 * c0, _M1 * c2                   # < 2**64: exact in uint64
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & _LO, p1 >> np.uint64(32), p1 & _LO
        c0, c1, c2, c3 = hi1 ^ c1 ^ np.uint64(k0), lo1, hi0 ^ c3 ^ np.uint64(k1), lo0
        k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
    return c0, c1, c2, c3


def normals(seed, idx):
    """normal numbers idx (int array) of the stream `seed`, float64"""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    i = np.asarray(idx, dtype=np.uint64)
    n = i >> np.uint64(1)
    w0, w1, w2, w3 = philox4x32_10((n & _LO, n >> np.uint64(32), 0, 0), (seed & 0xFFFFFFFF, seed >> 32))
    u1 = ((((w0 << np.uint64(32)) | w1) >> np.uint64(11)) + np.uint64(1)).astype(np.float64) * 2.0 ** -53
    u2 = (((w2 << np.uint64(32)) | w3) >> np.uint64(11)).astype(np.float64) * 2.0 ** -53
    r = np.sqrt(-2.0 * np.log(u1))
    a = 2.0 * np.pi * u2
    return np.where((i & np.uint64(1)) == 1, r * np.sin(a), r * np.cos(a))


def philox_ref(seed, S, M, k):
    """the (S, M, k) normals a call with z = NULL draws: element (s, m, c) is normal number (s M + m) k + c"""
    return normals(seed, np.arange(S * M * k, dtype=np.uint64)).reshape(S, M, k)
