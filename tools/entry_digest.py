"""One SHA-256 per call of the host-buffer unit-test entry points, on fixed-seed inputs: the seven kernel-matrix calls,
gpx_potrf, gpx_trsm, gpx_gemm_nt and gpx_path_distance.  Two builds of the library that print the same lines on the same
machine compute the same bits through these entry points.

    python tools/entry_digest.py [--lib path/to/libgpx.so] [--out file.json]

Shapes: (na, nb) = (65, 63) and (64, 64), d = 3, n_ls = 1 and d, symmetric and cross, ids and kinds with and without -1,
ka / kb each null and given, fp64 and fp32, every kernel family; gpx_potrf n = 256 in blocks of 128, gpx_trsm m = nb = 128,
gpx_gemm_nt 128 x 64 x 32 and lower 128 x 128 x 32, gpx_path_distance P = 70, C = 65, L = 5 from host and device memory."""
import argparse
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gaussianprocesspathmodelling_amd import _abi  # noqa: E402

KERNELS = ("rbf", "matern52", "matern32", "matern12")
D = 3


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def ip(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_int32))


def kernel_calls(lib):
    dp = _abi.dptr
    for na, nb in ((65, 63), (64, 64)):
        rng = np.random.default_rng(1000 * na + nb)
        A, B = rng.uniform(0.0, 1.0, (na, D)), rng.uniform(0.0, 1.0, (nb, D))
        B[:20] = A[:20] + 0.01 * rng.standard_normal((20, D))
        B[0] = A[0]
        side = {"all": (rng.integers(0, 4, na).astype(np.int32), rng.integers(0, 4, nb).astype(np.int32)),
                "some": (rng.integers(-1, 4, na).astype(np.int32), rng.integers(-1, 4, nb).astype(np.int32))}
        kind = {"all": (rng.integers(0, D, na).astype(np.int32), rng.integers(0, D, nb).astype(np.int32)),
                "some": (rng.integers(-1, D, na).astype(np.int32), rng.integers(-1, D, nb).astype(np.int32))}
        for n_ls in (1, D):
            ls, lsp = np.linspace(0.3, 0.6, D)[:n_ls].copy(), np.linspace(0.2, 0.1, D)[:n_ls].copy()
            for kname in KERNELS:
                k, smooth = _abi.KERNEL_IDS[kname], kname != "matern12"
                tag = f"{kname} {na}x{nb} n_ls={n_ls}"
                K = np.full((na, na), 7.0)
                rc = lib.gpx_kernel_matrix(k, dp(A), na, None, 0, D, dp(ls), n_ls, 1.5, 0.25, dp(K))
                yield f"gpx_kernel_matrix sym {tag}", rc, K
                K = np.full((na, nb), 7.0)
                rc = lib.gpx_kernel_matrix(k, dp(A), na, dp(B), nb, D, dp(ls), n_ls, 1.5, 0.0, dp(K))
                yield f"gpx_kernel_matrix cross {tag}", rc, K
                if smooth:
                    G = np.full((D, na, nb), 7.0)
                    rc = lib.gpx_kernel_deriv_matrix(k, dp(A), na, dp(B), nb, D, dp(ls), n_ls, 1.5, dp(G))
                    yield f"gpx_kernel_deriv_matrix {tag}", rc, G
                    if kname in ("rbf", "matern52"):
                        G = np.full((D, na, nb), 7.0)
                        rc = lib.gpx_kernel_grad_matrix(k, dp(A), na, dp(B), nb, D, dp(ls), n_ls, 1.5, dp(G))
                        yield f"gpx_kernel_grad_matrix {tag}", rc, G
                for which, (ga, gb) in side.items():
                    for dtype in (0, 1):
                        K = np.full((na, nb), 7.0)
                        rc = lib.gpx_kernel_path_matrix(k, dtype, dp(A), ip(ga), na, dp(B), ip(gb), nb, D, dp(ls), n_ls, 1.5,
                                                        dp(lsp), n_ls, 0.4, dp(K))
                        yield f"gpx_kernel_path_matrix {tag} ids={which} dtype={dtype}", rc, K
                        if smooth:
                            G = np.full((D, na, nb), 7.0)
                            rc = lib.gpx_kernel_path_grad_matrix(k, dtype, dp(A), ip(ga), na, dp(B), ip(gb), nb, D, dp(ls), n_ls,
                                                                 1.5, dp(lsp), n_ls, 0.4, dp(G))
                            yield f"gpx_kernel_path_grad_matrix {tag} ids={which} dtype={dtype}", rc, G
                    G = np.full((1 + n_ls, na, nb), 7.0)
                    rc = lib.gpx_kernel_path_dtheta_matrix(k, dp(A), ip(ga), na, dp(B), ip(gb), nb, D, dp(lsp), n_ls, 0.4, dp(G))
                    yield f"gpx_kernel_path_dtheta_matrix {tag} ids={which}", rc, G
                for which, (ka, kb) in kind.items():
                    for ua, ub in ((1, 1), (1, 0), (0, 1), (0, 0)):
                        if not smooth and (ua or ub):
                            continue
                        pa, pb = (ka if ua else None), (kb if ub else None)
                        sides = f"kinds={which} ka={'given' if ua else 'null'} kb={'given' if ub else 'null'}"
                        for dtype in (0, 1):
                            K = np.full((na, nb), 7.0)
                            rc = lib.gpx_kernel_mixed_matrix(k, dtype, dp(A), ip(pa), na, dp(B), ip(pb), nb, D, dp(ls), n_ls, 1.5,
                                                             dp(K))
                            yield f"gpx_kernel_mixed_matrix {tag} {sides} dtype={dtype}", rc, K
                        G = np.full((n_ls, na, nb), 7.0)
                        rc = lib.gpx_kernel_dl_matrix(k, dp(A), ip(pa), na, dp(B), ip(pb), nb, D, dp(ls), n_ls, 1.5, dp(G))
                        yield f"gpx_kernel_dl_matrix {tag} {sides}", rc, G


def dense_calls(lib):
    dp = _abi.dptr
    rng = np.random.default_rng(77)
    R = rng.standard_normal((256, 256))
    A = R @ R.T / 256 + 2.0 * np.eye(256)
    info = C.c_int64(-7)
    rc = lib.gpx_potrf(dp(A), 256, 128, C.byref(info))
    yield "gpx_potrf n=256 block=128", rc, np.tril(A), np.array([info.value])
    L = np.tril(rng.standard_normal((128, 128)) * 0.1) + 2.0 * np.eye(128)
    X = rng.standard_normal((128, 128))
    rc = lib.gpx_trsm(dp(X), 128, dp(L), 128)
    yield "gpx_trsm m=128 nb=128", rc, X
    for m, n, k, lower in ((128, 64, 32, 0), (128, 128, 32, 1)):
        Cm, Am, Bm = rng.standard_normal((m, n)), rng.standard_normal((m, k)), rng.standard_normal((n, k))
        rc = lib.gpx_gemm_nt(dp(Cm), m, n, dp(Am), dp(Bm), k, lower)
        yield f"gpx_gemm_nt {m}x{n}x{k} lower={lower}", rc, Cm
    P, Cn, L5 = 70, 65, 5
    paths, cents = rng.standard_normal((P, L5, 2)), rng.standard_normal((Cn, L5, 2))
    Dm = np.full((P, Cn), 7.0)
    vp = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    rc = lib.gpx_path_distance(vp(paths), P, vp(cents), Cn, L5, vp(Dm), _abi.MEM_HOST)
    yield "gpx_path_distance P=70 C=65 L=5 host", rc, Dm
    import torch
    tp, tc = torch.as_tensor(paths, device="cuda"), torch.as_tensor(cents, device="cuda")
    tD = torch.full((P, Cn), 7.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    rc = lib.gpx_path_distance(C.c_void_p(tp.data_ptr()), P, C.c_void_p(tc.data_ptr()), Cn, L5, C.c_void_p(tD.data_ptr()),
                               _abi.MEM_DEVICE)
    yield "gpx_path_distance P=70 C=65 L=5 device", rc, tD.cpu().numpy()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--lib", help="the libgpx.so to load (default: the in-tree build)")
    ap.add_argument("--out", help="write the digests here as well")
    args = ap.parse_args()
    if args.lib:
        _abi.LIB_PATH = os.path.abspath(args.lib)
    lib = _abi.load()
    digests = {}
    for gen in (kernel_calls, dense_calls):
        for label, rc, *arrays in gen(lib):
            if rc != 0:
                raise SystemExit(f"{label}: return code {rc}: {lib.gpx_last_error(None).decode()}")
            assert label not in digests, label
            digests[label] = sha(*arrays)
    text = json.dumps(digests, indent=0)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
