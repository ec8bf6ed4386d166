"""CPU: what the host-buffer unit-test entry points refuse, call by call — the seven kernel-matrix calls (and
gpx_kernel_grad_matrix, the two-family front of gpx_kernel_deriv_matrix), gpx_potrf, gpx_trsm, gpx_gemm_nt and
gpx_path_distance.  Every refusal precedes any HIP call (so it is the same with and without a device), returns the code of
the table, sets a message only where the table names one, and leaves every output buffer untouched.  The tables are literal:
one row per bad call, (changed arguments, return code, substring of gpx_last_error(NULL) or None for "no message set")."""
import ctypes as C

import numpy as np
import pytest

from gaussianprocesspathmodelling_amd import _abi

ARG, UNS = _abi.E_ARG, _abi.E_UNSUPPORTED
M52, M32, M12 = 1, 2, 3
NO_GRAD = "Matern-1/2 is not differentiable"
NAN, INF = float("nan"), float("inf")

# argument order of each kernel-matrix call; upper-case names are arrays (None in a row: a null pointer)
ORDER = {
    "gpx_kernel_matrix": "kernel A na B nb d LS n_ls sf2 diag OUT",
    "gpx_kernel_grad_matrix": "kernel A na B nb d LS n_ls sf2 OUT",
    "gpx_kernel_deriv_matrix": "kernel A na B nb d LS n_ls sf2 OUT",
    "gpx_kernel_path_matrix": "kernel dtype A GA na B GB nb d LS n_ls sf2 LSP n_lsp sg2 OUT",
    "gpx_kernel_path_grad_matrix": "kernel dtype A GA na B GB nb d LS n_ls sf2 LSP n_lsp sg2 OUT",
    "gpx_kernel_mixed_matrix": "kernel dtype A KA na B KB nb d LS n_ls sf2 OUT",
    "gpx_kernel_dl_matrix": "kernel A KA na B KB nb d LS n_ls sf2 OUT",
    "gpx_kernel_path_dtheta_matrix": "kernel A GA na B GB nb d LSP n_lsp sg2 OUT",
}

# rows every kernel-matrix call shares (those that name an argument a call does not take are left out for it)
COMMON = [
    (dict(A=None), ARG, None), (dict(B=None), ARG, None), (dict(OUT=None), ARG, None), (dict(LS=None), ARG, None),
    (dict(na=0), ARG, None), (dict(nb=0), ARG, None), (dict(nb=-1), ARG, None), (dict(d=0), ARG, None), (dict(d=33), ARG, None),
    (dict(n_ls=2), ARG, None), (dict(kernel=4), ARG, None), (dict(kernel=-1), ARG, None), (dict(dtype=2), ARG, None),
    (dict(dtype=-1), ARG, None),
]
IDS = [
    (dict(GA=None), ARG, None), (dict(GB=None), ARG, None), (dict(LSP=None), ARG, None), (dict(n_lsp=2), ARG, None),
    (dict(GA=[0, 1, -2, 3]), ARG, None), (dict(GB=[-2, 1, 0, 3]), ARG, None),
    (dict(LSP=[0.0, 1.0, 1.0]), ARG, None), (dict(LSP=[INF, 1.0, 1.0]), ARG, None), (dict(LSP=[NAN, 1.0, 1.0]), ARG, None),
    (dict(LSP=[1.0, 1.0, -1.0], n_lsp=3), ARG, None),
    (dict(sg2=-1.0), ARG, None), (dict(sg2=NAN), ARG, None), (dict(sg2=INF), ARG, None),
]
KINDS = [
    (dict(KA=[-1, 0, 3, 1]), ARG, None), (dict(KB=[3, -1, -1, -1]), ARG, None),          # kind d
    (dict(KA=[-2, 0, 1, 1]), ARG, None), (dict(KB=[-1, -1, -1, -2]), ARG, None),
]


def _kinds_m12(fn):
    return [
        (dict(kernel=M12, KA=[-1, 0, -1, -1]), UNS, fn + ": " + NO_GRAD), (dict(kernel=M12, KB=[2, -1, -1, -1]), UNS, fn + ": " + NO_GRAD),
        (dict(kernel=M12, KA=[0, -1, -1, -1], KB=[-1, 3, -1, -1]), ARG, None),            # two faults: the bad kind wins
        (dict(kernel=M12, KA=[0, -1, -1, -1], n_ls=2), ARG, None),
    ]


TABLE = {
    # (B = NULL is the symmetric call, so it is no refusal here)
    "gpx_kernel_matrix": [r for r in COMMON if "B" not in r[0]] + [(dict(kernel=M12, na=0), ARG, None)],
    "gpx_kernel_grad_matrix": COMMON + [(dict(kernel=M32), ARG, None), (dict(kernel=M12), ARG, None)],
    "gpx_kernel_deriv_matrix": COMMON + [
        (dict(kernel=M12), UNS, "gpx_kernel_deriv_matrix: " + NO_GRAD),
        (dict(kernel=M12, na=0), ARG, None), (dict(kernel=M12, OUT=None), ARG, None)],
    "gpx_kernel_path_matrix": COMMON + IDS + [(dict(kernel=M12, GA=[0, -2, 0, 0]), ARG, None)],
    "gpx_kernel_path_grad_matrix": COMMON + IDS + [
        (dict(kernel=M12), UNS, "gpx_kernel_path_grad_matrix: " + NO_GRAD),
        (dict(kernel=M12, dtype=1), UNS, "gpx_kernel_path_grad_matrix: " + NO_GRAD),
        (dict(kernel=M12, GA=[0, -2, 0, 0]), ARG, None), (dict(kernel=M12, GB=[0, 0, 0, -2]), ARG, None),   # two faults: the bad id wins
        (dict(kernel=M12, sg2=-1.0), ARG, None), (dict(kernel=M12, dtype=2), ARG, None)],
    "gpx_kernel_mixed_matrix": COMMON + KINDS + _kinds_m12("gpx_kernel_mixed_matrix") + [
        (dict(kernel=M12, dtype=2, KA=[0, -1, -1, -1]), ARG, None)],
    "gpx_kernel_dl_matrix": COMMON + KINDS + _kinds_m12("gpx_kernel_dl_matrix"),
    "gpx_kernel_path_dtheta_matrix": COMMON + IDS + [(dict(kernel=M12, GB=[0, -2, 0, 0]), ARG, None)],
}


def _prime(gpx):
    """a known message in gpx_last_error(NULL): a refusal that sets none leaves it"""
    assert gpx.gpx_create(None, None) == ARG
    assert gpx.gpx_last_error(None) == b"gpx_create: null argument"


def _kernel_call(gpx, fn, out, **kw):
    v = dict(kernel=M52, dtype=0, na=4, nb=4, d=3, n_ls=1, sf2=1.5, diag=0.0, n_lsp=1, sg2=0.4, A=np.zeros((4, 3)), B=np.zeros((4, 3)),
             LS=np.ones(3), LSP=np.ones(3), GA=[0, 1, -1, 1], GB=[1, -1, 0, 0], KA=[-1, 0, 2, -1], KB=[1, -1, -1, 2], OUT=out)
    v.update(kw)
    keep = []           # (the arrays must outlive the call)

    def arg(name):
        x = v[name]
        if not name.isupper() or x is None:
            return x
        if name in ("GA", "GB", "KA", "KB"):
            x = np.asarray(x, dtype=np.int32)
            keep.append(x)
            return x.ctypes.data_as(C.POINTER(C.c_int32))
        x = np.ascontiguousarray(x, dtype=np.float64)
        keep.append(x)
        return _abi.dptr(x)

    return getattr(gpx, fn)(*[arg(n) for n in ORDER[fn].split()])


@pytest.mark.parametrize("fn", sorted(TABLE))
def test_kernel_matrix_entry_points(gpx, fn):
    names = set(ORDER[fn].split())
    out = np.full((4, 4, 4), 7.0)      # (room for the d, n_ls or 1 + n_ls_path blocks of a call that ran by mistake)
    rows = [r for r in TABLE[fn] if set(r[0]) <= names]
    assert len(rows) >= 12
    for kw, code, msg in rows:
        _prime(gpx)
        assert _kernel_call(gpx, fn, out, **kw) == code, (fn, kw)
        got = gpx.gpx_last_error(None).decode()
        assert (msg in got) if msg else (got == "gpx_create: null argument"), (fn, kw, got)
        assert np.all(out == 7.0), (fn, kw)


def _potrf(gpx, out, A="a", n=128, block=128, info="i"):
    a, i = out["a"], out["i"]
    return gpx.gpx_potrf(_abi.dptr(a) if A else None, n, block, C.cast(i.ctypes.data, C.POINTER(C.c_int64)) if info else None)


def _trsm(gpx, out, X="x", m=64, L="l", nb=64):
    return gpx.gpx_trsm(_abi.dptr(out["x"]) if X else None, m, _abi.dptr(out["l"]) if L else None, nb)


def _gemm(gpx, out, Cm="c", m=64, n=64, A="a", B="b", k=16, lower=0):
    return gpx.gpx_gemm_nt(_abi.dptr(out["c"]) if Cm else None, m, n, _abi.dptr(out["a"]) if A else None,
                           _abi.dptr(out["b"]) if B else None, k, lower)


def _dist(gpx, out, paths="p", P=3, cents="c", Cn=2, L=5, D="d", mem_kind=0):
    p = lambda k: C.c_void_p(out[k].ctypes.data)  # noqa: E731
    return gpx.gpx_path_distance(p("p") if paths else None, P, p("c") if cents else None, Cn, L, p("d") if D else None, mem_kind)


DENSE = {
    "gpx_potrf": (_potrf, dict(a=(128, 128), i=(1,)), [
        dict(A=None), dict(info=None), dict(n=0), dict(n=-64), dict(n=65), dict(n=100), dict(block=64), dict(block=192),
        dict(block=-128), dict(n=65, block=64)]),
    "gpx_trsm": (_trsm, dict(x=(64, 64), l=(64, 64)), [
        dict(X=None), dict(L=None), dict(m=0), dict(nb=0), dict(m=65), dict(nb=65), dict(m=-64), dict(nb=32)]),
    "gpx_gemm_nt": (_gemm, dict(c=(128, 128), a=(128, 32), b=(128, 32)), [
        dict(Cm=None), dict(A=None), dict(B=None), dict(m=0), dict(n=0), dict(k=0), dict(m=65), dict(n=65), dict(k=17),
        dict(m=128, n=64, lower=1), dict(m=64, n=128, lower=1)]),
    "gpx_path_distance": (_dist, dict(p=(3, 65, 2), c=(2, 65, 2), d=(3, 2)), [
        dict(paths=None), dict(cents=None), dict(D=None), dict(P=0), dict(Cn=0), dict(L=0), dict(L=65), dict(L=-1),
        dict(mem_kind=2), dict(mem_kind=-1), dict(L=65, mem_kind=1)]),
}


@pytest.mark.parametrize("fn", sorted(DENSE))
def test_dense_entry_points(gpx, fn):
    call, shapes, bad = DENSE[fn]
    bufs = {k: (np.full(s, 7, dtype=np.int64) if k == "i" else np.full(s, 7.0)) for k, s in shapes.items()}
    for kw in bad:                       # every one of these is GPX_E_ARG without a message
        _prime(gpx)
        assert call(gpx, bufs, **kw) == ARG, (fn, kw)
        assert gpx.gpx_last_error(None) == b"gpx_create: null argument", (fn, kw)
        assert all(np.all(b == 7) for b in bufs.values()), (fn, kw)
