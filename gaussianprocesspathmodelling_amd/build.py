"""Build recipe for libgpx.so (hipcc, gfx950 only, in-tree output).

``python -m gaussianprocesspathmodelling_amd.build`` or ``__graft_entry__.build()``.
The shared object lands next to its sources (``csrc/libgpx.so``) so that it travels
with the repo snapshot to the GPU box; it is git-ignored.
"""
from __future__ import annotations

import os
import shutil
import subprocess
import sys

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc")
SOURCES = ["gpx_api.hip", "gpx_blas.hip", "gpx_grad.hip", "gpx_kbuild.hip", "gpx_misc.hip", "gpx_mixed.hip", "gpx_paths.hip", "gpx_posterior.hip", "gpx_deriv.hip", "gpx_hess.hip", "gpx_score.hip", "gpx_update.hip", "gpx_basis.hip", "gpx_loo.hip", "gpx_pathwise.hip", "gpx_sparse.hip"]
HEADERS = ["gpx_internal.h", "gpx_tile.h", "gpx_cov.h", "gpx_env.h", "gpx_shard.inc", "gpx_group.inc", "gpx_sparse.inc", os.path.join("..", "..", "include", "gpx.h")]
LIB = os.path.join(CSRC, "libgpx.so")
ARCH = "gfx950"


def _hipcc() -> str:
    exe = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(exe):
        raise RuntimeError("hipcc not found: libgpx.so cannot be built (no CPU fallback exists)")
    return exe


def needs_build() -> bool:
    if not os.path.exists(LIB):
        return True
    t = os.path.getmtime(LIB)
    deps = [os.path.join(CSRC, s) for s in SOURCES + HEADERS]
    return any(os.path.getmtime(p) > t for p in deps)


def build(force: bool = False, verbose: bool = False) -> str:
    """Compile every HIP translation unit for gfx950 and link libgpx.so.  Objects older than their source or any
    shared header are recompiled (all of them with ``force``), a few at a time."""
    if not force and not needs_build():
        return LIB
    from concurrent.futures import ThreadPoolExecutor
    hipcc = _hipcc()
    hdr_t = max(os.path.getmtime(os.path.join(CSRC, h)) for h in HEADERS)
    objs, jobs = [], []
    for src in SOURCES:
        path = os.path.join(CSRC, src)
        obj = os.path.join(CSRC, src.replace(".hip", ".o"))
        objs.append(obj)
        if force or not os.path.exists(obj) or os.path.getmtime(obj) < max(hdr_t, os.path.getmtime(path)):
            jobs.append([hipcc, "-O3", f"--offload-arch={ARCH}", "-std=c++17", "-fPIC", "-c", path, "-o", obj])

    def run(cmd):
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.run(cmd, check=True)

    with ThreadPoolExecutor(max_workers=min(4, max(1, len(jobs)))) as pool:
        list(pool.map(run, jobs))
    run([hipcc, f"--offload-arch={ARCH}", "-shared", "-fPIC", "-o", LIB + ".tmp"] + objs)
    os.replace(LIB + ".tmp", LIB)
    return LIB


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
