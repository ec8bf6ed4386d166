"""CPU: the Matern-3/2 / Matern-1/2 reference (tests/matern_ref.py) against scikit-learn's ``Matern`` kernel and the
scikit-learn fixture tests/golden/G8.npz, and the Python kernel ids against the ``#define``s of include/gpx.h."""
import os
import re
import sys

import numpy as np
import pytest

from gaussianprocesspathmodelling_amd import _abi

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import matern_ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NU = {"matern32": 1.5, "matern12": 0.5}


def g8_case(p):
    g = np.load(os.path.join(ROOT, "tests", "golden", "G8.npz"))
    c = {k[len(p) + 1:]: g[k] for k in g.files if k.startswith(p + "_")}
    ls = c["lengthscale"]
    return c, (ls[0] if ls.size == 1 else ls)


def test_kernel_ids_match_header():
    text = open(os.path.join(ROOT, "include", "gpx.h")).read()
    ids = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define GPX_KERNEL_(\w+)\s+(\d+)", text)}
    assert ids == {"RBF": 0, "MATERN52": 1, "MATERN32": 2, "MATERN12": 3}
    assert _abi.KERNEL_IDS == {name.lower(): v for name, v in ids.items()}


@pytest.mark.parametrize("kernel", matern_ref.KERNELS)
@pytest.mark.parametrize("ls", [0.4, (0.3, 0.5, 0.7)])
def test_kernel_against_sklearn(kernel, ls):
    kernels = pytest.importorskip("sklearn.gaussian_process.kernels")
    rng = np.random.default_rng(5)
    A, B = rng.uniform(0, 1, (40, 3)), rng.uniform(0, 1, (23, 3))
    A[7] = A[2]                                                    # r = 0 off the diagonal
    sf2 = 1.7
    k = kernels.ConstantKernel(sf2) * kernels.Matern(np.asarray(ls, float) if np.ndim(ls) else ls, nu=NU[kernel])
    assert np.allclose(matern_ref.kernel_matrix(A, B, kernel, ls, sf2), k(A, B), rtol=1e-14, atol=0)
    K, Kg = k(A, eval_gradient=True)                               # theta = (log sf2, log l...)
    dK = matern_ref.kernel_dtheta(A, kernel, ls, sf2, 0.1)
    assert np.allclose(matern_ref.kernel_matrix(A, A, kernel, ls, sf2), K, rtol=1e-14, atol=0)
    for t, ref in enumerate(dK[:-2]):
        assert np.allclose(ref, Kg[:, :, 1 + t], rtol=1e-12, atol=1e-15), t
    assert np.allclose(dK[-2], Kg[:, :, 0], rtol=1e-14, atol=0)
    assert np.all(np.isfinite(dK[0])) and dK[0][2, 7] == 0.0


@pytest.mark.parametrize("ls", [0.3, (0.3, 0.5)])
def test_kernel_grad_against_finite_differences(ls):
    rng = np.random.default_rng(6)
    A, B = rng.uniform(0, 1, (9, 2)), rng.uniform(0, 1, (11, 2))
    G = matern_ref.kernel_grad(A, B, "matern32", ls, 1.3)
    h = 1e-6
    for j in range(2):
        Ap, Am = A.copy(), A.copy()
        Ap[:, j] += h
        Am[:, j] -= h
        fd = (matern_ref.kernel_matrix(Ap, B, "matern32", ls, 1.3) - matern_ref.kernel_matrix(Am, B, "matern32", ls,
                                                                                                 1.3)) / (2 * h)
        assert np.max(np.abs(fd - G[j])) <= 1e-7
    with pytest.raises(ValueError):
        matern_ref.kernel_grad(A, B, "matern12", ls, 1.3)


@pytest.mark.parametrize("p", ["m32", "m12"])
def test_dense_gp_against_g8(p):
    c, ls = g8_case(p)
    gp = matern_ref.DenseGP(str(c["kernel"]), ls, float(c["variance"]), float(c["noise"])).fit(c["X"], c["y"])
    mean, cov = gp.predict_cov(c["Xs"])
    m2, var = gp.predict(c["Xs"])
    assert np.max(np.abs(mean - c["mean"])) <= 1e-10 * np.max(np.abs(c["mean"]))
    assert np.max(np.abs(cov - c["cov"])) <= 1e-10 * float(c["variance"])
    assert np.array_equal(m2, mean) and np.max(np.abs(var - np.diag(cov))) <= 1e-12
    assert abs(gp.lml() - float(c["lml"])) <= 1e-10 * abs(float(c["lml"]))
    assert np.max(np.abs(gp.lml_grad() - c["lml_grad"])) <= 1e-9 * np.max(np.abs(c["lml_grad"]))


def test_g8_has_duplicate_inputs_for_matern12():
    c, _ = g8_case("m12")
    X = c["X"]
    assert len(np.unique(X, axis=0)) < len(X)
    assert len(c["Xs"]) % 64 != 0 and c["y"].shape[1] == 2
