"""No GPU: the host-side argument checks of the four flat-Matern entries (csrc/flat_matern.hip, csrc/gp_mll_matern.hip), the ValueErrors of
the Python layers, and the numpy reference itself (tests/_cpu_flat_matern.py) - its derivatives against central differences and the positive
definiteness of its Gram matrices for every lengthscale, which is what the kernels are for."""
import math
import os

import numpy as np
import pytest
import torch

from gabotorch_amd import _lib, ops
from gabotorch_amd.kernel_utils import kernels_spd
from tests import _cpu_flat_matern as ref

NAN = float("nan")


@pytest.fixture(scope="module", autouse=True)
def _built_library():
    if not os.path.exists(_lib.LIB_PATH):
        from gabotorch_amd import _build
        _build.build()


def _pairwise(lib, n1=4, n2=4, d=3, lengthscale=1.0, nu2=5):
    return lib.gabo_flat_matern_pairwise(None, None, None, 1, n1, n2, d, 0, 0, lengthscale, nu2, None)


def _backward(lib, n1=4, n2=4, d=3, lengthscale=1.0, nu2=5):
    return lib.gabo_flat_matern_backward(None, None, None, None, 1, n1, n2, d, 0, 0, n1 * n2, n2, 1, lengthscale, nu2, 1.0, None)


def _from_distance(lib, count=4, lengthscale=1.0, nu2=5, order=0):
    return lib.gabo_flat_matern_from_distance(None, None, count, lengthscale, nu2, order, None)


def _mll(lib, n=4, lengthscale=1.0, nu2=5):
    return lib.gabo_gp_mll_matern(None, None, n, lengthscale, nu2, 1.0, 0.01, 0.0, None, None)


def test_return_codes_before_any_launch():
    lib = _lib.load()
    ARG, DIM, OK = _lib.GABO_ERR_ARG, _lib.GABO_ERR_DIM, _lib.GABO_OK
    for entry in (_pairwise, _backward, _from_distance, _mll):
        assert entry(lib, nu2=2) == ARG, entry.__name__
        for nu2 in (0, -1, 4, 7):
            assert entry(lib, nu2=nu2) == ARG, (entry.__name__, nu2)
        for lengthscale in (0.0, NAN, -1.0, math.inf):
            assert entry(lib, lengthscale=lengthscale) == ARG, (entry.__name__, lengthscale)
        assert entry(lib) == ARG, entry.__name__                       # valid numbers, null pointers
    assert _pairwise(lib, d=65) == DIM and _pairwise(lib, d=0) == DIM
    assert _backward(lib, d=65) == DIM and _backward(lib, d=_lib.GABO_SPD_MAX_DIM + 1) == DIM
    assert _pairwise(lib, n1=0) == OK and _pairwise(lib, n2=0) == OK and _backward(lib, n1=0) == OK and _from_distance(lib, count=0) == OK
    assert _pairwise(lib, n1=-1) == ARG and _from_distance(lib, count=-1) == ARG
    assert _from_distance(lib, order=2) == ARG and _from_distance(lib, order=-1) == ARG
    assert _mll(lib, n=0) == DIM and _mll(lib, n=161) == DIM and _mll(lib, n=_lib.GABO_GP_MLL_MAX_N) == ARG
    for nu2 in (1, 3, 5):
        assert _pairwise(lib, n1=0, nu2=nu2) == OK


def test_value_errors_of_the_classes_and_of_ops():
    for cls in (kernels_spd.SpdLogEuclideanMaternKernel, kernels_spd.SpdFrobeniusMaternKernel):
        for nu in (0.0, 1.0, 2.0, 3.5, math.inf, NAN, "2.5", None, True):
            with pytest.raises(ValueError):
                cls(nu=nu)
        for nu in ref.NUS:
            k = cls(nu=nu)
            assert k.nu == nu and k.has_lengthscale and [n for n, _ in k.named_parameters()] == ["raw_lengthscale"]
        assert cls().nu == 2.5
        assert type(cls()).__mro__[1].__mro__[1] is kernels_spd.Kernel          # not a subclass of the Gaussian classes
        assert not isinstance(cls(), (kernels_spd.SpdLogEuclideanGaussianKernel, kernels_spd.SpdFrobeniusGaussianKernel))
        x = torch.zeros(2, 5, 6, dtype=torch.float64)
        ones = cls().forward(x, x, diagonal_distance=True)
        assert ones.shape == (2, 5, 1) and bool((ones == 1).all())
    x = torch.zeros(3, 6, dtype=torch.float64)
    g, r = torch.zeros(3, 3, dtype=torch.float64), torch.zeros(3, 3, dtype=torch.float64)
    y = torch.zeros(3, dtype=torch.float64)
    for nu in (1.0, 2.0, 0.0, math.inf, NAN, 0.5000001):
        for call in (lambda: ops.flat_matern_pairwise(x, x, 1.0, nu), lambda: ops.flat_matern_backward(x, x, g, 1.0, nu),
                     lambda: ops.flat_matern_from_distance(r, 1.0, nu), lambda: ops.flat_matern_kernel(x, x, 1.0, nu),
                     lambda: ops.gp_mll_matern(r, y, 1.0, nu, 1.0, 0.01, 0.0)):
            with pytest.raises(ValueError):
                call()
    for lengthscale in (0.0, -2.0, NAN, math.inf):
        for call in (lambda: ops.flat_matern_pairwise(x, x, lengthscale, 2.5), lambda: ops.flat_matern_backward(x, x, g, lengthscale, 2.5),
                     lambda: ops.flat_matern_from_distance(r, lengthscale, 2.5), lambda: ops.flat_matern_kernel(x, x, lengthscale, 2.5),
                     lambda: ops.gp_mll_matern(r, y, lengthscale, 2.5, 1.0, 0.01, 0.0)):
            with pytest.raises(ValueError):
                call()
    with pytest.raises(ValueError):
        ops.flat_matern_from_distance(r, 1.0, 2.5, order=2)
    with pytest.raises(ValueError):
        ops.flat_matern_backward(x, x, g, 1.0, 2.5, wrt=3)


def test_kernel_parameters_does_not_take_the_matern_classes():
    from gabotorch_amd.kernel_utils import kernel_parameters
    for cls in (kernels_spd.SpdLogEuclideanMaternKernel, kernels_spd.SpdFrobeniusMaternKernel):
        with pytest.raises(TypeError):
            kernel_parameters.parameter_map(cls())


@pytest.mark.parametrize("nu", ref.NUS)
def test_reference_derivatives_against_central_differences(nu):
    """h = 1e-5 relative: the truncation error of a central difference is h^2 f''' / 6 ~ 1e-10 relative, its rounding error u / h ~ 1e-11"""
    rng = np.random.default_rng(5)
    for d in (2, 3):
        dv = d * (d + 1) // 2
        x1, x2 = rng.standard_normal((4, dv)), rng.standard_normal((6, dv))
        g = rng.standard_normal((4, 6))
        for ls in (0.3, 1.0, 4.0):
            h = 1e-5 * ls
            r = ref.distance(x1, x2)
            fd = (ref.value(r, ls + h, nu) - ref.value(r, ls - h, nu)) / (2 * h)
            np.testing.assert_allclose(ref.dlengthscale(r, ls, nu), fd, rtol=1e-7, atol=1e-9)
            for wrt, x in ((1, x1), (2, x2)):
                got, _ = ref.backward(x1, x2, g, ls, nu, wrt=wrt)
                fd = np.zeros_like(x)
                for i in range(x.shape[0]):
                    for e in range(dv):
                        step = np.zeros_like(x)
                        step[i, e] = 1e-6
                        args = (lambda s: (x1 + s, x2)) if wrt == 1 else (lambda s: (x1, x2 + s))
                        fd[i, e] = ((g * ref.gram(*args(step), ls, nu)).sum() - (g * ref.gram(*args(-step), ls, nu)).sum()) / 2e-6
                np.testing.assert_allclose(got, fd, rtol=1e-6, atol=1e-8)


@pytest.mark.parametrize("metric", ["log_euclidean", "frobenius"])
@pytest.mark.parametrize("nu", ref.NUS)
def test_reference_gram_is_positive_definite_for_every_lengthscale(metric, nu):
    x = ref.random_spd(np.random.default_rng(40), 40, 3)
    feat = ref.logm_mandel(x) if metric == "log_euclidean" else ref.to_mandel(x)
    for ls in (0.05, 1.0, 20.0):
        k = ref.gram(feat, feat, ls, nu)
        k = 0.5 * (k + k.T)           # (the epsilon makes r_ij and r_ji differ by ~1e-15)
        assert np.linalg.eigvalsh(k).min() > 0.0, (metric, nu, ls)


def test_the_mandel_map_of_the_reference_is_an_isometry():
    x = ref.random_spd(np.random.default_rng(2), 5, 4)
    v = ref.to_mandel(x)
    np.testing.assert_allclose((v[:, None] - v[None]) ** 2 @ np.ones(v.shape[-1]),
                               ((x[:, None] - x[None]) ** 2).sum((-1, -2)), rtol=1e-13, atol=1e-14)
