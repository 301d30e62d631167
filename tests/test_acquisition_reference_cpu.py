"""The CPU reference of the fused acquisition evaluators (tests/_cpu_acquisition.py) checked on its own: its value is the oracle's EI of the
oracle's posterior, its gradient the central differences of its own value, and the inputs of tests/test_gpu_acquisition_reference.py hold the
conditions that file relies on (a sample of its grid; the GPU tests assert them for every case)."""
import numpy as np
import pytest

from oracle import gp as ogp
from tests import _cpu_acquisition as ref

MEAN, OUTPUTSCALE, NOISE, BEST_F = 0.1, 1.3, 0.05, 0.2


def _problem(kernel, size, rng):
    if kernel.startswith("sphere"):
        return ref.rand_sphere(rng, 4, size), ref.rand_sphere(rng, 11, size)
    return ref.rand_spd_mandel(rng, 4, size), ref.rand_spd_mandel(rng, 11, size)


@pytest.mark.parametrize("kernel,size", [(k, 3) for k in ref.SPD_KERNELS] + [(k, 4) for k in ref.SPHERE_KERNELS])
def test_reference_value_is_the_oracle_and_its_gradient_its_own_central_differences(kernel, size):
    rng = np.random.default_rng(21)
    x, train = _problem(kernel, size, rng)
    y = rng.standard_normal(len(train))
    beta = 0.4
    gram = ref.strip(kernel, train, train, beta)
    for kind, maximize in (("ei", False), ("ei", True), ("mean", False), ("mean", True)):
        def value(pts):
            return ref.acquisition(kernel, pts, train, y, beta, MEAN, OUTPUTSCALE, NOISE, BEST_F, kind, maximize, gram=gram)
        out = value(x)
        mu, var = ogp.gp_posterior(gram, out["ks"], np.full(len(x), ref.kxx(kernel, beta)), y, MEAN, OUTPUTSCALE, NOISE)
        want = ogp.expected_improvement(mu, var, BEST_F, maximize) if kind == "ei" else (mu if maximize else -mu)
        np.testing.assert_allclose(out["value"], want, rtol=1e-12, atol=1e-15)
        np.testing.assert_allclose(value(x)["value"], ref.acquisition(kernel, x, train, y, beta, MEAN, OUTPUTSCALE, NOISE, BEST_F, kind, maximize,
                                                                      solver="cholesky")["value"], rtol=1e-12, atol=1e-15)
        h = 1e-6
        fd = np.zeros_like(x)
        for idx in np.ndindex(x.shape):
            xp, xm = x.copy(), x.copy()
            xp[idx] += h
            xm[idx] -= h
            fd[idx] = (value(xp)["value"][idx[0]] - value(xm)["value"][idx[0]]) / (2 * h)
        assert np.abs(out["grad"]).max() > 1e-2
        np.testing.assert_allclose(out["grad"], fd, rtol=2e-6, atol=1e-7)


def test_reference_kxx_is_the_kernel_at_coincident_arguments():
    rng = np.random.default_rng(3)
    for kernel in ref.SPD_KERNELS:
        x = ref.rand_spd_mandel(rng, 3, 4)
        np.testing.assert_allclose(np.diagonal(ref.strip(kernel, x, x, 0.7)), ref.kxx(kernel, 0.7), rtol=0, atol=2e-15 if kernel != "ai_laplace" else 1e-9)
    e = np.eye(5)[:2]
    for kernel in ref.SPHERE_KERNELS:
        np.testing.assert_allclose(np.diagonal(ref.strip(kernel, e, e, 0.7)), ref.kxx(kernel, 0.7), rtol=4e-16, atol=0)


def test_inputs_of_the_gpu_comparison_hold_their_conditions():
    """the smallest and the largest dimension of every kernel at the largest training set, and one sphere case per kernel: |u| <= 4, variance >= 1e-3,
    max|g| >= 1e-3, and the reference's own spread (dense solve against Cholesky) 10 x below the tolerances of the comparison"""
    import tests.test_gpu_acquisition_reference as gpu          # (its case builders and conditions run on the CPU; only its tests need the device)
    cases = [gpu.spd_case(k, d, 129) for k, d in gpu.SPD_GRID if d in (2, 8, 12)] + [gpu.sphere_case(k, 65, 300) for k in ref.SPHERE_KERNELS]
    for case in cases:
        for kind, maximize in gpu.ACQS:
            a, b = gpu.reference(case, kind, maximize), gpu.reference(case, kind, maximize, solver="cholesky")
            gpu.assert_conditions(a, kind)
            assert (np.abs(a["value"] - b["value"]) <= 0.1 * (gpu.VALUE_RTOL * np.abs(a["value"]) + gpu.VALUE_ATOL)).all()
            assert np.abs(a["grad"] - b["grad"]).max() <= 0.1 * gpu.GRAD_ATOL * np.abs(a["grad"]).max()
