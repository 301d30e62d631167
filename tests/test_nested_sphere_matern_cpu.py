"""Host side of the nested-sphere Riemannian Matern kernel (no GPU): the constructor of NestedSphereRiemannianMaternKernel, the random axes
NestedSphereGaussianKernel still draws, the argument checks of gabo_nested_sphere_fit_evaluate_series, and the chain rule of
SingleTaskGP._fast_scalar_objective when its evaluator takes the lengthscale itself."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

from gabotorch_amd import _lib, models
from gabotorch_amd._compat import ScaleKernel
from gabotorch_amd.kernel_utils.kernels_nested_sphere import NestedSphereGaussianKernel, NestedSphereRiemannianMaternKernel
from gabotorch_amd.kernel_utils.kernels_sphere import SphereLaplaceKernel


@pytest.fixture(scope="module", autouse=True)
def _built_library():
    if not os.path.exists(_lib.LIB_PATH):
        from gabotorch_amd import _build
        _build.build()


def test_constructor_parameters_and_validation():
    k = NestedSphereRiemannianMaternKernel(6, 3, nu=1.5, num_levels=16)
    names = [n for n, _ in k.named_parameters()]
    assert sorted(names) == sorted(["raw_lengthscale", "raw_axis_S6", "raw_axis_S5", "raw_axis_S4"])
    assert k.nu == 1.5 and k.num_levels == 16 and k.dim == 6 and k.latent_dim == 3
    assert [tuple(a.shape) for a in k.axes] == [(1, 6), (1, 5), (1, 4)]
    gauss = NestedSphereGaussianKernel(6, 3, beta_min=0.6)
    for d in (6, 5, 4):
        assert type(getattr(k, f"raw_axis_S{d}_manifold")) is type(getattr(gauss, f"raw_axis_S{d}_manifold"))
        assert getattr(k, f"raw_axis_S{d}_manifold")._shape == getattr(gauss, f"raw_axis_S{d}_manifold")._shape
    assert len(k.distances_to_axis) == 3
    for r, rg in zip(k.distances_to_axis, gauss.distances_to_axis):       # pi / 2, as the Gaussian kernel holds it
        assert r.shape == (1, 1) and torch.equal(r, rg) and float(r) == pytest.approx(math.pi / 2, rel=1e-7)
    assert float(k.lengthscale) > 0.0
    new = [np.eye(d)[:1] for d in (6, 5, 4)]
    k.axes = new
    for a, b in zip(k.axes, new):
        np.testing.assert_array_equal(a.detach().numpy(), b)
    assert math.isinf(NestedSphereRiemannianMaternKernel(5, 2, nu=math.inf).nu)
    for bad in (dict(nu=0.0), dict(nu=-1.0), dict(num_levels=0), dict(num_levels=129), dict(num_levels=2.5)):
        with pytest.raises(ValueError):
            NestedSphereRiemannianMaternKernel(5, 3, **bad)
    for latent in (1, 0):
        with pytest.raises(ValueError):
            NestedSphereRiemannianMaternKernel(5, latent)


@pytest.mark.parametrize("cls", ["gaussian", "matern"])
def test_seeded_axes_are_the_randn_sequence(cls):
    """the axes are drawn by torch.randn(1, d), d = dim ... latent + 1 in that order, and nothing else is drawn in the constructor: seeded
    tests of the Gaussian kernel keep the axes they had before the two kernels shared this code"""
    dim, latent = 7, 3
    torch.manual_seed(4)
    k = NestedSphereGaussianKernel(dim, latent, beta_min=0.6) if cls == "gaussian" else NestedSphereRiemannianMaternKernel(dim, latent)
    torch.manual_seed(4)
    for d, axis in zip(range(dim, latent, -1), k.axes):
        a = torch.randn(1, d)
        np.testing.assert_array_equal(axis.detach().numpy(), (a / torch.norm(a)).numpy())
    assert [n for n, _ in k.named_parameters() if n.startswith("raw_axis")] == [f"raw_axis_S{d}" for d in range(dim, latent, -1)]


def test_entry_validates_on_the_host_before_any_hip_call():
    lib = _lib.load()
    f, size = lib.gabo_nested_sphere_fit_evaluate_series, lib.gabo_nested_sphere_fit_series_workspace_bytes

    def call(n=12, D=5, levels=2, n_coeff=33):
        return f(None, None, None, None, n, D, levels, None, None, n_coeff, 1.0, 0.1, 0.0, 1, None, None, 0, None, 0, None)

    assert call(D=5, levels=4) == _lib.GABO_ERR_DIM                      # latent dimension 1: series dimension 0
    assert call(D=80, levels=10) == _lib.GABO_ERR_DIM                    # latent dimension > 64
    assert call(D=5, levels=5) == _lib.GABO_ERR_DIM and call(D=5, levels=0) == _lib.GABO_ERR_DIM
    assert call(n=0) == _lib.GABO_ERR_DIM and call(n=_lib.GABO_GP_MLL_LARGE_MAX_N + 1) == _lib.GABO_ERR_DIM
    assert call() == _lib.GABO_ERR_ARG                                   # null pointers
    assert call(n_coeff=0) == _lib.GABO_ERR_ARG and call(n_coeff=130) == _lib.GABO_ERR_ARG
    # every pointer given: the coefficient count, then the two buffer sizes
    n, D, L, nc = 12, 5, 2, 33
    total = D + (D - 1)
    need_ws, need_pinned = size(n, D, L, nc), 2 * total + L + 1 + 4 * nc + 7
    buf = (ctypes.c_double * 1024)()
    ptr = ctypes.addressof(buf)

    def full(n_coeff=nc, ws=need_ws, pinned=need_pinned, skip=None):
        args = [ptr, ptr, ptr, ptr, n, D, L, ptr, ptr, n_coeff, 1.0, 0.1, 0.0, 1, ptr, ptr, ws, ptr, pinned, None]
        if skip is not None:
            args[skip] = None
        return f(*args)

    for bad in (0, 130):
        assert full(n_coeff=bad) == _lib.GABO_ERR_ARG
    assert full(ws=need_ws - 1) == _lib.GABO_ERR_ARG and full(pinned=need_pinned - 1) == _lib.GABO_ERR_ARG
    for skip in (0, 1, 2, 3, 7, 8, 14, 15, 17):
        assert full(skip=skip) == _lib.GABO_ERR_ARG, skip
    # the size function: zero for what the entry rejects, growing in every argument otherwise
    assert size(0, 5, 2, 33) == 0 and size(12, 5, 5, 33) == 0 and size(12, 5, 2, 0) == 0 and size(12, 5, 2, 130) == 0
    assert 0 < size(12, 5, 2, 33) <= size(12, 5, 2, 129) and size(12, 5, 2, 33) < size(13, 5, 2, 33) < size(13, 21, 18, 33)
    assert size(190, 12, 10, 17) > lib.gabo_gp_mll_large_workspace_bytes(190) + 2 * 190 * 190 * 8
    assert size(12, 51, 47, 33) > 12 * (51 * 47 - 47 * 46 // 2) * 8


def _model(base, n=6, dim=5):
    rng = np.random.default_rng(5)
    x = rng.standard_normal((n, dim))
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    y = rng.standard_normal(n)
    cm = ScaleKernel(base, outputscale_prior=models.GammaPrior(2.0, 0.15)).double()
    return models.SingleTaskGP(torch.tensor(x), torch.tensor(y), cm, noise_prior=models.GammaPrior(1.1, 0.05)), n


def _scalar_plan(gp, base):
    cm = gp.covar_module
    params = [base.raw_lengthscale, cm.raw_outputscale, gp.raw_noise, gp.mean_constant]
    return params


def test_fast_scalar_objective_hands_the_lengthscale_itself_to_the_evaluator():
    base = NestedSphereRiemannianMaternKernel(5, 3)
    gp, n = _model(base)
    params = _scalar_plan(gp, base)
    seen = []
    stub = (-3.25, 0.7, -0.4, 1.3, 0.2, 0.0)              # ll, d kappa, d outputscale, d noise, d mean, flag

    def evaluator(kappa, outputscale, noise, mean):
        seen.append((kappa, outputscale, noise, mean))
        return stub

    objective = gp._fast_scalar_objective(params, evaluator=evaluator, evaluator_takes_value=True)
    assert objective is not None
    v = np.array([0.3, -0.2, 0.5, 0.1])
    loss, grad = objective(v)
    lower = float(base.raw_lengthscale_constraint.lower_bound)
    raw = float(np.float32(v[0])) if base.raw_lengthscale.dtype == torch.float32 else float(v[0])
    softplus = math.log1p(math.exp(raw))
    kappa = lower + softplus
    assert len(seen) == 1 and seen[0][0] == pytest.approx(kappa, rel=1e-15) and seen[0][3] == v[3]
    dsoft = 1.0 / (1.0 + math.exp(-raw))
    # (no prior on the lengthscale here: the gradient entry is the stub's d / d kappa through the softplus alone)
    assert grad[0] == pytest.approx(-(stub[1] * dsoft) / n, rel=1e-14)
    assert grad[3] == pytest.approx(-stub[4] / n, rel=1e-14)
    assert np.isfinite(loss)
    # the not-positive-definite flag: the barrier value and a zero gradient
    flagged = gp._fast_scalar_objective(params, evaluator=lambda *a: (0.0, 0.0, 0.0, 0.0, 0.0, 1.0), evaluator_takes_value=True)
    loss, grad = flagged(v)
    assert loss == 1e10 and not grad.any()


def test_fast_scalar_objective_default_keeps_the_inverse_square_lengthscale():
    """without the keyword an evaluator of a lengthscale kernel receives theta = l^-2 and its derivative is chained through -2 l^-3"""
    base = SphereLaplaceKernel()
    gp, n = _model(base)
    params = [base.raw_lengthscale, gp.covar_module.raw_outputscale, gp.raw_noise, gp.mean_constant]
    seen = []
    stub = (-3.25, 0.7, -0.4, 1.3, 0.2, 0.0)

    def evaluator(theta, outputscale, noise, mean):
        seen.append(theta)
        return stub

    objective = gp._fast_scalar_objective(params, evaluator=evaluator)
    assert objective is not None
    v = np.array([0.3, -0.2, 0.5, 0.1])
    _, grad = objective(v)
    raw = float(np.float32(v[0])) if base.raw_lengthscale.dtype == torch.float32 else float(v[0])
    ls = float(base.raw_lengthscale_constraint.lower_bound) + math.log1p(math.exp(raw))
    assert seen == [pytest.approx(ls ** -2, rel=1e-15)]
    assert grad[0] == pytest.approx(-(stub[1] * (-2.0 * ls ** -3)) / (1.0 + math.exp(-raw)) / n, rel=1e-14)
