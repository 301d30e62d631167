"""The one-launch marginal likelihood of the sphere Matern kernel on the MI355X: gabo_gp_mll_series (csrc/gp_mll_series.hip) against the numpy
reference of tests/_cpu_gp_mll_series.py, its bit-level contract with the existing series and Gram-form launches, and the fit built on it.

Tolerance of the kernel against the reference, per output:  (64 + 8 cond_2(Ky)) 2^-53 x (the sum of the absolute values of that output's terms).
Every output is a sum of n or n^2 terms whose factors come out of Ky^-1, so an error is relative to the sum of |terms| and amplified by the
condition number; relative to the RESULT it would be meaningless - with few levels the lengthscale gradient cancels from ~1e7 down to ~0.2.
The form and the constant 8 are those of tests/test_gpu_gp_condition.py; cond_2(Ky) < 1e4 for every case below.
Conditioning beyond 1e4 (up to 1e12) of the sweep bodies this launch shares is covered by tests/test_gpu_gp_ill_conditioned.py."""
import math

import numpy as np
import pytest
import torch

from gabotorch_amd import _lib, models, ops
from gabotorch_amd._compat import ScaleKernel
from gabotorch_amd.kernel_utils.kernels_sphere import SphereGaussianKernel, SphereRiemannianMaternKernel
from tests._cpu_gp_mll_series import reference, sphere_points

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -53
KAPPA, PAR = 0.5, (1.7, 0.03, -0.2)            # lengthscale; outputscale, noise, mean
SIZES = (1, 2, 5, 30, 31, 39, 40, 65, 160)     # the two layouts (<= 30 packed, tiles beyond), one wave (<= 39) / several, the maximum
NAMES = ("ll", "d kappa", "d outputscale", "d noise", "d mean")


def t(x):
    return torch.tensor(np.ascontiguousarray(x), dtype=torch.float64, device=DEV)


def _case(n, dim):
    rng = np.random.default_rng(1000 * dim + n)
    x = sphere_points(rng, n, dim)
    return x @ x.T, rng.standard_normal(n)


# Cases that miss the bound with the constant 8, and the constant they get instead: twice what the composed path this launch replaces
# (sphere_zonal_from_inner + gabo_gp_mll_gram + the reduction of W o dK) shows against the reference on that case.  Measured on the MI355X for
# the lengthscale gradient: 1.22e14 and 1.57e15, the new launch and the composed path agreeing bit for bit.  At n = 1 the gradient's only term
# is W_00 dK_00 with dK_00 = sum_k dp_k P_k(1) = sum_k dp_k, which is 0 in exact arithmetic: reference and device each return the rounding of
# their own summation (~2^-53 sum_k |dp_k|, 1e-15 here), and the "sum of absolute terms" - that same rounding - is no scale for it.  In
# dimension 3 the two happen to round alike and the constant 8 holds.
D_KAPPA_CONSTANT = {(1, 10, 2.5, 32): 2 * 1.22e14, (1, 10, math.inf, 32): 2 * 1.57e15}


def _against_the_reference(n, dim, nu, levels):
    c, y = _case(n, dim)
    want, scale, cond = reference(c, y, dim, KAPPA, nu, levels, *PAR)
    p, dp, sd = ops.sphere_matern_coefficients_and_derivative(dim, KAPPA, nu, levels)
    assert len(p) == levels + 1
    out = ops.gp_mll_series(t(c), t(y), p, dp, sd, *PAR)
    assert out[5] == 0.0 and cond < 1e4
    tol = (64.0 + 8.0 * cond) * U * scale
    tol[1] = (64.0 + D_KAPPA_CONSTANT.get((n, dim, nu, levels), 8.0) * cond) * U * scale[1]
    err = np.abs(np.array(out[:5]) - want)
    print(f"n {n} dim {dim} nu {nu} levels {levels}: cond {cond:.3e}; error / tolerance "
          + ", ".join(f"{name} {e / s:.3f}" for name, e, s in zip(NAMES, err, tol)))
    for name, e, s, w in zip(NAMES, err, tol, want):
        assert e <= s, (name, e, s, w)


# every size with 32 levels in both dimensions and for both kernels; every level count - 2, 3, 4 coefficients: the odd tail of the loop that
# takes two levels per iteration; 129: the limit - at n = 40 and n = 160
CASES = [(n, dim, nu, 32) for n in SIZES for dim in (3, 10) for nu in (2.5, math.inf)] \
    + [(n, dim, nu, levels) for n in (40, 160) for dim in (3, 10) for nu in (2.5, math.inf) for levels in (1, 2, 3, 128)]


@pytest.mark.parametrize("n,dim,nu,levels", CASES)
def test_kernel_against_the_numpy_reference(n, dim, nu, levels):
    _against_the_reference(n, dim, nu, levels)


@pytest.mark.parametrize("n", [5, 40, 160])
def test_bits_of_the_series_and_the_sweeps_are_those_of_the_existing_launches(n):
    """the likelihood and its outputscale, noise and mean derivatives equal, bit for bit, gabo_gp_mll_gram on the matrix the element-wise
    series launch returns: the in-kernel series is that evaluator's and the sweeps are the shared body.  The lengthscale derivative against
    (W o dK).sum() / 2 from that call's W: fewer than 32 roundings per term through 16-entry chains and the block tree, a factor 2 on top."""
    dim, nu, levels = 3, 2.5, 32
    c, y = _case(n, dim)
    c, y = t(c), t(y)
    p, dp, sd = ops.sphere_matern_coefficients_and_derivative(dim, KAPPA, nu, levels)
    out = ops.gp_mll_series(c, y, p, dp, sd, *PAR)
    gram, w = ops.gp_mll_gram(ops.sphere_zonal_from_inner(c, p, sd), y, *PAR)
    gram = gram.tolist()
    assert out[5] == 0.0 and gram[5] == 0.0
    for i in (0, 2, 3, 4):
        assert np.float64(out[i]).tobytes() == np.float64(gram[i]).tobytes(), (i, out[i], gram[i])
    terms = (w * ops.sphere_zonal_from_inner(c, dp, sd)).cpu().numpy()
    want, scale = 0.5 * PAR[0] * terms.sum(), 0.5 * PAR[0] * np.abs(terms).sum()
    assert abs(out[1] - want) <= 64 * U * scale, (out[1], want, scale)


@pytest.mark.parametrize("n", [3, 45])
def test_a_matrix_that_is_not_positive_definite_is_reported(n):
    p, dp, sd = ops.sphere_matern_coefficients_and_derivative(3, KAPPA, 2.5, 32)
    ones, y = torch.ones(n, n, dtype=torch.float64, device=DEV), torch.ones(n, dtype=torch.float64, device=DEV)
    out = ops.gp_mll_series(ones, y, p, dp, sd, 1.0, -0.5, 0.0)           # K = ones (sum p = 1) + a negative "noise": indefinite
    assert out[5] == 1.0 and out[:5] == [0.0] * 5


@pytest.mark.parametrize("n", [3, 45])
def test_without_derivative_coefficients_the_lengthscale_gradient_is_zero(n):
    c, y = _case(n, 3)
    c, y = t(c), t(y)
    p, dp, sd = ops.sphere_matern_coefficients_and_derivative(3, KAPPA, 2.5, 32)
    full = ops.gp_mll_series(c, y, p, dp, sd, *PAR)
    none = ops.gp_mll_series(c, y, p, None, sd, *PAR)
    assert none[1] == 0.0 and full[1] != 0.0
    assert [np.float64(v).tobytes() for v in none[:1] + none[2:]] == [np.float64(v).tobytes() for v in full[:1] + full[2:]]


def test_beyond_one_workgroup_the_composed_route_meets_the_same_bound():
    assert _lib.GABO_GP_MLL_MAX_N == 160
    _against_the_reference(170, 3, 2.5, 32)


# ---- the model layer: the existing Matern tests' problem (n = 20 on S^2) and a second one (n = 45 on S^3), under ScaleKernel with Gamma
# priors on outputscale, lengthscale and noise, and bare -----------------------------------------------------------------------------------
def _problem(n, dim, seed):
    if (n, dim) == (20, 3):                                                  # _problem() of tests/test_gpu_sphere_matern.py
        rng = np.random.default_rng(11)
        x = rng.standard_normal((32, 3))
        x /= np.linalg.norm(x, axis=1, keepdims=True)
        y = np.arccos(np.clip(x[:, 0], -1, 1)) ** 2 + 0.05 * rng.standard_normal(32)
        return x[:20], y[:20]
    rng = np.random.default_rng(seed)
    x = sphere_points(rng, n, dim)
    return x, np.arccos(np.clip(x[:, 0], -1, 1)) ** 2 + 0.05 * rng.standard_normal(n)


def _models():
    out = []
    for n, dim in ((20, 3), (45, 4)):
        x, y = _problem(n, dim, 17)

        def scaled(x=x, y=y):
            base = SphereRiemannianMaternKernel(nu=2.5, num_levels=32).double()
            base.register_prior("lengthscale_prior", models.GammaPrior(2.0, 2.0), lambda base=base: base.lengthscale)      # (on kappa)
            base.lengthscale = torch.tensor(0.7, dtype=torch.float64)
            cm = ScaleKernel(base, outputscale_prior=models.GammaPrior(2.0, 0.15)).double()
            return models.SingleTaskGP(t(x), t(y), cm, noise_prior=models.GammaPrior(1.1, 0.05))

        def bare(x=x, y=y):
            base = SphereRiemannianMaternKernel(nu=2.5, num_levels=32).double()
            base.lengthscale = torch.tensor(0.7, dtype=torch.float64)
            return models.SingleTaskGP(t(x), t(y), base, initial_noise=1e-2)

        out += [scaled, bare]
    return out


def test_fast_value_and_gradients_match_autograd():
    """tolerances of tests/test_gpu_gp_fit.py for the plain kernels: value rtol 1e-11 (closure), 1e-7 (scalar objective); gradients rtol 2e-6, atol 1e-9"""
    for make in _models():
        gp = make()
        with torch.no_grad():
            for p in gp.parameters():
                p.add_(0.3)
        for p in gp.parameters():
            p.requires_grad_(True)
        ref = gp.marginal_log_likelihood()
        ref.backward()
        want = [p.grad.clone() for p in gp.parameters()]
        for p in gp.parameters():
            p.grad = None
        assert gp._stationary_form() is None and gp._series_form() is not None
        fast = gp._fast_mll_closure()
        assert fast is not None
        value, proxy = fast()
        proxy.backward()
        np.testing.assert_allclose(value, float(ref), rtol=1e-11)
        for p, w in zip(gp.parameters(), want):
            np.testing.assert_allclose(p.grad.numpy(), w.numpy(), rtol=2e-6, atol=1e-9)
        params = list(gp.parameters())
        objective = gp._fast_scalar_objective(params)
        assert objective is not None
        loss, grad = objective(np.array([float(p) for p in params]))
        np.testing.assert_allclose(loss, -float(ref), rtol=1e-7)
        np.testing.assert_allclose(grad, [-float(w) for w in want], rtol=2e-6, atol=1e-9)


def test_other_kernels_have_no_series_form():
    x, y = _problem(20, 3, 0)
    gp = models.SingleTaskGP(t(x), t(y), ScaleKernel(SphereGaussianKernel(beta_min=0.5)))
    assert gp._series_form() is None and gp._stationary_form() is not None


def test_fast_fit_reaches_the_autograd_fit_without_a_kernel_launch(monkeypatch):
    """fast=True and fast=False from the same start: the same likelihood and hyper-parameters (the plain kernels' tolerances); after
    _series_form() returned, the fast fit calls neither the kernel's forward nor ops.sphere_matern_kernel"""
    for make in _models()[:3]:
        a, b = make(), make()
        calls = {"forward": 0, "ops": 0, "series": 0, "counting": False}
        forward, entry, series_form = SphereRiemannianMaternKernel.forward, ops.sphere_matern_kernel, models.SingleTaskGP._series_form

        def counted_forward(self, *args, **kwargs):
            calls["forward"] += calls["counting"]
            return forward(self, *args, **kwargs)

        def counted_entry(*args, **kwargs):
            calls["ops"] += calls["counting"]
            return entry(*args, **kwargs)

        def counted_series_form(self):
            form = series_form(self)
            calls["series"] += 1
            calls["counting"] = True
            return form

        with monkeypatch.context() as m:
            m.setattr(SphereRiemannianMaternKernel, "forward", counted_forward)
            m.setattr(ops, "sphere_matern_kernel", counted_entry)
            m.setattr(models.SingleTaskGP, "_series_form", counted_series_form)
            models.fit_gpytorch_model(a, fast=True)
        assert calls["series"] >= 1 and calls["forward"] == 0 and calls["ops"] == 0, calls
        models.fit_gpytorch_model(b, fast=False)
        for m_ in (a, b):
            for p in m_.parameters():
                p.requires_grad_(True)
        np.testing.assert_allclose(float(a.marginal_log_likelihood()), float(b.marginal_log_likelihood()), rtol=1e-6, atol=1e-8)
        base = lambda m_: getattr(m_.covar_module, "base_kernel", m_.covar_module)                     # noqa: E731
        hyper = lambda m_: [float(m_.noise), float(m_.mean_constant), float(base(m_).lengthscale)] \
            + ([float(m_.covar_module.outputscale)] if base(m_) is not m_.covar_module else [])      # noqa: E731
        np.testing.assert_allclose(hyper(a), hyper(b), rtol=2e-3, atol=1e-4)


def test_example_runs_with_the_matern_kernel():
    """examples/gabo_sphere.py --kernel matern --dim 3 --iters 3: fast fit and native sweep for the whole loop"""
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "gabo_sphere.py")
    spec = importlib.util.spec_from_file_location("gabo_sphere_example", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    x, y, best = mod.run(dim=3, iters=3, device=DEV, verbose=False, kernel="matern")
    assert x.shape == (8, 3) and y.shape == (8,) and len(best) == 4
    assert bool(torch.isfinite(x).all()) and bool(torch.isfinite(y).all()) and all(math.isfinite(b) for b in best)
    assert all(b1 <= b0 for b0, b1 in zip(best, best[1:]))
