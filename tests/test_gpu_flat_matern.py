"""The Matern kernels of the log-Euclidean and Frobenius SPD metrics on the MI355X (csrc/flat_matern.hip, csrc/gp_mll_matern.hip) against the
numpy reference tests/_cpu_flat_matern.py, from the launches up to the fit and the acquisition maximiser.

Tolerances, u = 2^-53, dv = d (d + 1) / 2:
  Gram          |K - K_ref| <= (8 + dv) u.  The argument x = a r carries a relative error of at most (dv / 2 + 4) u (dv fused terms under a square
                root, the epsilon, a, the product), max |x k'(x)| is 0.37 / 0.54 / 0.60 for nu = 1/2, 3/2, 5/2, polynomial and exp add a few u.
  x-gradient    (8 + dv) u sum_j |terms|, the same constant.  Its inputs keep x = a r of order 1 (feature scale 0.3, lengthscale 0.7 and 4),
                where |x w'(x) / w(x)| <= 1 + x stays of the size the Gram bound assumes for |x k'(x)|; the summation adds rounding errors of
                random sign, far below its worst case of n2 u.
  likelihood    (64 + 8 cond_2(Ky)) u sum |terms| per output: the bound of tests/test_gpu_gp_mll_series.py for the same sweeps.
  acquisition   value rtol 1e-9, atol 1e-13, gradient rtol 1e-8, atol 1e-10 max|g|: VALUE_RTOL ... GRAD_ATOL of
                tests/test_gpu_acquisition_reference.py:44, which test_gp_acquisition_kernel_against_the_cpu_reference (:268-269) applies to
                gabo_gp_acquisition, the launch in the middle of the separate-launch chain.
Every comparison prints its worst error / tolerance ratio before it asserts."""
import functools
import math
import os

import numpy as np
import pytest
import torch

from gabotorch_amd import _lib, manifolds, models, ops
from gabotorch_amd._compat import ScaleKernel
from gabotorch_amd.fused_acquisition import FusedAcquisition
from gabotorch_amd.kernel_utils.kernels_spd import (SpdFrobeniusMaternKernel, SpdLogEuclideanGaussianKernel, SpdLogEuclideanMaternKernel)
from gabotorch_amd.manifold_optimization.batched_trust_regions import BatchedTrustRegions
from gabotorch_amd.manifold_optimization.manifold_optimize import joint_optimize_manifold, sequential_optimize_manifold
from gabotorch_amd.Riemannian_utils import spd_constraints_utils_torch as scut
from gabotorch_amd.Riemannian_utils.spd_utils_torch import (symmetric_matrix_to_vector_mandel_torch, vector_to_symmetric_matrix_mandel_torch)
from oracle import spd as ospd
from tests import _cpu_acquisition as cpu_acq
from tests import _cpu_flat_matern as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = ref.U
NUS = ref.NUS
CLASSES = {"le": SpdLogEuclideanMaternKernel, "frob": SpdFrobeniusMaternKernel}


def t(x):
    return torch.tensor(np.ascontiguousarray(x), dtype=torch.float64, device=DEV)


def bits(x):
    return x.detach().contiguous().view(torch.int64).cpu().numpy()


def spd_mandel(rng, n, d, lo=0.3, hi=3.0):
    return ref.to_mandel(ref.random_spd(rng, n, d, lo, hi))


def features(metric, x_mandel):
    mats = ospd.vector_to_symmetric_matrix_mandel(np.asarray(x_mandel))
    return ref.logm_mandel(mats) if metric == "le" else ref.to_mandel(mats)


def kernel(metric, nu, lengthscale):
    k = CLASSES[metric](nu=nu).double()
    k.lengthscale = torch.tensor(lengthscale, dtype=torch.float64)
    return k.to(DEV)


# ------------------------------------------------------------------------------------------------------------- 1. Gram
@pytest.mark.parametrize("n1,n2", [(1, 1), (5, 65), (70, 257)])
@pytest.mark.parametrize("d", [2, 3, 4, 10])
def test_gram_on_given_features_against_the_reference(d, n1, n2):
    dv = d * (d + 1) // 2
    tol = (8 + dv) * U
    rng = np.random.default_rng([d, n1, n2])
    worst = 0.0
    for si, scale in enumerate((1e-3, 0.3, 3.0)):
        for batch in (1, 3):
            shared_left = batch == 3 and si % 2 == 0            # batch 3: one side is one set under a zero batch stride
            a = scale * rng.standard_normal((1 if (batch == 1 or shared_left) else 3, n1, dv))
            b = scale * rng.standard_normal((1 if (batch == 1 or not shared_left) else 3, n2, dv))
            r = ref.distance(np.broadcast_to(a, (batch, n1, dv)), np.broadcast_to(b, (batch, n2, dv)))
            ta, tb = t(a).expand(batch, n1, dv), t(b).expand(batch, n2, dv)
            if batch == 3:
                assert (ta.stride(0) == 0) != (tb.stride(0) == 0)
            for ls in (0.05, 0.7, 4.0):
                for nu in NUS:
                    got = ops.flat_matern_pairwise(ta, tb, ls, nu)
                    assert got.shape == (batch, n1, n2)
                    err = float(np.abs(got.cpu().numpy() - ref.value(r, ls, nu)).max())
                    worst = max(worst, err / tol)
                    assert err <= tol, (scale, batch, ls, nu, err / tol)
    print(f"gram d {d} ({n1}, {n2}): worst error / tolerance {worst:.3f}")


# ------------------------------------------------------------------------------------------------------------- 2. one point set, NaN
def _fused(metric, nu, ls, x, y):
    gp = models.ExactGP(x, y, kernel(metric, nu, ls), outputscale=1.1, noise=1e-2)
    acq = models.ExpectedImprovement(gp, best_f=float(y.min()), maximize=False)
    return acq, FusedAcquisition.build(acq, symmetric_matrix_to_vector_mandel_torch, torch.device(DEV))


@pytest.mark.parametrize("metric", ["le", "frob"])
@pytest.mark.parametrize("d", [2, 3, 5])
def test_one_point_set_gives_a_symmetric_matrix_whose_diagonal_is_kxx(metric, d):
    rng = np.random.default_rng(20 + d)
    x, y = t(spd_mandel(rng, 70, d)), t(rng.standard_normal(70))
    for nu in NUS:
        for ls in (0.05, 0.7, 4.0):
            kern = kernel(metric, nu, ls)
            ls = float(kern.lengthscale.detach())          # (the softplus of the raw parameter: ls to a rounding)
            with torch.no_grad():
                k = kern.forward(x, x)
            assert np.array_equal(bits(k), bits(k.t())), (nu, ls)
            _, fused = _fused(metric, nu, ls, x, y)
            assert fused is not None and not fused.single_launch and fused.matern == (ls, nu) and fused.flavour == metric
            assert np.array_equal(bits(torch.diagonal(k)), np.full(70, np.float64(fused.kxx).view(np.int64))), (nu, ls, fused.kxx)
            want = float(ref.value(d * 1e-15, ls, nu))
            assert abs(fused.kxx - want) <= 4 * U, (fused.kxx, want)
            # the lower triangle and the diagonal are what two separate sets give
            feat = ops.spd_logm_mandel(x) if metric == "le" else x
            two = ops.flat_matern_pairwise(feat, feat.clone(), ls, nu)
            assert np.array_equal(bits(torch.tril(k)), bits(torch.tril(two)))


def test_a_nan_feature_row_gives_nan_in_its_row_and_column_only():
    rng = np.random.default_rng(3)
    for d in (2, 4):
        dv = d * (d + 1) // 2
        f = rng.standard_normal((9, dv))
        f[3, dv - 1] = np.nan
        other = t(rng.standard_normal((6, dv)))
        f = t(f)
        for nu in NUS:
            k = ops.flat_matern_pairwise(f, f, 0.7, nu)
            want = torch.zeros(9, 9, dtype=torch.bool, device=DEV)
            want[3, :] = True
            want[:, 3] = True
            assert torch.equal(torch.isnan(k), want)
            k = ops.flat_matern_pairwise(f, other, 0.7, nu)
            assert torch.equal(torch.isnan(k), want[:, :6] & (torch.arange(9, device=DEV) == 3)[:, None])
            k = ops.flat_matern_pairwise(other, f, 0.7, nu)
            assert torch.equal(torch.isnan(k), (torch.arange(9, device=DEV) == 3)[None, :].expand(6, 9))


def test_a_non_spd_input_gives_nan_where_the_gaussian_class_gives_them():
    rng = np.random.default_rng(4)
    x = spd_mandel(rng, 8, 3)
    bad = ospd.vector_to_symmetric_matrix_mandel(x[2])
    lam, v = np.linalg.eigh(bad)
    lam[0] = -0.4
    x[2] = ref.to_mandel(v @ np.diag(lam) @ v.T)
    x, z = t(x), t(spd_mandel(rng, 5, 3))
    gauss = SpdLogEuclideanGaussianKernel().double().to(DEV)
    prev = ops.set_error_checking(False)
    try:
        for nu in NUS:
            kern = kernel("le", nu, 0.9)
            with torch.no_grad():
                for a, b in ((x, x), (x, z), (z, x), (x, x.clone())):
                    want = torch.isnan(gauss.forward(a, b))
                    assert bool(want.any()) and torch.equal(torch.isnan(kern.forward(a, b)), want)
    finally:
        ops.set_error_checking(prev)


# ------------------------------------------------------------------------------------------------------------- 3. class forwards
@pytest.mark.parametrize("d", [2, 5])
@pytest.mark.parametrize("metric", ["le", "frob"])
def test_class_forward_is_the_pairwise_launch_on_the_features(metric, d):
    rng = np.random.default_rng(30 + d)
    x1, x2 = t(spd_mandel(rng, 7, d)), t(spd_mandel(rng, 66, d))
    for nu in NUS:
        kern = kernel(metric, nu, 0.8)
        with torch.no_grad():
            got = kern.forward(x1, x2)
        f1, f2 = (ops.spd_logm_mandel(x1), ops.spd_logm_mandel(x2)) if metric == "le" else (x1, x2)
        assert np.array_equal(bits(got), bits(ops.flat_matern_pairwise(f1, f2, float(kern.lengthscale.detach()), nu)))
        ones = kern.forward(x1, x2, diagonal_distance=True)
        assert ones.shape == (66, 1) and bool((ones == 1).all())
    np.testing.assert_allclose(ops.spd_logm_mandel(x1).cpu().numpy(), features("le", x1.cpu().numpy()), rtol=0, atol=1e-13)


# ------------------------------------------------------------------------------------------------------------- 4. backward
def _check_backward(x1, x2, g, ls, nu, label):
    dv = x1.shape[-1]
    worst = 0.0
    for wrt in (1, 2):
        want, scale = ref.backward(x1, x2, g, ls, nu, wrt=wrt)
        # a strided grad_out: every second column of a wider matrix (wrt 1), the transpose of a contiguous one (wrt 2)
        if wrt == 1:
            wide = np.zeros((g.shape[0], 2 * g.shape[1]))
            wide[:, ::2] = g
            tg = t(wide)[:, ::2]
        else:
            tg = t(g.T.copy()).t()
        assert not tg.is_contiguous() or min(g.shape) == 1
        got = ops.flat_matern_backward(t(x1), t(x2), tg, ls, nu, wrt=wrt)
        again = ops.flat_matern_backward(t(x1), t(x2), tg, ls, nu, wrt=wrt)
        assert np.array_equal(bits(got), bits(again))
        assert np.array_equal(bits(got), bits(ops.flat_matern_backward(t(x1), t(x2), t(g), ls, nu, wrt=wrt)))
        assert bool(torch.isfinite(got).all())
        ratio = np.abs(got.cpu().numpy() - want) / ((8 + dv) * U * scale)
        worst = max(worst, float(ratio.max()))
        assert ratio.max() <= 1.0, (label, wrt, ratio.max())
    return worst


@pytest.mark.parametrize("n1,n2", [(3, 1), (7, 300)])
@pytest.mark.parametrize("d", [2, 10])
def test_backward_against_the_reference(d, n1, n2):
    dv = d * (d + 1) // 2
    rng = np.random.default_rng([4, d, n1, n2])
    x1, x2 = 0.3 * rng.standard_normal((n1, dv)), 0.3 * rng.standard_normal((n2, dv))
    g = rng.standard_normal((n1, n2))
    worst = max(_check_backward(x1, x2, g, ls, nu, (ls, nu)) for ls in (0.7, 4.0) for nu in NUS)
    print(f"backward d {d} ({n1}, {n2}): worst error / tolerance {worst:.3f}")


@pytest.mark.parametrize("d", [2, 10])
def test_gradient_at_a_training_point_is_finite_for_the_smooth_members(d):
    """x1 = rows of x2: r = d 1e-15 on those pairs; the weights of nu = 3/2, 5/2 contain no division by r"""
    dv = d * (d + 1) // 2
    rng = np.random.default_rng([5, d])
    x2 = 0.3 * rng.standard_normal((40, dv))
    x1 = x2[[0, 7, 39]].copy()
    g = rng.standard_normal((3, 40))
    worst = max(_check_backward(x1, x2, g, ls, nu, (ls, nu)) for ls in (0.7, 4.0) for nu in (1.5, 2.5))
    print(f"backward at training points d {d}: worst error / tolerance {worst:.3f}")


@pytest.mark.parametrize("metric", ["le", "frob"])
@pytest.mark.parametrize("d", [2, 4])
def test_autograd_through_the_classes(metric, d):
    """x1, x2 and the lengthscale.  Frobenius: the features are the inputs, the bound of the backward launch.  Log-Euclidean: the chain ends in the
    adjoint of dlogm, compared with the oracle's at the project's tolerance for SPD gradients against the oracle (rtol 1e-8, atol 1e-10 max|g|)."""
    dv = d * (d + 1) // 2
    rng = np.random.default_rng([6, d])
    x1, x2 = spd_mandel(rng, 6, d, 0.5, 2.0), spd_mandel(rng, 70, d, 0.5, 2.0)
    if metric == "frob":
        x1, x2 = 0.3 * x1, 0.3 * x2
    g = rng.standard_normal((6, 70))
    f1, f2 = features(metric, x1), features(metric, x2)
    for nu in NUS:
        for ls in (0.7, 4.0):
            kern = kernel(metric, nu, ls)
            ls = float(kern.lengthscale.detach())
            a, b = t(x1).requires_grad_(True), t(x2).requires_grad_(True)
            k = kern.forward(a, b)
            ga, gb, gl = torch.autograd.grad((k * t(g)).sum(), [a, b, kern.raw_lengthscale])
            # d / d lengthscale, through the softplus of the raw parameter
            terms = g * ref.dlengthscale(ref.distance(f1, f2), ls, nu)
            raw = float(kern.raw_lengthscale.detach())
            dsoft = 1.0 / (1.0 + math.exp(-raw))
            assert abs(float(gl) - terms.sum() * dsoft) <= ((8 + dv) * U * np.abs(terms).sum() + 4 * U * abs(terms.sum())) * dsoft + 1e-300, (nu, ls)
            for got, wrt, x in ((ga, 1, x1), (gb, 2, x2)):
                want, scale = ref.backward(f1, f2, g, ls, nu, wrt=wrt)
                if metric == "frob":
                    assert (np.abs(got.cpu().numpy() - want) <= (8 + dv) * U * scale).all(), (nu, ls, wrt)
                else:
                    mats = ospd.vector_to_symmetric_matrix_mandel(x)
                    want = ospd.symmetric_matrix_to_vector_mandel(ospd.dlogm_adjoint(mats, ospd.vector_to_symmetric_matrix_mandel(want)))
                    np.testing.assert_allclose(got.cpu().numpy(), want, rtol=1e-8, atol=1e-10 * np.abs(want).max())


# ------------------------------------------------------------------------------------------------------------- 5. likelihood
PAR = (1.7, 0.03, -0.2)                          # outputscale, noise, mean
SIZES = (1, 2, 5, 30, 31, 39, 40, 65, 160)       # the two layouts (<= 30 packed, tiles beyond), one wave (<= 39) / several, the maximum
NAMES = ("ll", "d lengthscale", "d outputscale", "d noise", "d mean")
MLL_LENGTHSCALE = 0.9


@functools.lru_cache(maxsize=None)
def _mll_case(n, d):
    rng = np.random.default_rng(1000 * d + n)
    x = spd_mandel(rng, n, d)
    r = ops.frobenius_pairwise(ops.spd_logm_mandel(t(x)), ops.spd_logm_mandel(t(x)), 1.0, _lib.GABO_OUT_DISTANCE).contiguous()
    return r, t(rng.standard_normal(n))


def _mll_against_the_reference(n, d, nu):
    r, y = _mll_case(n, d)
    want, scale, cond = ref.likelihood(r.cpu().numpy(), y.cpu().numpy(), MLL_LENGTHSCALE, nu, *PAR)
    out = ops.gp_mll_matern(r, y, MLL_LENGTHSCALE, nu, *PAR)
    assert out[5] == 0.0
    tol = (64.0 + 8.0 * cond) * U * scale
    err = np.abs(np.array(out[:5]) - want)
    print(f"n {n} d {d} nu {nu}: cond {cond:.3e}; error / tolerance " + ", ".join(f"{name} {e / s:.3f}" for name, e, s in zip(NAMES, err, tol)))
    for name, e, s, w in zip(NAMES, err, tol, want):
        assert e <= s, (name, e, s, w)
    return out, r, y


@pytest.mark.parametrize("nu", NUS)
@pytest.mark.parametrize("d", [2, 5])
@pytest.mark.parametrize("n", SIZES)
def test_likelihood_against_the_reference_and_the_gram_form(n, d, nu):
    out, r, y = _mll_against_the_reference(n, d, nu)
    gram, _ = ops.gp_mll_gram(ops.flat_matern_from_distance(r, MLL_LENGTHSCALE, nu), y, *PAR, want_w=False)
    gram = gram.tolist()
    for i in (0, 2, 3, 4, 5):
        assert np.float64(out[i]).tobytes() == np.float64(gram[i]).tobytes(), (i, out[i], gram[i])


def test_from_distance_against_the_reference():
    r, _ = _mll_case(65, 5)
    dv = 15
    for nu in NUS:
        for ls in (0.05, 0.7, 4.0):
            k, dk = ops.flat_matern_from_distance(r, ls, nu), ops.flat_matern_from_distance(r, ls, nu, order=1)
            assert (np.abs(k.cpu().numpy() - ref.value(r.cpu().numpy(), ls, nu)) <= (8 + dv) * U).all()
            want = ref.dlengthscale(r.cpu().numpy(), ls, nu)
            # |x d/dx (x^2 q(x) exp(-x))| <= 0.75 and x^2 q(x) exp(-x) <= 0.6 for the three members (nu = 5/2 near x = 5 and x = 2.7):
            # the Gram bound's constant covers both, over the lengthscale
            assert (np.abs(dk.cpu().numpy() - want) <= (8 + dv) * U / ls).all()


@pytest.mark.parametrize("n", [3, 45])
def test_a_matrix_that_is_not_positive_definite_is_reported(n):
    zeros, y = torch.zeros(n, n, dtype=torch.float64, device=DEV), torch.ones(n, dtype=torch.float64, device=DEV)
    for nu in NUS:
        out = ops.gp_mll_matern(zeros, y, 1.0, nu, 1.0, -0.5, 0.0)           # K = ones (r = 0) + a negative "noise": indefinite
        assert out[5] == 1.0 and out[:5] == [0.0] * 5


@pytest.mark.parametrize("nu", NUS)
def test_beyond_one_workgroup_the_composed_route_meets_the_same_bound(nu):
    assert _lib.GABO_GP_MLL_MAX_N == 160
    _mll_against_the_reference(170, 2, nu)


# ------------------------------------------------------------------------------------------------------------- 6. fit
def _fit_problem(n=25, d=3, seed=17):
    rng = np.random.default_rng(seed)
    x = spd_mandel(rng, n, d, 0.5, 2.0)
    mats = ospd.vector_to_symmetric_matrix_mandel(x)
    y = np.log(np.linalg.det(mats)) + 0.3 * np.trace(mats, axis1=-2, axis2=-1) + 0.05 * rng.standard_normal(n)
    return x, y


def _fit_models():
    x, y = _fit_problem()
    out = []
    for metric in ("le", "frob"):
        def scaled(metric=metric):
            base = CLASSES[metric](nu=2.5).double()
            base.register_prior("lengthscale_prior", models.GammaPrior(2.0, 2.0), lambda base=base: base.lengthscale)      # (on the lengthscale)
            base.lengthscale = torch.tensor(1.1, dtype=torch.float64)
            cm = ScaleKernel(base, outputscale_prior=models.GammaPrior(2.0, 0.15)).double()
            return models.SingleTaskGP(t(x), t(y), cm, noise_prior=models.GammaPrior(1.1, 0.05))

        def bare(metric=metric):
            base = CLASSES[metric](nu=1.5).double()
            base.lengthscale = torch.tensor(1.1, dtype=torch.float64)
            return models.SingleTaskGP(t(x), t(y), base, initial_noise=1e-2)

        out += [scaled, bare]
    return out


def test_fast_value_and_gradients_match_autograd():
    """tolerances of tests/test_gpu_gp_mll_series.py: value rtol 1e-11 (closure), 1e-7 (scalar objective); gradients rtol 2e-6, atol 1e-9"""
    for make in _fit_models():
        gp = make()
        with torch.no_grad():
            for p in gp.parameters():
                p.add_(0.3)
        for p in gp.parameters():
            p.requires_grad_(True)
        ref_ll = gp.marginal_log_likelihood()
        ref_ll.backward()
        want = [p.grad.clone() for p in gp.parameters()]
        for p in gp.parameters():
            p.grad = None
        assert gp._stationary_form() is None and gp._series_form() is None and gp._matern_form() is not None
        fast = gp._fast_mll_closure()
        assert fast is not None
        value, proxy = fast()
        proxy.backward()
        np.testing.assert_allclose(value, float(ref_ll), rtol=1e-11)
        for p, w in zip(gp.parameters(), want):
            np.testing.assert_allclose(p.grad.cpu().numpy(), w.cpu().numpy(), rtol=2e-6, atol=1e-9)
        params = list(gp.parameters())
        objective = gp._fast_scalar_objective(params)
        assert objective is not None
        loss, grad = objective(np.array([float(p) for p in params]))
        np.testing.assert_allclose(loss, -float(ref_ll), rtol=1e-7)
        np.testing.assert_allclose(grad, [-float(w) for w in want], rtol=2e-6, atol=1e-9)


def test_other_kernels_have_no_matern_form():
    x, y = _fit_problem()
    gp = models.SingleTaskGP(t(x), t(y), ScaleKernel(SpdLogEuclideanGaussianKernel()))
    assert gp._matern_form() is None and gp._stationary_form() is not None
    gp = models.SingleTaskGP(t(x), t(y), ScaleKernel(SpdLogEuclideanMaternKernel(nu=0.5)))
    r, ls_fn, nu, os_fn = gp._matern_form()
    assert tuple(r.shape) == (25, 25) and nu == 0.5 and ls_fn().numel() == 1 and os_fn().numel() == 1


def test_fast_fit_reaches_the_autograd_fit_without_a_kernel_launch(monkeypatch):
    """fast=True and fast=False from the same start end at likelihoods that agree to 1e-6 relative (the gap tests/test_gpu_gp_mll_series.py allows
    its two fits); after _matern_form() returned, the fast fit calls neither a kernel's forward nor the Gram / differentiable entries of ops"""
    for make in _fit_models():
        a, b = make(), make()
        calls = {"forward": 0, "ops": 0, "form": 0, "counting": False}
        cls = type(getattr(a.covar_module, "base_kernel", a.covar_module))
        forward, entry, pairwise, matern_form = cls.forward, ops.flat_matern_kernel, ops.flat_matern_pairwise, models.SingleTaskGP._matern_form

        def counted_forward(self, *args, **kwargs):
            calls["forward"] += calls["counting"]
            return forward(self, *args, **kwargs)

        def counted_entry(*args, **kwargs):
            calls["ops"] += calls["counting"]
            return entry(*args, **kwargs)

        def counted_pairwise(*args, **kwargs):
            calls["ops"] += calls["counting"]
            return pairwise(*args, **kwargs)

        def counted_form(self):
            form = matern_form(self)
            calls["form"] += 1
            calls["counting"] = True
            return form

        with monkeypatch.context() as m:
            m.setattr(cls, "forward", counted_forward)
            m.setattr(ops, "flat_matern_kernel", counted_entry)
            m.setattr(ops, "flat_matern_pairwise", counted_pairwise)
            m.setattr(models.SingleTaskGP, "_matern_form", counted_form)
            models.fit_gpytorch_model(a, fast=True)
        assert calls["form"] >= 1 and calls["forward"] == 0 and calls["ops"] == 0, calls
        models.fit_gpytorch_model(b, fast=False)
        for m_ in (a, b):
            for p in m_.parameters():
                p.requires_grad_(True)
        la, lb = float(a.marginal_log_likelihood()), float(b.marginal_log_likelihood())
        print(f"{cls.__name__}: fast fit {la:.12g}, autograd fit {lb:.12g}")
        np.testing.assert_allclose(la, lb, rtol=1e-6)


# ------------------------------------------------------------------------------------------------------------- 7. acquisition
OS, NOISE, BEST_OFFSET = 1.3, 0.05, 0.0


@functools.lru_cache(maxsize=None)
def _acq_case(metric, nu):
    rng = np.random.default_rng([7, len(metric), int(2 * nu)])
    x = spd_mandel(rng, 12, 3, 0.5, 2.0)
    y = rng.standard_normal(12)
    base = CLASSES[metric](nu=nu).double()
    base.lengthscale = torch.tensor(0.9, dtype=torch.float64)
    cm = ScaleKernel(base).double()
    cm.outputscale = torch.tensor(OS, dtype=torch.float64)
    gp = models.SingleTaskGP(t(x), t(y), cm, initial_noise=NOISE)
    with torch.no_grad():
        gp.mean_constant.fill_(0.1)
    acq = models.ExpectedImprovement(gp, best_f=float(y.min()), maximize=False)
    return x, y, gp, acq


@pytest.mark.parametrize("nu", NUS)
@pytest.mark.parametrize("metric", ["le", "frob"])
def test_fused_acquisition_runs_the_separate_launch_chain_and_matches_the_cpu_reference(metric, nu):
    x, y, gp, acq = _acq_case(metric, nu)
    post = symmetric_matrix_to_vector_mandel_torch
    fused = FusedAcquisition.build(acq, post, torch.device(DEV))
    assert fused is not None and not fused.single_launch and not fused.one_launch and fused.flavour == metric
    assert fused.mode is None and fused.beta is None
    with pytest.raises(RuntimeError):
        fused.acq_params()
    ls, os_, noise, mean = float(gp.covar_module.base_kernel.lengthscale), float(gp.covar_module.outputscale), float(gp.noise), float(gp.mean_constant)
    rng = np.random.default_rng(71)
    cand = spd_mandel(rng, 5, 3, 0.5, 2.0)
    ft, fc = features(metric, x), features(metric, cand)
    gram = ref.gram(ft, ft, ls, nu)
    gram = np.tril(gram) + np.tril(gram, -1).T
    out = cpu_acq.acquisition_of_strip(ref.gram(fc, ft, ls, nu), gram, y, mean, os_, noise, float(ref.value(3e-15, ls, nu)),
                                       float(y.min()), "ei", False)
    g_feat, _ = ref.backward(fc, ft, out["grad_k"], ls, nu, wrt=1)
    if metric == "le":
        mats = ospd.vector_to_symmetric_matrix_mandel(cand)
        g_want = ospd.symmetric_matrix_to_vector_mandel(ospd.dlogm_adjoint(mats, ospd.vector_to_symmetric_matrix_mandel(g_feat)))
    else:
        g_want = g_feat
    assert np.abs(out["u"]).max() <= 6.0 and out["var"].min() >= 1e-3 and np.abs(g_want).max() >= 1e-4          # conditions on the inputs
    pts = t(cand)
    value, egrad = fused.cost_egrad(vector_to_symmetric_matrix_mandel_torch(pts))
    g_got = fused.egrad_mandel(pts)
    # tests/test_gpu_acquisition_reference.py:44
    np.testing.assert_allclose(-value.cpu().numpy(), out["value"], rtol=1e-9, atol=1e-13)
    np.testing.assert_allclose(-g_got.cpu().numpy(), g_want, rtol=1e-8, atol=1e-10 * np.abs(g_want).max())
    np.testing.assert_allclose(ops.matrix_to_mandel(egrad).cpu().numpy(), g_got.cpu().numpy(), rtol=1e-12, atol=1e-14)
    assert np.array_equal(bits(fused.cost(vector_to_symmetric_matrix_mandel_torch(pts))), bits(value))
    # ... and the model's own route (autograd through the class) says the same
    np.testing.assert_allclose(acq(pts[:, None]).detach().cpu().numpy(), out["value"], rtol=1e-9, atol=1e-13)


def _sweep(acq, options, recorded=None):
    """8 restarts from 32 raw samples under lambda_max <= 2.5; the samples' eigenvalues lie in [0.3, 2.4], so every start is feasible"""
    man = manifolds.PositiveDefinite(3)
    man.min_eig, man.max_eig = 0.3, 2.4

    def rand():
        p = _spd_sample(man)
        if recorded is not None:
            recorded.append(np.asarray(p))
        return p
    man.rand = rand
    cons = [functools.partial(scut.max_eigenvalue_constraint_torch, maximum_eigenvalue=2.5)]
    np.random.seed(0)
    torch.manual_seed(0)
    solver = BatchedTrustRegions(mingradnorm=1e-5, maxiter=30)
    return joint_optimize_manifold(acq, man, solver, q=1, num_restarts=8, raw_samples=32, bounds=None, options=dict(options, device=DEV),
                                   inequality_constraints=cons, pre_processing_manifold=vector_to_symmetric_matrix_mandel_torch,
                                   post_processing_manifold=symmetric_matrix_to_vector_mandel_torch, approx_hessian=True)


def _spd_sample(man):
    """a random SPD matrix with eigenvalues in the manifold's box, from numpy's global stream"""
    lam = man.min_eig + (man.max_eig - man.min_eig) * np.random.rand(3)
    q = np.linalg.qr(np.random.randn(3, 3))[0]
    m = q @ np.diag(lam) @ q.T
    return 0.5 * (m + m.T)


@pytest.mark.parametrize("metric", ["le", "frob"])
def test_joint_optimize_manifold_with_a_matern_surrogate(metric):
    _, _, _, acq = _acq_case(metric, 2.5)
    prev = ops.set_error_checking(False)
    try:
        raw = []
        best = _sweep(acq, {}, raw)
        again = _sweep(acq, {})
        plain = _sweep(acq, {"fused_acquisition": False})
    finally:
        ops.set_error_checking(prev)
    assert best.shape == (1, 6) and np.array_equal(bits(best), bits(again))
    lam = np.linalg.eigvalsh(ospd.vector_to_symmetric_matrix_mandel(best.cpu().numpy()))
    assert lam.min() > 0 and lam.max() <= 2.5 + 1e-6, lam
    value = float(acq(best[:, None].to(DEV)))
    assert len(raw) >= 32
    raw_values = acq(t(ref.to_mandel(np.stack(raw)))[:, None])
    assert value >= float(raw_values.max()), (value, float(raw_values.max()))
    np.testing.assert_allclose(float(acq(plain[:, None].to(DEV))), value, rtol=1e-8, atol=1e-12)


def test_sequential_optimize_manifold_conditions_the_matern_surrogate():
    _, _, _, acq = _acq_case("le", 2.5)
    man = manifolds.PositiveDefinite(3)
    man.min_eig, man.max_eig = 0.3, 3.0
    man.rand = lambda: _spd_sample(man)
    np.random.seed(1)
    torch.manual_seed(1)
    prev = ops.set_error_checking(False)
    try:
        rows = sequential_optimize_manifold(acq, man, BatchedTrustRegions(mingradnorm=1e-4, maxiter=20), q=2, num_restarts=4, raw_samples=16,
                                            bounds=None, options={"device": DEV}, pre_processing_manifold=vector_to_symmetric_matrix_mandel_torch,
                                            post_processing_manifold=symmetric_matrix_to_vector_mandel_torch, approx_hessian=True)
    finally:
        ops.set_error_checking(prev)
    assert rows.shape == (2, 6) and bool(torch.isfinite(rows).all())
    lam = np.linalg.eigvalsh(ospd.vector_to_symmetric_matrix_mandel(rows.cpu().numpy()))
    assert lam.min() > 0
    assert float((rows[0] - rows[1]).abs().max()) > 1e-6          # the believer's observation moved the second proposal


# ------------------------------------------------------------------------------------------------------------- 8. examples
def _example(name):
    import importlib.util
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", name + ".py")
    spec = importlib.util.spec_from_file_location(name + "_example", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_example_runs():
    results = _example("spd_matern_kernel").run(nu=2.5, nb_samples_post=2, verbose=False, device=DEV)
    assert set(results) == {"Log-Euclidean Matern kernel", "Frobenius Matern kernel"}
    for title, res in results.items():
        assert np.isfinite(res["mean"]).all() and (res["variance"] > 0).all() and res["samples"].shape[0] == 2, title
        assert math.isfinite(res["rmse"]) and res["lengthscale"] > 0, title


def test_gabo_spd_example_takes_the_matern_kernel():
    x, y, best = _example("gabo_spd").run(dim=2, iters=2, restarts=3, raw=12, verbose=False, device=DEV, kernel="matern52")
    assert x.shape == (7, 3) and bool(torch.isfinite(x).all()) and bool(torch.isfinite(y).all())
    assert all(b1 <= b0 + 1e-12 for b0, b1 in zip(best, best[1:]))
    with pytest.raises(ValueError):
        _example("gabo_spd").run(kernel="rbf")
