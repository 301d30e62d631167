"""The one-call surrogate fit of the affine-invariant SPD Matern / heat kernels on the MI355X (csrc/spd_ai_spectral_fit.hip) against the numpy
reference tests/_cpu_spd_ai_spectral_fit.py, launch by launch, as a chain, and through the model layer.

In every comparison the device's own log-diagonals (ops.spd_ai_logdiag) are handed to the reference: their error is the business of
tests/test_gpu_spd_ai_spectral.py.  Tolerances, u = 2^-53:
  points     lam, w, c: 64 u relative; q: 64 u (|q| + the sum of the absolute values of its terms).
  Gd         fit.gdot_tolerance: the rounding of the phase and the log-amplitude, amplified by 1 + |c theta| + |q| (derived there; the fp64 numpy
             evaluation stays within 1/8 of it of its own long-double evaluation: tests/test_spd_ai_spectral_fit_cpu.py).
  K          tol_K of tests/test_gpu_spd_ai_spectral.py with tol_a = 64 u max|a| (the reference reads the device's a, so only that floor of
             tol_a is left), plus 2L u for the sum of 2L products.
  chain      (64 + 8 cond_2(Ky)) u (sum of the absolute values of the output's terms), the form and constants of
             tests/test_gpu_gp_mll_series.py and tests/test_gpu_gp_condition.py; cond_2(Ky) <= (1.3 * 200 + 0.05) / 0.05 < 1e4 is asserted.
Every comparison prints its worst error / tolerance ratio before it asserts."""
import functools
import math

import numpy as np
import pytest
import torch

from gabotorch_amd import _lib, models, ops
from gabotorch_amd._compat import ScaleKernel
from gabotorch_amd.kernel_utils.kernels_spd import SpdAffineInvariantMaternKernel
from tests import _cpu_spd_ai_spectral as ref
from tests import _cpu_spd_ai_spectral_fit as fit

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = ref.U
LD = np.longdouble
NUS = (0.5, 2.5, math.inf)
N_SET, L_SET = 200, 130
OUTPUTSCALE, NOISE, MEAN = 1.3, 0.05, 0.2


def t(x):
    return torch.tensor(np.ascontiguousarray(x), dtype=torch.float64, device=DEV)


def bits(x):
    return x.detach().contiguous().view(torch.int64).cpu().numpy()


def fbits(values):
    return [np.float64(v).tobytes() for v in values]


@functools.lru_cache(maxsize=None)
def input_set(d, nu):
    """-> dict(v Mandel vectors (N_SET), y, base = (e, gamma, H) with L_SET features, a_dev = the DEVICE's log-diagonals, a = the same on the host)"""
    rng = np.random.default_rng([d, 0])
    mats = ref.random_spd(rng, N_SET, d, 0.3, 3.0)
    v = ref.to_mandel(mats)
    y = np.log(np.linalg.det(mats)) + 0.05 * rng.standard_normal(N_SET)
    base = ref.base_draw(d, L_SET, nu, 100 + d)
    a_dev = ops.spd_ai_logdiag(t(v), t(base[2]))
    return dict(v=v, y=y, base=base, a_dev=a_dev, a=a_dev.cpu().numpy())


@functools.lru_cache(maxsize=None)
def case(d, nu, n, L):
    """the first n points and L features of the input set -> dict(base, a_dev contiguous, a, y_dev, y)"""
    s = input_set(d, nu)
    e, gamma, h = s["base"]
    base = (np.ascontiguousarray(e[:L]), None if gamma is None else np.ascontiguousarray(gamma[:L]), np.ascontiguousarray(h[:L]))
    return dict(base=base, a_dev=s["a_dev"][:n, :L].contiguous(), a=np.ascontiguousarray(s["a"][:n, :L]), y_dev=t(s["y"][:n]), y=s["y"][:n],
                v=s["v"][:n])


@functools.lru_cache(maxsize=None)
def reference(d, nu, n, L, kappa):
    c = case(d, nu, n, L)
    return fit.likelihood(c["a"], c["y"], c["base"], kappa, nu, OUTPUTSCALE, NOISE, MEAN)


def chain(d, nu, n, L, kappa, outputscale=OUTPUTSCALE, noise=NOISE, mean=MEAN):
    c = case(d, nu, n, L)
    return ops.gp_mll_spd_ai_spectral(c["a_dev"], c["y_dev"], c["base"], kappa, nu, outputscale, noise, mean)


# ------------------------------------------------------------------------------------------------------------- 1. the points launch
@pytest.mark.parametrize("kappa", [0.3, 1.0, 3.0])
@pytest.mark.parametrize("nu", NUS)
@pytest.mark.parametrize("d", [2, 3, 10])
def test_points_against_the_reference(d, nu, kappa):
    for L in (1, 65, 130):
        base = case(d, nu, 1, L)["base"]
        lam, w, q, c = ops.spd_ai_spectral_points_dkappa(base, kappa, nu, device=DEV)
        assert lam.shape == (L, d) and w.shape == (L,) and q.shape == (L,) and c.shape == ()
        rl, rw, rq, rc, rq_scale = fit.points_and_derivative(base, kappa, nu)
        tiny = 1e-300                    # (a term of q underflows to 0 where sinh overflows: 0 error over 0 tolerance is a ratio of 0)
        ratios = dict(lam=(np.abs(lam.cpu().numpy() - rl) / (64 * U * np.abs(rl) + tiny)).max(),
                      w=(np.abs(w.cpu().numpy() - rw) / (64 * U * rw + tiny)).max(),
                      q=(np.abs(q.cpu().numpy() - rq) / (64 * U * (np.abs(rq) + rq_scale) + tiny)).max(),
                      c=abs(float(c) - rc) / (64 * U * abs(rc)))
        print(f"d={d} nu={nu} kappa={kappa} L={L}: error / tolerance " + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
        assert all(v <= 1.0 for v in ratios.values()), ratios
        # ... and the torch points of the kernel class, to the same rounding
        tl, tw = ops.spd_ai_spectral_points(base, torch.tensor(kappa, dtype=torch.float64, device=DEV), nu)
        assert bool(((tl - lam).abs() <= 64 * U * lam.abs()).all()) and bool(((tw - w).abs() <= 64 * U * w).all())


# ------------------------------------------------------------------------------------------------------------- 2. features and their derivative
@pytest.mark.parametrize("kappa", [0.3, 1.0, 3.0])
@pytest.mark.parametrize("nu", NUS)
@pytest.mark.parametrize("d", [2, 3, 10])
def test_feature_bits_and_the_derivative_against_the_reference(d, nu, kappa):
    for n, L in ((5, 1), (17, 64), (17, 65), (70, 130)):
        c = case(d, nu, n, L)
        lam, w, q, cc = ops.spd_ai_spectral_points_dkappa(c["base"], kappa, nu, device=DEV)
        fh, gd = ops.spd_ai_spectral_features_dkappa(c["a_dev"], lam, w, q, cc)
        assert fh.shape == (n, 2 * L) and gd.shape == (n, 2 * L)
        assert np.array_equal(bits(fh), bits(ops.spd_ai_spectral_features(t(c["v"]), t(c["base"][2]), lam, w)))
        # the reference on the device's own a, lam, w, q, c, in long double
        host = [x.cpu().numpy() for x in (lam, w, q)]
        want = fit.features_and_derivative(c["a"], *host, float(cc), LD)[1].astype(np.float64)
        ratio = float((np.abs(gd.cpu().numpy() - want) / fit.gdot_tolerance(c["a"], *host, float(cc))).max())
        print(f"d={d} nu={nu} kappa={kappa} n={n} L={L}: Gd worst error / tolerance {ratio:.4f}")
        assert ratio <= 1.0
        # the bits of row i do not depend on the other rows
        f1, g1 = ops.spd_ai_spectral_features_dkappa(c["a_dev"][:1].contiguous(), lam, w, q, float(cc))
        assert np.array_equal(bits(f1), bits(fh[:1])) and np.array_equal(bits(g1), bits(gd[:1]))


# ------------------------------------------------------------------------------------------------------------- 3. the Gram launch
def tol_k(d, lam, a, L):
    return 4.0 * (np.abs(lam).sum(-1).max() + np.abs(ref.rho(d)).sum()) * 64.0 * U * np.abs(a).max() + 64.0 * U + 2 * L * U


@pytest.mark.parametrize("nu", NUS)
@pytest.mark.parametrize("d", [2, 3, 10])
def test_gram_launch(d, nu):
    kappa = 1.0
    for n, L in ((1, 1), (5, 1), (17, 65), (70, 64), (200, 130)):
        c = case(d, nu, n, L)
        lam, w, q, cc = ops.spd_ai_spectral_points_dkappa(c["base"], kappa, nu, device=DEV)
        fh = ops.spd_ai_spectral_features_dkappa(c["a_dev"], lam, w, q, cc)[0]
        k = ops.spd_ai_feature_gram(fh)
        assert k.shape == (n, n) and np.array_equal(bits(k), bits(k.t())) and np.array_equal(bits(k.diagonal()), bits(torch.ones(n, dtype=torch.float64)))
        rl, rw, rq, rc, _ = fit.points_and_derivative(c["base"], kappa, nu, LD)
        want = fit.gram_and_derivative(*fit.features_and_derivative(c["a"], rl, rw, rq, rc, LD))[0].astype(np.float64)
        tol = tol_k(d, rl.astype(np.float64), c["a"], L)
        err = np.abs(k.cpu().numpy() - want).max()
        print(f"d={d} nu={nu} n={n} L={L}: K error {err:.3e} tol {tol:.3e} ratio {err / tol:.4f}")
        assert err <= tol
        # the bits of K_ij depend on rows i and j alone: the launch on the first m rows gives the leading block
        for m in (1, 5, 16, 17, 31):
            if m < n:
                assert np.array_equal(bits(ops.spd_ai_feature_gram(fh[:m].contiguous())), bits(k[:m, :m])), m


# ------------------------------------------------------------------------------------------------------------- 4. the chain
# (d, nu, n, L, kappa): every n at one setting - 30 | 31 the packed / tiled boundary of the likelihood launch, 39 | 40 its single-wave boundary,
# 160 | 161 GABO_GP_MLL_MAX_N, 200 the tiled likelihood; 17 and 161: the last 16-row tile holds one row - then the corners of (d, nu, kappa)
# and the feature counts 1, 64, 65 (2L = 2: fourteen padded columns; a whole wave of features; one more)
CHAIN_CASES = [(3, 2.5, n, 130, 1.0) for n in (1, 5, 17, 30, 31, 39, 40, 70, 160, 161, 200)] \
    + [(d, nu, 40, 65, kappa) for d in (2, 10) for nu in (0.5, math.inf) for kappa in (0.3, 3.0)] \
    + [(3, 2.5, n, L, 1.0) for n in (17, 161) for L in (1, 64)] + [(10, 2.5, 70, 130, 0.3), (2, 2.5, 200, 65, 3.0)]
# Cases that miss the bound with the constant 8 for d/d kappa, and the constant they get instead (none so far): the numpy fp64 route against
# the long-double reference, fit.numpy_route_d_kappa, never the device against itself.
D_KAPPA_CONSTANT = {}


@pytest.mark.parametrize("d,nu,n,L,kappa", CHAIN_CASES)
def test_chain_against_the_reference(d, nu, n, L, kappa):
    want = reference(d, nu, n, L, kappa)
    out = chain(d, nu, n, L, kappa)
    assert out[5] == 0.0 and want.cond < 1e4
    tol = (64.0 + 8.0 * want.cond) * U * want.scale
    tol[1] = (64.0 + D_KAPPA_CONSTANT.get((d, nu, n, L, kappa), 8.0) * want.cond) * U * want.scale[1]
    err = np.abs(np.array(out[:5]) - want.out)
    print(f"d={d} nu={nu} n={n} L={L} kappa={kappa}: cond {want.cond:.3e}; error / tolerance "
          + ", ".join(f"{name} {e / s if s > 0 else (0.0 if e == 0 else math.inf):.4f}" for name, e, s in zip(fit.NAMES, err, tol)))
    for name, e, s, w in zip(fit.NAMES, err, tol, want.out):
        assert e <= s, (name, e, s, w)


# ------------------------------------------------------------------------------------------------------------- 5. bits
@pytest.mark.parametrize("n", [30, 40, 160, 161])
def test_likelihood_bits_are_those_of_the_gram_launches(n):
    d, nu, L, kappa = 3, 2.5, 130, 1.0
    c = case(d, nu, n, L)
    out = chain(d, nu, n, L, kappa)
    lam, w, q, cc = ops.spd_ai_spectral_points_dkappa(c["base"], kappa, nu, device=DEV)
    fh, gd = ops.spd_ai_spectral_features_dkappa(c["a_dev"], lam, w, q, cc)
    k = ops.spd_ai_feature_gram(fh)
    gram, wm = ops.gp_mll_gram(k, c["y_dev"], OUTPUTSCALE, NOISE, MEAN)
    gram = gram.tolist()
    assert out[5] == 0.0 and gram[5] == 0.0
    assert fbits([out[0], out[2], out[3], out[4]]) == fbits([gram[0], gram[2], gram[3], gram[4]])
    # d/d kappa against outputscale sum_{i != j} W_ij (Gd_i . Fh_j) from that call's W, summed on the host in long double.  The chain rounds
    # every product of 2L terms - relative to the sum of the absolute values of ITS terms - then the product with W_ij and the additions of
    # its trees (8 levels in a tile, at most 8 + 6 over the tiles): (2L + 64) u of sum |W_ij| (|Gd_i| . |Fh_j|)
    gl, fl, wl = (x.cpu().numpy().astype(LD) for x in (gd, fh, wm))
    m, m_abs = (gl @ fl.T) * wl, (np.abs(gl) @ np.abs(fl).T) * np.abs(wl)
    np.fill_diagonal(m, 0)
    np.fill_diagonal(m_abs, 0)
    want, scale = float(OUTPUTSCALE * m.sum()), float(OUTPUTSCALE * m_abs.sum())
    print(f"n={n}: d/d kappa {out[1]:.15e} against the launch-by-launch route {want:.15e}, error / (64 + 2L) u scale "
          f"{abs(out[1] - want) / ((64 + 2 * L) * U * scale):.4f}")
    assert abs(out[1] - want) <= (64 + 2 * L) * U * scale
    assert fbits(chain(d, nu, n, L, kappa)) == fbits(out)                  # two calls, the same six numbers bit for bit


@pytest.mark.parametrize("n", [5, 161])
def test_heat_kernel_runs_without_gamma(n):
    c = case(3, math.inf, n, 65)
    assert c["base"][1] is None
    out = chain(3, math.inf, n, 65, 1.0)
    assert out[5] == 0.0 and all(math.isfinite(v) for v in out) and fbits(chain(3, math.inf, n, 65, 1.0)) == fbits(out)


# ------------------------------------------------------------------------------------------------------------- 6. not positive definite
@pytest.mark.parametrize("n", [3, 45, 170])
def test_a_matrix_that_is_not_positive_definite_is_reported(n):
    """n copies of one point: K = ones, and a negative "noise" makes Ky = ones - I / 2 indefinite (tests/test_gpu_gp_mll_series.py)"""
    c = case(3, 2.5, 1, 65)
    a = c["a_dev"].expand(n, -1, -1).contiguous()
    y = torch.ones(n, dtype=torch.float64, device=DEV)
    out = ops.gp_mll_spd_ai_spectral(a, y, c["base"], 1.0, 2.5, 1.0, -0.5, 0.0)
    assert out[5] == 1.0 and out[:5] == [0.0] * 5


# ------------------------------------------------------------------------------------------------------------- 7. a NaN row
def test_a_nan_row_behaves_as_the_likelihood_launch_on_the_nan_gram_matrix():
    d, nu, n, L, kappa = 3, 2.5, 5, 65, 1.0
    c = case(d, nu, n, L)
    a = c["a_dev"].clone()
    a[3, 7, 1] = math.nan
    prev = ops.set_error_checking(True)
    try:
        out = ops.gp_mll_spd_ai_spectral(a, c["y_dev"], c["base"], kappa, nu, OUTPUTSCALE, NOISE, MEAN)
        lam, w, q, cc = ops.spd_ai_spectral_points_dkappa(c["base"], kappa, nu, device=DEV)
        fh, gd = ops.spd_ai_spectral_features_dkappa(a, lam, w, q, cc)
        k = ops.spd_ai_feature_gram(fh)
        ops.check_deferred()                  # nothing is reported
    finally:
        ops.set_error_checking(prev)
    bad = np.zeros(n, dtype=bool)
    bad[3] = True
    assert np.array_equal(torch.isnan(k).cpu().numpy(), bad[:, None] | bad[None, :])
    assert bool(torch.isnan(fh[3]).all()) and bool(torch.isnan(gd[3]).all()) and not bool(torch.isnan(fh[~t(bad).bool()]).any())
    gram = ops.gp_mll_gram(k, c["y_dev"], OUTPUTSCALE, NOISE, MEAN)[0].tolist()
    assert fbits([out[0], out[2], out[3], out[4], out[5]]) == fbits([gram[0], gram[2], gram[3], gram[4], gram[5]])
    assert out[1] == 0.0 if out[5] != 0.0 else math.isnan(out[1])


# ------------------------------------------------------------------------------------------------------------- 8. the model layer
def _problem(d, n):
    rng = np.random.default_rng([9, d, n])
    mats = ref.random_spd(rng, n + 6, d, 0.5, 2.0)
    return ref.to_mandel(mats), np.log(np.linalg.det(mats)) + 0.05 * rng.standard_normal(n + 6)


def _models():
    out = []
    for d, n in ((2, 12), (3, 45)):
        v, y = _problem(d, n)

        def scaled(d=d, n=n, v=v, y=y):
            base = SpdAffineInvariantMaternKernel(d, nu=2.5, num_features=128, seed=1)
            return models.SingleTaskGP(t(v[:n]), t(y[:n]), ScaleKernel(base, outputscale_prior=models.GammaPrior(2.0, 0.15)),
                                       noise_prior=models.GammaPrior(1.1, 0.05))

        def bare(d=d, n=n, v=v, y=y):
            base = SpdAffineInvariantMaternKernel(d, nu=2.5, num_features=128, seed=1)
            return models.SingleTaskGP(t(v[:n]), t(y[:n]), base, initial_noise=1e-2)

        out += [(scaled, v[n:]), (bare, v[n:])]
    return out


def _base_of(gp):
    return getattr(gp.covar_module, "base_kernel", gp.covar_module)


def test_fast_value_and_gradients_match_autograd():
    """tolerances of tests/test_gpu_gp_fit.py: scalar objective rtol 1e-7; gradients rtol 2e-6, atol 1e-9.  The closure's value against
    marginal_log_likelihood() within (64 + 8 cond) u scale: the two Gram matrices differ only by the summation order of their products."""
    for make, _ in _models():
        gp = make()
        with torch.no_grad():
            for p in gp.parameters():
                p.add_(0.3)
        for p in gp.parameters():
            p.requires_grad_(True)
        want_value = gp.marginal_log_likelihood()
        want_value.backward()
        want = [p.grad.clone() for p in gp.parameters()]
        for p in gp.parameters():
            p.grad = None
        form = gp._spectral_form()
        assert form is not None and gp._stationary_form() is None and gp._series_form() is None and gp._matern_form() is None
        a, draw, ls_fn, nu, os_fn = form
        n = a.shape[0]
        with torch.no_grad():
            lik = fit.likelihood(a.cpu().numpy(), gp.train_y.cpu().numpy(), draw, float(ls_fn()), nu, float(os_fn()), float(gp.noise),
                                 float(gp.mean_constant))
            prior = float(gp._priors())
        fast = gp._fast_mll_closure()
        assert fast is not None
        value, proxy = fast()
        proxy.backward()
        tol = (64.0 + 8.0 * lik.cond) * U * (lik.scale[0] + abs(prior)) / n
        print(f"n={n}: closure {value:.15e} marginal_log_likelihood {float(want_value):.15e} cond {lik.cond:.3e} "
              f"error / tolerance {abs(value - float(want_value)) / tol:.4f}")
        assert abs(value - float(want_value)) <= tol
        for p, w in zip(gp.parameters(), want):
            np.testing.assert_allclose(p.grad.cpu().numpy(), w.cpu().numpy(), rtol=2e-6, atol=1e-9)
        params = list(gp.parameters())
        objective = gp._fast_scalar_objective(params)
        assert objective is not None
        loss, grad = objective(np.array([float(p) for p in params]))
        np.testing.assert_allclose(loss, -float(want_value), rtol=1e-7)
        np.testing.assert_allclose(grad, [-float(w) for w in want], rtol=2e-6, atol=1e-9)


# ------------------------------------------------------------------------------------------------------------- 9. the fit
def test_fast_fit_reaches_the_autograd_fit_with_one_logdiag_launch(monkeypatch):
    """fast=True and fast=False from the same start: the same likelihood and hyper-parameters (the numbers of the series test); the fast fit
    makes chain calls, no kernel forward and exactly one ops.spd_ai_logdiag call"""
    for make, x_test in _models():
        a, b = make(), make()
        calls = {"forward": 0, "chain": 0, "logdiag": 0}
        forward, entry, logdiag = SpdAffineInvariantMaternKernel.forward, ops.gp_mll_spd_ai_spectral, ops.spd_ai_logdiag

        def counted_forward(self, *args, **kwargs):
            calls["forward"] += 1
            return forward(self, *args, **kwargs)

        def counted_entry(*args, **kwargs):
            calls["chain"] += 1
            return entry(*args, **kwargs)

        def counted_logdiag(*args, **kwargs):
            calls["logdiag"] += 1
            return logdiag(*args, **kwargs)

        with monkeypatch.context() as m:
            m.setattr(SpdAffineInvariantMaternKernel, "forward", counted_forward)
            m.setattr(ops, "gp_mll_spd_ai_spectral", counted_entry)
            m.setattr(ops, "spd_ai_logdiag", counted_logdiag)
            models.fit_gpytorch_model(a, fast=True)
        assert calls["chain"] >= 1 and calls["forward"] == 0 and calls["logdiag"] == 1, calls
        models.fit_gpytorch_model(b, fast=False)
        for m_ in (a, b):
            for p in m_.parameters():
                p.requires_grad_(True)
        np.testing.assert_allclose(float(a.marginal_log_likelihood()), float(b.marginal_log_likelihood()), rtol=1e-6, atol=1e-8)
        hyper = lambda m_: [float(m_.noise), float(m_.mean_constant), float(_base_of(m_).lengthscale)] \
            + ([float(m_.covar_module.outputscale)] if _base_of(m_) is not m_.covar_module else [])      # noqa: E731
        np.testing.assert_allclose(hyper(a), hyper(b), rtol=2e-3, atol=1e-4)
        preds = a(t(x_test))
        assert bool(torch.isfinite(preds.mean).all()) and bool((preds.variance > 0).all())


def test_dimension_and_size_limits_raise():
    c = case(3, 2.5, 5, 65)
    with pytest.raises(RuntimeError, match="contiguous"):
        ops.gp_mll_spd_ai_spectral(c["a_dev"][:, :, :2], c["y_dev"], c["base"], 1.0, 2.5, 1.0, 0.1, 0.0)
    with pytest.raises(RuntimeError, match="base draw"):
        ops.gp_mll_spd_ai_spectral(c["a_dev"], c["y_dev"], case(3, 2.5, 5, 64)["base"], 1.0, 2.5, 1.0, 0.1, 0.0)
    assert _lib.load().gabo_gp_mll_spd_ai_spectral_workspace_bytes(5, 65, 3) > 0
