"""The random phase features of the affine-invariant Matern / heat kernels on the MI355X (csrc/spd_ai_spectral.hip) against the numpy
reference tests/_cpu_spd_ai_spectral.py, from the two launches up to the class, the fit and the acquisition maximiser.

Tolerances, u = 2^-53:
  log-diagonals  per input set (one X set, one H set; the launch shapes are leading slices of it, since a(i, l) depends on X_i and H_l alone)
                 tol_a = max(8 max|a_numpy - a_mpmath|, 64 u max|a|): the reference against the 50-digit truth, never the device against
                 itself.  The mpmath factorisations are taken on 48 (point, feature) pairs of the set drawn at random (a 10 x 10 one costs
                 20 ms): a maximum over a subset, so never a wider bound than the whole set would give.
  features, Gram tol_K = 4 (max_l |lam_l|_1 + |rho|_1) tol_a + 64 u: phase and log-amplitude are linear in a, every value is at most 1.
  gradients      against central differences of the reference, within the difference's own truncation term (estimated from the doubled step)
                 plus its rounding term.
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
from gabotorch_amd.kernel_utils.kernels_spd import SpdAffineInvariantMaternKernel
from gabotorch_amd.manifold_optimization.batched_trust_regions import BatchedTrustRegions
from gabotorch_amd.manifold_optimization.manifold_optimize import joint_optimize_manifold
from gabotorch_amd.Riemannian_utils.spd_utils_torch import (symmetric_matrix_to_vector_mandel_torch, vector_to_symmetric_matrix_mandel_torch)
from tests import _cpu_spd_ai_spectral as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = ref.U
NUS = (0.5, 2.5, math.inf)
N_SET, L_SET, MP_PAIRS = 70, 130, 48


def t(x):
    return torch.tensor(np.ascontiguousarray(x), dtype=torch.float64, device=DEV)


def bits(x):
    return x.detach().contiguous().view(torch.int64).cpu().numpy()


@functools.lru_cache(maxsize=None)
def input_set(d, hard=False):
    """-> dict(v Mandel vectors, x matrices (to the bit what the launch factors), h, a numpy log-diagonals, tol_a).  hard: condition number 1e6"""
    rng = np.random.default_rng([d, int(hard)])
    n, L = (5, 65) if hard else (N_SET, L_SET)
    if hard:
        q = np.linalg.qr(rng.standard_normal((n, d, d)))[0]
        lam = np.stack([rng.permutation(np.logspace(-3.0, 3.0, d)) for _ in range(n)])
        mats = np.einsum("nab,nb,ncb->nac", q, lam, q)
        mats = 0.5 * (mats + mats.transpose(0, 2, 1))
    else:
        mats = ref.random_spd(rng, n, d, 0.3, 3.0)
    v = ref.to_mandel(mats)
    x = ref.from_mandel(v)
    h = ref.base_draw(d, L, 2.5, 100 + d)[2]
    a = ref.logdiag(x, h)
    pairs = [(int(i), int(l)) for i, l in zip(rng.integers(0, n, MP_PAIRS), rng.integers(0, L, MP_PAIRS))]
    truth = ref.logdiag_mp(x, h, pairs)
    err = max(np.abs(a[i, l] - truth[k]).max() for k, (i, l) in enumerate(pairs))
    tol_a = max(8.0 * err, 64.0 * U * np.abs(a).max())
    return dict(v=v, x=x, h=h, a=a, tol_a=tol_a, ref_err=err)


@functools.lru_cache(maxsize=None)
def device_logdiag(d, hard=False):
    s = input_set(d, hard)
    return ops.spd_ai_logdiag(t(s["v"]), t(s["h"]))


def spectral(d, L, nu, kappa, seed=3):
    """(lam, w) of the reference for a base draw of its own (the H of the input set is used with them)"""
    return ref.spectral_points(ref.base_draw(d, L, nu, seed), kappa, nu)


def tol_k(d, lam, tol_a):
    return 4.0 * (np.abs(lam).sum(-1).max() + np.abs(ref.rho(d)).sum()) * tol_a + 64.0 * U


# ------------------------------------------------------------------------------------------------------------- 1. log-diagonals
@pytest.mark.parametrize("L", [1, 64, 65, 130])
@pytest.mark.parametrize("n", [1, 5, 70])
@pytest.mark.parametrize("d", [2, 3, 5, 8, 10])
def test_logdiag_against_the_reference(d, n, L):
    s = input_set(d)
    got = ops.spd_ai_logdiag(t(s["v"][:n]), t(s["h"][:L]))
    assert got.shape == (n, L, d)
    err = np.abs(got.cpu().numpy() - s["a"][:n, :L]).max()
    print(f"d={d} n={n} L={L}: err {err:.3e} tol {s['tol_a']:.3e} (reference against mpmath {s['ref_err']:.3e}) ratio {err / s['tol_a']:.3f}")
    assert err <= s["tol_a"]
    # the bits of a(i, l) depend on X_i and H_l alone: the launch on the whole set gives the same ones
    assert np.array_equal(bits(got), bits(device_logdiag(d)[:n, :L]))


def test_logdiag_at_condition_number_1e6():
    s = input_set(10, hard=True)
    err = np.abs(device_logdiag(10, True).cpu().numpy() - s["a"]).max()
    print(f"d=10 cond 1e6: err {err:.3e} tol {s['tol_a']:.3e} (reference against mpmath {s['ref_err']:.3e}) ratio {err / s['tol_a']:.3f}")
    assert err <= s["tol_a"]


def test_dimension_limits():
    v = ref.to_mandel(ref.random_spd(np.random.default_rng(0), 3, 11))
    h = ref.base_draw(11, 4, 2.5, 0)[2]
    lib = _lib.load()
    assert lib.gabo_spd_ai_logdiag(None, None, None, 3, 4, 11, None) == _lib.GABO_ERR_DIM
    with pytest.raises(RuntimeError, match="unsupported dimension"):
        ops.spd_ai_logdiag(t(v), t(h))
    with pytest.raises(RuntimeError, match="unsupported dimension"):
        ops.spd_ai_spectral_features(t(v), t(h), t(np.ones((4, 11))), t(np.ones(4)))


# ------------------------------------------------------------------------------------------------------------- 2. features and Gram
@pytest.mark.parametrize("nu", NUS)
@pytest.mark.parametrize("d", [2, 3, 5, 10])
def test_features_and_gram_against_the_reference(d, nu):
    s = input_set(d)
    lam, w = spectral(d, L_SET, nu, 0.7)
    tol = tol_k(d, lam, s["tol_a"])
    x, h, tl, tw = t(s["v"]), t(s["h"]), t(lam), t(w)
    f = ops.spd_ai_spectral_features(x, h, tl, tw)
    assert f.shape == (N_SET, 2 * L_SET)
    worst = np.abs(f.cpu().numpy() - ref.features(s["a"], lam, w)).max() / tol
    split = 30
    x1, x2 = x[:split], x[split:]
    k_ref = ref.kernel_from_logdiag(s["a"][:split], s["a"][split:], lam, w)
    k = ops.spd_ai_matern_kernel(x1, x2, h, tl, tw)
    worst = max(worst, np.abs(k.cpu().numpy() - k_ref).max() / tol)
    # the route through stored log-diagonals
    a_dev = device_logdiag(d)
    k_ld = ops.spd_ai_matern_kernel(x1, x2, h, tl, tw, logdiag1=a_dev[:split], logdiag2=a_dev[split:])
    worst = max(worst, np.abs(k_ld.cpu().numpy() - k_ref).max() / tol, float((k_ld - k).abs().max()) / tol)
    assert np.abs(ops.spd_ai_spectral_features(x, h, tl, tw, logdiag=a_dev).cpu().numpy() - f.cpu().numpy()).max() <= tol
    # one point set
    for kw in ({}, {"logdiag1": a_dev}):
        ks = ops.spd_ai_matern_kernel(x, x, h, tl, tw, **kw)
        assert np.array_equal(bits(ks), bits(ks.t())) and float((ks.diagonal() - 1.0).abs().max()) <= 8 * U
        worst = max(worst, np.abs(ks.cpu().numpy() - ref.kernel_from_logdiag(s["a"], None, lam, w)).max() / tol)
    assert np.array_equal(bits(ops.spd_ai_matern_kernel(x, x, h, tl, tw, diag=True)), bits(torch.ones(N_SET, dtype=torch.float64)))
    print(f"d={d} nu={nu}: worst error / tol_K {worst:.3f} (tol_K {tol:.3e})")
    assert worst <= 1.0
    # the bits of row i do not change when other rows are added to the batch
    for n in (1, 5):
        assert np.array_equal(bits(ops.spd_ai_spectral_features(x[:n], h, tl, tw)), bits(f[:n]))


# ------------------------------------------------------------------------------------------------------------- 3. NaN and non-SPD rows
@pytest.mark.parametrize("d", [3, 10])
def test_a_nan_row_and_a_non_spd_row_stay_in_their_own_row_and_column(d):
    s = input_set(d)
    lam, w = spectral(d, L_SET, 2.5, 0.7)
    h, tl, tw = t(s["h"]), t(lam), t(w)
    v = s["v"][:12].copy()
    clean = v.copy()
    v[3, 1] = np.nan
    v[7] = -v[7]                              # negative definite
    bad = np.zeros(12, dtype=bool)
    bad[[3, 7]] = True
    prev = ops.set_error_checking(True)
    try:
        a = ops.spd_ai_logdiag(t(v), h)
        f = ops.spd_ai_spectral_features(t(v), h, tl, tw)
        k = ops.spd_ai_matern_kernel(t(v), t(v), h, tl, tw)
        ops.check_deferred()                  # nothing is reported, as for the launch behind SpdLogEuclideanMaternKernel
    finally:
        ops.set_error_checking(prev)
    assert bool(torch.isnan(a[bad]).all()) and bool(torch.isnan(f[bad]).all())
    # the other rows have the bits of the run without the two rows
    good = torch.tensor(~bad, device=DEV)
    assert np.array_equal(bits(a[good]), bits(ops.spd_ai_logdiag(t(v[~bad]), h)))
    assert np.array_equal(bits(f[good]), bits(ops.spd_ai_spectral_features(t(v[~bad]), h, tl, tw)))
    # ... and the Gram matrix is NaN in the two rows and columns only, every other entry with the bits of the run on valid rows in their place
    kn = torch.isnan(k).cpu().numpy()
    assert np.array_equal(kn, bad[:, None] | bad[None, :])
    k_clean = ops.spd_ai_matern_kernel(t(clean), t(clean), h, tl, tw)
    assert np.array_equal(bits(k[good][:, good]), bits(k_clean[good][:, good]))


# ------------------------------------------------------------------------------------------------------------- 4. the class
def make_kernel(d, nu, L, kappa, seed=0):
    k = SpdAffineInvariantMaternKernel(d, nu=nu, num_features=L, seed=seed).double()
    k.lengthscale = torch.tensor(kappa, dtype=torch.float64)
    return k.to(DEV)


@pytest.mark.parametrize("nu", NUS)
def test_class_forward_without_gradients_is_the_op(nu):
    d, L = 5, 130
    s = input_set(d)
    kern = make_kernel(d, nu, L, 0.8)
    x1, x2 = t(s["v"][:9]), t(s["v"][9:30])
    h = t(kern.spectral_base[2])
    with torch.no_grad():
        lam, w = ops.spd_ai_spectral_points(kern.spectral_base, kern.lengthscale.double().reshape(()), nu)
        assert np.array_equal(bits(kern.forward(x1, x2)), bits(ops.spd_ai_matern_kernel(x1, x2, h, lam, w)))
        assert np.array_equal(bits(kern.forward(x1, x1)), bits(ops.spd_ai_matern_kernel(x1, x1, h, lam, w)))
        ones = kern.forward(x1, x2, diagonal_distance=True)
    assert ones.shape == (21, 1) and bool((ones == 1).all())
    k = kern.forward(x1.detach(), x2.detach())          # the lengthscale requires grad: the log-diagonal route, the same values to rounding
    lam_np, w_np = ref.spectral_points(kern.spectral_base, 0.8, nu)
    assert k.requires_grad and float((k.detach() - ops.spd_ai_matern_kernel(x1, x2, h, lam, w)).abs().max()) <= tol_k(d, lam_np, s["tol_a"])


def _richardson(f, at, step):
    """central difference of f at `at`, and the bound on its error: the truncation term estimated from the doubled step (cd(h) - f' =
    (cd(2h) - cd(h)) / 3 + O(h^4); twice that), plus the rounding term 16 u |f| / h"""
    f1p, f1m, f2p, f2m = f(at + step), f(at - step), f(at + 2 * step), f(at - 2 * step)
    cd1, cd2 = (f1p - f1m) / (2 * step), (f2p - f2m) / (4 * step)
    return cd1, 2.0 * abs(cd2 - cd1) / 3.0 + 16.0 * U * max(abs(f1p), abs(f1m), 1.0) / step


@pytest.mark.parametrize("nu", NUS)
def test_class_gradient_in_the_lengthscale(nu):
    d, L, kappa = 3, 130, 0.9
    s = input_set(d)
    kern = make_kernel(d, nu, L, kappa)
    x1, x2 = t(s["v"][:8]), t(s["v"][8:20])
    c = np.random.default_rng(4).standard_normal((8, 12))
    loss = (t(c) * kern.forward(x1, x2)).sum()
    (g_raw,) = torch.autograd.grad(loss, kern.raw_lengthscale)
    got = float(g_raw) / float(torch.sigmoid(kern.raw_lengthscale.detach().double()))          # d kappa / d raw = sigmoid(raw) (softplus)
    mats1, mats2 = ref.from_mandel(s["v"][:8]), ref.from_mandel(s["v"][8:20])

    def f(kap):
        return float((c * ref.kernel(mats1, mats2, kern.spectral_base, kap, nu)).sum())
    want, bound = _richardson(f, kappa, 1e-5)
    print(f"nu={nu}: d/dkappa {got:.12e} central difference {want:.12e} bound {bound:.3e} ratio {abs(got - want) / bound:.3f}")
    assert abs(got - want) <= bound


@pytest.mark.parametrize("d", [2, 4])
def test_class_gradient_in_x(d):
    n, L, kappa, nu = 6, 64, 0.9, 2.5
    rng = np.random.default_rng([5, d])
    v1, v2 = ref.to_mandel(ref.random_spd(rng, n, d, 0.5, 2.0)), ref.to_mandel(ref.random_spd(rng, n, d, 0.5, 2.0))
    kern = make_kernel(d, nu, L, kappa)
    c = rng.standard_normal((n, n))
    x1 = t(v1).requires_grad_(True)
    k = kern.forward(x1, t(v2))
    (got,) = torch.autograd.grad((t(c) * k).sum(), x1)
    got = got.cpu().numpy()
    mats2 = ref.from_mandel(v2)
    # the torch composition's value: eigenvalues in [0.5, 2], so the floor of tol_a applies (64 u max|a|)
    lam_np, _ = ref.spectral_points(kern.spectral_base, kappa, nu)
    a_all = np.concatenate([ref.logdiag(ref.from_mandel(v1), kern.spectral_base[2]), ref.logdiag(mats2, kern.spectral_base[2])])
    assert np.abs(k.detach().cpu().numpy() - ref.kernel(ref.from_mandel(v1), mats2, kern.spectral_base, kappa, nu)).max() \
        <= tol_k(d, lam_np, 64.0 * U * np.abs(a_all).max())
    worst = 0.0
    for i in range(n):
        for e in range(v1.shape[1]):
            def f(val):
                vv = v1.copy()
                vv[i, e] = val
                return float((c * ref.kernel(ref.from_mandel(vv), mats2, kern.spectral_base, kappa, nu)).sum())
            want, bound = _richardson(f, v1[i, e], 1e-4)
            worst = max(worst, abs(got[i, e] - want) / bound)
    print(f"d={d}: x-gradient worst error / bound {worst:.3f}")
    assert worst <= 1.0


def test_the_logdiag_launch_runs_once_across_a_fit(monkeypatch):
    d, L = 3, 64
    s = input_set(d)
    kern = make_kernel(d, 2.5, L, 1.0)
    x = t(s["v"][:10])
    calls = []
    real = ops.spd_ai_logdiag
    monkeypatch.setattr(ops, "spd_ai_logdiag", lambda *a, **kw: (calls.append(1), real(*a, **kw))[1])
    values = []
    for kappa in np.linspace(0.3, 3.0, 10):
        kern.lengthscale = torch.tensor(float(kappa), dtype=torch.float64)
        k = kern.forward(x, x)
        k.sum().backward()
        values.append(float(k[0, 1]))
    assert len(calls) == 1 and len(set(values)) == 10 and kern.raw_lengthscale.grad is not None
    other = t(s["v"][10:20])
    kern.forward(other, other)          # another point set: a new launch
    assert len(calls) == 2


# ------------------------------------------------------------------------------------------------------------- 5. end to end
def _spd2_sample(man):
    lam = man.min_eig + (man.max_eig - man.min_eig) * np.random.rand(2)
    q = np.linalg.qr(np.random.randn(2, 2))[0]
    m = q @ np.diag(lam) @ q.T
    return 0.5 * (m + m.T)


def test_fit_predict_condition_and_maximise_an_acquisition():
    rng = np.random.default_rng(9)
    d, n = 2, 10
    mats = ref.random_spd(rng, n + 6, d, 0.5, 2.0)
    v = ref.to_mandel(mats)
    y = np.log(np.linalg.det(mats)) + 0.05 * rng.standard_normal(n + 6)
    base = SpdAffineInvariantMaternKernel(d, nu=2.5, num_features=128, seed=1)
    gp = models.SingleTaskGP(t(v[:n]), t(y[:n]), ScaleKernel(base, outputscale_prior=models.GammaPrior(2.0, 0.15)),
                             noise_prior=models.GammaPrior(1.1, 0.05))
    models.fit_gpytorch_model(gp)
    assert float(base.lengthscale) > 0 and math.isfinite(float(base.lengthscale))
    preds = gp(t(v[n:]))
    mean, var = preds.mean.cpu().numpy(), preds.variance.cpu().numpy()
    assert np.isfinite(mean).all() and (var > 0).all()
    more = gp.condition_on_observations(t(v[n:n + 1]), t(y[n:n + 1]))
    m2, v2 = more.posterior(t(v[n + 1:]))
    assert bool(torch.isfinite(m2).all()) and bool((v2 > 0).all()) and more.train_x.shape[0] == n + 1
    # the maximiser does not know the class: the generic autograd path
    acq = models.ExpectedImprovement(gp, best_f=float(y[:n].min()), maximize=False)
    assert FusedAcquisition.build(acq, symmetric_matrix_to_vector_mandel_torch, torch.device(DEV)) is None
    man = manifolds.PositiveDefinite(2)
    man.min_eig, man.max_eig = 0.5, 2.0
    raw = []

    def rand():
        p = _spd2_sample(man)
        raw.append(np.asarray(p))
        return p
    man.rand = rand
    np.random.seed(0)
    torch.manual_seed(0)
    best = joint_optimize_manifold(acq, man, BatchedTrustRegions(mingradnorm=1e-5, maxiter=5), q=1, num_restarts=3, raw_samples=12, bounds=None,
                                   options={"device": DEV}, pre_processing_manifold=vector_to_symmetric_matrix_mandel_torch,
                                   post_processing_manifold=symmetric_matrix_to_vector_mandel_torch, approx_hessian=True)
    assert best.shape == (1, 3) and bool(torch.isfinite(best).all())
    assert np.linalg.eigvalsh(ref.from_mandel(best.cpu().numpy())).min() > 0
    value = float(acq(best[:, None].to(DEV)))
    assert len(raw) >= 12
    raw_best = float(acq(t(ref.to_mandel(np.stack(raw)))[:, None]).max())
    print(f"acquisition at the candidate {value:.6e}, best raw sample {raw_best:.6e}")
    assert math.isfinite(value) and value >= raw_best


# ------------------------------------------------------------------------------------------------------------- 6. the example
def test_example_runs():
    import importlib.util
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "spd_ai_matern_kernel.py")
    spec = importlib.util.spec_from_file_location("spd_ai_matern_kernel_example", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    res = mod.run(nu=2.5, num_features=128, nb_samples_post=2, table_points=24, verbose=False, device=DEV)
    gp = res["regression"]
    assert np.isfinite(gp["mean"]).all() and (gp["variance"] > 0).all() and gp["samples"].shape[0] == 2
    assert math.isfinite(gp["rmse"]) and gp["lengthscale"] > 0
    table = res["table"]
    assert len(table["matern"]) >= 3 and len(table["gaussian"]) >= 3
    assert all(math.isfinite(lmin) and lmin >= -1e-10 for _, lmin in table["matern"])
    assert all(math.isfinite(lmin) for _, lmin in table["gaussian"])
