"""No GPU: the random phase features of the affine-invariant Matern / heat kernels as the numpy reference states them
(tests/_cpu_spd_ai_spectral.py) against the truth at d = 2, their invariance and positive definiteness, and the host-side pieces of the
library (the base draw, ops.spd_ai_spectral_points and its derivative, the argument checks of the two entries) against that reference."""
import math

import numpy as np
import pytest
import torch

from gabotorch_amd import _lib, ops
from gabotorch_amd.kernel_utils import kernels_spd
from tests import _cpu_spd_ai_spectral as ref

U = ref.U
L_MC = 16384
SEEDS = range(8)
# Monte-Carlo bound at L = 16384: 3 x the largest error of the reference's heat kernel against the closed form over seeds 0 .. 7, the two
# lengthscales and the three points of ref.HEAT_D2 - measured 0.01187 (mean 0.0028; the Matern cases reach 0.0113 at nu = 2.5, 0.0189 at 0.5)
MC_BOUND = 3 * 0.01187

IDENTITY = np.eye(2)[None]
YS = np.stack([ref.d2_point(*p) for p in ref.D2_POINTS])


def test_heat_table_closed_form_and_spectral_quadrature_agree():
    """the stored constants are McKean's closed form where scipy imports, and the quadrature of the spectral integral gives the same"""
    for (kappa, pt), want in ref.HEAT_D2.items():
        assert abs(ref.spectral_truth_d2(kappa, math.inf, *pt, s_max=40.0) - want) < 1e-10
        try:
            import scipy.integrate  # noqa: F401
        except ImportError:
            continue
        assert abs(ref.heat_truth_d2(kappa, *pt) - want) < 1e-10


def test_heat_kernel_d2_against_closed_form():
    assert MC_BOUND < 0.05
    worst = 0.0
    for seed in SEEDS:
        base = ref.base_draw(2, L_MC, math.inf, seed)
        for kappa in (0.7, 1.5):
            k = ref.kernel(IDENTITY, YS, base, kappa, math.inf)[0]
            for j, pt in enumerate(ref.D2_POINTS):
                try:
                    truth = ref.heat_truth_d2(kappa, *pt)
                except ImportError:
                    truth = ref.HEAT_D2[(kappa, pt)]
                worst = max(worst, abs(k[j] - truth))
    print(f"heat d=2 L={L_MC}: largest error {worst:.5f} (bound {MC_BOUND:.5f})")
    assert worst <= MC_BOUND


def test_matern_truth_is_stable_under_grid_refinement():
    """one of the stored Matern values recomputed on a coarser and narrower grid: stable far below the 1e-4 the Monte-Carlo test needs"""
    for nu in (2.5, 0.5):
        pt = ref.D2_POINTS[1]
        coarse = ref.spectral_truth_d2(1.0, nu, *pt, s_max=100.0, ds=0.02, angles=360)
        assert abs(coarse - ref.MATERN_D2[(nu, pt)]) < 1e-6


@pytest.mark.parametrize("nu", [2.5, 0.5])
def test_matern_kernel_d2_against_spectral_quadrature(nu):
    worst = 0.0
    for seed in SEEDS:
        k = ref.kernel(IDENTITY, YS, ref.base_draw(2, L_MC, nu, seed), 1.0, nu)[0]
        worst = max(worst, max(abs(k[j] - ref.MATERN_D2[(nu, pt)]) for j, pt in enumerate(ref.D2_POINTS)))
    print(f"Matern nu={nu} d=2 L={L_MC}: largest error {worst:.5f} (bound {MC_BOUND:.5f})")
    assert worst <= MC_BOUND


def test_invariance_d3():
    """k(A X A^T, A Y A^T) = k(X, Y): two estimates from one draw, each within the Monte-Carlo bound of the common truth"""
    rng = np.random.default_rng(3)
    x = ref.random_spd(rng, 2, 3)
    a = rng.standard_normal((3, 3)) + 2.0 * np.eye(3)
    xa = a @ x @ a.T
    worst = 0.0
    for seed in SEEDS:
        for nu in (math.inf, 2.5):
            base = ref.base_draw(3, L_MC, nu, seed)
            worst = max(worst, abs(ref.kernel(x[:1], x[1:], base, 1.0, nu)[0, 0] - ref.kernel(xa[:1], xa[1:], base, 1.0, nu)[0, 0]))
    print(f"invariance d=3 L={L_MC}: largest difference {worst:.5f} (bound {MC_BOUND:.5f})")
    assert worst <= MC_BOUND


@pytest.mark.parametrize("nu", [0.5, 2.5, math.inf])
def test_positive_definite_for_every_lengthscale(nu):
    n = 60
    x = ref.random_spd(np.random.default_rng(7), n, 3)
    base = ref.base_draw(3, 256, nu, 0)
    for kappa in (0.05, 0.3, 5.0):
        k = ref.kernel(x, None, base, kappa, nu)
        assert np.array_equal(k, k.T)
        assert np.abs(np.diagonal(k) - 1.0).max() <= 8 * U
        assert np.linalg.eigvalsh(k).min() >= -64 * n * U


@pytest.mark.parametrize("nu", [0.5, 2.5, math.inf])
def test_base_draw_and_spectral_points_match_the_reference(nu):
    d, L = 4, 96
    base, want = ops.spd_ai_spectral_base(d, L, nu, 11), ref.base_draw(d, L, nu, 11)
    for got, exp in zip(base, want):
        assert (got is None and exp is None) or np.array_equal(got, exp)
    h = base[2]
    assert np.abs(h.transpose(0, 2, 1) @ h - np.eye(d)).max() < 64 * U
    for kappa in (0.05, 0.7, 5.0):
        ls = torch.tensor(kappa, dtype=torch.float64, requires_grad=True)
        lam, w = ops.spd_ai_spectral_points(base, ls, nu)
        lam_ref, w_ref = ref.spectral_points(want, kappa, nu)
        assert np.abs(lam.detach().numpy() - lam_ref).max() <= 8 * U * np.abs(lam_ref).max()
        assert np.abs(w.detach().numpy() - w_ref).max() <= 8 * d * d * U and w_ref.min() >= 0.0 and w_ref.max() <= 1.0
        # d/dkappa of sum(c_lam * lam) + sum(c_w * w) against the central difference of the reference; the bound is the difference's own
        # truncation term, estimated from the step 2h (err(h) = (cd(2h) - cd(h)) / 3 + O(h^4)), plus its rounding term 8 U |f| / h
        rng = np.random.default_rng(5)
        c_lam, c_w = rng.standard_normal(lam_ref.shape), rng.standard_normal(w_ref.shape)

        def f(kap):
            a, b = ref.spectral_points(want, kap, nu)
            return (c_lam * a).sum() + (c_w * b).sum()
        (grad,) = torch.autograd.grad((torch.tensor(c_lam) * lam).sum() + (torch.tensor(c_w) * w).sum(), ls)
        h_step = 1e-3 * kappa
        cd1, cd2 = (f(kappa + h_step) - f(kappa - h_step)) / (2 * h_step), (f(kappa + 2 * h_step) - f(kappa - 2 * h_step)) / (4 * h_step)
        scale = np.abs(c_lam * lam_ref).sum() + np.abs(c_w * w_ref).sum()
        bound = 2.0 * abs(cd2 - cd1) / 3.0 + 8 * U * scale / h_step
        assert abs(float(grad) - cd1) <= bound, (float(grad), cd1, bound)


def test_arguments_are_checked_on_the_host():
    lib = _lib.load()
    for d in (1, 11, 32):
        assert lib.gabo_spd_ai_logdiag(None, None, None, 4, 4, d, None) == _lib.GABO_ERR_DIM
        assert lib.gabo_spd_ai_spectral_features(None, None, None, None, None, 4, 4, d, None) == _lib.GABO_ERR_DIM
    assert lib.gabo_spd_ai_logdiag(None, None, None, -1, 4, 3, None) == _lib.GABO_ERR_ARG
    assert lib.gabo_spd_ai_logdiag(None, None, None, 4, 4, 3, None) == _lib.GABO_ERR_ARG
    assert lib.gabo_spd_ai_logdiag(None, None, None, 0, 4, 3, None) == _lib.GABO_OK
    assert lib.gabo_spd_ai_spectral_features(None, None, None, None, None, 4, -1, 3, None) == _lib.GABO_ERR_ARG
    assert lib.gabo_spd_ai_spectral_features(None, None, None, None, None, 4, 4, 3, None) == _lib.GABO_ERR_ARG
    assert lib.gabo_spd_ai_spectral_features(None, None, None, None, None, 4, 0, 3, None) == _lib.GABO_OK
    for bad in (0.0, -1.0, float("nan"), "2.5", True, None):
        with pytest.raises(ValueError):
            ops.spd_ai_spectral_base(3, 8, bad, 0)
        with pytest.raises(ValueError):
            kernels_spd.SpdAffineInvariantMaternKernel(3, nu=bad)
    with pytest.raises(ValueError):
        ops.spd_ai_spectral_base(1, 8, 2.5, 0)
    with pytest.raises(ValueError):
        ops.spd_ai_spectral_base(3, 0, 2.5, 0)


def test_class_surface():
    k = kernels_spd.SpdAffineInvariantMaternKernel(3, nu=math.inf, num_features=16, seed=4)
    assert k.nu == math.inf and k.dim == 3 and k.num_features == 16 and not hasattr(k, "beta_min")
    assert [n for n, _ in k.named_parameters()] == ["raw_lengthscale"]
    assert kernels_spd.SpdAffineInvariantMaternKernel(3).nu == 2.5
    ones = k.forward(torch.zeros(5, 6), torch.zeros(4, 6), diagonal_distance=True)
    assert ones.shape == (4, 1) and bool((ones == 1).all())
    # the x-gradient route is a plain torch composition: it needs no launch, and matches the reference
    rng = np.random.default_rng(0)
    v = ref.to_mandel(ref.random_spd(rng, 4, 3))
    a = ops._spectral_logdiag_torch(torch.tensor(v), torch.tensor(k.spectral_base[2]))
    want = ref.logdiag(ref.from_mandel(v), k.spectral_base[2])
    assert np.abs(a.numpy() - want).max() <= 64 * U * np.abs(want).max()
