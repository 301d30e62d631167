"""CPU side of the one-call fit of the affine-invariant SPD Matern / heat kernels: the numpy reference tests/_cpu_spd_ai_spectral_fit.py against
central differences of itself and against torch autograd through ops.spd_ai_spectral_points, the host-side refusals of the new C entries, and
which model forms the kernel classes have.  No GPU."""
import math
import os

import numpy as np
import pytest
import torch

from gabotorch_amd import _lib, models, ops
from gabotorch_amd._compat import ScaleKernel
from gabotorch_amd.kernel_utils import kernels_spd, kernels_sphere
from tests import _cpu_spd_ai_spectral as ref
from tests import _cpu_spd_ai_spectral_fit as fit

U = ref.U
LD = np.longdouble
NUS = (0.5, 2.5, math.inf)


@pytest.fixture(scope="module", autouse=True)
def _built_library():
    """The .so is a build artefact (git-ignored): build it with hipcc when a fresh checkout has none."""
    if not os.path.exists(_lib.LIB_PATH):
        from gabotorch_amd import _build
        _build.build()


def _inputs(d, n=6, L=65, nu=2.5, seed=0):
    rng = np.random.default_rng([d, seed])
    base = ref.base_draw(d, L, nu, 7 + d)
    a = ref.logdiag(ref.random_spd(rng, n, d, 0.3, 3.0), base[2])
    return base, a


def _central(f, kappa, step, evaluation_error=0.0):
    """central difference of the array-valued f at kappa and the bound on its error, entry by entry: the third-derivative term h^2 f''' / 6,
    estimated from the doubled step (cd(2h) - cd(h) = h^2 f''' / 2 + O(h^4): a third of it, doubled), plus the rounding of the difference,
    (16 u max|f| + the error the evaluation of f itself carries) / h"""
    f1p, f1m, f2p, f2m = f(kappa + step), f(kappa - step), f(kappa + 2 * step), f(kappa - 2 * step)
    cd1, cd2 = (f1p - f1m) / (2 * step), (f2p - f2m) / (4 * step)
    rounding = 16.0 * U * np.maximum(np.maximum(np.abs(f1p), np.abs(f1m)), 1.0) + evaluation_error
    return cd1, 2.0 * np.abs(cd2 - cd1) / 3.0 + rounding / step


@pytest.mark.parametrize("kappa", [0.3, 1.0, 3.0])
@pytest.mark.parametrize("nu", NUS)
@pytest.mark.parametrize("d", [2, 3, 10])
def test_closed_form_derivatives_agree_with_central_differences(d, nu, kappa):
    """d lam / d kappa = c lam, d w / d kappa = 2 q w, Gd and dK against central differences of the reference's own lam, w, Fh, K.  The step
    balances the two terms of the bound: h^2 |f'''| / 6 = 16 u |f| / h at h = (96 u |f| / |f'''|)^(1/3), and a derivative in kappa brings a
    factor of the order of 1 / kappa, so h = kappa (96 u)^(1/3) = 2.2e-5 kappa.  The features carry the rounding of their phase and
    log-amplitude, two chains of d products: (d + 1) u sum_k (|lam_k a_k| + |rho_k a_k|), relative to a feature of at most 1; the largest of a row
    bounds the error of the normalised row (a factor 4 for the two row sums, as in tol_K of tests/test_gpu_spd_ai_spectral.py), and an entry
    of K carries those of its two rows."""
    base, a = _inputs(d, nu=nu)
    step = kappa * (96.0 * U) ** (1.0 / 3.0)
    lam, w, q, c, _ = fit.points_and_derivative(base, kappa, nu)
    fh, gd = fit.features_and_derivative(a, lam, w, q, c)
    _, dk = fit.gram_and_derivative(fh, gd)
    row_error = 4.0 * (d + 1) * U * (np.abs(a * lam).sum(-1) + np.abs(a * ref.rho(d)).sum(-1)).max(-1)          # (n,), lam at kappa: the
    row_error = row_error * (1.0 + 2.0 * step / kappa) ** 2                                # points at kappa +- 2h are larger by less than that
    evaluation_error = {"lam": 0.0, "w": 0.0, "Gd": row_error[:, None], "dK": row_error[:, None] + row_error[None, :]}

    def at(kap):
        lam_, w_, q_, c_, _ = fit.points_and_derivative(base, kap, nu)
        fh_, gd_ = fit.features_and_derivative(a, lam_, w_, q_, c_)
        return lam_, w_, fh_, fit.gram_and_derivative(fh_, gd_)[0]
    worst = {}
    for name, closed, pick in (("lam", c * lam, 0), ("w", 2.0 * q * w, 1), ("Gd", gd, 2), ("dK", dk, 3)):
        want, bound = _central(lambda kap: at(kap)[pick], kappa, step, evaluation_error[name])
        worst[name] = float((np.abs(closed - want) / bound).max())
    print(f"d={d} nu={nu} kappa={kappa}: worst error / bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert all(v <= 1.0 for v in worst.values()), worst


@pytest.mark.parametrize("nu", NUS)
@pytest.mark.parametrize("d", [2, 3, 10])
def test_points_and_derivative_agree_with_autograd_through_the_torch_points(d, nu):
    """lam, w to 64 u relative (the same formulas in the same format); their kappa-derivatives to 64 u of the sum of the absolute values of the
    derivative's terms as autograd forms them"""
    kappa = 0.8
    base, _ = _inputs(d, nu=nu)
    lam, w, q, c, q_scale = fit.points_and_derivative(base, kappa, nu)
    ls = torch.tensor(kappa, dtype=torch.float64, requires_grad=True)
    tl, tw = ops.spd_ai_spectral_points(base, ls, nu)
    assert np.abs(tl.detach().numpy() - lam).max() <= 64 * U * np.abs(lam).max()
    assert (np.abs(tw.detach().numpy() - w) <= 64 * U * w).all()
    dlam = torch.autograd.functional.jacobian(lambda k: ops.spd_ai_spectral_points(base, k, nu)[0], ls).numpy()
    dw = torch.autograd.functional.jacobian(lambda k: ops.spd_ai_spectral_points(base, k, nu)[1], ls).numpy()
    assert (np.abs(dlam - c * lam) <= 64 * U * np.abs(c * lam) + 1e-300).all()
    # autograd's term for the pair (i, j) is (the other factors, at most 1) (1 - tanh^2) pi sign (c lam_i - c lam_j): 1 - tanh^2 formed from
    # the rounded tanh carries an ABSOLUTE error of 2 u where the closed form has the small 2 / sinh(2x), and the last factor is the difference
    # of two rounded derivatives: the scale of a term is pi |c| (|lam_i| + |lam_j|)
    pair_scale = np.zeros(len(w))
    for i in range(d):
        for j in range(i + 1, d):
            pair_scale += math.pi * abs(c) * (np.abs(lam[:, i]) + np.abs(lam[:, j]))
    assert (2.0 * w * q_scale <= pair_scale).all()
    assert (np.abs(dw - 2.0 * q * w) <= 64 * U * pair_scale).all()


def test_weight_derivative_is_finite_where_two_spectral_points_coincide():
    e = np.array([[0.5, 0.5, -1.0], [1.0, 2.0, 3.0]])
    lam, w, q, c, _ = fit.points_and_derivative((e, None, None), 1.0, math.inf)
    assert w[0] == 0.0 and np.isfinite(q).all()
    x = math.pi * 1.5
    assert abs(q[0] - c * (0.5 + 2 * x / math.sinh(2 * x))) <= 8 * U * abs(q[0])


@pytest.mark.parametrize("kappa", [0.3, 1.0, 3.0])
@pytest.mark.parametrize("nu", NUS)
@pytest.mark.parametrize("d", [2, 3, 10])
def test_fp64_gdot_stays_within_an_eighth_of_the_device_tolerance_of_its_long_double_evaluation(d, nu, kappa):
    """the tolerance the device's Gd gets (fit.gdot_tolerance) is a bound on fp64 rounding: the numpy fp64 evaluation, on the same fp64
    inputs, stays within 1/8 of it of the long-double one (as tol_a = 8 err in tests/test_gpu_spd_ai_spectral.py)"""
    base, a = _inputs(d, n=17, L=130, nu=nu)
    lam, w, q, c, _ = fit.points_and_derivative(base, kappa, nu)
    g64 = fit.features_and_derivative(a, lam, w, q, c)[1]
    gld = fit.features_and_derivative(a, lam, w, q, c, LD)[1]
    assert gld.dtype == LD and g64.dtype == np.float64
    ratio = float((np.abs(g64 - gld.astype(np.float64)) / fit.gdot_tolerance(a, lam, w, q, c)).max())
    print(f"d={d} nu={nu} kappa={kappa}: fp64 against long double, worst error / tolerance {ratio:.4f}")
    assert ratio <= 0.125


def test_new_entries_refuse_bad_arguments_on_the_host():
    """every refusal comes back before any HIP call: this machine needs no GPU for it"""
    lib = _lib.load()
    inf = math.inf
    P = 1 << 20          # a non-null address the entries never dereference on a refusal

    def chain(n=12, L=8, d=3, a=P, y=P, e=P, gamma=P, nu=2.5, ls=1.0, out=P, ws=P, wsb=1 << 40, pin=P, pinned=7):
        return lib.gabo_gp_mll_spd_ai_spectral(a, y, e, gamma, n, L, d, nu, ls, 1.3, 0.05, 0.0, out, ws, wsb, pin, pinned, None)
    assert chain(a=None) == chain(y=None) == chain(e=None) == chain(out=None) == chain(ws=None) == chain(pin=None) == _lib.GABO_ERR_ARG
    assert chain(gamma=None) == _lib.GABO_ERR_ARG and chain(L=0) == _lib.GABO_ERR_ARG
    assert chain(n=0) == chain(n=2049) == chain(d=1) == chain(d=11) == _lib.GABO_ERR_DIM
    assert chain(ls=0.0) == chain(ls=inf) == chain(nu=0.0) == chain(nu=float("nan")) == _lib.GABO_ERR_ARG
    assert chain(wsb=8) == chain(pinned=6) == _lib.GABO_ERR_ARG
    wsb = lib.gabo_gp_mll_spd_ai_spectral_workspace_bytes
    assert wsb(0, 8, 3) == wsb(2049, 8, 3) == wsb(12, 8, 1) == wsb(12, 8, 11) == wsb(12, 0, 3) == 0
    # the padded features (16 rows x 16 columns, twice), K and W, lam, w, q
    assert wsb(12, 8, 3) >= (2 * 16 * 16 + 2 * 12 * 12 + 8 * 3 + 2 * 8) * 8
    assert wsb(2048, 8, 3) > wsb(161, 8, 3) > wsb(160, 8, 3) > wsb(12, 8, 3)
    assert wsb(161, 8, 3) - wsb(160, 8, 3) >= lib.gabo_gp_mll_large_workspace_bytes(161)       # the tiled likelihood's block
    pts = lib.gabo_spd_ai_spectral_points_dkappa
    assert pts(P, P, 8, 1, 1.0, 2.5, P, P, P, P, None) == pts(P, P, 8, 11, 1.0, 2.5, P, P, P, P, None) == _lib.GABO_ERR_DIM
    assert pts(None, P, 8, 3, 1.0, 2.5, P, P, P, P, None) == pts(P, None, 8, 3, 1.0, 2.5, P, P, P, P, None) == _lib.GABO_ERR_ARG
    assert pts(P, P, 0, 3, 1.0, 2.5, P, P, P, P, None) == pts(P, P, 8, 3, -1.0, 2.5, P, P, P, P, None) == _lib.GABO_ERR_ARG
    feat = lib.gabo_spd_ai_spectral_features_dkappa
    assert feat(P, P, P, P, P, P, P, 4, 8, 1, None) == feat(P, P, P, P, P, P, P, 4, 8, 11, None) == _lib.GABO_ERR_DIM
    assert feat(None, P, P, P, P, P, P, 4, 8, 3, None) == feat(P, P, P, P, None, P, P, 4, 8, 3, None) == _lib.GABO_ERR_ARG
    assert feat(P, P, P, P, P, P, P, 0, 8, 3, None) == feat(P, P, P, P, P, P, P, 4, 0, 3, None) == _lib.GABO_ERR_ARG
    gram, gram_wsb = lib.gabo_spd_ai_feature_gram, lib.gabo_spd_ai_feature_gram_workspace_bytes
    assert gram_wsb(17, 130) == 32 * 144 * 8 and gram_wsb(0, 4) == gram_wsb(2049, 4) == gram_wsb(4, 0) == 0
    assert gram(P, P, 0, 4, P, 1 << 40, None) == gram(P, P, 2049, 4, P, 1 << 40, None) == _lib.GABO_ERR_DIM
    assert gram(None, P, 4, 4, P, 1 << 40, None) == gram(P, P, 4, 0, P, 1 << 40, None) == gram(P, P, 4, 4, P, 8, None) == _lib.GABO_ERR_ARG


def _gp(base, d=3, n=6):
    rng = np.random.default_rng(1)
    x = torch.tensor(ref.to_mandel(ref.random_spd(rng, n, d, 0.5, 2.0)))
    return models.SingleTaskGP(x, torch.tensor(rng.standard_normal(n)), base)


def test_only_the_affine_invariant_matern_kernel_has_a_spectral_form():
    others = [kernels_spd.SpdAffineInvariantGaussianKernel(beta_min=0.5), kernels_spd.SpdAffineInvariantLaplaceKernel(beta_min=0.5),
              kernels_spd.SpdLogEuclideanGaussianKernel(), kernels_spd.SpdFrobeniusGaussianKernel(),
              kernels_spd.SpdLogEuclideanMaternKernel(nu=2.5), kernels_spd.SpdFrobeniusMaternKernel(nu=1.5),
              kernels_spd.NestedSpdAffineInvariantGaussianKernel(3, 2, beta_min=0.5), kernels_spd.NestedSpdLogEuclideanGaussianKernel(3, 2),
              kernels_spd.NestedSpdLogEuclideanMaternKernel(3, 2, nu=2.5),
              kernels_sphere.SphereGaussianKernel(beta_min=0.5), kernels_sphere.SphereLaplaceKernel(),
              kernels_sphere.SphereRiemannianMaternKernel(nu=2.5, num_levels=4)]
    for kern in others:
        assert _gp(kern)._spectral_form() is None, type(kern).__name__
        assert _gp(ScaleKernel(kern))._spectral_form() is None, type(kern).__name__


def test_the_affine_invariant_matern_kernel_has_none_of_the_other_forms_and_its_limits():
    for wrap in (lambda k: k, ScaleKernel):
        gp = _gp(wrap(kernels_spd.SpdAffineInvariantMaternKernel(3, nu=2.5, num_features=8)))
        assert gp._stationary_form() is None and gp._series_form() is None and gp._matern_form() is None
    # the limits of the spectral form are decided before any device work: dim > 10, a batched point set, a point set of another dimension
    gp = _gp(kernels_spd.SpdAffineInvariantMaternKernel(11, nu=2.5, num_features=4), d=11)
    assert gp._spectral_form() is None
    gp = _gp(kernels_spd.SpdAffineInvariantMaternKernel(3, nu=2.5, num_features=4))
    gp.train_x = gp.train_x.unsqueeze(0)
    assert gp._spectral_form() is None
    gp = _gp(kernels_spd.SpdAffineInvariantMaternKernel(4, nu=2.5, num_features=4), d=3)
    assert gp._spectral_form() is None
    gp = _gp(kernels_spd.SpdAffineInvariantMaternKernel(2, nu=2.5, num_features=4), d=2, n=_lib.GABO_GP_MLL_LARGE_MAX_N + 1)
    assert gp._spectral_form() is None
