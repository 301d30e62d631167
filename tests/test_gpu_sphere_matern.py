"""Riemannian Matern / heat kernels on the sphere on the MI355X: the zonal-series launches (csrc/sphere_zonal.hip) against 50-digit values
(tests/golden/make_golden_sphere_matern.py), their bit-level contracts, autograd, positive definiteness, and the layers above the kernel.

Tolerances.  tests/_cpu_sphere_zonal.py restates the device arithmetic in numpy; its own maximum error against the golden values measures
what the fp64 recurrence can deliver for a case.  A launch gets 8 x that (an equally valid operation order: fma against multiply and add),
floored at 4 * 2^-53 max|f|.  Where the inner product is formed on the device too, its rounding (dim * 2^-53 in c for unit vectors, twice
that allowed) is carried through max|f'|, taken from the golden values."""
import math

import numpy as np
import pytest
import torch

from gabotorch_amd import manifolds, models, ops
from gabotorch_amd._compat import ScaleKernel
from gabotorch_amd.fused_acquisition import FusedAcquisition
from gabotorch_amd.kernel_utils.kernels_sphere import SphereGaussianKernel, SphereRiemannianMaternKernel
from gabotorch_amd.manifold_optimization.batched_trust_regions import BatchedTrustRegions
from gabotorch_amd.manifold_optimization.manifold_optimize import joint_optimize_manifold
from tests._cpu_sphere_zonal import matern_gram, zonal_series

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -53
KEYS = ("0", "1", "2", "k")          # f, f', f'', df/dkappa


def t(x):
    return torch.tensor(np.ascontiguousarray(x), dtype=torch.float64, device=DEV)


@pytest.fixture(scope="module")
def gold(golden):
    g = golden("sphere_matern.npz")
    return {k: g[k] for k in g.files}


def _series(gold, i, key):
    dim = int(gold["cases"][i, 0])
    o = KEYS.index(key)
    return gold["coef" + key][gold["off" + key][i]:gold["off" + key][i + 1]], dim - 1 + (2 * o if o < 3 else 0)


def _tolerance(gold, i, key):
    coeff, sd = _series(gold, i, key)
    want = gold["vals"][i, KEYS.index(key)]
    own = np.abs(zonal_series(gold["c"], coeff, sd) - want).max()
    return max(8.0 * own, 4.0 * U * np.abs(want).max())


def _case_index(gold, dim, kappa, nu, L):
    hit = np.nonzero(np.all(gold["cases"] == np.array([dim, kappa, nu, L]), axis=1))[0]
    assert len(hit) == 1
    return int(hit[0])


def test_from_inner_against_the_golden_values(gold):
    """every golden case, orders 0 - 2 and d/dkappa, on the grid of c that includes -1, 1, 1 - 1e-15 and 1 + 2^-52"""
    c = t(gold["c"])
    worst = 0.0
    for i in range(len(gold["cases"])):
        for key in KEYS:
            coeff, sd = _series(gold, i, key)
            got = ops.sphere_zonal_from_inner(c, coeff, sd).cpu().numpy()
            err, tol = np.abs(got - gold["vals"][i, KEYS.index(key)]).max(), _tolerance(gold, i, key)
            worst = max(worst, err / tol if tol > 0 else 0.0)          # (L = 1: f'' = 0 exactly, on both sides)
            assert err <= tol, (gold["cases"][i], key, err, tol)
    print(f"from_inner: worst error / tolerance {worst:.3f} over {len(gold['cases'])} cases")


def test_from_inner_shapes_and_grid_stride():
    """any shape; more elements than one pass of the grid covers (4 x 16384 x 256), odd size"""
    coeff, sd = ops.sphere_matern_coefficients(3, 0.4, 2.5, 9)
    rng = np.random.default_rng(5)
    small = rng.uniform(-1, 1, (3, 5, 7))
    np.testing.assert_array_equal(ops.sphere_zonal_from_inner(t(small), coeff, sd).cpu().numpy().shape, small.shape)
    n = 4 * 16384 * 256 + 1027
    c = torch.linspace(-1.0, 1.0, 4099, dtype=torch.float64, device=DEV).repeat(n // 4099 + 1)[:n].contiguous()
    out = ops.sphere_zonal_from_inner(c, coeff, sd)
    ref = ops.sphere_zonal_from_inner(c[:4099].contiguous(), coeff, sd)
    assert torch.equal(out, ref.repeat(n // 4099 + 1)[:n])


@pytest.fixture(scope="module")
def grams(gold):
    """per dim: the point sets on the device, the golden Gram, its series and tolerance, and the (65, 130) launch every test shares"""
    out = {}
    for dim in (2, 3, 10, 17):
        i = _case_index(gold, *gold[f"gram_case_{dim}"])
        coeff, sd = _series(gold, i, "0")
        fp_max = np.abs(gold["vals"][i, 1]).max()
        tol = _tolerance(gold, i, "0") + fp_max * dim * 2.0 ** -52
        x1, x2 = t(gold[f"x1_{dim}"]), t(gold[f"x2_{dim}"])
        out[dim] = dict(i=i, coeff=coeff, sd=sd, tol=tol, x1=x1, x2=x2, want=gold[f"gram_{dim}"],
                        full=ops.sphere_zonal_pairwise(x1, x2, coeff, sd))
    return out


@pytest.mark.parametrize("dim", [2, 3, 10, 17])
def test_pairwise_against_the_golden_gram(grams, dim):
    """tile edges ((1, 1), (7, 33), (65, 130)), dim not a multiple of the MFMA k-step, d = 1, batches with unequal batch strides, diag"""
    g = grams[dim]
    x1, x2, want, tol = g["x1"], g["x2"], g["want"], g["tol"]
    assert np.abs(want).max() <= 1.0 + 1e-12 and want[3, 5] == pytest.approx(1.0, abs=1e-12)      # x2[5] is x1[3]: an inner product at 1
    for n1, n2 in ((1, 1), (7, 33), (65, 130)):
        got = g["full"] if (n1, n2) == (65, 130) else ops.sphere_zonal_pairwise(x1[:n1].contiguous(), x2[:n2].contiguous(), g["coeff"], g["sd"])
        assert got.shape == (n1, n2)
        err = np.abs(got.cpu().numpy() - want[:n1, :n2]).max()
        print(f"dim {dim} ({n1}, {n2}): error {err:.3e}, tolerance {tol:.3e}")
        assert err <= tol
    # batch (3,): x1 shared by the batch (batch stride 0), x2 one set per element
    a = x1[:20].expand(3, 20, dim)
    b = torch.stack([x2[0:40], x2[40:80], x2[80:120]])
    got = ops.sphere_zonal_pairwise(a, b, g["coeff"], g["sd"])
    assert got.shape == (3, 20, 40)
    for k in range(3):
        assert np.abs(got[k].cpu().numpy() - want[:20, 40 * k:40 * k + 40]).max() <= tol
    # ... and the other way round, the per-element sets a strided view
    a = torch.stack([x1[0:20], x1[20:40], x1[40:60]])
    big = torch.zeros(3, 33, 2 * dim, dtype=torch.float64, device=DEV)
    big[..., :dim] = x2[:33]
    got = ops.sphere_zonal_pairwise(a, big[..., :dim], g["coeff"], g["sd"])
    for k in range(3):
        assert np.abs(got[k].cpu().numpy() - want[20 * k:20 * k + 20, :33]).max() <= tol
    # diag: row k with row k
    got = ops.sphere_zonal_pairwise(x1, x2[:65].contiguous(), g["coeff"], g["sd"], diag=True)
    assert got.shape == (65, 1)
    assert np.abs(got[:, 0].cpu().numpy() - np.diagonal(want[:, :65])).max() <= tol
    got = ops.sphere_zonal_pairwise(a, torch.stack([x2[0:20], x2[20:40], x2[40:60]]), g["coeff"], g["sd"], diag=True)
    for k in range(3):
        assert np.abs(got[k, :, 0].cpu().numpy() - np.diagonal(want[20 * k:20 * k + 20, 20 * k:20 * k + 20])).max() <= tol


@pytest.mark.parametrize("dim", [2, 3, 10, 17])
def test_pairwise_bits_depend_on_the_two_rows_only(grams, dim):
    g = grams[dim]
    x1, x2 = g["x1"], g["x2"]
    block = ops.sphere_zonal_pairwise(x1[3:41].contiguous(), x2[5:71].contiguous(), g["coeff"], g["sd"])
    assert torch.equal(block, g["full"][3:41, 5:71])
    a = torch.stack([x1[0:20], x1[20:40], x1[40:60]])
    b = torch.stack([x2[0:40], x2[40:80], x2[80:120]])
    batched = ops.sphere_zonal_pairwise(a, b, g["coeff"], g["sd"])
    alone = ops.sphere_zonal_pairwise(a[1].contiguous(), b[1].contiguous(), g["coeff"], g["sd"])
    assert torch.equal(alone, batched[1]) and torch.equal(alone, g["full"][20:40, 40:80])


@pytest.mark.parametrize("dim", [2, 3, 10, 17])
def test_symmetric_launch(grams, dim):
    """x1 is x2: exactly symmetric; the blocks that pair the two golden sets against the golden Gram; and - the bits depending on the two rows
    only - equal to the plain launch throughout.  70 and 195 points: one and several column groups, neither a multiple of the tile."""
    g = grams[dim]
    for n1, n2 in ((30, 40), (65, 130)):
        z = torch.cat([g["x1"][:n1], g["x2"][:n2]]).contiguous()
        k = ops.sphere_zonal_pairwise(z, z, g["coeff"], g["sd"], symmetric=True)
        assert torch.equal(k, k.t())
        assert np.abs(k[:n1, n1:].cpu().numpy() - g["want"][:n1, :n2]).max() <= g["tol"]
        assert torch.equal(k, ops.sphere_zonal_pairwise(z, z, g["coeff"], g["sd"]))
    zb = torch.stack([torch.cat([g["x1"][:30], g["x2"][:40]]), torch.cat([g["x1"][30:60], g["x2"][40:80]])])
    kb = ops.sphere_zonal_pairwise(zb, zb, g["coeff"], g["sd"], symmetric=True)
    assert torch.equal(kb, kb.transpose(-1, -2))
    assert np.abs(kb[1, :30, 30:].cpu().numpy() - g["want"][30:60, 40:80]).max() <= g["tol"]


def test_kernel_entry_takes_the_fused_and_the_symmetric_launch(grams, gold):
    dim = 3
    g = grams[dim]
    _, kappa, nu, L = gold[f"gram_case_{dim}"]
    k = SphereRiemannianMaternKernel(nu=nu, num_levels=int(L)).double()
    k.lengthscale = torch.tensor(kappa, dtype=torch.float64)
    for p in k.parameters():
        p.requires_grad_(False)
    x1, x2 = g["x1"], g["x2"]
    host, sd = ops.sphere_matern_coefficients(dim, float(k.lengthscale), nu, int(L))
    assert torch.equal(k.forward(x1, x2), ops.sphere_zonal_pairwise(x1, x2, host, sd))
    assert np.abs(k.forward(x1, x2).cpu().numpy() - g["want"]).max() <= g["tol"] + 16 * U      # (the host's coefficients: a few ulp off the golden ones)
    ks = k.forward(x1, x1)
    assert torch.equal(ks, ks.t()) and torch.equal(ks, ops.sphere_zonal_pairwise(x1, x1, host, sd, symmetric=True))
    assert k.forward(x1, x2[:65].contiguous(), diag=True).shape == (65, 1)
    cpu_out = k.forward(x1.cpu(), x2.cpu())            # CPU tensors in, CPU tensors out
    assert cpu_out.device.type == "cpu" and torch.equal(cpu_out, k.forward(x1, x2).cpu())


@pytest.mark.parametrize("dim", [2, 3, 10, 17])
def test_autograd_against_the_golden_derivatives(grams, gold, dim):
    """gradients in x1, x2 and the lengthscale assembled from the golden f' and df/dkappa on the (7, 33) block; a double-backward
    Hessian-vector product in x1 from the golden f''; a third order raises.  Tolerances: the series' tolerance of that order, the rounding of
    c through the next derivative (max at c = 1: the sum of the next order's coefficients), and the rounding of the matrix products that
    assemble the gradient ((n + 2) 2^-53 of the sum of magnitudes), all times the row sum of the weights (|x| <= 1)."""
    g = grams[dim]
    i = g["i"]
    _, kappa, nu, L = gold[f"gram_case_{dim}"]
    x1n, x2n = gold[f"x1_{dim}"][:7], gold[f"x2_{dim}"][:33]
    f1, f2, fk = gold[f"gram1_{dim}"], gold[f"gram2_{dim}"], gold[f"gramk_{dim}"]
    rng = np.random.default_rng(77)
    w, v = rng.standard_normal((7, 33)), rng.standard_normal((7, dim))
    c2, sd2 = _series(gold, i, "2")
    kk = np.arange(1, len(c2), dtype=np.float64)
    f3_max = float(np.sum(c2[1:] * kk * (kk + sd2 - 1) / sd2))
    f2_max, f1_max = np.abs(gold["vals"][i, 2]).max(), np.abs(gold["vals"][i, 1]).max()
    tol1 = _tolerance(gold, i, "1") + f2_max * dim * 2.0 ** -52 + 35 * U * f1_max
    tol2 = _tolerance(gold, i, "2") + f3_max * dim * 2.0 ** -52 + 35 * U * f2_max
    ck, sdk = _series(gold, i, "k")
    kk = np.arange(1, len(ck), dtype=np.float64)
    fk_max = np.abs(gold["vals"][i, 3]).max()
    dfk_dc = float(np.sum(np.abs(ck[1:]) * kk * (kk + sdk - 1) / sdk))          # |d/dc df/dkappa| <= its series with |coefficients| at c = 1
    tolk = _tolerance(gold, i, "k") + dfk_dc * dim * 2.0 ** -52 + (w.size + 2) * U * fk_max
    x1, x2 = t(x1n).requires_grad_(True), t(x2n).requires_grad_(True)
    ls = torch.tensor(kappa, dtype=torch.float64, requires_grad=True)
    k = ops.sphere_matern_kernel(x1, x2, ls, nu, int(L))
    assert np.abs(k.detach().cpu().numpy() - g["want"][:7, :33]).max() <= g["tol"] + 16 * U
    loss = (k * t(w)).sum()
    g1, g2, gl = torch.autograd.grad(loss, (x1, x2, ls), create_graph=True)
    row, col = np.abs(w).sum(1).max(), np.abs(w).sum(0).max()
    assert np.abs(g1.detach().cpu().numpy() - (w * f1) @ x2n).max() <= tol1 * row
    assert np.abs(g2.detach().cpu().numpy() - (w * f1).T @ x1n).max() <= tol1 * col
    assert gl.shape == ls.shape and abs(float(gl) - float((w * fk).sum())) <= tolk * np.abs(w).sum()
    (hv,) = torch.autograd.grad((g1 * t(v)).sum(), x1, create_graph=True)
    want_hv = (w * f2 * (v @ x2n.T)) @ x2n
    assert np.abs(hv.detach().cpu().numpy() - want_hv).max() <= tol2 * row * np.abs(v).sum(1).max()
    with pytest.raises(RuntimeError, match="differentiable twice"):
        torch.autograd.grad(hv.sum(), x1)


def _sphere_points(seed, n, dim):
    x = np.random.default_rng(seed).standard_normal((n, dim))
    return x / np.linalg.norm(x, axis=1, keepdims=True)


@pytest.mark.parametrize("dim", [3, 10])
def test_positive_definite_for_every_lengthscale(dim):
    """lambda_min >= -64 N 2^-53, the rounding of a matrix of norm <= N - where the geodesic Gaussian kernel on the same S^2 points is
    indefinite by 4.3e-3 at beta = 0.5"""
    n = 96
    x = t(_sphere_points(1234, n, dim))
    worst = 0.0
    for kappa in (0.05, 0.3, 1.0, 3.0):
        for nu in (0.5, 2.5, math.inf):
            coeff, sd = ops.sphere_matern_coefficients(dim, kappa, nu, 32)
            k = ops.sphere_zonal_pairwise(x, x, coeff, sd, symmetric=True).cpu().numpy()
            lam = np.linalg.eigvalsh(k).min()
            worst = min(worst, lam)
            assert lam >= -64 * n * U, (kappa, nu, lam)
            # k(x, x) = f(<x, x>) = 1 up to the rounding of <x, x> (dim 2^-52 allowed) through f'(1) = the sum of the order-1 coefficients
            slope = float(ops.sphere_matern_coefficients(dim, kappa, nu, 32, 1)[0].sum())
            np.testing.assert_allclose(np.diagonal(k), 1.0, rtol=0, atol=64 * U + slope * dim * 2.0 ** -52)
    print(f"dim {dim}: smallest eigenvalue over the grid {worst:.3e} (bound {-64 * n * U:.3e})")
    if dim == 3:
        kg = SphereGaussianKernel(beta_min=0.1)
        kg.beta = torch.tensor(0.5)
        with torch.no_grad():
            lam = np.linalg.eigvalsh(kg.forward(x, x).double().cpu().numpy()).min()
        print(f"SphereGaussianKernel, beta = 0.5, same points: {lam:.3e}")
        assert lam < -1e-3


# ---- the layers above the kernel: n = 20 training points on S^2, the kernel under ScaleKernel ----------------------------------------
NU, LEVELS = 2.5, 32


def _problem():
    rng = np.random.default_rng(11)
    x = rng.standard_normal((32, 3))
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    y = np.arccos(np.clip(x[:, 0], -1, 1)) ** 2 + 0.05 * rng.standard_normal(32)
    return x[:20], y[:20], x[20:]


def _model(kappa=0.7, outputscale=1.5, noise=1e-2):
    xtr, y, _ = _problem()
    base = SphereRiemannianMaternKernel(nu=NU, num_levels=LEVELS).double()
    base.lengthscale = torch.tensor(kappa, dtype=torch.float64)
    cm = ScaleKernel(base).double()
    cm.outputscale = torch.tensor(outputscale, dtype=torch.float64)
    return models.SingleTaskGP(t(xtr), t(y), cm, initial_noise=noise), base


def _numpy_posterior(xtr, y, xte, kappa, os_, noise, mean):
    ky = os_ * matern_gram(xtr, xtr, kappa, NU, LEVELS) + noise * np.eye(len(xtr))
    ks = os_ * matern_gram(xte, xtr, kappa, NU, LEVELS)
    kss = os_ * matern_gram(xte, xte, kappa, NU, LEVELS)
    sol = np.linalg.solve(ky, np.concatenate([(y - mean)[:, None], ks.T], axis=1))
    return mean + ks @ sol[:, 0], kss - ks @ sol[:, 1:], np.linalg.cond(ky)


def test_fit_lowers_the_negative_marginal_likelihood():
    model, base = _model()
    assert [n for n, _ in model.named_parameters() if "nu" in n] == [] and model._stationary_form() is None
    start = -float(model.marginal_log_likelihood().detach())
    models.fit_gpytorch_model(model, maxiter=30)
    for p in model.parameters():
        p.requires_grad_(True)
    end = -float(model.marginal_log_likelihood().detach())
    print(f"negative marginal likelihood {start:.6f} -> {end:.6f}, lengthscale {float(base.lengthscale.detach()):.4f}")
    assert end < start
    assert all(bool(torch.isfinite(p).all()) for p in model.parameters())


def test_lengthscale_gradient_of_the_likelihood_against_differences():
    """what the fit descends along: d mll / d raw_lengthscale by autograd through the kernel, against central differences of the likelihood"""
    model, base = _model()
    for p in model.parameters():
        p.requires_grad_(True)
    (g,) = torch.autograd.grad(model.marginal_log_likelihood(), base.raw_lengthscale)
    h, vals = 1e-5, []
    raw0 = base.raw_lengthscale.detach().clone()
    for s in (1.0, -1.0):
        with torch.no_grad():
            base.raw_lengthscale.copy_(raw0 + s * h)
            vals.append(float(model.marginal_log_likelihood()))
    fd = (vals[0] - vals[1]) / (2 * h)
    assert abs(float(g) - fd) <= 1e-6 * max(1.0, abs(fd))       # (truncation h^2 |f'''| / 6 ~ 1e-10, rounding 2^-53 |f| / h ~ 1e-10: ample)


def test_posterior_against_numpy():
    xtr, y, xte = _problem()
    model, base = _model()
    preds = model(t(xte))
    kappa, os_, noise = float(base.lengthscale.detach()), float(model.covar_module.outputscale.detach()), float(model.noise.detach())
    mu, cov, cond = _numpy_posterior(xtr, y, xte, kappa, os_, noise, float(model.mean_constant.detach()))
    tol = 16 * 20 * 2.0 ** -52 * cond * os_
    err_m, err_c = np.abs(preds.mean.cpu().numpy() - mu).max(), np.abs(preds.covariance_matrix.cpu().numpy() - cov).max()
    print(f"cond(Ky) {cond:.3e}: mean error {err_m:.3e}, covariance error {err_c:.3e}, tolerance {tol:.3e}")
    assert err_m <= tol * max(1.0, np.abs(y).max()) and err_c <= tol


def test_condition_on_observations_against_a_rebuild():
    xtr, y, xte = _problem()
    model, base = _model()
    xnew, ynew = xte[:3], np.array([0.3, -0.2, 0.9])
    cond_model = model.condition_on_observations(t(xnew), t(ynew))
    preds = cond_model(t(xte[3:]))
    kappa, os_, noise = float(base.lengthscale.detach()), float(model.covar_module.outputscale.detach()), float(model.noise.detach())
    mu, cov, cond = _numpy_posterior(np.concatenate([xtr, xnew]), np.concatenate([y, ynew]), xte[3:], kappa, os_, noise,
                                     float(model.mean_constant.detach()))
    tol = 16 * 23 * 2.0 ** -52 * cond * os_
    assert np.abs(preds.mean.cpu().numpy() - mu).max() <= tol * max(1.0, np.abs(y).max())
    assert np.abs(preds.covariance_matrix.cpu().numpy() - cov).max() <= tol


def _acquisition():
    xtr, y, _ = _problem()
    base = SphereRiemannianMaternKernel(nu=NU, num_levels=LEVELS).double()
    base.lengthscale = torch.tensor(0.7, dtype=torch.float64)
    gp = models.ExactGP(t(xtr), t(y), base, outputscale=1.5, noise=1e-2)
    return models.ExpectedImprovement(gp, best_f=float(y.min()), maximize=False), gp, xtr, y


def test_fused_acquisition_matches_autograd_through_the_generic_path():
    acq, gp, xtr, y = _acquisition()
    fused = FusedAcquisition.build(acq, None, torch.device(DEV))
    assert fused is not None and fused.family == "sphere" and not fused.single_launch
    p, _ = ops.sphere_matern_coefficients(3, float(gp.base_kernel.lengthscale.double()), NU, LEVELS)
    assert fused.kxx == float(p.sum())
    x = t(_sphere_points(8, 50, 3))
    xx = x.clone().requires_grad_(True)
    f_ref = -acq(xx[:, None])
    (g_ref,) = torch.autograd.grad(f_ref.sum(), xx)
    f, g = fused.cost_egrad(x)
    # The two Euclidean gradients belong to two extensions of the cost off the sphere: the generic path differentiates k(x, x) = f(<x, x>)
    # along x, the fused one holds it at f(1) (on the sphere both are 1).  What the solvers use is the tangential part: compared here.
    tangent = lambda v: v - (v * x).sum(-1, keepdim=True) * x          # noqa: E731
    radial = float(((g_ref - g) - tangent(g_ref - g)).abs().max())
    g, g_ref = tangent(g), tangent(g_ref)
    cond = np.linalg.cond(1.5 * matern_gram(xtr, xtr, 0.7, NU, LEVELS) + 1e-2 * np.eye(20))
    tol = 16 * 20 * 2.0 ** -52 * cond          # rounding x cond(K_y), the scale of tests/test_gpu_acquisition_reference.py
    err_f = np.abs(f.cpu().numpy() - f_ref.detach().cpu().numpy()).max()
    err_g = np.abs(g.cpu().numpy() - g_ref.cpu().numpy()).max()
    print(f"cond(Ky) {cond:.3e}: value error {err_f:.3e}, gradient error {err_g:.3e}, tolerance {tol:.3e} (radial difference {radial:.3e})")
    assert float(f_ref.detach().abs().max()) > 1e-3 and float(g_ref.abs().max()) > 1e-3
    assert err_f <= tol * max(1.0, float(f_ref.detach().abs().max())) and err_g <= tol * max(1.0, float(g_ref.abs().max()))
    assert torch.equal(fused.cost(x), f)


@pytest.mark.parametrize("approx_hessian", [True, False])
def test_joint_optimize_returns_a_point_no_worse_than_the_raw_samples(approx_hessian):
    acq, gp, xtr, y = _acquisition()
    np.random.seed(3)
    torch.manual_seed(3)
    best = joint_optimize_manifold(acq, manifolds.Sphere(3), BatchedTrustRegions(), q=1, num_restarts=8, raw_samples=64, bounds=None,
                                   options={"device": DEV}, approx_hessian=approx_hessian)
    assert best.shape == (1, 3) and abs(best.norm().item() - 1) < 1e-12
    np.random.seed(3)           # the sweep's raw samples: the first 64 draws of manifold.rand() after the seed
    raw = torch.tensor(np.stack([manifolds.Sphere(3).rand() for _ in range(64)]), device=DEV)[:, None]
    ei_best, ei_raw = acq(best[None]).item(), acq(raw).max().item()
    print(f"approx_hessian {approx_hessian}: EI at the candidate {ei_best:.6e}, best raw sample {ei_raw:.6e}")
    assert ei_raw > 0.0 and ei_best >= ei_raw - 1e-12


def test_example_runs_and_shows_the_contrast():
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "sphere_matern_kernel.py")
    spec = importlib.util.spec_from_file_location("sphere_matern_kernel_example", path)
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    res = ex.regression(verbose=False, device=DEV)
    assert len(res) == 2 and all(np.isfinite(r["rmse"]) and r["variance"].min() >= 0.0 and r["covariance"].shape == (10, 10) for r in res.values())
    rows = ex.smallest_eigenvalues(verbose=False, device=DEV)
    assert all(lam >= -64 * 96 * U for name, _, lam in rows if name.startswith("Matern"))
    assert dict((par, lam) for name, par, lam in rows if name.startswith("geodesic"))["beta 0.5"] < -1e-3
