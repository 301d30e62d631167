"""Joint GP posterior over a test set and posterior samples on the device (csrc/gp_posterior.hip, ops.gp_posterior_joint, ops.mvn_sample,
models.MultivariateNormal, SingleTaskGP.forward / ExactGP.forward) against the numpy references of tests/_cpu_gp_posterior.py.

Every tolerance is derived there or stated where it is used; each test prints the worst ratio error / bound before it asserts."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest
import torch

from gabotorch_amd import _compat, _lib, models, ops
from gabotorch_amd.kernel_utils import kernels_spd as kspd
from gabotorch_amd.kernel_utils import kernels_sphere as ksph
from tests import _cpu_gp_posterior as cpu
from tests.conftest import load_golden

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))

DEV = "cuda:0"
U = cpu.U
EPS = np.finfo(np.float64).eps
MAX_M = _lib.GABO_MVN_SAMPLE_MAX_M


def t(x):
    return torch.tensor(np.ascontiguousarray(x), dtype=torch.float64, device=DEV)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


# ---- 1. the covariance launch ------------------------------------------------------------------------------------------------------------------
# (m, n): the tile edges of a 16 x 16 x 4 instruction in m and in n, one past GABO_GP_FACTOR_MAX_N, one past GABO_GP_MLL_MAX_N
JOINT_SHAPES = [(1, 1), (15, 3), (16, 4), (17, 5), (33, 96), (100, 79), (130, 161)]


@functools.lru_cache(maxsize=None)
def joint_case(m, n):
    """inputs, reference and device results of one shape (computed once, read-only)"""
    kstar, kss, linv, alpha, mean, os_ = cpu.random_joint_case(m, n, seed=100 * m + n)
    ref = cpu.joint_reference(kstar, kss, linv, alpha, mean, os_)
    mu, var, cov = ops.gp_posterior_joint(t(kstar), t(kss), t(linv), t(alpha), mean, os_)
    return (kstar, kss, linv, alpha, mean, os_), ref, (mu.cpu().numpy(), var.cpu().numpy(), cov.cpu().numpy())


@pytest.mark.parametrize("m,n", JOINT_SHAPES)
def test_covariance_launch_within_the_running_error_bound(m, n):
    _, ref, (mu, var, cov) = joint_case(m, n)
    assert cov.shape == (m, m) and mu.shape == (m,) and var.shape == (m,)
    err, bound = np.abs(cov - ref["cov"]), (2 * n + 8) * U * ref["cov_scale"]
    merr, mbound = np.abs(mu - ref["mean"]), (n + 8) * U * ref["mean_scale"]
    print(f"m {m} n {n}: cov worst error / bound {np.max(err / bound):.3f}, mean {np.max(merr / mbound):.3f}")
    assert np.all(err <= bound)
    assert np.all(merr <= mbound)
    assert np.array_equal(bits(cov), bits(cov.T)), "the covariance must be bit-symmetric"
    assert np.array_equal(bits(var), bits(np.diagonal(cov))), "var_out must be the diagonal, bit for bit"


def test_upper_triangle_of_kss_is_not_read_and_inplace_is_honoured():
    (kstar, kss, linv, alpha, mean, os_), _, (_, _, cov) = joint_case(33, 96)
    junk = np.tril(kss) + np.triu(np.full_like(kss, np.nan), 1)
    linv_junk = linv + np.triu(np.full_like(linv, np.nan), 1)            # (only the non-zero triangle of linv is read)
    kj = t(junk)
    _, _, got = ops.gp_posterior_joint(t(kstar), kj, t(linv_junk), t(alpha), mean, os_)
    assert got.data_ptr() == kj.data_ptr()
    assert np.array_equal(bits(got.cpu().numpy()), bits(cov))
    keep = t(kss)
    _, _, got = ops.gp_posterior_joint(t(kstar), keep, t(linv), t(alpha), mean, os_, inplace=False)
    assert got.data_ptr() != keep.data_ptr() and np.array_equal(keep.cpu().numpy(), kss)
    assert np.array_equal(bits(got.cpu().numpy()), bits(cov))


def test_rows_do_not_depend_on_the_size_of_the_test_set():
    (kstar, kss, linv, alpha, mean, os_), _, (mu, _, cov) = joint_case(130, 161)
    mu17, var17, cov17 = ops.gp_posterior_joint(t(kstar[:17]), t(kss[:17, :17]), t(linv), t(alpha), mean, os_)
    assert np.array_equal(bits(cov17.cpu().numpy()), bits(cov[:17, :17]))
    assert np.array_equal(bits(mu17.cpu().numpy()), bits(mu[:17]))


def test_non_finite_input_marks_what_it_touches():
    (kstar, kss, linv, alpha, mean, os_), _, (mu, _, cov) = joint_case(33, 96)
    ks = kstar.copy()
    ks[5, 40] = np.nan
    mu2, var2, cov2 = (x.cpu().numpy() for x in ops.gp_posterior_joint(t(ks), t(kss), t(linv), t(alpha), mean, os_))
    ops.check_deferred()                                                   # (no error is raised)
    assert np.isnan(mu2[5]) and np.isnan(cov2[5]).all() and np.isnan(cov2[:, 5]).all() and np.isnan(var2[5])
    rest = np.delete(np.arange(33), 5)
    assert np.array_equal(bits(cov2[np.ix_(rest, rest)]), bits(cov[np.ix_(rest, rest)])) and np.array_equal(bits(mu2[rest]), bits(mu[rest]))


# ---- 2. model level ------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def letters():
    g = load_golden("letters_gp.npz")
    return {k: g[k] for k in g.files}


def _scaled(base, outputscale):
    k = _compat.ScaleKernel(base.double()).double()
    k.outputscale = outputscale
    return k


def _letters_model(kind, base):
    g = letters()
    x = t(g["x_test"])
    xtr, ytr = x[torch.as_tensor(g["train_idx"], device=DEV)], t(g["y_train"])
    if kind == "SingleTaskGP":
        model = models.SingleTaskGP(xtr, ytr, _scaled(base, float(g["outputscale"])), initial_noise=float(g["noise"]))
        hyper = (float(model.covar_module.outputscale.detach()), float(model.noise.detach()), float(model.mean_constant.detach()))
    else:
        model = models.ExactGP(xtr, ytr, base.double(), outputscale=float(g["outputscale"]), noise=float(g["noise"]), mean=float(g["mean"]))
        hyper = (model.outputscale, model.noise, model.mean)
    return model, x, hyper


def _marginals_agree(model, x, preds, linv, alpha, base, os_, mean):
    """model(x) against the model's own posterior(x): the same two sums in another order - each side within its running-error bound"""
    mu0, var0 = (v.cpu().numpy() for v in model.posterior(x))
    with torch.no_grad():
        ks = np.abs(base.forward(x, model.train_x).double().cpu().numpy())
    n = ks.shape[1]
    vabs = os_ * ks @ np.abs(linv.cpu().numpy()).T
    mscale = abs(mean) + os_ * ks @ np.abs(alpha.cpu().numpy())
    vscale = os_ * 1.0 + (vabs * vabs).sum(1)                               # (k(x, x) = 1 for every kernel of the library)
    dm, dv = np.abs(preds.mean.cpu().numpy() - mu0), np.abs(torch.diagonal(preds.covariance_matrix).cpu().numpy() - var0)
    print(f"mean vs posterior(): worst / bound {np.max(dm / (2 * (n + 8) * U * mscale)):.3f}, variance {np.max(dv / (2 * (2 * n + 8) * U * vscale)):.3f}")
    assert np.all(dm <= 2 * (n + 8) * U * mscale) and np.all(dv <= 2 * (2 * n + 8) * U * vscale)
    assert torch.equal(preds.variance, torch.diagonal(preds.covariance_matrix).clamp_min(0.0))


@pytest.mark.parametrize("kind", ["SingleTaskGP", "ExactGP"])
def test_letters_posterior_against_numpy_on_the_reference_distances(kind):
    g = letters()
    base = kspd.SpdAffineInvariantGaussianKernel(beta_min=0.0).double()
    base.beta = float(g["beta"])
    model, x, (os_, noise, mean) = _letters_model(kind, base)
    preds = model(x)
    assert isinstance(preds, models.MultivariateNormal) and preds.covariance_matrix.shape == (100, 100)
    beta = float(base.beta.detach())                                       # (the constraint's transform leaves fp32's 1.3: the reference below takes what the model holds)
    assert abs(beta - 1.3) < 1e-6 and os_ == pytest.approx(2000.0, rel=1e-14) and noise == pytest.approx(2.0, rel=1e-14)
    mu, cov, cond = cpu.gaussian_posterior(g["dist_train_train"], g["dist_test_train"], g["dist_test_test"], g["y_train"], beta, os_, noise, mean)
    n = len(g["y_train"])
    tol = 16 * n * EPS * cond * os_
    err = np.abs(preds.covariance_matrix.cpu().numpy() - cov).max()
    print(f"{kind}: cond(Ky) {cond:.3e}, covariance max error {err:.3e}, tolerance {tol:.3e}")
    assert err <= tol
    cache = model._ensure_cache() if kind == "SingleTaskGP" else model._train_cache()
    _marginals_agree(model, x, preds, cache[0], cache[1], base, os_, mean)
    lo, hi = preds.confidence_region()
    assert torch.equal(lo, preds.mean - 2.0 * preds.stddev) and torch.equal(hi, preds.mean + 2.0 * preds.stddev)


def test_letters_log_euclidean_kernel():
    g = letters()
    base = kspd.SpdLogEuclideanGaussianKernel().double()
    base.lengthscale = 0.9
    model, x, (os_, noise, mean) = _letters_model("SingleTaskGP", base)
    preds = model(x)
    linv, alpha, _ = model._ensure_cache()
    _marginals_agree(model, x, preds, linv, alpha, base, os_, mean)
    assert np.array_equal(bits(preds.covariance_matrix.cpu().numpy()), bits(preds.covariance_matrix.cpu().numpy().T))
    assert bool(torch.isfinite(preds.mean).all()) and float(preds.variance.min()) >= 0.0


def test_sphere_demo_sizes():
    """SphereGaussianKernel, dim 3, n = 20, m = 10: the sizes of the reference's sphere demo"""
    rng = np.random.default_rng(1234)
    pts = rng.standard_normal((30, 3)) * np.sqrt(0.1) + np.array([1.0, 0.0, 0.0])
    pts /= np.linalg.norm(pts, axis=1, keepdims=True)
    xtr, xte, y = t(pts[:20]), t(pts[20:]), t(np.sin(3.0 * pts[:20, 1]))
    base = ksph.SphereGaussianKernel(beta_min=6.5).double()
    model = models.SingleTaskGP(xtr, y, _scaled(base, 1.5), initial_noise=1e-2)
    preds = model(xte)
    linv, alpha, _ = model._ensure_cache()
    _marginals_agree(model, xte, preds, linv, alpha, base, float(model.covar_module.outputscale.detach()), 0.0)
    from oracle import sphere as osph
    beta, os_, noise = float(base.beta.detach()), float(model.covar_module.outputscale.detach()), float(model.noise.detach())
    d = lambda a, b: osph.sphere_distance(a, b)                             # noqa: E731
    mu, cov, cond = cpu.gaussian_posterior(d(pts[:20], pts[:20]), d(pts[20:], pts[:20]), d(pts[20:], pts[20:]), y.cpu().numpy(), beta, os_, noise, 0.0)
    err, tol = np.abs(preds.covariance_matrix.cpu().numpy() - cov).max(), 16 * 20 * EPS * cond * os_
    print(f"sphere: cond(Ky) {cond:.3e}, covariance max error {err:.3e}, tolerance {tol:.3e}")
    assert err <= tol
    assert preds.sample(torch.Size([4]), seed=3).shape == (4, 10)


def test_forward_takes_one_test_set_only():
    base = ksph.SphereGaussianKernel(beta_min=6.5).double()
    pts = torch.nn.functional.normalize(torch.randn(6, 3, dtype=torch.float64, device=DEV), dim=-1)
    model = models.ExactGP(pts, pts[:, 0], base)
    with pytest.raises(ValueError, match="one test set"):
        model(pts.unsqueeze(0))


# ---- 3. the sampler with base samples given -----------------------------------------------------------------------------------------------------
def _spd_case(m, seed):
    rng = np.random.default_rng(seed)
    b = rng.standard_normal((m, m))
    return b @ b.T + 1e-3 * np.eye(m), rng.standard_normal((3, m))


def _sample_residual(out, z, L, m):
    """out = Z L^T (mean 0) against the returned factor: (m + 2) u |Z| |L|^T, a length-m dot product and the final sum"""
    Ll, zl = L.astype(np.longdouble), z.astype(np.longdouble)
    err = np.abs(out.astype(np.longdouble) - zl @ Ll.T)
    bound = (m + 2) * U * (np.abs(zl) @ np.abs(Ll).T)
    return float(np.max(err / bound)), bool(np.all(err <= bound))


@pytest.mark.parametrize("m", [1, 2, 63, 64, 65, 100, MAX_M])
def test_sampler_factor_and_samples(m):
    cov, z = _spd_case(m, seed=m)
    np.linalg.cholesky(cov)                                                 # (numpy agrees that this factors without jitter)
    out, L, rung = ops.mvn_sample(torch.zeros(m, dtype=torch.float64, device=DEV), t(cov), (3,), base_samples=t(z), return_scale_tril=True)
    ops.check_deferred()
    out, L = out.cpu().numpy(), L.cpu().numpy()
    assert int(rung) == 0 and np.array_equal(L, np.tril(L)) and out.shape == (3, m)
    ok, ratio = cpu.cholesky_residual_ok(L, cov)
    sratio, sok = _sample_residual(out, z, L, m)
    print(f"m {m}: |L L^T - cov| worst / bound {ratio:.3f}; |out - Z L^T| worst / bound {sratio:.3f}")
    assert ok and sok
    # a mean: out = mean + (Z L^T as above), one more rounding of the sum
    mean = np.linspace(-3.0, 7.0, m)
    out2 = ops.mvn_sample(t(mean), t(cov), (3,), base_samples=t(z)).cpu().numpy()
    assert np.all(np.abs(out2 - (mean + out)) <= U * np.abs(out2) * 1.0000001)
    dist = models.MultivariateNormal(t(mean), t(cov))
    assert dist.jitter_used == 0.0 and np.array_equal(dist.scale_tril.cpu().numpy(), L)
    assert np.array_equal(dist.sample(torch.Size([3]), base_samples=t(z)).cpu().numpy(), out2)
    assert dist.sample().shape == (m,) and dist.rsample(torch.Size([2, 2]), seed=1).shape == (2, 2, m)


def test_letters_covariance_needs_the_ladder():
    g = letters()
    base = kspd.SpdAffineInvariantGaussianKernel(beta_min=0.0).double()
    base.beta = float(g["beta"])
    model, x, _ = _letters_model("SingleTaskGP", base)
    preds = model(x)
    z = np.random.default_rng(7).standard_normal((3, 100))
    out = preds.sample(torch.Size([3]), base_samples=t(z)).cpu().numpy()
    jitter = preds.jitter_used
    print(f"letters: jitter used {jitter:g}")
    assert jitter <= 1e-8 and jitter in (0.0, 1e-8)                        # (which of the two is decided by rounding)
    L = preds.scale_tril.cpu().numpy()
    sigma = preds.covariance_matrix.cpu().numpy()
    ok, ratio = cpu.cholesky_residual_ok(L, sigma + jitter * np.eye(100))
    print(f"letters: |L L^T - (Sigma + j I)| worst / bound {ratio:.3f}")
    assert ok
    mu = preds.mean.cpu().numpy()
    zl = z.astype(np.longdouble) @ L.astype(np.longdouble).T
    bound = (100 + 2) * U * (np.abs(z) @ np.abs(L).T) + U * (np.abs(mu) + np.abs(out))     # + the rounding of mean + (.) and of out - mean
    assert np.all(np.abs(out - mu - zl) <= bound)


# ---- 4. the sampler's own normals ---------------------------------------------------------------------------------------------------------------
def test_normals_are_the_philox_stream_of_the_oracle():
    seed = 0x1234_5678_9ABC_DEF0
    for samples, m in ((5, 7), (3, 64), (2, MAX_M)):
        want = cpu.mvn_normals(seed, samples, m)
        eye = torch.eye(m, dtype=torch.float64, device=DEV)
        got = ops.mvn_sample(torch.zeros(m, dtype=torch.float64, device=DEV), eye, (samples,), seed=seed)
        again = ops.mvn_sample(torch.zeros(m, dtype=torch.float64, device=DEV), eye, (samples,), seed=seed)
        np.testing.assert_allclose(got.cpu().numpy(), want, rtol=0, atol=1e-13)
        assert torch.equal(got, again)
        assert torch.equal(ops.mvn_base_samples(samples, m, seed, device=DEV), got)
        assert not torch.equal(ops.mvn_sample(torch.zeros(m, dtype=torch.float64, device=DEV), eye, (samples,), seed=seed + 1), got)


def test_a_seed_gives_the_same_normals_on_both_paths():
    seed = 99
    z = {}
    for m in (MAX_M, MAX_M + 1):
        z[m] = ops.mvn_sample(torch.zeros(m, dtype=torch.float64, device=DEV), torch.eye(m, dtype=torch.float64, device=DEV), (4,), seed=seed)
        np.testing.assert_allclose(z[m].cpu().numpy(), cpu.mvn_normals(seed, 4, m), rtol=0, atol=1e-13)
    # item = sample, draw k -> coordinates 2k, 2k + 1: the first 192 coordinates of a sample do not depend on m
    assert torch.equal(z[MAX_M], z[MAX_M + 1][:, :MAX_M])


def test_torch_path_beyond_the_fused_size():
    m = MAX_M + 8
    cov, z = _spd_case(m, seed=5)
    out, L, rung = ops.mvn_sample(torch.zeros(m, dtype=torch.float64, device=DEV), t(cov), (3,), base_samples=t(z), return_scale_tril=True)
    assert int(rung) == 0
    np.testing.assert_allclose(out.cpu().numpy(), z @ np.linalg.cholesky(cov).T, rtol=1e-10, atol=1e-10)
    with pytest.raises(RuntimeError, match="not positive definite"):
        ops.mvn_sample(torch.zeros(m, dtype=torch.float64, device=DEV), -torch.eye(m, dtype=torch.float64, device=DEV), (1,), seed=0)


# ---- 5. errors ----------------------------------------------------------------------------------------------------------------------------------
def test_indefinite_covariance_raises(raising):
    with raising("not positive definite"):
        ops.mvn_sample(torch.zeros(8, dtype=torch.float64, device=DEV), -torch.eye(8, dtype=torch.float64, device=DEV), (2,), seed=1)


def test_nan_covariance_raises(raising):
    cov = torch.eye(8, dtype=torch.float64, device=DEV)
    cov[6, 2] = float("nan")
    with raising("not positive definite"):
        ops.mvn_sample(torch.zeros(8, dtype=torch.float64, device=DEV), cov, (2,), seed=1)


def test_c_entry_refuses_more_than_the_fused_size():
    lib = _lib.load()
    m = MAX_M + 1
    mean, cov = torch.zeros(m, dtype=torch.float64, device=DEV), torch.eye(m, dtype=torch.float64, device=DEV)
    out, status = torch.zeros(1, m, dtype=torch.float64, device=DEV), torch.zeros(2, dtype=torch.int32, device=DEV)
    rc = lib.gabo_mvn_sample(mean.data_ptr(), cov.data_ptr(), m, 1, ctypes.c_uint64(0), None, out.data_ptr(), None, status.data_ptr(), None)
    assert rc == _lib.GABO_ERR_DIM
    assert status.tolist() == [0, 0] and float(out.abs().sum()) == 0.0


# ---- 6. the two examples ------------------------------------------------------------------------------------------------------------------------
def test_spd_kernels_example_with_the_fixture_hyper_parameters():
    import spd_kernels
    res = spd_kernels.run(nb_samples_post=10, fixed=True, verbose=False)
    r = res["Affine-invariant kernel"]
    assert r["samples"].shape == (10, 100) and np.isfinite(r["samples"]).all() and np.isfinite(r["rmse"])
    assert r["variance"].min() >= 0.0 and r["covariance"].shape == (100, 100) and r["jitter"] <= 1e-8
    # the training points are reproduced to within the noise, the left-out stretches are not: the variance there is larger
    g = letters()
    left_out = np.setdiff1d(np.arange(100), g["train_idx"])
    assert r["variance"][left_out].max() > 10.0 * r["variance"][g["train_idx"]].max()


def test_sphere_kernels_example():
    import sphere_kernels
    res = sphere_kernels.run(verbose=False)
    assert set(res) == {"Manifold-RBF kernel", "Laplace kernel"}
    for r in res.values():
        assert np.isfinite(r["rmse"]) and r["mean"].shape == (10,) and r["covariance"].shape == (10, 10) and r["variance"].min() >= 0.0
