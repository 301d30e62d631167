"""Which route fills the prediction caches of models.ExactGP and models.SingleTaskGP on the device - ops.spd_gp_prepare, the kernel's forward and
ops.gp_factor, or torch.linalg - what each route leaves reachable through models._held, that the two models write the same bits at equal
hyper-parameters, and that a factor that does not exist drops every cache on every route.  At most 6 training points, except for the one case
that needs one point more than gabo_gp_factor takes."""
import numpy as np
import pytest
import torch

from gabotorch_amd import _compat, _lib, models, ops
from gabotorch_amd.kernel_utils.kernels_spd import SpdAffineInvariantGaussianKernel
from gabotorch_amd.kernel_utils.kernels_sphere import SphereGaussianKernel
from gabotorch_amd.Riemannian_utils.spd_utils_torch import symmetric_matrix_to_vector_mandel_torch as to_vec

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HELD = ("_cache_linv_t", "_cache_kinv", "_cache_factors")


def _spd(n, d, seed=0):
    rng = np.random.default_rng(seed)
    q = np.linalg.qr(rng.standard_normal((n, d, d)))[0]
    m = np.einsum("nab,nb,ncb->nac", q, rng.uniform(0.5, 2.0, (n, d)), q)
    return to_vec(torch.tensor(0.5 * (m + m.transpose(0, 2, 1)), device=DEV)), torch.tensor(rng.standard_normal(n), device=DEV)


def _sphere(n, dim=3, seed=0):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, dim))
    return torch.tensor(x / np.linalg.norm(x, axis=1, keepdims=True), device=DEV), torch.tensor(rng.standard_normal(n), device=DEV)


# name -> (training set, kernel, the route's launch, shape of the held training factors or None)
ROUTES = {
    "prepare_2x2": (lambda: _spd(4, 2), lambda: SpdAffineInvariantGaussianKernel(beta_min=0.5), "spd_gp_prepare", (3, 4)),
    "factor_13x13": (lambda: _spd(3, 13), lambda: SpdAffineInvariantGaussianKernel(beta_min=0.5), "gp_factor", None),      # d_vec = 91 > 78
    "factor_sphere": (lambda: _sphere(5), lambda: SphereGaussianKernel(beta_min=0.5), "gp_factor", None),
}


@pytest.fixture
def calls(monkeypatch):
    count = {"spd_gp_prepare": 0, "gp_factor": 0, "cholesky": 0}

    def counted(name, fn):
        def wrapper(*args, **kwargs):
            count[name] += 1
            return fn(*args, **kwargs)
        return wrapper
    monkeypatch.setattr(ops, "spd_gp_prepare", counted("spd_gp_prepare", ops.spd_gp_prepare))
    monkeypatch.setattr(ops, "gp_factor", counted("gp_factor", ops.gp_factor))
    monkeypatch.setattr(torch.linalg, "cholesky", counted("cholesky", torch.linalg.cholesky))
    return count


def _single_task(x, y, kernel, **kw):
    assert not _compat.HAVE_GPYTORCH
    cm = _compat.ScaleKernel(kernel)
    st = models.SingleTaskGP(x, y, cm, **kw)
    with torch.no_grad():
        cm.raw_outputscale.fill_(0.5)
        st.mean_constant.fill_(0.3)
    return st


def _exact_like(st, x, y, kernel):
    """ExactGP at the hyper-parameters of the SingleTaskGP"""
    return models.ExactGP(x, y, kernel, outputscale=float(st.covar_module.outputscale.detach()), noise=float(st.noise.detach()),
                          mean=float(st.mean_constant.detach()))


def _check_device_route(model, cache, n, launch, factors_shape, calls):
    ops.check_deferred()
    assert calls == {"spd_gp_prepare": int(launch == "spd_gp_prepare"), "gp_factor": int(launch == "gp_factor"), "cholesky": 0}
    linv, alpha = cache[0], cache[1]
    assert model._cache is cache and tuple(linv.shape) == (n, n) and tuple(alpha.shape) == (n,) and linv.is_cuda
    linv_t, kinv, factors = (models._held(model, k) for k in HELD)
    assert torch.equal(linv_t, linv.t()) and tuple(kinv.shape) == (n, n) and torch.equal(kinv, kinv.t())
    if factors_shape is None:
        assert factors is None
    else:
        assert tuple(factors.shape) == factors_shape and factors.dtype == torch.float64 and factors.is_cuda
    return linv, alpha, linv_t, kinv, factors


@pytest.mark.parametrize("route", sorted(ROUTES))
def test_both_models_take_the_device_route_and_write_the_same_bits(route, calls):
    data, make_kernel, launch, factors_shape = ROUTES[route]
    x, y = data()
    kernel = make_kernel()
    n = x.shape[0]
    st = _single_task(x, y, kernel, initial_noise=0.05)
    cache = st._ensure_cache()
    assert len(cache) == 3 and torch.equal(cache[2].cpu(), st.mean_constant.detach()) and cache[2].is_cuda
    assert not any(p.requires_grad for p in st.covar_module.parameters())
    from_st = _check_device_route(st, cache, n, launch, factors_shape, calls)
    assert st._ensure_cache() is cache and sum(calls.values()) == 1
    for k in calls:
        calls[k] = 0
    gp = _exact_like(st, x, y, kernel)
    cache = gp._train_cache()
    assert len(cache) == 2
    from_gp = _check_device_route(gp, cache, n, launch, factors_shape, calls)
    assert gp._train_cache() is cache and sum(calls.values()) == 1
    for name, a, b in zip(("linv", "alpha") + HELD, from_st, from_gp):
        assert (a is None and b is None) or torch.equal(a, b), name
    # the factor is one: L^-1 (outputscale K + noise I) L^-T = I to a few rounding errors of the conditioning (bounded by 1 / noise)
    with torch.no_grad():
        ky = gp.outputscale * kernel.forward(x, x) + gp.noise * torch.eye(n, dtype=torch.float64, device=DEV)
    err = float((from_gp[0] @ ky @ from_gp[0].t() - torch.eye(n, dtype=torch.float64, device=DEV)).abs().max())
    bound = 64 * n * float(torch.linalg.cond(ky)) * 2.0 ** -53
    print(f"{route}: |L^-1 Ky L^-T - I| = {err:.3g}, bound {bound:.3g}")
    assert err <= bound


def test_single_task_gp_with_a_bare_kernel_takes_torch(calls):
    x, y = _sphere(5)
    st = models.SingleTaskGP(x, y, SphereGaussianKernel(beta_min=0.5), initial_noise=0.05)
    cache = st._ensure_cache()
    ops.check_deferred()
    assert calls == {"spd_gp_prepare": 0, "gp_factor": 0, "cholesky": 1}
    assert len(cache) == 3 and tuple(cache[0].shape) == (5, 5) and all(models._held(st, k) is None for k in HELD)
    # ... where ExactGP takes the launch for the same kernel
    gp = models.ExactGP(x, y, st.covar_module, noise=0.05)
    gp._train_cache()
    ops.check_deferred()
    assert calls == {"spd_gp_prepare": 0, "gp_factor": 1, "cholesky": 1}


def test_exact_gp_beyond_the_factor_launch_takes_torch(calls):
    n = _lib.GABO_GP_FACTOR_MAX_N + 1
    x, y = _sphere(n)
    gp = models.ExactGP(x, y, SphereGaussianKernel(beta_min=0.5), noise=0.05)
    cache = gp._train_cache()
    ops.check_deferred()
    assert calls == {"spd_gp_prepare": 0, "gp_factor": 0, "cholesky": 1}
    assert len(cache) == 2 and tuple(cache[0].shape) == (n, n) and all(models._held(gp, k) is None for k in HELD)


# ExactGP on the prepare route: tests/test_gpu_errors.py::test_a_failed_factorisation_drops_the_models_cache
@pytest.mark.parametrize("model,route", [("exact", "factor_sphere"), ("single_task", "prepare_2x2"), ("single_task", "factor_sphere")])
def test_a_failed_factorisation_drops_every_cache(model, route, calls):
    """K + noise I is indefinite through a negative noise: the launch reports it in its status word, ops.check_deferred drops the caches the
    launch was to fill and raises - on the second request as on the first."""
    data, make_kernel, launch, _ = ROUTES[route]
    x, y = data()
    if model == "exact":
        gp = models.ExactGP(x, y, make_kernel(), outputscale=1.0, noise=-2.0)
    else:
        gp = models.SingleTaskGP(x, y, _compat.ScaleKernel(make_kernel()), noise_lower_bound=-2.0, initial_noise=-1.5)
        assert float(gp.noise.detach()) == pytest.approx(-1.5)
    for attempt in (1, 2):
        with pytest.raises(RuntimeError, match="not positive definite"):
            gp.posterior(x[:3, None])
        assert gp._cache is None and gp._cache_linv_t is None and gp._cache_kinv is None and gp._cache_factors is None
        assert calls[launch] == attempt and calls["cholesky"] == 0
