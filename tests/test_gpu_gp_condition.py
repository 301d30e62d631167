"""Conditioning the prediction cache on the device (csrc/gp_condition.hip, ops.gp_condition, models.*.condition_on_observations) against the
from-scratch references of tests/_cpu_gp_condition.py.  The bound on linv, alpha and kinv is cpu.bound: (8 + 4 cond_2(K_new)) 2^-53 max|ref|;
what is derived from it is stated where it is used.  Each test prints its worst ratio before it asserts."""
import functools

import numpy as np
import pytest
import torch

from gabotorch_amd import _compat, _lib, models, ops
from gabotorch_amd.fused_acquisition import FusedAcquisition
from gabotorch_amd.kernel_utils import kernels_spd as kspd
from gabotorch_amd.kernel_utils import kernels_sphere as ksph
from gabotorch_amd.Riemannian_utils.spd_utils_torch import symmetric_matrix_to_vector_mandel_torch as to_vec
from tests import _cpu_gp_condition as cpu

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
EPS = cpu.EPS
# (n, t): the wave edge, both sides of GABO_GP_FACTOR_MAX_N, one past GABO_GP_MLL_MAX_N, the size limit
SHAPES = [(1, 1), (3, 2), (63, 1), (64, 1), (65, 5), (96, 1), (97, 3), (161, 5), (2040, 8)]
NOISE = 1e-2


def t(x):
    return torch.tensor(np.ascontiguousarray(x), dtype=torch.float64, device=DEV)


def bits(a):
    a = a.cpu().numpy() if torch.is_tensor(a) else a
    return np.ascontiguousarray(a).view(np.uint64)


def host(outs):
    return tuple(None if o is None else o.cpu().numpy() for o in outs)


@functools.lru_cache(maxsize=None)
def op_case(n, tt):
    """inputs, reference and device results (targets given) of one shape: computed once, read-only"""
    if n + tt > 512:            # the size limit: fp64 numpy from scratch, dim 6 and beta 6 keep cond below 1e3
        case = cpu.make_case(n, tt, NOISE, dim=6, beta=6.0)
        old, ref = cpu.reference_fp64(case, n), cpu.reference_fp64(case)
    else:
        case = cpu.make_case(n, tt, NOISE)
        _, linv_full = cpu.ld_factor(cpu.covariance(case))
        old = tuple(np.asarray(v, dtype=np.float64) for v in cpu.ld_cache(linv_full, case["y"], case["mean"], n))
        ref = cpu.ld_cache(linv_full, case["y"], case["mean"], n + tt)
    cond = cpu.cond2(case)
    dev = dict(linv=t(old[0]), alpha=t(old[1]), kinv=t(old[2]), kcross=t(case["kcross"]), knew=t(case["knew"]), y_new=t(case["y"][n:]))
    got = host(_call(case, dev))
    ops.check_deferred()
    return case, dev, ref, cond, got


def _call(case, dev, **over):
    a = dict(dev, **over)
    return ops.gp_condition(a["linv"], a["alpha"], a["kcross"], a["knew"], a["y_new"], outputscale=case["outputscale"], noise=case["noise"],
                            mean=case["mean"], kinv=a["kinv"])


@pytest.mark.parametrize("n,tt", SHAPES)
def test_outputs_within_the_bound_and_of_the_stated_structure(n, tt):
    case, _, ref, cond, (linv, linv_t, alpha, kinv, y_used) = op_case(n, tt)
    if n + tt > 512:
        assert cond < 1e3
    m = n + tt
    assert linv.shape == (m, m) and linv_t.shape == (m, m) and alpha.shape == (m,) and kinv.shape == (m, m) and y_used.shape == (tt,)
    for name, g, r in (("linv", linv, ref[0]), ("linv_t", linv_t, ref[0].T), ("alpha", alpha, ref[1]), ("kinv", kinv, ref[2])):
        err = float(np.max(np.abs(g - r)))
        print(f"n {n} t {tt} cond {cond:.3g} {name}: error / bound {err / cpu.bound(cond, r):.3f} ({err / float(np.max(np.abs(r))) / EPS:.2f} eps max|ref|)")
        assert err <= cpu.bound(cond, r), name
    assert np.array_equal(bits(linv_t), bits(linv.T)), "linv_t must be the transpose bit for bit"
    assert np.array_equal(bits(kinv), bits(kinv.T)), "kinv must be bit-symmetric"
    assert np.array_equal(bits(np.triu(linv, 1)), bits(np.zeros((m, m)))), "exact zeros above the diagonal of linv"
    assert np.array_equal(bits(y_used), bits(case["y"][n:]))


@pytest.mark.parametrize("n,tt", [s for s in SHAPES if s[1] > 1])
def test_one_call_with_t_points_equals_t_calls_with_one(n, tt):
    case, dev, _, _, want = op_case(n, tt)
    linv, alpha, kinv = dev["linv"], dev["alpha"], dev["kinv"]
    ys = []
    for j in range(tt):
        kcross = torch.cat([dev["kcross"][j], dev["knew"][j, :j]]).reshape(1, n + j)
        linv, linv_t, alpha, kinv, y = _call(case, dict(linv=linv, alpha=alpha, kinv=kinv, kcross=kcross, knew=dev["knew"][j:j + 1, j:j + 1].contiguous(),
                                                        y_new=dev["y_new"][j:j + 1]))
        ys.append(y)
    ops.check_deferred()
    for name, g, w in zip(("linv", "linv_t", "alpha", "kinv", "y_used"), (linv, linv_t, alpha, kinv, torch.cat(ys)), want):
        assert np.array_equal(bits(g), bits(w)), name


@pytest.mark.parametrize("n,tt", [(65, 5), (97, 3)])
def test_junk_outside_the_triangles_that_are_read_changes_no_bit(n, tt):
    case, dev, _, _, want = op_case(n, tt)
    nan_above = lambda a: torch.tril(a) + torch.triu(torch.full_like(a, float("nan")), 1)       # noqa: E731
    got = host(_call(case, dev, linv=nan_above(dev["linv"]), knew=nan_above(dev["knew"])))
    ops.check_deferred()
    for name, g, w in zip(("linv", "linv_t", "alpha", "kinv", "y_used"), got, want):
        assert np.array_equal(bits(g), bits(w)), name


@pytest.mark.parametrize("n,tt", SHAPES)
def test_believer_copies_alpha_and_reports_the_posterior_mean(n, tt):
    case, dev, ref, cond, want = op_case(n, tt)
    linv, linv_t, alpha, kinv, y_used = host(_call(case, dev, y_new=None))
    ops.check_deferred()
    a_old = dev["alpha"].cpu().numpy()
    assert np.array_equal(bits(alpha[:n]), bits(a_old)), "alpha[:n] must be copied untouched"
    assert np.array_equal(bits(alpha[n:]), bits(np.zeros(tt))), "the appended entries must be exact (positive) zeros"
    os_, mean = case["outputscale"], case["mean"]
    mu = mean + os_ * (case["kcross"].astype(np.longdouble) @ a_old.astype(np.longdouble))
    scale = abs(mean) + os_ * np.abs(case["kcross"]) @ np.abs(a_old)
    err = np.abs(y_used - mu)
    print(f"n {n} t {tt}: y_used error / bound {float(np.max(err / ((n + 8) * EPS * scale))):.3f}")
    assert np.all(err <= (n + 8) * EPS * scale)
    # the factors do not depend on the targets
    for name, g, w in zip(("linv", "linv_t", None, "kinv"), (linv, linv_t, None, kinv), want):
        if name:
            assert np.array_equal(bits(g), bits(w)), name


def test_a_point_that_breaks_positive_definiteness_is_reported_not_faulted():
    case, dev, _, _, want = op_case(65, 5)
    kcross, knew = dev["kcross"].clone(), dev["knew"].clone()
    kcross[2] = t(case["kbase"][7, :65])                      # new point 2 repeats training point 7 ...
    knew[2, :2] = t(case["kbase"][7, 65:67])
    knew[2, 2] = 0.1                                          # ... with a prior variance its covariance with that point exceeds
    called = []
    ops.gp_condition(dev["linv"], dev["alpha"], kcross, knew, None, outputscale=case["outputscale"], noise=case["noise"], mean=case["mean"],
                     kinv=dev["kinv"], on_fail=lambda: called.append(1))
    with pytest.raises(RuntimeError, match=r"gabo_gp_condition.*new point #2.*not positive definite"):
        ops.check_deferred()
    assert called == [1]
    got = host(_call(case, dev))                              # a following valid call succeeds
    ops.check_deferred()
    for g, w in zip(got, want):
        assert np.array_equal(bits(g), bits(w))


def test_wrapper_refuses_what_does_not_belong_together():
    case, dev, _, _, _ = op_case(3, 2)
    with pytest.raises(ValueError, match="do not belong together"):
        _call(case, dev, kcross=dev["kcross"][:, :2].contiguous())
    with pytest.raises(ValueError, match="HIP device"):
        _call(case, dev, knew=dev["knew"].cpu())
    with pytest.raises(ValueError, match="outside"):
        ops.gp_condition(torch.eye(3, dtype=torch.float64, device=DEV), torch.zeros(3, dtype=torch.float64, device=DEV),
                         torch.zeros(17, 3, dtype=torch.float64, device=DEV), torch.eye(17, dtype=torch.float64, device=DEV))


# ---- models ------------------------------------------------------------------------------------------------------------------------------------
def _spd_mandel(rng, count, d):
    q = np.linalg.qr(rng.standard_normal((count, d, d)))[0]
    x = np.einsum("nab,nb,ncb->nac", q, rng.uniform(0.3, 3.0, (count, d)), q)
    return to_vec(torch.tensor(0.5 * (x + x.transpose(0, 2, 1)))).numpy(), (np.log(np.linalg.eigvalsh(x)) ** 2).sum(1)


def _sphere(rng, count, dim):
    x = cpu.sphere_points(rng, count, dim)
    return x, np.arccos(np.clip(x[:, 0], -1.0, 1.0)) ** 2 + 0.05 * rng.standard_normal(count)


def _scaled(base, outputscale):
    k = _compat.ScaleKernel(base.double()).double()
    k.outputscale = outputscale
    return k


SETUPS = ("exact_ai_d3_n12", "single_task_sphere_dim4_n20", "exact_le_d2_n10", "exact_sphere_n100")
T_NEW = 3


@functools.lru_cache(maxsize=None)
def setup(name):
    """-> dict: make(x, y) building a fresh model with the set-up's hyper-parameters, the n + T_NEW points and targets, what the model is made of"""
    rng = np.random.default_rng(len(name))
    if name == "exact_ai_d3_n12":
        n, (x, y) = 12, _spd_mandel(rng, 12 + T_NEW, 3)
        base, os_, noise, mean = kspd.SpdAffineInvariantGaussianKernel(beta_min=0.25).double(), 1.2, 1e-2, float(y[:12].mean())
        post = to_vec
    elif name == "exact_le_d2_n10":
        n, (x, y) = 10, _spd_mandel(rng, 10 + T_NEW, 2)
        base, os_, noise, mean = kspd.SpdLogEuclideanGaussianKernel().double(), 1.0, 1e-2, float(y[:10].mean())
        base.lengthscale = 1.5
        post = to_vec
    elif name == "single_task_sphere_dim4_n20":
        n, (x, y) = 20, _sphere(rng, 20 + T_NEW, 4)
        base, os_, noise, mean = ksph.SphereGaussianKernel(beta_min=2.0).double(), 1.5, 1e-2, 0.0
        post = None
    else:
        n, (x, y) = 100, _sphere(rng, 100 + T_NEW, 4)
        base, os_, noise, mean = ksph.SphereGaussianKernel(beta_min=2.0).double(), 1.0, 1e-2, float(y[:100].mean())
        post = None
    if name.startswith("single_task"):
        cm = _scaled(base, os_)
        make = lambda xx, yy: models.SingleTaskGP(xx, yy, cm, initial_noise=noise)       # noqa: E731
        os_ = float(cm.outputscale.detach())
    else:
        make = lambda xx, yy: models.ExactGP(xx, yy, base, outputscale=os_, noise=noise, mean=mean)     # noqa: E731
    return dict(make=make, n=n, x=t(x), y=t(y), base=base, os=os_, noise=noise, mean=mean, post=post)


def _cache(model):
    return model._ensure_cache() if type(model) is models.SingleTaskGP else model._train_cache()


@functools.lru_cache(maxsize=None)
def conditioned(name):
    """the source model, its caches before conditioning, the model conditioned on T_NEW observed points and the longdouble reference built from
    the device Gram matrix of the concatenated set"""
    s = setup(name)
    n = s["n"]
    src = s["make"](s["x"][:n], s["y"][:n])
    cache = _cache(src)
    ops.check_deferred()
    held = {k: getattr(src, k, None) for k in ("_cache_linv_t", "_cache_kinv", "_cache_factors")}
    before = dict(cache=cache, held=held, linv=cache[0].clone(), alpha=cache[1].clone(),
                  kinv=None if models._held(src, "_cache_kinv") is None else models._held(src, "_cache_kinv").clone())
    new = src.condition_on_observations(s["x"][n:], s["y"][n:])
    ops.check_deferred()
    with torch.no_grad():
        kb = s["base"].forward(s["x"], s["x"]).double().cpu().numpy()
    noise = float(src.noise.detach()) if type(src) is models.SingleTaskGP else src.noise
    k = s["os"] * kb + noise * np.eye(n + T_NEW)
    _, linv_ld = cpu.ld_factor(k)
    ref = cpu.ld_cache(linv_ld, s["y"].cpu().numpy(), s["mean"], n + T_NEW)
    return s, src, before, new, ref, float(np.linalg.cond(k))


@pytest.mark.parametrize("name", SETUPS)
def test_conditioned_caches_within_the_bound_of_the_reference(name):
    s, src, before, new, ref, cond = conditioned(name)
    n = s["n"]
    assert type(new) is type(src) and new is not src
    assert tuple(new.train_x.shape) == (n + T_NEW, s["x"].shape[1]) and torch.equal(new.train_x, s["x"]) and torch.equal(new.train_y, s["y"])
    linv, alpha = new._cache[0], new._cache[1]
    assert _cache(new) is new._cache, "the prefilled cache must be what the model serves"
    linv_t, kinv = models._held(new, "_cache_linv_t"), models._held(new, "_cache_kinv")
    assert linv_t is not None and np.array_equal(bits(linv_t), bits(linv.t().contiguous()))
    assert (kinv is None) == (before["kinv"] is None) == (n > _lib.GABO_GP_FACTOR_MAX_N)
    for label, g, r in (("linv", linv, ref[0]), ("alpha", alpha, ref[1])) + ((("kinv", kinv, ref[2]),) if kinv is not None else ()):
        err = float(np.max(np.abs(g.cpu().numpy() - r)))
        print(f"{name} cond {cond:.3g} {label}: error / bound {err / cpu.bound(cond, r):.3f}")
        assert err <= cpu.bound(cond, r), label
    if type(new) is models.SingleTaskGP:
        assert new.covar_module is src.covar_module and new.raw_noise is src.raw_noise and new.mean_constant is src.mean_constant
    else:
        assert new.base_kernel is src.base_kernel and (new.outputscale, new.noise, new.mean) == (src.outputscale, src.noise, src.mean)


@pytest.mark.parametrize("name", SETUPS)
def test_training_factors_follow_the_concatenated_set(name):
    s, src, before, new, _, _ = conditioned(name)
    had = before["held"]["_cache_factors"] is not None and before["held"]["_cache_factors"][1] is not None
    assert had == (name == "exact_ai_d3_n12")
    factors = models._held(new, "_cache_factors")
    assert (factors is not None) == had
    if had:
        want = ops.spd_acq_prepare_train(s["x"])
        ops.check_deferred()
        assert np.array_equal(bits(factors), bits(want))


@pytest.mark.parametrize("name", SETUPS)
def test_original_model_is_untouched(name):
    _, src, before, _, _, _ = conditioned(name)
    assert src._cache is before["cache"]
    for k, v in before["held"].items():
        assert getattr(src, k, None) is v, k
    assert np.array_equal(bits(src._cache[0]), bits(before["linv"])) and np.array_equal(bits(src._cache[1]), bits(before["alpha"]))
    if before["kinv"] is not None:
        assert np.array_equal(bits(models._held(src, "_cache_kinv")), bits(before["kinv"]))
    assert src.train_x.shape[0] == setup(name)["n"]


@pytest.mark.parametrize("name", SETUPS)
def test_posterior_and_forward_agree_with_a_fresh_model_on_the_concatenated_data(name):
    """Both caches are within cpu.bound of the same reference, so the two means differ by at most 2 os sum|k*| bound(alpha) and the two
    variances by at most 2 . 2 |v|_1 os |k*|_1 bound(linv) (v = os linv k*), each plus the rounding of its own sums ((n + 8) and (2 n + 8) units
    per side, as tests/test_gpu_gp_posterior.py derives them)."""
    s, src, _, new, ref, cond = conditioned(name)
    fresh = s["make"](s["x"], s["y"])
    rng = np.random.default_rng(5)
    xq = s["x"][rng.permutation(s["x"].shape[0])[:6]]
    if s["post"] is None:
        xq = torch.nn.functional.normalize(xq + 0.3 * t(rng.standard_normal(tuple(xq.shape))), dim=-1)
    else:
        xq = 0.5 * (xq + xq.flip(0))               # (midpoints of SPD matrices are SPD; Mandel vectors are linear in the matrix)
    with torch.no_grad():
        ks = s["os"] * np.abs(s["base"].forward(xq, s["x"]).double().cpu().numpy())
    m = s["x"].shape[0]
    a_ref, l_ref = np.asarray(ref[1], dtype=np.float64), np.asarray(ref[0], dtype=np.float64)
    mscale = abs(s["mean"]) + ks @ np.abs(a_ref)
    vabs = ks @ np.abs(l_ref).T
    tol_m = 2 * ks.sum(1) * cpu.bound(cond, a_ref) + 2 * (m + 8) * EPS * mscale
    tol_v = 4 * vabs.sum(1) * ks.sum(1) * cpu.bound(cond, l_ref) + 2 * (2 * m + 8) * EPS * (s["os"] + (vabs * vabs).sum(1))
    for how in ("posterior", "forward"):
        if how == "posterior":
            (m1, v1), (m2, v2) = new.posterior(xq), fresh.posterior(xq)
        else:
            p1, p2 = new(xq), fresh(xq)
            (m1, v1), (m2, v2) = (p1.mean, torch.diagonal(p1.covariance_matrix)), (p2.mean, torch.diagonal(p2.covariance_matrix))
        dm, dv = (m1 - m2).abs().cpu().numpy(), (v1 - v2).abs().cpu().numpy()
        print(f"{name} {how}: mean worst / tolerance {float(np.max(dm / tol_m)):.3f}, variance {float(np.max(dv / tol_v)):.3f}")
        assert np.all(dm <= tol_m) and np.all(dv <= tol_v), how


@pytest.mark.parametrize("name", SETUPS)
def test_chained_calls_give_the_bits_of_one_call(name):
    s, src, _, new, _, _ = conditioned(name)
    n = s["n"]
    for targets in (True, False):
        y = (lambda a, b: s["y"][a:b]) if targets else (lambda a, b: None)
        one = new if targets else src.condition_on_observations(s["x"][n:])
        chain = src.condition_on_observations(s["x"][n:n + 1], y(n, n + 1)).condition_on_observations(s["x"][n + 1:], y(n + 1, n + T_NEW))
        ops.check_deferred()
        assert torch.equal(chain.train_x, one.train_x) and np.array_equal(bits(chain.train_y), bits(one.train_y))
        for i in range(2):
            assert np.array_equal(bits(chain._cache[i]), bits(one._cache[i])), (targets, i)
        for k in ("_cache_linv_t", "_cache_kinv", "_cache_factors"):
            a, b = models._held(chain, k), models._held(one, k)
            assert (a is None) == (b is None) and (a is None or np.array_equal(bits(a), bits(b))), (targets, k)


@pytest.mark.parametrize("name", SETUPS)
def test_believer_pins_the_latent_variance_at_the_new_points(name):
    s, src, _, _, _, _ = conditioned(name)
    n = s["n"]
    mu_before, _ = src.posterior(s["x"][n:n + 1])
    bel = src.condition_on_observations(s["x"][n:n + 1])
    ops.check_deferred()
    assert np.array_equal(bits(bel.train_y[:n]), bits(s["y"][:n])) and bel.train_y.device == s["x"].device
    mu, var = bel.posterior(s["x"][n:n + 1])
    print(f"{name}: latent variance at the believer's point {float(var):.3e} (noise {s['noise']:.1e})")
    assert float(var) <= s["noise"] * (1 + 1e-6)
    # the fantasy is the posterior mean: the same sum in another order, (n + 8) units of its terms per side
    with torch.no_grad():
        ks = s["os"] * np.abs(s["base"].forward(s["x"][n:n + 1], s["x"][:n]).double().cpu().numpy())
    scale = abs(s["mean"]) + float((ks @ np.abs(src._cache[1].cpu().numpy())).sum())
    assert abs(float(bel.train_y[n]) - float(mu_before)) <= 2 * (n + 8) * EPS * scale


@pytest.mark.parametrize("name", SETUPS)
def test_fused_acquisition_takes_the_conditioned_model_like_its_source(name):
    s, src, _, new, _, _ = conditioned(name)
    best = float(s["y"].min())
    f_src = FusedAcquisition.build(models.ExpectedImprovement(src, best_f=best, maximize=False), s["post"], DEV)
    f_new = FusedAcquisition.build(models.ExpectedImprovement(new, best_f=best, maximize=False), s["post"], DEV)
    assert f_src is not None and f_new is not None and f_new.single_launch == f_src.single_launch
    assert f_src.single_launch, "every set-up here is one the single-launch evaluators cover"
    assert f_new.linv_t is models._held(new, "_cache_linv_t")
    if name == "exact_ai_d3_n12":
        assert f_new.train_factors is models._held(new, "_cache_factors") and f_new.kinv is models._held(new, "_cache_kinv")


def test_a_failed_update_drops_all_four_caches_of_the_conditioned_model_only():
    s, src, before, _, _, _ = conditioned("exact_ai_d3_n12")
    bad = src.condition_on_observations(s["x"][:1], s["y"][:1])        # a training point again: lambda^2 = noise-sized but positive ...
    ops.check_deferred()
    assert bad._cache is not None
    sick = models.ExactGP(src.train_x, src.train_y, src.base_kernel, outputscale=src.outputscale, noise=-0.5, mean=src.mean)
    models._install_caches(sick, src._cache, models._held(src, "_cache_linv_t"), models._held(src, "_cache_kinv"), models._held(src, "_cache_factors"))
    worse = sick.condition_on_observations(s["x"][:1])                  # ... and with a negative noise it is not
    with pytest.raises(RuntimeError, match="gabo_gp_condition"):
        ops.check_deferred()
    assert worse._cache is None and worse._cache_linv_t is None and worse._cache_kinv is None and worse._cache_factors is None
    assert sick._cache is src._cache is before["cache"]
