"""SphereRiemannianMaternKernel through the single-launch evaluator, solve and native sweep drivers (the ZONAL instantiations of
csrc/sphere_tr.hip, GABO_OUT_ZONAL).  Needs an MI355X.

  1. the evaluator against a numpy posterior built from tests/_cpu_sphere_zonal.matern_gram and against the lock-step chain, at points that
     include training points and antipodes of training points (c = +-1: f' and f'' are finite and not zero there, nothing is masked);
  2. the single-launch solve, LDS-resident or not, and the propose / update plan against the CPU record tests/golden/sphere_matern_tr.npz;
  3. the native sweeps: two calls against the Python path bit for bit, one call with the device's selection and sampler;
  4. what the entry points refuse;
  5. the geodesic kernels' sweeps against candidates recorded before this file's code existed (tests/golden/sphere_native_pin.npz)."""
import copy
import ctypes
import functools
import importlib.util
import math
import os

import numpy as np
import pytest
import torch

from gabotorch_amd import _lib, manifolds, models, ops
from gabotorch_amd.fused_acquisition import FusedAcquisition
from gabotorch_amd.kernel_utils.kernels_sphere import SphereRiemannianMaternKernel
from gabotorch_amd.manifold_optimization import manifold_optimize as mo
from gabotorch_amd.manifold_optimization.constrained_trust_regions import ConstrainedTrustRegions
from gabotorch_amd.manifold_optimization.manifold_optimize import gen_candidates_manifold, joint_optimize_manifold
from gabotorch_amd.manifold_optimization.robust_trust_regions import TrustRegions
from gabotorch_amd.Riemannian_utils import sphere_constraints_utils_torch as scu
from tests._cpu_sphere_zonal import matern_gram
from tests._traces import compare_with_reference_trace

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = 2.0 ** -52
KAPPA, OS, NOISE = 0.6, 1.5, 1e-2


def t(a):
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device=DEV)


def _golden_module(name):
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", name + ".py")
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ----------------------------------------------------------------------------------------------- 1. the evaluator
def _series_f(x, xtr, dim, nu, levels, order):
    """f^(order) of the series of `levels` terms at the inner products of x and xtr (numpy); one term: the constant kernel, p = [1]"""
    if levels == 1:
        return np.ones((len(x), len(xtr))) if order == 0 else np.zeros((len(x), len(xtr)))
    return matern_gram(x, xtr, KAPPA, nu, levels - 1, order)


def _coefficients(dim, nu, levels):
    return (np.ones(1), dim - 1) if levels == 1 else ops.sphere_matern_coefficients(dim, KAPPA, nu, levels - 1)


_erf = np.vectorize(math.erf)


def _best(y):
    """the incumbent of the evaluator test's EI (minimisation): above every observation, so that the improvement is of order one at every point and
    neither EI nor its gradient underflows where a two-term kernel leaves a posterior deviation of 1e-2"""
    return float(y.max()) + 0.25


def _numpy_acquisition(x, xtr, y, dim, nu, levels, kind):
    """-> (value, Euclidean gradient with k(x, x) held at f(1), cond(K_y)) of out_sign = -1 times EI (minimisation) or the posterior mean"""
    mean, best = float(y.mean()), _best(y)
    ky = OS * _series_f(xtr, xtr, dim, nu, levels, 0) + NOISE * np.eye(len(xtr))
    ks, k1 = OS * _series_f(x, xtr, dim, nu, levels, 0), OS * _series_f(x, xtr, dim, nu, levels, 1)
    sol = np.linalg.solve(ky, np.concatenate([(y - mean)[:, None], ks.T], axis=1))
    alpha, v = sol[:, 0], sol[:, 1:].T                               # v: R x n, K_y^-1 ks
    mu = mean + ks @ alpha
    dmu = (k1 * alpha[None, :]) @ xtr
    cond = float(np.linalg.cond(ky))
    if kind == _lib.GABO_ACQ_POSTERIOR_MEAN:
        return mu, dmu, cond                                          # out_sign * sgn = (-1) * (-1)
    kxx = OS * float(_coefficients(dim, nu, levels)[0].sum())
    var = kxx - (ks * v).sum(1)
    assert (var > 1e-6).all()                                        # (nothing near the clamp at 1e-9)
    dvar = -2.0 * (k1 * v) @ xtr
    sigma = np.sqrt(var)
    u = -(mu - best) / sigma
    pdf, cdf = np.exp(-0.5 * u * u) * 0.3989422804014327, 0.5 * (1.0 + _erf(u * 0.7071067811865476))
    ei = sigma * (pdf + u * cdf)
    return -ei, -((-cdf)[:, None] * dmu + (0.5 * pdf / sigma)[:, None] * dvar), cond


def _evaluation_problem(n, dim):
    rng = np.random.RandomState(100 * n + dim)
    xtr = rng.randn(n, dim)
    xtr /= np.linalg.norm(xtr, axis=1, keepdims=True)
    y = np.sin(3.0 * xtr[:, 0]) + xtr[:, 1] * xtr[:, -1] + 0.5 * xtr[:, -1]
    x = rng.randn(50, dim)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    x[:3] = xtr[[0, n // 2, n - 1]]                                  # three training points themselves ...
    x[3:6] = -xtr[[1, n // 3, n - 2]]                                # ... and the antipodes of three others
    return xtr, y, x


@pytest.mark.parametrize("levels", [1, 2, 3, 32, 129])
@pytest.mark.parametrize("n,dim", [(20, 3), (70, 2), (70, 10), (130, 17)])
def test_evaluator_against_numpy_and_the_lock_step_chain(n, dim, levels):
    """value and gradient within 16 n 2^-52 cond(K_y) x the scale of the quantity (the bound of tests/test_gpu_sphere_matern.py).  n = 20, 70, 130:
    below, above and at two strips per lane; dim 2: series dimension 1, Chebyshev; 1, 2, 3, 32, 129 levels: both loop tails and the cap.  One level
    is the constant kernel, whose gradient IS zero; the Python kernel class starts at two levels, so the lock-step comparison does too."""
    xtr, y, x = _evaluation_problem(n, dim)
    mean, best = float(y.mean()), _best(y)
    X, Xt, xd = t(xtr), t(xtr.T), t(x)
    for nu in (0.5, 2.5, math.inf):
        coeff, sd = _coefficients(dim, nu, levels)
        table = ops.sphere_zonal_table(coeff, sd)
        assert table.shape == (3, levels, 2)
        series = t(table)
        ky = OS * _series_f(xtr, xtr, dim, nu, levels, 0) + NOISE * np.eye(n)
        kinv = np.linalg.inv(ky)
        kinv = t(0.5 * (kinv + kinv.T))
        alpha = t(np.linalg.solve(ky, y - mean))
        lock = None
        if levels >= 2:
            kern = SphereRiemannianMaternKernel(nu=nu, num_levels=levels - 1).double()
            kern.lengthscale = torch.tensor(KAPPA, dtype=torch.float64)
            gp = models.ExactGP(X, t(y), kern, outputscale=OS, noise=NOISE)
        for kind in (_lib.GABO_ACQ_EXPECTED_IMPROVEMENT, _lib.GABO_ACQ_POSTERIOR_MEAN):
            params = _lib.SphereAcqParams(X.data_ptr(), Xt.data_ptr(), alpha.data_ptr(), kinv.data_ptr(), kinv.data_ptr(), n, dim, 0.0,
                                          _lib.GABO_OUT_ZONAL, mean, OS, float(coeff.sum()), best, kind, 0, -1.0, series.data_ptr(), levels, sd)
            val, grad = ops.sphere_acq_eval(xd, params, need_grad=True)
            val, grad = val.cpu().numpy(), grad.cpu().numpy()
            ref_v, ref_g, cond = _numpy_acquisition(x, xtr, y, dim, nu, levels, kind)
            tol = 16 * n * EPS * cond
            tol_v, tol_g = tol * max(1.0, np.abs(ref_v).max()), tol * max(1.0, np.abs(ref_g).max())
            err_v, err_g = np.abs(val - ref_v).max(), np.abs(grad - ref_g).max()
            print(f"n {n} dim {dim} levels {levels} nu {nu} kind {kind}: cond {cond:.2e} value error {err_v:.2e} (tol {tol_v:.2e}) gradient error "
                  f"{err_g:.2e} (tol {tol_g:.2e}) |gradient| at c = +-1 rows {np.abs(grad[:6]).max(1).min():.2e}")
            assert err_v <= tol_v and err_g <= tol_g
            assert np.abs(grad[:6] - ref_g[:6]).max() <= tol_g
            if levels >= 2:
                assert (np.abs(grad[:6]).max(1) > 0.0).all() and (np.abs(ref_g[:6]).max(1) > 0.0).all()
                acq = (models.ExpectedImprovement(gp, best_f=best, maximize=False) if kind == _lib.GABO_ACQ_EXPECTED_IMPROVEMENT
                       else models.PosteriorMean(gp, maximize=False))
                fused = FusedAcquisition.build(acq, None, torch.device(DEV))
                assert fused.series_launch and fused.one_launch and not fused.single_launch and fused.series_levels == levels
                lock = copy.copy(fused)
                lock.series_launch = False                          # the lock-step chain: strip by sphere_zonal_from_inner, gabo_gp_acquisition
                fa, ga = fused.cost_egrad(xd)
                fb, gb = lock.cost_egrad(xd)
                assert torch.equal(fused.cost(xd), fa)
                tangent = lambda g_: g_ - (g_ * xd).sum(-1, keepdim=True) * xd          # noqa: E731
                d_v, d_g = float((fa - fb).abs().max()), float((tangent(ga) - tangent(gb)).abs().max())
                print(f"    against the lock-step chain: value {d_v:.2e} tangential gradient {d_g:.2e}")
                assert d_v <= tol * max(1.0, float(fb.abs().max())) and d_g <= tol * max(1.0, float(tangent(gb).abs().max()))
                assert np.abs(fa.cpu().numpy() - ref_v).max() <= tol_v


# ----------------------------------------------------------------------------------------------- 2. Hessian-vector product and solve
def _record_acq(g, symmetric_inverse=True):
    kern = SphereRiemannianMaternKernel(nu=float(g["nu"]), num_levels=int(g["num_levels"])).double()
    kern.lengthscale = torch.tensor(float(g["lengthscale"]), dtype=torch.float64)
    gp = models.ExactGP(t(g["X"]), t(g["y"]), kern, outputscale=float(g["outputscale"]), noise=float(g["noise"]))
    if not symmetric_inverse:
        gp._train_cache()
        gp._cache_kinv = None          # the two factors L^-1, L^-T instead of A: the solve runs from the caller's workspace
    return models.ExpectedImprovement(gp, best_f=float(g["best_f"]), maximize=False)


@pytest.mark.parametrize("plan", ["lds", "workspace", "propose_update"])
@pytest.mark.parametrize("run", ["fd", "exact", "con"])
def test_device_plans_follow_the_cpu_record(golden, run, plan):
    """every outer iteration of every restart of the CPU record: same radius, same tCG stop reason, iterate within 1e-6 - no exclusions (the record's
    generator kept a problem on which equally valid roundings agree throughout)"""
    g = golden("sphere_matern_tr.npz")
    acq = _record_acq(g, symmetric_inverse=(plan != "workspace"))
    fused = FusedAcquisition.build(acq, None, torch.device(DEV))
    assert fused.series_launch
    resident = _lib.load().gabo_sphere_tr_solve_lds_resident(ctypes.byref(fused.sphere_acq_params()), 8, 1 if run == "con" else 0)
    assert resident == (0 if plan == "workspace" else 1)
    solver = (ConstrainedTrustRegions if run == "con" else TrustRegions)(mingradnorm=1e-6, maxiter=int(g["maxiter"]))
    solver.trace = []
    cons = {}
    if run == "con":
        cons = {"inequality_constraints": [functools.partial(scu.coordinate_lower_bound_constraint_torch, index=0, lower_bound=float(g["lower_bound"]))]}
    x, _ = gen_candidates_manifold(t(g["con_x0"] if run == "con" else g["x0"])[:, None], acq, manifolds.Sphere(3), solver,
                                   approx_hessian=(run == "fd"), options={"device_solve": False} if plan == "propose_update" else {}, **cons)
    if plan == "propose_update":
        assert not solver.log.get("one_launch_solve") and solver.trace and "eta" not in solver.trace[0]      # (the generic plan records eta)
    else:
        assert solver.log["one_launch_solve"] and solver.log["lds_resident"] is (plan == "lds")
    res = compare_with_reference_trace(solver.trace, g, run, atol_x=1e-6)
    print(run, plan, [(agree, nit, f"{worst:.1e}") for agree, nit, worst, _, _ in res])
    for s, (agree, nit, worst, parted_at, drift) in enumerate(res):
        assert agree == nit, (run, plan, s, agree, nit, worst, parted_at, drift)
    last = g[f"{run}_xs"][np.arange(8), g[f"{run}_nit"]]
    np.testing.assert_allclose(x[:, 0].cpu().numpy(), last, rtol=0, atol=1e-6)


def test_lock_step_plan_is_still_reachable(golden):
    g = golden("sphere_matern_tr.npz")
    solver = TrustRegions(mingradnorm=1e-6, maxiter=int(g["maxiter"]))
    solver.trace = []
    gen_candidates_manifold(t(g["x0"])[:, None], _record_acq(g), manifolds.Sphere(3), solver, approx_hessian=True,
                            options={"device_solve": False, "device_iteration": False, "device_tcg": False})
    assert not solver.log.get("one_launch_solve") and "eta" in solver.trace[0]
    res = compare_with_reference_trace(solver.trace, g, "fd", atol_x=1e-6)
    assert all(agree == nit for agree, nit, *_ in res), res


# ----------------------------------------------------------------------------------------------- 3. the plans
def _feasible_sample():
    while True:
        p = np.random.randn(3)
        p /= np.linalg.norm(p)
        if p[0] > 0.35:
            return p


def _sweep(acq, constrained, options, approx, R=16, raw=64):
    np.random.seed(21)
    torch.manual_seed(21)
    man = manifolds.Sphere(3)
    cons = None
    if constrained:
        solver = ConstrainedTrustRegions(maxiter=100)
        man.rand = _feasible_sample
        cons = [functools.partial(scu.coordinate_lower_bound_constraint_torch, index=0, lower_bound=0.3)]
    else:
        solver = TrustRegions(maxiter=100)
    best = joint_optimize_manifold(acq, man, solver, q=1, num_restarts=R, raw_samples=raw, bounds=None, inequality_constraints=cons,
                                   approx_hessian=approx, options=dict(options, device=DEV))
    return best, solver.log


def _raw_samples(raw, dim):
    ws = [v for k, v in mo._sweep_workspaces.items() if k[0] == "sphere"][0]
    return ws[:raw * dim * 8].view(torch.float64).reshape(raw, dim).clone()


@pytest.mark.parametrize("constrained,approx", [(False, True), (False, False), (True, False), (True, True)])
def test_two_call_native_sweep_returns_the_python_path_candidate_bit_for_bit(golden, constrained, approx):
    acq = _record_acq(golden("sphere_matern_tr.npz"))
    best_n, log_n = _sweep(acq, constrained, {"device_selection": False}, approx)
    assert log_n["native_sweep"] is True and log_n["device_selection"] is False and log_n["one_launch_solve"] and log_n["lds_resident"] is True
    best_p, log_p = _sweep(acq, constrained, {"native_sweep": False}, approx)
    assert not log_p.get("native_sweep") and log_p.get("one_launch_solve")
    assert torch.equal(best_n, best_p)
    np.testing.assert_array_equal(log_n["final_cost"].cpu().numpy(), log_p["final_cost"].cpu().numpy())
    np.testing.assert_array_equal(log_n["per_restart_iterations"].cpu().numpy(), log_p["per_restart_iterations"].cpu().numpy())
    assert int(log_n["per_restart_iterations"].max()) > 1
    if constrained:
        assert float(best_n[0, 0]) >= 0.3 - 2e-3


@pytest.mark.parametrize("approx", [True, False])
def test_one_call_native_sweep_with_the_device_selection_and_sampler(golden, approx):
    acq = _record_acq(golden("sphere_matern_tr.npz"))
    best, log = _sweep(acq, False, {"device_selection": True, "device_rand": True}, approx)
    assert log["native_sweep"] is True and log["one_launch_solve"]
    assert best.shape == (1, 3) and abs(float(best.norm()) - 1.0) <= 1e-14
    raw = _raw_samples(64, 3)
    np.testing.assert_allclose(raw.norm(dim=1).cpu().numpy(), 1.0, rtol=0, atol=1e-14)
    ei_best, ei_raw = float(acq(best[None])), float(acq(raw[:, None]).max())
    print(f"approx {approx}: device selection {log['device_selection']}, EI at the candidate {ei_best:.6e}, best raw sample {ei_raw:.6e}")
    assert ei_raw > 0.0 and ei_best >= ei_raw


# ----------------------------------------------------------------------------------------------- 4. argument checking
def test_malformed_series_are_refused_on_the_host(golden):
    lib = _lib.load()
    fused = FusedAcquisition.build(_record_acq(golden("sphere_matern_tr.npz")), None, torch.device(DEV))
    x = t(golden("sphere_matern_tr.npz")["x0"])
    val, grad = torch.zeros(8, dtype=torch.float64, device=DEV), torch.zeros(8, 3, dtype=torch.float64, device=DEV)
    stream = ops._stream_ptr(torch.device(DEV))

    def calls(p):
        ref = ctypes.byref(p)
        return (lib.gabo_sphere_acq_eval(x.data_ptr(), ref, val.data_ptr(), grad.data_ptr(), 8, stream), lib.gabo_sphere_tr_solve_lds_resident(ref, 8, 0))
    good = fused.sphere_acq_params()
    assert good.flags == _lib.GABO_OUT_ZONAL and good.series_levels == 25 and good.series_dim == 2
    assert calls(good) == (_lib.GABO_OK, 1)
    for field, value in (("series", None), ("series_levels", 0), ("series_levels", 130), ("series_dim", 1), ("series_dim", 3)):
        bad = fused.sphere_acq_params()
        setattr(bad, field, value)
        rc = calls(bad)
        assert rc[0] == _lib.GABO_ERR_ARG and rc[1] < 0, (field, value, rc)
    torch.cuda.synchronize()
    # the SPD entries keep refusing the flag
    assert lib.gabo_spd_acq_eval(None, None, None, None, None, None, None, None, 4, 8, 5, 1.0, _lib.GABO_OUT_ZONAL, 0.0, 1.0, 1.0, 0.0, 0, 1, 1.0,
                                 None, None, None) == _lib.GABO_ERR_ARG


# ----------------------------------------------------------------------------------------------- 5. the geodesic kernels
def test_geodesic_sweeps_return_the_candidates_recorded_before(golden):
    """SphereGaussianKernel and SphereLaplaceKernel: native sweeps (one call, two calls, constrained), the Python path and the propose / update plan,
    bit for bit what the parent of the commit that added the series instantiations returned"""
    pin, gen = golden("sphere_native_pin.npz"), _golden_module("make_golden_sphere_native_pin")
    for i, case in enumerate(gen.CASES):
        res = gen.run_case(case)
        for k, v in res.items():
            np.testing.assert_array_equal(v, pin[f"case{i}_{k}"], err_msg=f"case {i} {case}: {k}")
