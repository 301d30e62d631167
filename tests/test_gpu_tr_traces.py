"""The HIP path against the reference solvers' get_hessianfd values and per-iteration traces (tests/golden/tr_traces.npz; see
tests/test_tr_traces_cpu.py for what the fixture holds and how "f32" / "f64" differ).  Needs an MI355X.

  * Hessian-vector products: autograd through the HIP kernels + HIP manifold operations, <= 1e-8 of the reference's fp64 run;
  * the generic lock-step path with HIP kernels and HIP manifold operations follows the reference iterate by iterate;
  * the device-resident plans (tCG launches, propose/update launches, single-launch solve) follow the reference iterate by iterate as
    well (round 5, after their finite-difference step was corrected to the reference's 2^-14) and end on its fp64 optima within 1e-8
    relative at the size of config 4 (S^5_++, 50 terms, lambda_max bound), unconstrained and constrained."""
import functools

import numpy as np
import pytest
import torch

from gabotorch_amd import _lib, manifolds, models, ops
from gabotorch_amd.kernel_utils.kernels_spd import SpdAffineInvariantGaussianKernel
from gabotorch_amd.manifold_optimization.batched_trust_regions import BatchedProblem
from gabotorch_amd.manifold_optimization.constrained_trust_regions import ConstrainedTrustRegions, StrictConstrainedTrustRegions
from gabotorch_amd.manifold_optimization.manifold_optimize import gen_candidates_manifold
from gabotorch_amd.manifold_optimization.robust_trust_regions import TrustRegions
from gabotorch_amd.Riemannian_utils import spd_constraints_utils_torch as scut
from gabotorch_amd.Riemannian_utils.spd_utils_torch import (symmetric_matrix_to_vector_mandel_torch,
                                                            vector_to_symmetric_matrix_mandel_torch)
from oracle import spd as ospd
from tests._traces import compare_with_reference_trace

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def t(x):
    return torch.tensor(np.ascontiguousarray(x), dtype=torch.float64, device=DEV)


def _problem(g, name, approx):
    if name.startswith("sph"):
        n = int(name[3:])
        Y, w, beta = t(g[f"{name}_Y"]), t(g[f"{name}_w"]), float(g[f"{name}_beta"])
        return BatchedProblem(manifolds.Sphere(n), lambda x: -(ops.sphere_kernel(x, Y, beta) * w).sum(-1), approx_hessian=approx)
    d = int(name.rstrip("c")[3:])
    Ym = t(ospd.symmetric_matrix_to_vector_mandel(g[f"{name}_Y"]))
    w, beta = t(g[f"{name}_w"]), float(g[f"{name}_beta"])

    def cost(x):                                     # x: R x d x d matrices (the solver's representation)
        return -(ops.spd_ai_kernel(symmetric_matrix_to_vector_mandel_torch(x), Ym, beta) * w).sum(-1)
    return BatchedProblem(manifolds.PositiveDefinite(d), cost, approx_hessian=True)


@pytest.mark.parametrize("name", ["sph3", "sph5", "spd2", "spd3", "spd5"])
def test_get_hessianfd_through_the_hip_kernels(golden, name):
    g = golden("tr_traces.npz")
    prob = _problem(g, name, True)
    x, a = t(g[f"{name}_x0"]), t(g[f"{name}_hv_a"])
    f, grad = prob.cost_grad(x)
    np.testing.assert_allclose(f.cpu().numpy(), g[f"{name}_hv_cost_f64"], rtol=1e-12)
    gref = g[f"{name}_hv_grad_f64"]
    assert np.max(np.abs(grad.cpu().numpy() - gref)) < 1e-11 * np.abs(gref).max()
    hv = prob.hess(x, a, grad_x=grad).cpu().numpy()
    ref64 = g[f"{name}_hv_fd_f64"]
    scale = np.abs(ref64).reshape(len(ref64), -1).max(1).reshape((-1,) + (1,) * (ref64.ndim - 1))
    assert np.max(np.abs(hv - ref64) / scale) < 1e-8


@pytest.mark.parametrize("name,run,cls,kw", [
    ("sph5", "tr_exact", TrustRegions, {}), ("sph5", "tr_fd", TrustRegions, {}),
    ("sph3", "con", ConstrainedTrustRegions, {"mingradnorm": 1e-6, "maxiter": 100}),
    ("spd3", "tr_fd", TrustRegions, {"mingradnorm": 1e-4, "maxiter": 100}),
    ("spd5", "tr_fd", TrustRegions, {"mingradnorm": 1e-4, "maxiter": 100}),
    ("spd3", "con", ConstrainedTrustRegions, {"mingradnorm": 1e-4, "maxiter": 100}),
    ("spd5c", "con", ConstrainedTrustRegions, {"mingradnorm": 1e-4, "maxiter": 100}),
])
def test_generic_path_on_hip_kernels_follows_the_reference_trace(golden, name, run, cls, kw):
    g = golden("tr_traces.npz")
    prob = _problem(g, name, approx=(run == "tr_fd" or name.startswith("spd")))
    solver = cls(**kw)
    solver.trace = []
    constrained = run in ("con", "strict")
    x0 = t(g[f"{name}_con_x0"] if (constrained and name.startswith("sph")) else g[f"{name}_x0"])
    ok = g[f"{name}_{run}_f64_ok"]
    ops.set_error_checking(False)
    try:
        if constrained:
            if name.startswith("sph"):
                cons = [lambda x: x[..., 0] - 0.3]
            else:
                mx = float(g[f"{name}_maxeig"])
                cons = [lambda x: scut.max_eigenvalue_constraint_torch(x, mx)]
            x = solver.solve(prob, x0, ineq_constraints=cons)
        else:
            x = solver.solve(prob, x0)
    finally:
        ops.set_error_checking(True)
    res = compare_with_reference_trace(solver.trace, g, f"{name}_{run}_f64", atol_x=1e-6)
    for s, (agree, nit, worst, parted_at, drift) in enumerate(res):
        if ok[s]:
            assert agree == nit, (name, run, s, agree, nit, worst, parted_at, drift)
    np.testing.assert_allclose(x.cpu().numpy()[ok], g[f"{name}_{run}_f64_x"][ok], rtol=0, atol=1e-6)
    np.testing.assert_allclose(prob.cost(x).cpu().numpy()[ok], g[f"{name}_{run}_f64_f"][ok], rtol=1e-8, atol=1e-12)


@pytest.mark.parametrize("name", ["spd2", "spd3", "spd5", "spd5c"])
def test_device_resident_plans_reach_the_reference_fp64_optima(golden, name):
    """cost(x) = -sum_j w_j exp(-beta d_AI(x, Y_j)^2) is the posterior mean of a GP with alpha = w: the fused acquisition kernels and
    the device-resident trust regions (propose/update launches; the single-launch solve with the constraint built by functools.partial
    as in examples/gabo_spd.py:136-138) against the END POINTS of the reference's solvers run in fp64."""
    g = golden("tr_traces.npz")
    d = int(name.rstrip("c")[3:])
    Y = ospd.symmetric_matrix_to_vector_mandel(g[f"{name}_Y"])
    w, beta, mx = g[f"{name}_w"], float(g[f"{name}_beta"]), float(g[f"{name}_maxeig"])
    kern = SpdAffineInvariantGaussianKernel(beta_min=0.1).double()
    kern.beta = torch.tensor(beta, dtype=torch.float64)
    gp = models.ExactGP(t(Y), t(np.zeros(len(w))), kern, outputscale=1.0, noise=1.0, mean=0.0)
    gp._cache = (torch.eye(len(w), dtype=torch.float64, device=DEV), t(w))          # posterior mean = sum_j w_j k(x, Y_j)
    acq = models.PosteriorMean(gp, maximize=True)                                      # cost = -acq = the golden cost
    man = manifolds.PositiveDefinite(d)
    pre, post = vector_to_symmetric_matrix_mandel_torch, symmetric_matrix_to_vector_mandel_torch
    partial = [functools.partial(scut.max_eigenvalue_constraint_torch, maximum_eigenvalue=mx)]
    opaque = [lambda m: scut.max_eigenvalue_constraint_torch(m, mx)]
    x0 = ops.matrix_to_mandel(t(g[f"{name}_x0"]))[:, None]
    rel = lambda a, b: np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-3))            # noqa: E731
    ops.set_error_checking(False)
    try:
        for opts in ({}, {"device_solve": False}, {"device_solve": False, "hip_graphs": True}):
            c, v = gen_candidates_manifold(x0, acq, man, TrustRegions(mingradnorm=1e-4, maxiter=100), pre, post, approx_hessian=True,
                                           options=opts)
            ok = g[f"{name}_tr_fd_f64_ok"]
            assert rel(-v.cpu().numpy()[ok], g[f"{name}_tr_fd_f64_f"][ok]) < 1e-8, (name, opts)
        ok = g[f"{name}_con_f64_ok"]
        # restarts the reference brought to |grad| < mingradnorm and restarts it stopped at maxiter = 100 while they crawl along the bound
        # (compared mid-trajectory) alike: 1e-8.  (Rounds 1-4: 1e-5 and 1e-3, "the device kernels evaluate the same formulas in another
        # order" - they evaluated the finite differences at twice the reference's step.)
        conv = ok & (g[f"{name}_con_f64_nit"] < 100)
        for cons in (partial, opaque):
            c, v = gen_candidates_manifold(x0, acq, man, ConstrainedTrustRegions(mingradnorm=1e-4, maxiter=100), pre, post,
                                           inequality_constraints=cons, approx_hessian=True)
            if conv.any():
                assert rel(-v.cpu().numpy()[conv], g[f"{name}_con_f64_f"][conv]) < 1e-8, (name, "con", cons is partial)
            assert rel(-v.cpu().numpy()[ok], g[f"{name}_con_f64_f"][ok]) < 1e-8, (name, "con at maxiter", cons is partial)
        ok = g[f"{name}_strict_f64_ok"]
        for cons in (partial, opaque):
            strict = StrictConstrainedTrustRegions(mingradnorm=2e-4, maxiter=100, minstepsize=1e-4)
            c, v = gen_candidates_manifold(x0, acq, man, strict, pre, post, inequality_constraints=cons, approx_hessian=True)
            lam = np.linalg.eigvalsh(ospd.vector_to_symmetric_matrix_mandel(c[:, 0].cpu().numpy()))
            assert lam.max() <= mx + 1e-9                                            # the strict solver never leaves the feasible set
            # strict runs crawl along the bound with rounding-decided accept/reject steps (tests/test_tr_traces_cpu.py): end costs of
            # two such runs agree to the progress of a few of those steps when they are cut off at maxiter, to 1e-5 when they converge
            sconv = ok & (g[f"{name}_strict_f64_nit"] < 100)
            if sconv.any():
                assert rel(-v.cpu().numpy()[sconv], g[f"{name}_strict_f64_f"][sconv]) < 1e-5, (name, "strict", cons is partial)
            assert rel(-v.cpu().numpy()[ok], g[f"{name}_strict_f64_f"][ok]) < 2e-3, (name, "strict at maxiter", cons is partial)
    finally:
        ops.set_error_checking(True)


@pytest.mark.parametrize("plan", ["tcg_launches", "propose_update_launches", "single_launch_solve", "single_launch_solve_no_shortcuts"])
@pytest.mark.parametrize("name,run", [("spd3", "tr_fd"), ("spd5", "tr_fd"), ("spd2", "tr_fd"), ("spd3", "con"), ("spd5c", "con"),
                                      ("spd3", "strict"), ("spd5c", "strict")])
def test_device_plans_follow_the_reference_trace(golden, name, run, plan):
    """The device-resident plans - the tCG launches (gabo_spd_tcg_begin / _fd_point / _step / _end around the fused acquisition evaluation)
    and the two launches per iteration (gabo_spd_tr_propose / _update: whitened coordinates, another eigen-solver, another summation order
    than the reference's numpy) - walked against the REFERENCE solver's own fp64 record iteration by iteration: radius (exact), tCG stop
    reason, iterate within 1e-6, like the generic path above - and the single-launch solve (gabo_spd_tr_solve with the eigenvalue bound
    built by functools.partial as in examples/gabo_spd.py:136-138, evaluated inside the kernel), which writes its own record
    (gabo_tr_solve_record) - with its shortcuts on and, "no_shortcuts", off (gabo_spd_tr_shortcuts(0): no value-first evaluation, no step reuse; a
    recording solve never fast-forwards, see test_single_launch_fast_forward_ends_where_the_recorded_run_ends).  Round 5: the kernels' finite-difference
    step had been 2^-13 instead of approximate_hessian.py:40's 2^-14 - 1e-4 of H delta, enough to reach the same optima by other iterates."""
    from tests.test_gpu_solve_shortcuts import switches
    g = golden("tr_traces.npz")
    d = int(name.rstrip("c")[3:])
    Y = ospd.symmetric_matrix_to_vector_mandel(g[f"{name}_Y"])
    w, beta, mx = g[f"{name}_w"], float(g[f"{name}_beta"]), float(g[f"{name}_maxeig"])
    kern = SpdAffineInvariantGaussianKernel(beta_min=0.1).double()
    kern.beta = torch.tensor(beta, dtype=torch.float64)
    gp = models.ExactGP(t(Y), t(np.zeros(len(w))), kern, outputscale=1.0, noise=1.0, mean=0.0)
    gp._cache = (torch.eye(len(w), dtype=torch.float64, device=DEV), t(w))          # posterior mean = sum_j w_j k(x, Y_j)
    acq = models.PosteriorMean(gp, maximize=True)                                      # cost = -acq = the golden cost
    man = manifolds.PositiveDefinite(d)
    pre, post = vector_to_symmetric_matrix_mandel_torch, symmetric_matrix_to_vector_mandel_torch
    x0 = ops.matrix_to_mandel(t(g[f"{name}_x0"]))[:, None]
    constrained = run in ("con", "strict")
    if run == "strict":
        solver = StrictConstrainedTrustRegions(mingradnorm=2e-4, maxiter=100, minstepsize=1e-4)
    else:
        solver = (ConstrainedTrustRegions if constrained else TrustRegions)(mingradnorm=1e-4, maxiter=100)
    solver.trace = []
    one_launch = plan.startswith("single_launch_solve")
    if one_launch:
        cons = [functools.partial(scut.max_eigenvalue_constraint_torch, maximum_eigenvalue=mx)] if constrained else None
    else:
        cons = [lambda m: scut.max_eigenvalue_constraint_torch(m, mx)] if constrained else None
    options = {"tcg_launches": {"device_iteration": False}, "propose_update_launches": {"device_solve": False}}.get(plan, {})
    lib = _lib.load()
    ops.set_error_checking(False)
    try:
        with switches(plan != "single_launch_solve_no_shortcuts", lib.gabo_spd_tr_two_waves(-1)):
            gen_candidates_manifold(x0, acq, man, solver, pre, post, inequality_constraints=cons, approx_hessian=True, options=options)
    finally:
        ops.set_error_checking(True)
    assert solver.trace and ("one_launch_solve" in solver.log) == one_launch
    assert ("eta" in solver.trace[0]) == (plan == "tcg_launches")                      # (which plan recorded it)
    ok = g[f"{name}_{run}_f64_ok"]
    res = compare_with_reference_trace(solver.trace, g, f"{name}_{run}_f64", atol_x=1e-6)
    # (strict runs crawl along the bound with rounding-decided accept / reject steps: as tests/test_tr_traces_cpu.py accepts for the generic path)
    whole = [agree == nit or (run == "strict" and agree >= 30 and drift < 1e-6) for s, (agree, nit, worst, parted_at, drift) in enumerate(res) if ok[s]]
    print(name, run, plan, "restarts followed to the end:", sum(whole), "of", len(whole), [r[:2] for s, r in enumerate(res) if ok[s] and r[0] != r[1]])
    assert all(whole), [(s,) + r for s, r in enumerate(res) if ok[s] and r[0] != r[1]]


@pytest.mark.parametrize("name,run", [("spd3", "con"), ("spd5c", "con"), ("spd3", "strict"), ("spd5c", "strict")])
def test_single_launch_fast_forward_ends_where_the_recorded_run_ends(golden, name, run):
    """A solve that writes its record (gabo_tr_solve_record) runs every rejected iteration; one that does not applies runs of rejections with an
    unchanged first tCG step as scalar updates (tr_repeat_rejected: one more iteration, the radius quartered).  The restarts of these runs reject
    4-97 proposals in a row down to radii of 1e-58.  The recorded run follows the reference's fp64 record iteration by iteration, radius exact
    (test_device_plans_follow_the_reference_trace); the run without the record must end in its state bit for bit - iterate, cost, gradient norm,
    radius, iteration count - with the fast-forward shown to have run, and on the reference's iteration counts exactly."""
    from tests.test_gpu_solve_shortcuts import FAST_FORWARDED, new_counters, switches
    g = golden("tr_traces.npz")
    d = int(name.rstrip("c")[3:])
    Y = ospd.symmetric_matrix_to_vector_mandel(g[f"{name}_Y"])
    w, beta, mx = g[f"{name}_w"], float(g[f"{name}_beta"]), float(g[f"{name}_maxeig"])
    kern = SpdAffineInvariantGaussianKernel(beta_min=0.1).double()
    kern.beta = torch.tensor(beta, dtype=torch.float64)
    gp = models.ExactGP(t(Y), t(np.zeros(len(w))), kern, outputscale=1.0, noise=1.0, mean=0.0)
    gp._cache = (torch.eye(len(w), dtype=torch.float64, device=DEV), t(w))          # posterior mean = sum_j w_j k(x, Y_j)
    acq = models.PosteriorMean(gp, maximize=True)
    man = manifolds.PositiveDefinite(d)
    x0 = ops.matrix_to_mandel(t(g[f"{name}_x0"]))[:, None]
    cons = [functools.partial(scut.max_eigenvalue_constraint_torch, maximum_eigenvalue=mx)]
    lib = _lib.load()
    counters = new_counters()
    out = []
    for recorded in (True, False):
        if run == "strict":
            solver = StrictConstrainedTrustRegions(mingradnorm=2e-4, maxiter=100, minstepsize=1e-4)
        else:
            solver = ConstrainedTrustRegions(mingradnorm=1e-4, maxiter=100)
        if recorded:
            solver.trace = []
        ops.set_error_checking(False)
        try:
            with switches(True, lib.gabo_spd_tr_two_waves(-1), counters):
                c, v = gen_candidates_manifold(x0, acq, man, solver, vector_to_symmetric_matrix_mandel_torch, symmetric_matrix_to_vector_mandel_torch,
                                               inequality_constraints=cons, approx_hessian=True)
                cnt = counters.cpu().tolist()
        finally:
            ops.set_error_checking(True)
        assert solver.log.get("one_launch_solve")
        log = solver.log
        out.append(({"x": c.cpu().numpy(), "value": v.cpu().numpy(), "final_cost": log["final_cost"].cpu().numpy(),
                     "final_gradnorm": log["final_gradnorm"].cpu().numpy(), "final_radius": log["final_radius"].cpu().numpy(),
                     "per_restart_iterations": log["per_restart_iterations"].cpu().numpy()}, cnt, solver.trace))
    (rec, c_rec, trace), (ff, c_ff, _) = out
    print(name, run, "recorded", c_rec, "not recorded", c_ff, "radii", ff["final_radius"])
    assert trace and c_rec[FAST_FORWARDED] == 0 and c_ff[FAST_FORWARDED] > 0, (c_rec, c_ff)
    for k in rec:
        np.testing.assert_array_equal(ff[k], rec[k], err_msg=k)
    ok = g[f"{name}_{run}_f64_ok"]
    np.testing.assert_array_equal(ff["per_restart_iterations"][ok], g[f"{name}_{run}_f64_nit"][ok])


@pytest.mark.parametrize("name,run,kw", [("sph5", "tr_exact", {}), ("sph5", "tr_fd", {}), ("sph3", "tr_exact", {}), ("sph3", "tr_fd", {}),
                                         ("sph3", "con", {"mingradnorm": 1e-6, "maxiter": 100}),
                                         ("sph5", "con", {"mingradnorm": 1e-6, "maxiter": 100}),
                                         ("sph3", "strict", {"mingradnorm": 1e-6, "maxiter": 100}),
                                         ("sph5", "strict", {"mingradnorm": 1e-6, "maxiter": 100})])
@pytest.mark.parametrize("plan", ["propose_update_launches", "single_launch_solve"])
def test_sphere_device_plan_follows_the_reference_trace(golden, name, run, kw, plan):
    """The same for the sphere: gabo_sphere_tr_propose / _update (closed-form exact Hessian-vector products or the finite-difference ones,
    the constraint callable evaluated between the launches) and the single-launch gabo_sphere_tr_solve (unconstrained runs; its own
    record, gabo_tr_solve_record) against the reference solvers' fp64 record."""
    if plan == "single_launch_solve" and run in ("con", "strict"):
        pytest.skip("the sphere has no built-in constraints: constrained sweeps run the propose / update launches")
    from gabotorch_amd.kernel_utils.kernels_sphere import SphereGaussianKernel
    g = golden("tr_traces.npz")
    if f"{name}_{run}_f64_xs" not in g:
        pytest.skip("the fixture holds no such run")
    n = int(name[3:])
    Y, w, beta = g[f"{name}_Y"], g[f"{name}_w"], float(g[f"{name}_beta"])
    kern = SphereGaussianKernel(beta_min=0.1).double()
    kern.beta = torch.tensor(beta, dtype=torch.float64)
    gp = models.ExactGP(t(Y), t(np.zeros(len(w))), kern, outputscale=1.0, noise=1.0, mean=0.0)
    gp._cache = (torch.eye(len(w), dtype=torch.float64, device=DEV), t(w))
    acq = models.PosteriorMean(gp, maximize=True)
    constrained = run in ("con", "strict")
    solver = (StrictConstrainedTrustRegions if run == "strict" else ConstrainedTrustRegions if constrained else TrustRegions)(**kw)
    solver.trace = []
    x0 = t(g[f"{name}_con_x0"] if constrained else g[f"{name}_x0"])[:, None]
    cons = [lambda p: p[..., 0] - 0.3] if constrained else None
    gen_candidates_manifold(x0, acq, manifolds.Sphere(n), solver, inequality_constraints=cons, approx_hessian=(run == "tr_fd"),
                            options={} if plan == "single_launch_solve" else {"device_solve": False})
    assert solver.trace and ("one_launch_solve" in solver.log) == (plan == "single_launch_solve") and "eta" not in solver.trace[0]
    ok = g[f"{name}_{run}_f64_ok"]
    res = compare_with_reference_trace(solver.trace, g, f"{name}_{run}_f64", atol_x=1e-6)
    whole = [agree == nit or (run == "strict" and agree >= 30 and drift < 1e-6) for s, (agree, nit, worst, parted_at, drift) in enumerate(res) if ok[s]]
    print(name, run, plan, "restarts followed to the end:", sum(whole), "of", len(whole), [r[:2] for s, r in enumerate(res) if ok[s] and r[0] != r[1]])
    assert all(whole), [(s,) + r for s, r in enumerate(res) if ok[s] and r[0] != r[1]]


@pytest.mark.parametrize("plan", ["generic_on_hip_kernels", "propose_update_launches"])
@pytest.mark.parametrize("name,run", [("sph3", "eq"), ("sph5", "eq"), ("sph3", "eq_fd"), ("sph5", "eq_fd"), ("sph3", "eqoff"), ("sph5", "eqoff"),
                                      ("sph3", "eq_strict"), ("sph5", "eq_strict")])
def test_equality_constraints_follow_the_reference_trace(golden, name, run, plan):
    """EQUALITY constraints on the sphere (gabo_sphere_equality_constraints.py:100-118: the great circle x[1] = yc; tests/golden/
    tr_traces_eq.npz holds the reference's ConstrainedTrustRegions / StrictConstrainedTrustRegions records, 100 outer iterations each, from
    starts on the constraint and off it): the generic lock-step path on the HIP kernels and the device plan (gabo_sphere_tr_propose /
    _update, the constraint callable evaluated between the launches, neq = 1 inside the tCG) against them iteration by iteration."""
    from gabotorch_amd.kernel_utils.kernels_sphere import SphereGaussianKernel
    from tests.test_tr_traces_cpu import eq_run_setup
    g, ge = golden("tr_traces.npz"), golden("tr_traces_eq.npz")
    cls, kw, x0, cons, fd = eq_run_setup(ge, name, run)
    solver = cls(**kw)
    solver.trace = []
    n = int(name[3:])
    if plan == "generic_on_hip_kernels":
        solver.solve(_problem(g, name, approx=fd), t(x0), eq_constraints=cons)
    else:
        kern = SphereGaussianKernel(beta_min=0.1).double()
        kern.beta = torch.tensor(float(g[f"{name}_beta"]), dtype=torch.float64)
        w = g[f"{name}_w"]
        gp = models.ExactGP(t(g[f"{name}_Y"]), t(np.zeros(len(w))), kern, outputscale=1.0, noise=1.0, mean=0.0)
        gp._cache = (torch.eye(len(w), dtype=torch.float64, device=DEV), t(w))
        acq = models.PosteriorMean(gp, maximize=True)
        gen_candidates_manifold(t(x0)[:, None], acq, manifolds.Sphere(n), solver, equality_constraints=cons, approx_hessian=fd)
        assert "eta" not in solver.trace[0] and "one_launch_solve" not in solver.log       # (recorded between the two launches)
    res = compare_with_reference_trace(solver.trace, ge, f"{name}_{run}_f64", atol_x=1e-6)
    ok = ge[f"{name}_{run}_f64_ok"]
    whole = [agree == nit or (run == "eq_strict" and agree >= 30 and drift < 1e-6) for s, (agree, nit, worst, parted_at, drift) in enumerate(res) if ok[s]]
    print(name, run, plan, "restarts followed to the end:", sum(whole), "of", len(whole), [r[:2] for s, r in enumerate(res) if ok[s] and r[0] != r[1]])
    assert all(whole), [(s,) + r for s, r in enumerate(res) if ok[s] and r[0] != r[1]]


@pytest.mark.parametrize("plan", ["generic_on_hip_kernels", "propose_update_launches"])
@pytest.mark.parametrize("run", ["box", "box_strict", "box2", "box2_strict"])
def test_five_bound_constraints_follow_the_reference_trace(golden, run, plan):
    """Several inequality constraints at once - the five bound constraints of gabo_sphere_bound_constraints.py:94-121, and a tighter box with
    two bounds active at the solution (tests/golden/tr_traces_box.npz) - on the generic path over the HIP kernels and on the sphere's device
    plan (five callables evaluated between the launches, the violated subset selected inside the tCG kernel)."""
    from gabotorch_amd.kernel_utils.kernels_sphere import SphereGaussianKernel
    from tests.test_tr_traces_cpu import box_run_setup
    g, gb = golden("tr_traces.npz"), golden("tr_traces_box.npz")
    cls, x0, cons = box_run_setup(gb, run)
    solver = cls(maxiter=100)
    solver.trace = []
    if plan == "generic_on_hip_kernels":
        solver.solve(_problem(g, "sph3", approx=False), t(x0), ineq_constraints=cons)
    else:
        kern = SphereGaussianKernel(beta_min=0.1).double()
        kern.beta = torch.tensor(float(g["sph3_beta"]), dtype=torch.float64)
        w = g["sph3_w"]
        gp = models.ExactGP(t(g["sph3_Y"]), t(np.zeros(len(w))), kern, outputscale=1.0, noise=1.0, mean=0.0)
        gp._cache = (torch.eye(len(w), dtype=torch.float64, device=DEV), t(w))
        gen_candidates_manifold(t(x0)[:, None], models.PosteriorMean(gp, maximize=True), manifolds.Sphere(3), solver, inequality_constraints=cons,
                                approx_hessian=False)
        assert "eta" not in solver.trace[0] and "one_launch_solve" not in solver.log
    res = compare_with_reference_trace(solver.trace, gb, f"sph3_{run}_f64", atol_x=1e-6)
    ok = gb[f"sph3_{run}_f64_ok"]
    whole = [agree == nit or (run.endswith("strict") and agree >= 30 and drift < 1e-6) for s, (agree, nit, worst, parted_at, drift) in enumerate(res) if ok[s]]
    print(run, plan, "restarts followed to the end:", sum(whole), "of", len(whole), [r[:2] for s, r in enumerate(res) if ok[s] and r[0] != r[1]])
    assert all(whole), [(s,) + r for s, r in enumerate(res) if ok[s] and r[0] != r[1]]


@pytest.mark.parametrize("plan", ["generic_on_hip_kernels", "device_tcg_launches"])
@pytest.mark.parametrize("name,run,kw", [("sph3", "rand_exact", {}), ("sph5", "rand_exact", {}), ("sph3", "rand_fd", {}),
                                         ("spd3", "rand_fd", {"mingradnorm": 1e-4, "maxiter": 100})])
def test_use_rand_follows_the_reference_trace(golden, name, run, kw, plan):
    """`use_rand=True` against the reference's own record (tests/golden/tr_traces_rand.npz; the random tCG starts the reference drew are
    replayed): the generic path on the HIP kernels and, on S^d_++, the plan of device-resident tCG launches (gabo_spd_tcg_begin_rand, steps
    without the preconditioner, the Cauchy-point comparison)."""
    from tests.test_tr_traces_cpu import replay_random_starts
    g, gr = golden("tr_traces.npz"), golden("tr_traces_rand.npz")
    solver = TrustRegions(use_rand=True, **kw)
    solver.trace = []
    eta_in = gr[f"{name}_{run}_f64_eta_in"]
    if plan == "generic_on_hip_kernels":
        with replay_random_starts(eta_in, t):
            solver.solve(_problem(g, name, approx=(run == "rand_fd")), t(g[f"{name}_x0"]))
    else:
        if not name.startswith("spd"):
            pytest.skip("use_rand has a device plan on S^d_++ only")
        d = int(name[3:])
        w = g[f"{name}_w"]
        kern = SpdAffineInvariantGaussianKernel(beta_min=0.1).double()
        kern.beta = torch.tensor(float(g[f"{name}_beta"]), dtype=torch.float64)
        gp = models.ExactGP(t(ospd.symmetric_matrix_to_vector_mandel(g[f"{name}_Y"])), t(np.zeros(len(w))), kern, outputscale=1.0, noise=1.0, mean=0.0)
        gp._cache = (torch.eye(len(w), dtype=torch.float64, device=DEV), t(w))
        acq = models.PosteriorMean(gp, maximize=True)
        x0 = ops.matrix_to_mandel(t(g[f"{name}_x0"]))[:, None]
        ops.set_error_checking(False)
        try:
            with replay_random_starts(eta_in, t):
                gen_candidates_manifold(x0, acq, manifolds.PositiveDefinite(d), solver, vector_to_symmetric_matrix_mandel_torch,
                                        symmetric_matrix_to_vector_mandel_torch, approx_hessian=True)
        finally:
            ops.set_error_checking(True)
        assert solver.trace and "eta" in solver.trace[0]                       # (recorded by the plan of tCG launches)
    res = compare_with_reference_trace(solver.trace, gr, f"{name}_{run}_f64", atol_x=1e-6)
    bad = [(s,) + r for s, r in enumerate(res) if r[0] != r[1]]
    assert not bad, bad
