"""The library's sphere constraints evaluated on the device (csrc/sphere_tr.hip: gabo_sphere_constraints_eval and the constrained
instantiations of the single-launch solve, gabo_sphere_tr_solve_constrained).  Needs an MI355X.

  * the device evaluation against the torch functions + autograd + Sphere.egrad2rgrad;
  * the single launch, driven through gen_candidates_manifold with the library constraints, follows the reference solvers' fp64 records
    (tests/golden/tr_traces.npz, tr_traces_eq.npz, tr_traces_box.npz) iteration by iteration;
  * both instantiations (LDS-resident and caller's workspace) against the propose / update launches on the same constraints;
  * the record only observes; zero constraints are the unconstrained launch; one end-to-end sweep."""
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
from gabotorch_amd.kernel_utils.kernels_sphere import SphereGaussianKernel
from gabotorch_amd.manifold_optimization.constrained_trust_regions import ConstrainedTrustRegions, StrictConstrainedTrustRegions
from gabotorch_amd.manifold_optimization.manifold_optimize import gen_candidates_manifold, joint_optimize_manifold
from gabotorch_amd.Riemannian_utils import sphere_constraints_utils_torch as scu
from tests._traces import compare_with_reference_trace
from tests.test_sphere_constraints_cpu import ball, library_box_constraints, library_eq_constraints, lower, upper

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LO, UP, BALL = _lib.GABO_SPHERE_CONSTRAINT_COORD_LOWER, _lib.GABO_SPHERE_CONSTRAINT_COORD_UPPER, _lib.GABO_SPHERE_CONSTRAINT_GEODESIC_BALL


def t(x):
    return torch.tensor(np.ascontiguousarray(x), dtype=torch.float64, device=DEV)


# ----------------------------------------------------------------------------------------------- 1. device evaluation against torch
def _unit(gen, *shape):
    x = torch.randn(*shape, dtype=torch.float64, generator=gen)
    return x / x.norm(dim=-1, keepdim=True)


def _constraint_set(gen, dim, count, first_kind):
    """`count` constraints, the three kinds in turn starting with `first_kind`, coordinates spread over the lane-stride edges of `dim`"""
    cons = []
    coords = [0, dim - 1, dim // 2, min(63, dim - 1), min(64, dim - 1), 1 % dim]
    for k in range(count):
        kind = (first_kind + k) % 3
        if kind == LO:
            cons.append(lower(coords[k % len(coords)], -0.25 + 0.1 * k))
        elif kind == UP:
            cons.append(upper(coords[(k + 1) % len(coords)], torch.tensor(0.4 - 0.05 * k, dtype=torch.float64)))
        else:
            cons.append(ball(_unit(gen, dim), math.pi / 4 + 0.1 * k))
    return cons


def _torch_reference(cons, x):
    man = manifolds.Sphere(x.shape[-1])
    vals, grads = [], []
    for con in cons:
        xx = x.clone().requires_grad_(True)
        f = con(xx)
        (g,) = torch.autograd.grad(f.sum(), xx)
        vals.append(f.detach())
        grads.append(man.egrad2rgrad(x, g))
    return torch.stack(vals, dim=1), torch.stack(grads)


@pytest.mark.parametrize("dim", [2, 3, 64, 65, 130])
@pytest.mark.parametrize("r", [1, 5, 65])
def test_device_evaluation_against_the_torch_functions(r, dim):
    """Coordinate kinds: the value is one subtraction, bit-equal; gradients within 1e-15.  Ball: 1e-13 - a dozen ulps at values of order 1, the
    device's acos and torch's being different implementations.  The ball's gradient is centre / sin(theta) (theta the angle to the centre), so
    "order 1" is a statement about the points: they are drawn with |<x, centre>| < 0.85 for every centre of the set (1 / sin(theta) < 1.9; a
    rounding of the inner product is amplified by cos / sin^3 < 5.8).  The ends of the interval are test_ball_at_its_centre_and_antipode."""
    gen = torch.Generator().manual_seed(1000 * r + dim)
    for count, first_kind in ((1, LO), (1, UP), (1, BALL), (5, LO), (8, BALL)):
        cons = _constraint_set(gen, dim, count, first_kind)
        centres = [c.keywords["center"] for c in cons if "center" in c.keywords]
        pool = _unit(gen, 400 * r, dim)
        keep = torch.ones(pool.shape[0], dtype=torch.bool)
        for c in centres:
            keep &= (pool @ c).abs() < 0.85
        x = pool[keep][:r].to(DEV)
        assert x.shape[0] == r
        cons = [functools.partial(c.func, **{k: (v.to(DEV) if torch.is_tensor(v) and v.dim() else v) for k, v in c.keywords.items()}) for c in cons]
        group = scu.builtin_sphere_group(cons, dim, x.device)
        assert group is not None and group[0] == [(first_kind + k) % 3 for k in range(count)]
        vals, grads = ops.sphere_constraints_eval(x, *group)
        only = ops.sphere_constraints_eval(x, *group, want_grad=False)
        ref_v, ref_g = _torch_reference(cons, x)
        assert vals.shape == (r, count) and grads.shape == (count, r, dim) and torch.equal(only, vals)
        assert torch.isfinite(vals).all() and torch.isfinite(grads).all()
        for k, kind in enumerate(group[0]):
            dv = float((vals[:, k] - ref_v[:, k]).abs().max())
            dg = float((grads[k] - ref_g[k]).abs().max())
            print(f"r={r} dim={dim} C={count} k={k} kind={kind}: |dvalue| {dv:.2e} |dgrad| {dg:.2e} gradient bit-equal: {torch.equal(grads[k], ref_g[k])}")
            if kind == BALL:
                assert dv <= 1e-13 and dg <= 1e-13, (k, dv, dg)
            else:
                assert torch.equal(vals[:, k], ref_v[:, k]) and dg <= 1e-15, (k, dv, dg)


@pytest.mark.parametrize("dim", [3, 4, 65])
def test_ball_at_its_centre_and_antipode(dim):
    """x = +-centre: <x, centre> = +-1 (centres whose squares sum to exactly 1 in any order), where the gradient is defined as zero"""
    centre = torch.zeros(dim, dtype=torch.float64, device=DEV)
    if dim == 4:
        centre[:] = 0.5
    else:
        centre[dim - 1] = 1.0
    con = ball(centre, 0.3)
    x = torch.stack([centre, -centre])
    vals, grads = ops.sphere_constraints_eval(x, *scu.builtin_sphere_group([con], dim, x.device))
    ref_v, ref_g = _torch_reference([con], x)
    assert torch.isfinite(vals).all() and torch.isfinite(grads).all()
    assert torch.equal(vals, ref_v) and torch.equal(vals[:, 0], t([0.3, 0.3 - math.pi]))
    assert torch.equal(grads, ref_g) and not grads.any()


def test_malformed_calls_are_refused_on_the_host():
    lib = _lib.load()
    ints = lambda *v: (ctypes.c_int * 9)(*v)              # noqa: E731
    dbl = (ctypes.c_double * 9)(*([0.1] * 9))

    def call(n, kinds, idx, dim=3, n_centres=0, centres=None):
        # (r = 0: a well-formed call returns GABO_OK without a launch, so GABO_ERR_ARG is the verdict on the constraint set alone)
        return lib.gabo_sphere_constraints_eval(None, 0, dim, n, kinds, idx, dbl, centres, n_centres, None, None, None)
    assert call(8, ints(*[0] * 8), ints(*[2] * 8)) == _lib.GABO_OK
    assert call(2, ints(BALL, UP), ints(1, 0), n_centres=2, centres=ctypes.c_void_p(8)) == _lib.GABO_OK
    assert call(9, ints(*[0] * 9), ints(*[0] * 9)) == _lib.GABO_ERR_ARG                    # more than 8
    assert call(1, ints(LO), ints(3)) == _lib.GABO_ERR_ARG                                   # coordinate outside [0, dim)
    assert call(1, ints(UP), ints(-1)) == _lib.GABO_ERR_ARG
    assert call(1, ints(BALL), ints(0)) == _lib.GABO_ERR_ARG                                 # no centres
    assert call(1, ints(BALL), ints(2), n_centres=2, centres=ctypes.c_void_p(8)) == _lib.GABO_ERR_ARG      # centre outside [0, n_centres)
    assert call(1, ints(3), ints(0)) == _lib.GABO_ERR_ARG                                    # unknown kind
    acq = _lib.SphereAcqParams(8, 8, 8, 8, 8, 12, 3, 1.0, 0, 0.0, 1.0, 1.0, 0.0, _lib.GABO_ACQ_POSTERIOR_MEAN, 1, -1.0)

    def solve(n, neq, kinds, idx, n_centres=0):
        return lib.gabo_sphere_tr_solve_constrained(None, None, None, None, None, None, None, ctypes.byref(acq), None, 0, 0, 1.0, 0.1, 1, 3, 1, 1.0,
                                                    0.1, 1e3, 1e-6, 10, n, neq, kinds, idx, dbl, None, n_centres, 0, 1e-6, None)
    assert solve(2, 2, ints(LO, UP), ints(0, 1)) == _lib.GABO_OK and solve(0, 0, None, None) == _lib.GABO_OK
    assert solve(9, 0, ints(*[0] * 9), ints(*[0] * 9)) == _lib.GABO_ERR_ARG
    assert solve(2, 3, ints(LO, UP), ints(0, 1)) == _lib.GABO_ERR_ARG                       # more equalities than constraints
    assert solve(1, 0, ints(LO), ints(3)) == _lib.GABO_ERR_ARG
    assert solve(1, 0, ints(BALL), ints(0)) == _lib.GABO_ERR_ARG
    assert solve(1, 0, ints(7), ints(0)) == _lib.GABO_ERR_ARG
    # (one address in both factor slots = the symmetric inverse: 12 points on S^2 and 8 constraints fit the LDS)
    assert lib.gabo_sphere_tr_solve_lds_resident(ctypes.byref(acq), 4, 8) == 1 and lib.gabo_sphere_tr_solve_lds_resident(ctypes.byref(acq), 4, 9) < 0
    assert lib.gabo_sphere_tr_solve_lds_resident(None, 4, 0) < 0


# ----------------------------------------------------------------------------------------------- 2. the reference's records
def _fixture_acq(g, name):
    """the surrogate of the trace fixtures: posterior mean with the weights of the fixture (no symmetric inverse: the caller's workspace)"""
    kern = SphereGaussianKernel(beta_min=0.1).double()
    kern.beta = torch.tensor(float(g[f"{name}_beta"]), dtype=torch.float64)
    w = g[f"{name}_w"]
    gp = models.ExactGP(t(g[f"{name}_Y"]), t(np.zeros(len(w))), kern, outputscale=1.0, noise=1.0, mean=0.0)
    gp._cache = (torch.eye(len(w), dtype=torch.float64, device=DEV), t(w))
    return models.PosteriorMean(gp, maximize=True)


def _follows(solver, g, prefix, strict_run):
    res = compare_with_reference_trace(solver.trace, g, prefix, atol_x=1e-6)
    ok = g[prefix + "_ok"]
    whole = [agree == nit or (strict_run and agree >= 30 and drift < 1e-6) for s, (agree, nit, worst, parted_at, drift) in enumerate(res) if ok[s]]
    print(prefix, "restarts followed to the end:", sum(whole), "of", len(whole), [r[:2] for s, r in enumerate(res) if ok[s] and r[0] != r[1]])
    assert all(whole), [(s,) + r for s, r in enumerate(res) if ok[s] and r[0] != r[1]]


@pytest.mark.parametrize("name,run", [("sph3", "con"), ("sph5", "con"), ("sph3", "strict"), ("sph5", "strict")])
def test_single_launch_follows_the_reference_trace_with_an_inequality(golden, name, run):
    """as test_sphere_device_plan_follows_the_reference_trace (x[0] - 0.3 >= 0), the constraint a library function, the solve ONE launch"""
    g = golden("tr_traces.npz")
    solver = (StrictConstrainedTrustRegions if run == "strict" else ConstrainedTrustRegions)(mingradnorm=1e-6, maxiter=100)
    solver.trace = []
    gen_candidates_manifold(t(g[f"{name}_con_x0"])[:, None], _fixture_acq(g, name), manifolds.Sphere(int(name[3:])), solver,
                            inequality_constraints=[lower(0, 0.3)], approx_hessian=False, options={})
    assert solver.trace and solver.log["one_launch_solve"] and solver.log["lds_resident"] is False
    _follows(solver, g, f"{name}_{run}_f64", run == "strict")


@pytest.mark.parametrize("name,run", [("sph3", "eq"), ("sph5", "eq"), ("sph3", "eq_fd"), ("sph5", "eq_fd"), ("sph3", "eqoff"), ("sph5", "eqoff"),
                                      ("sph3", "eq_strict"), ("sph5", "eq_strict")])
def test_single_launch_follows_the_reference_trace_with_an_equality(golden, name, run):
    """as test_equality_constraints_follow_the_reference_trace (the great circle), neq = 1 inside the single launch"""
    from tests.test_tr_traces_cpu import eq_run_setup
    g, ge = golden("tr_traces.npz"), golden("tr_traces_eq.npz")
    cls, kw, x0, _, fd = eq_run_setup(ge, name, run)
    solver = cls(**kw)
    solver.trace = []
    gen_candidates_manifold(t(x0)[:, None], _fixture_acq(g, name), manifolds.Sphere(int(name[3:])), solver,
                            equality_constraints=library_eq_constraints(run), approx_hessian=fd, options={})
    assert solver.trace and solver.log["one_launch_solve"]
    _follows(solver, ge, f"{name}_{run}_f64", run == "eq_strict")


@pytest.mark.parametrize("run", ["box", "box_strict", "box2", "box2_strict"])
def test_single_launch_follows_the_reference_trace_with_five_bounds(golden, run):
    """as test_five_bound_constraints_follow_the_reference_trace, the violated subset selected inside the single launch"""
    from tests.test_tr_traces_cpu import box_run_setup
    g, gb = golden("tr_traces.npz"), golden("tr_traces_box.npz")
    cls, x0, _ = box_run_setup(gb, run)
    solver = cls(maxiter=100)
    solver.trace = []
    gen_candidates_manifold(t(x0)[:, None], _fixture_acq(g, "sph3"), manifolds.Sphere(3), solver,
                            inequality_constraints=library_box_constraints(run), approx_hessian=False, options={})
    assert solver.trace and solver.log["one_launch_solve"]
    _follows(solver, gb, f"sph3_{run}_f64", run.endswith("strict"))


# ----------------------------------------------------------------------------------------------- 3. both instantiations
@pytest.fixture(scope="module")
def fitted():
    """20 points on S^2, a factored ExactGP (its symmetric inverse in the cache: the LDS-resident instantiation), EI, 8 starts"""
    rng = np.random.RandomState(11)
    X = rng.randn(20, 3)
    X /= np.linalg.norm(X, axis=1, keepdims=True)
    y = np.sin(3.0 * X[:, 0]) + X[:, 1] * X[:, 2] + 0.5 * X[:, 2]
    kern = SphereGaussianKernel(beta_min=0.1).double()
    kern.beta = torch.tensor(6.5, dtype=torch.float64)
    gp = models.ExactGP(t(X), t(y), kern, outputscale=1.0, noise=1e-2)
    acq = models.ExpectedImprovement(gp, best_f=float(y.min()), maximize=False)
    s = rng.randn(8, 3)
    s[:, 0] = np.abs(s[:, 0]) + 0.8
    s /= np.linalg.norm(s, axis=1, keepdims=True)
    return acq, s


def _case(kind, starts):
    if kind == "box2":
        return dict(inequality_constraints=library_box_constraints("box2")), starts
    if kind == "ball":
        return dict(inequality_constraints=[ball(torch.eye(3, dtype=torch.float64)[0], math.pi / 4)]), starts
    on = starts.copy()                                    # the great circle x[1] = 0, started on it
    on[:, 1] = 0.0
    on /= np.linalg.norm(on, axis=1, keepdims=True)
    return dict(equality_constraints=library_eq_constraints("eq")), on


@pytest.mark.parametrize("kind", ["box2", "ball", "circle"])
def test_single_launch_against_the_propose_update_launches(golden, fitted, kind):
    acq, starts = fitted
    cons, x0 = _case(kind, starts)
    lib = _lib.load()
    ncons = sum(len(v) for v in cons.values())
    params = FusedAcquisition.build(acq, None, torch.device(DEV)).sphere_acq_params()
    assert lib.gabo_sphere_tr_solve_lds_resident(ctypes.byref(params), 8, ncons) == 1
    g = golden("tr_traces.npz")
    held = _fixture_acq(g, "sph3")
    fixture = FusedAcquisition.build(held, None, torch.device(DEV)).sphere_acq_params()
    assert lib.gabo_sphere_tr_solve_lds_resident(ctypes.byref(fixture), 8, ncons) == 0
    runs = {}
    for plan, options in (("one", {}), ("two", {"device_solve": False})):
        solver = ConstrainedTrustRegions(mingradnorm=1e-6, maxiter=100)
        solver.trace = []
        x, _ = gen_candidates_manifold(t(x0)[:, None], acq, manifolds.Sphere(3), solver, approx_hessian=False, options=options, **cons)
        assert bool(solver.log.get("one_launch_solve")) == (plan == "one")
        if plan == "one":
            assert solver.log["lds_resident"] is True
        runs[plan] = (x[:, 0], solver.log, solver.trace)
    (xa, la, ta), (xb, lb, tb) = runs["one"], runs["two"]
    assert torch.equal(la["per_restart_iterations"], lb["per_restart_iterations"])
    assert torch.equal(la["final_radius"], lb["final_radius"])
    assert len(ta) == len(tb) == int(la["per_restart_iterations"].max())
    worst, same = float((xa - xb).abs().max()), torch.equal(xa, xb)
    for ka, kb in zip(ta, tb):
        ran = kb["active"]
        assert torch.equal(ka["active"], ran)
        assert torch.equal(ka["stop_inner"][ran], kb["stop_inner"][ran])
        assert torch.equal(ka["Delta"][ran], kb["Delta"][ran])
        worst = max(worst, float((ka["x"][ran] - kb["x"][ran]).abs().max()))
        same = same and torch.equal(ka["x"][ran], kb["x"][ran])
    print(kind, "largest iterate difference", worst, "bit-identical:", same, "iterations", la["per_restart_iterations"].tolist())
    assert worst <= 1e-6
    assert int(la["per_restart_iterations"].max()) > 1


# ----------------------------------------------------------------------------------------------- 4. the record only observes
@pytest.mark.parametrize("strict", [False, True])
def test_the_record_only_observes(golden, strict):
    from tests.test_tr_traces_cpu import box_run_setup
    g, gb = golden("tr_traces.npz"), golden("tr_traces_box.npz")
    cls, x0, _ = box_run_setup(gb, "box2_strict" if strict else "box2")
    ends = []
    for trace in ([], None):
        solver = cls(maxiter=100)
        solver.trace = trace
        x, _ = gen_candidates_manifold(t(x0)[:, None], _fixture_acq(g, "sph3"), manifolds.Sphere(3), solver,
                                       inequality_constraints=library_box_constraints("box2"), approx_hessian=False, options={})
        assert solver.log["one_launch_solve"]
        ends.append((x, solver.log["final_cost"], solver.log["final_gradnorm"], solver.log["final_radius"], solver.log["per_restart_iterations"]))
    for a, b in zip(*ends):
        assert torch.equal(a, b)


# ----------------------------------------------------------------------------------------------- 5. zero constraints
def test_zero_constraints_are_the_unconstrained_launch(golden):
    g = golden("tr_traces.npz")
    acq = _fixture_acq(g, "sph5")
    fused = FusedAcquisition.build(acq, None, torch.device(DEV))
    x0 = t(g["sph5_x0"])
    R, dim = x0.shape
    lib = _lib.load()
    man = manifolds.Sphere(dim)
    ends = []
    for constrained_entry in (False, True):
        TR = ops.SphereTr(R, dim, 0, fused.sphere_acq_params(), x0.device, exact_hessian=False)
        x = x0.clone()
        fx, eg = fused.cost_egrad(x)
        fx, grad = fx.clone(), man.egrad2rgrad(x, eg).contiguous()
        ng = grad.norm(dim=-1)
        Delta = torch.full((R,), man.typicaldist / 8, dtype=torch.float64, device=DEV)
        active = torch.ones(R, dtype=torch.uint8, device=DEV)
        iters = torch.zeros(R, dtype=torch.int64, device=DEV)
        head = (x.data_ptr(), fx.data_ptr(), grad.data_ptr(), ng.data_ptr(), Delta.data_ptr(), active.data_ptr(), iters.data_ptr(), TR.acq_ref,
                TR.ws.data_ptr(), TR.wsb, R, 1.0, 0.1, 1, dim, 0, man.typicaldist, 0.1, 1e3, 1e-6, 1000)
        stream = ops._stream_ptr(x0.device)
        if constrained_entry:
            rc = lib.gabo_sphere_tr_solve_constrained(*head, 0, 0, None, None, None, None, 0, 0, 1e-6, stream)
        else:
            rc = lib.gabo_sphere_tr_solve(*head, stream)
        assert rc == _lib.GABO_OK
        torch.cuda.synchronize()
        ends.append((x, fx, grad, ng, Delta, active, iters))
    assert int(ends[0][6].min()) > 1 and not ends[0][5].any()
    for a, b in zip(*ends):
        assert torch.equal(a, b)


# ----------------------------------------------------------------------------------------------- 6. end to end
def _sweep(acq, cons, options):
    np.random.seed(21)
    torch.manual_seed(21)
    solver = ConstrainedTrustRegions(maxiter=200)
    man = manifolds.Sphere(3)

    def sample():                                      # the constrained sampler the bound example installs (gabo_sphere_bound_constraints.py:123-131)
        while True:
            p = np.array([np.random.uniform(0.0, 1.0), np.random.uniform(-0.6, 0.6), np.random.uniform(-0.6, 0.6)])
            p = p / np.linalg.norm(p)
            if p[0] > 0.0 and -0.6 < p[1] < 0.6 and -0.6 < p[2] < 0.6:
                return p
    man.rand = sample
    best = joint_optimize_manifold(acq, man, solver, q=1, num_restarts=16, raw_samples=64, bounds=None,
                                   inequality_constraints=cons, options=dict(options, device=DEV))
    return best, solver.log


def test_end_to_end_sweep_with_the_five_bounds(fitted):
    acq, _ = fitted
    cons = library_box_constraints("box")
    best, log = _sweep(acq, cons, {})
    assert log.get("one_launch_solve") and best.shape == (1, 3)
    p = best[0].cpu().numpy()
    assert p[0] > 0.0 - 2e-3 and -0.6 - 2e-3 < p[1] < 0.6 + 2e-3 and -0.6 - 2e-3 < p[2] < 0.6 + 2e-3, p       # (the example's feasibility test)
    two, log2 = _sweep(acq, cons, {"device_solve": False})
    assert not log2.get("one_launch_solve")
    graphed, log3 = _sweep(acq, cons, {"hip_graphs": True, "device_solve": False})
    assert not log3.get("one_launch_solve")
    print("candidate", p, "one launch vs two launches", float((best - two).abs().max()), "graphed", float((graphed - two).abs().max()))
    assert float((best - two).abs().max()) <= 1e-6
    assert float((graphed - two).abs().max()) <= 1e-6


def test_the_example_with_library_constraints_stays_feasible():
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "gabo_sphere_constraints.py")
    spec = importlib.util.spec_from_file_location("gabo_sphere_constraints_example", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    x_data, y_data, best, feasible = mod.run("bounds", "CTR", iters=3, builtin_constraints=True, verbose=False, device=DEV)
    assert x_data.shape == (8, 3) and all(feasible(p) for p in x_data[5:].cpu().numpy())
