"""Constrained sphere sweeps through the native sweep drivers (csrc/spd_sweep.hip: gabo_sphere_sweep_solve_constrained / _run_constrained, the
device sampler gabo_sphere_sample) with the library's own sphere constraints.  Needs an MI355X.

  * the sampler against the oracle's stream (oracle/selection.py: sphere_samples): sample i is the first feasible row among items i + t * count;
  * the two-call form (the default with constraints) against the Python path of joint_optimize_manifold, bit for bit, on both instantiations of
    the solve kernel; the one-call form against the Python path handed the same picks;
  * the final constraint values of the log; the device sampler inside the sweep; what stays off the native path.

The raw samples sit at the start of the sweep's workspace and the final iterates behind them and their values (sph_sweep_layout, blocks rounded to
256 bytes): the tests read both from there."""
import importlib.util
import math
import os
import warnings

import numpy as np
import pytest
import torch

from gabotorch_amd import _lib, manifolds, ops
from gabotorch_amd.manifold_optimization import manifold_optimize as mo
from gabotorch_amd.manifold_optimization.constrained_trust_regions import ConstrainedTrustRegions, StrictConstrainedTrustRegions
from gabotorch_amd.manifold_optimization.manifold_optimize import joint_optimize_manifold
from oracle import selection as osel
from tests.test_gpu_sphere_builtin_constraints import DEV, _fixture_acq, fitted  # noqa: F401  (fitted: a fixture)
from tests.test_sphere_constraints_cpu import ball, library_box_constraints, lower, upper

pytestmark = pytest.mark.gpu
LO, UP, BALL = _lib.GABO_SPHERE_CONSTRAINT_COORD_LOWER, _lib.GABO_SPHERE_CONSTRAINT_COORD_UPPER, _lib.GABO_SPHERE_CONSTRAINT_GEODESIC_BALL
E0 = torch.eye(3, dtype=torch.float64)[0]


# ----------------------------------------------------------------------------------------------- 1. the sampler against the oracle
def _values(cons, x):
    """numpy values (..., C) of library constraints at points x (..., dim): the statements of sphere_constraints_utils_torch"""
    out = []
    for c in cons:
        kw = c.keywords
        if "center" in kw:
            out.append(float(kw["angle"]) - np.arccos(np.clip(x @ kw["center"].numpy(), -1.0, 1.0)))
        elif "lower_bound" in kw:
            out.append(x[..., kw["index"]] - float(kw["lower_bound"]))
        else:
            out.append(float(kw["upper_bound"]) - x[..., kw["index"]])
    return np.stack(out, axis=-1)


SAMPLER_SETS = {"box": (3, lambda: library_box_constraints("box"), 64), "ball": (3, lambda: [ball(E0, math.pi / 4)], 64),
                "dim10": (10, lambda: [lower(0, 0.1)], 64), "dim65": (65, lambda: [lower(3, 0.2), upper(64, 0.1)], 256)}


@pytest.mark.parametrize("seed", [7, 1234567890123])
@pytest.mark.parametrize("name", list(SAMPLER_SETS))
def test_sampler_draws_the_first_feasible_rows_of_the_oracles_stream(name, seed):
    """try t of sample i is item i + t * 64 of the unconstrained stream, accepted when every constraint is > 0.  The replay of the oracle needs at most
    37 tries for the two sets on S^2, 12 for dim 10 and about 100 of the 256 for dim 65 (acceptance ~0.04).  1e-13: the oracle's log / sin / cos / sqrt against
    the device's, as for the unconstrained sampler; a row whose nearest constraint is within 1e-12 of zero at the accepted try may be decided the
    other way by that rounding and is left out - at most one of the 64."""
    dim, build, T = SAMPLER_SETS[name]
    cons = build()
    count = 64
    pts, exhausted = ops.sphere_sample(count, dim, seed, cons, device=DEV)
    assert exhausted is False and pts.shape == (count, dim) and pts.dtype == torch.float64
    got = pts.cpu().numpy()
    assert (_values(cons, got) > 0).all()
    np.testing.assert_allclose(np.linalg.norm(got, axis=1), 1.0, rtol=0, atol=1e-15)
    stream = osel.sphere_samples(seed, count * T, dim).reshape(T, count, dim)
    vals = _values(cons, stream)                                   # T x count x C
    ok = (vals > 0).all(-1)
    assert ok.any(0).all(), "the oracle's replay needs more tries than the cap"
    first = ok.argmax(0)
    want = stream[first, np.arange(count)]
    margin = np.abs(vals[first, np.arange(count)]).min(-1)
    keep = margin >= 1e-12
    print(name, seed, "tries: max", int(first.max()) + 1, "mean", float(first.mean()) + 1, "rows left out", int((~keep).sum()),
          "max |difference|", float(np.abs(got - want)[keep].max()))
    assert (~keep).sum() <= 1
    np.testing.assert_allclose(got[keep], want[keep], rtol=0, atol=1e-13)


def test_sampler_without_constraints_is_the_unconstrained_sampler_bit_for_bit():
    from tools.sphere_sweep_bench import run
    dt, val, its, log = run(approx=False, constrained=False, device=DEV, R=64, raw=256, device_rand=True)
    assert log.get("native_sweep") and log.get("device_selection")
    ws = [v for k, v in mo._sweep_workspaces.items() if k[0] == "sphere"][0]
    raw = ws[:256 * 10 * 8].view(torch.float64).reshape(256, 10).clone()
    np.random.seed(5)
    seed = int(np.random.randint(0, 2 ** 63 - 1, dtype=np.int64))      # what the driver drew after np.random.seed(5) in tools.sphere_sweep_bench.run
    for cons in (None, []):
        pts, exhausted = ops.sphere_sample(256, 10, seed, cons, device=DEV)
        assert exhausted is False and torch.equal(pts, raw)


def test_sampler_reports_that_it_ran_out_of_tries():
    """a ball of half-angle 0.02 on S^2 holds 1e-4 of the sphere: 256 tries find a point for about one sample in forty; the call returns normally"""
    cons = [ball(E0, 0.02)]
    pts, exhausted = ops.sphere_sample(64, 3, 7, cons, device=DEV)
    assert exhausted is True
    got = pts.cpu().numpy()
    assert np.isfinite(got).all()
    np.testing.assert_allclose(np.linalg.norm(got, axis=1), 1.0, rtol=0, atol=1e-15)      # (every row holds its last try)
    assert (_values(cons, got)[:, 0] <= 0).any()


# ----------------------------------------------------------------------------------------------- 2. the sweeps
def _example():
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "gabo_sphere_constraints.py")
    spec = importlib.util.spec_from_file_location("gabo_sphere_constraints_example", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _case(name):
    """(equality constraints, inequality constraints, the example's sampler of feasible points, its feasibility test)"""
    ex = _example()
    if name in ("box", "box2"):
        _, _, sample, feasible = ex.constraints("bounds", 3, True)
        return None, library_box_constraints(name), sample, feasible
    if name == "ball":
        return ex.constraints("inequality", 3, True)
    return ex.constraints("equality", 3, True)          # "circle": the sampler draws ON the great circle x[1] = 0


def _sweep(acq, name, options, solver_cls=ConstrainedTrustRegions, R=16, raw=64, approx=False):
    eqs, ineqs, sample, _ = _case(name)
    np.random.seed(21)
    torch.manual_seed(21)
    solver = solver_cls(maxiter=200)
    man = manifolds.Sphere(3)
    man.rand = sample
    best = joint_optimize_manifold(acq, man, solver, q=1, num_restarts=R, raw_samples=raw, bounds=None, equality_constraints=eqs,
                                   inequality_constraints=ineqs, approx_hessian=approx, options=dict(options, device=DEV))
    return best, solver.log, (eqs or []) + (ineqs or [])


def _same_end(a, b):
    (best_a, log_a, _), (best_b, log_b, _) = a, b
    assert torch.equal(best_a, best_b)
    np.testing.assert_array_equal(log_a["final_cost"].cpu().numpy(), log_b["final_cost"].cpu().numpy())
    np.testing.assert_array_equal(log_a["per_restart_iterations"].cpu().numpy(), log_b["per_restart_iterations"].cpu().numpy())
    assert log_a["iterations"] == log_b["iterations"]


def _workspace_views(R, raw):
    """(raw samples, final iterates) of the last sphere sweep, from its workspace"""
    ws = [v for k, v in mo._sweep_workspaces.items() if k[0] == "sphere"][0]
    a256 = lambda n: (n + 255) & ~255                      # noqa: E731
    x_off = a256(raw * 3 * 8) + a256((raw + 1) * 8)
    return (ws[:raw * 3 * 8].view(torch.float64).reshape(raw, 3).clone(), ws[x_off:x_off + R * 3 * 8].view(torch.float64).reshape(R, 3).clone())


def _check_final_constraints(log, cons, R, raw, strict):
    """log["final_constraints"] (R x C, equalities first) against the torch functions at the final iterates; strict: a restart that moved sits on an
    accepted proposal, and the strict solver accepts feasible proposals only"""
    pts, x = _workspace_views(R, raw)
    fc = log["final_constraints"]
    assert fc.shape == (R, len(cons)) and fc.dtype == torch.float64
    ref = torch.stack([c(x) for c in cons], dim=1)
    assert float((fc - ref).abs().max()) <= 1e-13
    if strict:
        start = pts[torch.as_tensor(log["picked"], device=pts.device)]
        moved = (x != start).any(1)
        assert bool(moved.any()) and bool((fc[moved] >= 0).all())


@pytest.mark.parametrize("name,solver_cls,approx,R,raw", [
    ("box2", ConstrainedTrustRegions, False, 16, 64), ("box2", StrictConstrainedTrustRegions, False, 16, 64),
    ("ball", ConstrainedTrustRegions, False, 16, 64), ("circle", ConstrainedTrustRegions, True, 16, 64),
    ("box2", ConstrainedTrustRegions, False, 7, 50)])
def test_two_call_native_sweep_returns_the_python_path_candidate_bit_for_bit(fitted, name, solver_cls, approx, R, raw):
    """the default with constraints: score, select_rows on the host, solve - numpy's and torch's generators consumed as on the Python path"""
    acq, _ = fitted
    strict = solver_cls is StrictConstrainedTrustRegions
    native = _sweep(acq, name, {"log_picked": True}, solver_cls, R, raw, approx)
    log = native[1]
    assert log["native_sweep"] is True and log["device_selection"] is False and log["one_launch_solve"] and log["lds_resident"] is True
    _check_final_constraints(log, native[2], R, raw, strict)
    python = _sweep(acq, name, {"native_sweep": False}, solver_cls, R, raw, approx)
    assert not python[1].get("native_sweep") and python[1].get("one_launch_solve")
    _same_end(native, python)
    assert int(log["per_restart_iterations"].max()) > 1


def test_two_call_native_sweep_from_the_callers_workspace(golden):
    """the trace fixtures' surrogate has no symmetric inverse: the solve kernel's other instantiation (not LDS-resident)"""
    acq = _fixture_acq(golden("tr_traces.npz"), "sph3")
    native = _sweep(acq, "ball", {})
    assert native[1]["native_sweep"] is True and native[1]["device_selection"] is False and native[1]["lds_resident"] is False
    _check_final_constraints(native[1], native[2], 16, 64, False)
    _same_end(native, _sweep(acq, "ball", {"native_sweep": False}))


@pytest.mark.parametrize("name,solver_cls", [("box2", ConstrainedTrustRegions), ("box2", StrictConstrainedTrustRegions), ("circle", ConstrainedTrustRegions)])
def test_one_call_native_sweep_against_the_python_path_with_the_same_picks(fitted, monkeypatch, name, solver_cls):
    """options["device_selection"] = True: gabo_sphere_sweep_run_constrained, one host wait; the restarts come from the selection kernel's stream"""
    acq, _ = fitted
    R, raw = 16, 64
    device = _sweep(acq, name, {"device_selection": True, "log_picked": True}, solver_cls)
    log = device[1]
    assert log["native_sweep"] is True and log["device_selection"] is True and log["one_launch_solve"]
    picks = log["picked"]
    assert picks.shape == (R,) and len(set(picks.tolist())) == R and picks.min() >= 0 and picks.max() < raw
    _check_final_constraints(log, device[2], R, raw, solver_cls is StrictConstrainedTrustRegions)
    monkeypatch.setattr(mo, "select_rows", lambda y, n, gen, nonneg, eta=1.0, alpha=1e-4: (picks.astype(np.int64), False))
    python = _sweep(acq, name, {"native_sweep": False}, solver_cls)
    assert not python[1].get("native_sweep")
    _same_end(device, python)


def test_device_sampler_inside_the_sweep(fitted):
    acq, _ = fitted
    R, raw = 16, 64
    best, log, cons = _sweep(acq, "box", {"device_rand": True, "device_selection": True})
    assert log["native_sweep"] is True and log["device_selection"] is True
    assert _case("box")[3](best[0].cpu().numpy()), best                 # (the example's feasibility test, 2e-3)
    pts, _ = _workspace_views(R, raw)
    np.random.seed(21)
    seed = int(np.random.randint(0, 2 ** 63 - 1, dtype=np.int64))       # the driver's first draw from numpy after _sweep seeded it
    want, exhausted = ops.sphere_sample(raw, 3, seed, cons, device=DEV)
    assert exhausted is False and torch.equal(pts, want)
    assert bool((torch.stack([c(pts) for c in cons], dim=1) > 0).all())
    # without the explicit device_selection the option has no effect on a constrained sweep: host sampler, two calls
    best2, log2, _ = _sweep(acq, "box", {"device_rand": True})
    assert log2["native_sweep"] is True and log2["device_selection"] is False
    _same_end((best2, log2, None), _sweep(acq, "box", {}))
    # an equality constraint: the same options run native on the host sampler's points (on the circle, where no rejection sampler lands)
    best3, log3, _ = _sweep(acq, "circle", {"device_rand": True, "device_selection": True})
    assert log3["native_sweep"] is True and log3["device_selection"] is True
    pts3, _ = _workspace_views(R, raw)
    assert bool((pts3[:, 1] == 0).all()) and abs(float(best3[0, 1])) < 2e-3


def test_exhausted_device_sampler_falls_back_to_the_host_sampler(fitted):
    """fallback 2 of gabo_sphere_sweep_run_constrained: one warning, then the two-call form on manifold.rand's points"""
    acq, _ = fitted
    cons = [ball(E0, 0.02)]
    np.random.seed(21)
    torch.manual_seed(21)
    man = manifolds.Sphere(3)
    man.rand = lambda: np.array([1.0, 0.0, 0.0]) * math.cos(0.01) + np.array([0.0, 1.0, 0.0]) * math.sin(0.01) * np.sign(np.random.randn())
    solver = ConstrainedTrustRegions(maxiter=5)
    mo._native_sweep_sphere._warned_exhausted = False
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        best = joint_optimize_manifold(acq, man, solver, q=1, num_restarts=2, raw_samples=8, bounds=None, inequality_constraints=cons,
                                       options={"device": DEV, "device_rand": True, "device_selection": True})
    assert any("device sampler" in str(w.message) for w in caught)
    assert solver.log["native_sweep"] is True and solver.log["device_selection"] is False and best.shape == (1, 3)


def test_opaque_constraints_and_the_augmented_lagrangian_stay_on_the_python_path(fitted):
    from gabotorch_amd.manifold_optimization.augmented_lagrange_method import AugmentedLagrangeMethod
    from gabotorch_amd.manifold_optimization.robust_trust_regions import TrustRegions
    acq, _ = fitted
    man = manifolds.Sphere(3)
    args = (1, 16, 64, None, torch.float64, {"device": DEV})
    tail = (None, None, False, False)
    ctr = ConstrainedTrustRegions(maxiter=5)
    assert mo._native_sweep_plan(acq, man, ctr, *args, library_box_constraints("box"), None, *tail) is not None
    assert mo._native_sweep_plan(acq, man, ctr, *args, [lambda x: x[..., 0] - 0.1], None, *tail) is None
    assert mo._native_sweep_plan(acq, man, ctr, *args, library_box_constraints("box") + [lambda x: x[..., 0] - 0.1], None, *tail) is None
    import functools
    from gabotorch_amd.Riemannian_utils import sphere_constraints_utils_torch as scu
    positional = functools.partial(scu.coordinate_lower_bound_constraint_torch, index=0)          # (lower_bound left open: not a built-in)
    assert mo._native_sweep_plan(acq, man, ctr, *args, [positional], None, *tail) is None
    alm = AugmentedLagrangeMethod(maxiter=3, inner_solver=TrustRegions(maxiter=5))
    assert mo._native_sweep_plan(acq, man, alm, *args, library_box_constraints("box"), None, *tail) is None
    # ... and the sweep itself with the lambda runs, on the Python path
    np.random.seed(21)
    torch.manual_seed(21)
    man.rand = _case("box")[2]
    best = joint_optimize_manifold(acq, man, ctr, q=1, num_restarts=4, raw_samples=16, bounds=None,
                                   inequality_constraints=[lambda x: x[..., 0] - 0.1], options={"device": DEV})
    assert not ctr.log.get("native_sweep") and best.shape == (1, 3)
