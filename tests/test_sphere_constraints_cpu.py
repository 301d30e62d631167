"""The library's sphere constraints (Riemannian_utils/sphere_constraints_utils_torch.py) on the CPU: closed forms and autograd gradients, the
recognition table of builtin_sphere_constraint, and the generic lock-step solver following the reference's own fp64 records
(tests/golden/tr_traces_eq.npz, tr_traces_box.npz) when the constraint sets of those records are rebuilt from the library functions."""
import functools
import math

import numpy as np
import pytest
import torch

from gabotorch_amd import _lib
from gabotorch_amd.Riemannian_utils import sphere_constraints_utils_torch as scu
from tests._traces import compare_with_reference_trace
from tests.test_tr_traces_cpu import EQ_RUNS, T, _problem, box_run_setup, eq_run_setup

lower = lambda i, b: functools.partial(scu.coordinate_lower_bound_constraint_torch, index=i, lower_bound=b)      # noqa: E731
upper = lambda i, b: functools.partial(scu.coordinate_upper_bound_constraint_torch, index=i, upper_bound=b)      # noqa: E731
ball = lambda c, a: functools.partial(scu.geodesic_ball_constraint_torch, center=c, angle=a)                      # noqa: E731


def library_eq_constraints(run):
    """the great circle x[1] = level of eq_run_setup"""
    return [lower(1, 0.2 if run == "eqoff" else 0.0)]


def library_box_constraints(run):
    """the five bounds of box_run_setup, in its order"""
    b = dict(xl=0.0, yl=-0.6, yu=0.6, zl=-0.6, zu=0.6)
    if run.startswith("box2"):
        b.update(yu=0.3, zu=0.05)
    return [lower(0, b["xl"]), lower(1, b["yl"]), upper(1, b["yu"]), lower(2, b["zl"]), upper(2, b["zu"])]


def _points(r, dim, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(r, dim, dtype=torch.float64, generator=g)
    return x / x.norm(dim=-1, keepdim=True)


def _value_and_grad(fn, x):
    xx = x.clone().requires_grad_(True)
    f = fn(xx)
    (g,) = torch.autograd.grad(f.sum(), xx)
    return f.detach(), g


@pytest.mark.parametrize("dim", [3, 5])
def test_values_and_gradients_against_the_closed_forms(dim):
    x = _points(6, dim)
    centre = _points(1, dim, seed=1)[0]
    for batch in (x, x[2]):                                    # a batch (R, dim) and one point (dim,)
        f, g = _value_and_grad(lower(1, 0.25), batch)
        assert f.shape == batch.shape[:-1] and torch.equal(f, batch[..., 1] - 0.25)
        e = torch.zeros_like(batch)
        e[..., 1] = 1.0
        assert torch.equal(g, e)
        f, g = _value_and_grad(upper(dim - 1, torch.tensor(0.5, dtype=torch.float64)), batch)
        assert f.shape == batch.shape[:-1] and torch.equal(f, 0.5 - batch[..., dim - 1])
        e = torch.zeros_like(batch)
        e[..., dim - 1] = -1.0
        assert torch.equal(g, e)
        f, g = _value_and_grad(ball(centre, math.pi / 4), batch)
        c = (batch * centre).sum(-1)
        assert f.shape == batch.shape[:-1]
        np.testing.assert_allclose(f.numpy(), math.pi / 4 - np.arccos(np.clip(c.numpy(), -1, 1)), rtol=0, atol=1e-15)
        np.testing.assert_allclose(g.numpy(), ((1 - c * c) ** -0.5)[..., None].numpy() * centre.numpy(), rtol=1e-14, atol=0)


def test_ball_gradient_is_zero_where_the_inner_product_leaves_the_open_interval():
    centre = torch.tensor([0.0, 0.6, 0.8], dtype=torch.float64)
    x = torch.stack([centre, -centre, 1.5 * centre, torch.tensor([1.0, 0.0, 0.0], dtype=torch.float64)])
    f, g = _value_and_grad(ball(centre, 0.3), x)
    assert torch.isfinite(f).all() and torch.isfinite(g).all()
    assert torch.equal(f[:3], torch.tensor([0.3, 0.3 - math.pi, 0.3], dtype=torch.float64))
    assert torch.equal(g[:3], torch.zeros(3, 3, dtype=torch.float64))
    np.testing.assert_allclose(g[3].numpy(), centre.numpy(), rtol=0, atol=1e-16)      # <x, centre> = 0: egrad = centre


def test_post_processing_init_sphere():
    x = torch.tensor([[3.0, 4.0, 0.0], [0.5, -0.5, 0.5], [0.0, 0.0, -2.0]], dtype=torch.float64)
    y = scu.post_processing_init_sphere_torch(x)
    assert torch.equal(y, x / x.pow(2).sum(-1, keepdim=True).sqrt())
    np.testing.assert_allclose(y.norm(dim=-1).numpy(), 1.0, rtol=0, atol=2e-16)


def test_recognition_table():
    LO, UP, BALL = (_lib.GABO_SPHERE_CONSTRAINT_COORD_LOWER, _lib.GABO_SPHERE_CONSTRAINT_COORD_UPPER,
                    _lib.GABO_SPHERE_CONSTRAINT_GEODESIC_BALL)
    assert (LO, UP, BALL) == (0, 1, 2)
    centre = torch.tensor([1.0, 0.0, 0.0], dtype=torch.float64)
    assert scu.builtin_sphere_constraint(lower(2, -0.6)) == (LO, 2, -0.6)
    assert scu.builtin_sphere_constraint(upper(1, torch.tensor([0.3]))) == (UP, 1, pytest.approx(0.3, abs=1e-7))
    assert scu.builtin_sphere_constraint(upper(1, torch.tensor(0.3, dtype=torch.float64))) == (UP, 1, 0.3)
    got = scu.builtin_sphere_constraint(ball(centre, math.pi / 4))
    assert got[:3] == (BALL, None, math.pi / 4) and got[3] is centre and len(got) == 4
    f = scu.coordinate_lower_bound_constraint_torch
    refused = [lambda x: x[..., 0] - 0.3,                                                         # a lambda
               functools.partial(f, 0.3),                                                          # nothing bound by keyword
               functools.partial(f, index=0),                                                      # a parameter left open
               functools.partial(f, index=0, upper_bound=0.3),                                     # a wrong keyword
               functools.partial(f, index=0, lower_bound=torch.tensor([0.1, 0.2])),                # a two-element bound
               functools.partial(f, index=0.0, lower_bound=0.1),                                   # not an index
               ball(centre.clone().requires_grad_(True), 0.5),                                     # a centre that requires grad
               ball(centre[None], 0.5),                                                            # not a vector
               ball([1.0, 0.0, 0.0], 0.5),                                                         # not a tensor
               functools.partial(scu.geodesic_ball_constraint_torch, centre, angle=0.5)]           # positional
    for con in refused:
        assert scu.builtin_sphere_constraint(con) is None, con


def test_group_packs_what_the_device_entries_take():
    centre = torch.tensor([1.0, 0.0, 0.0], dtype=torch.float64)
    other = torch.tensor([0.0, 0.0, 1.0], dtype=torch.float32)
    cons = [lower(1, 0.0), ball(centre, 0.5), upper(-1, 0.6), ball(other, 0.25)]
    kinds, indices, bounds, centres = scu.builtin_sphere_group(cons, 3, "cpu")
    assert kinds == [0, 2, 1, 2] and indices == [1, 0, 2, 1] and bounds == [0.0, 0.5, 0.6, 0.25]
    assert centres.dtype == torch.float64 and torch.equal(centres, torch.stack([centre, other.double()]))
    assert scu.builtin_sphere_group(cons, 3, "cpu")[3] is centres                       # remembered for the same list
    assert scu.builtin_sphere_group(cons, 4, "cpu") is None                             # the centres are not of that dimension
    assert scu.builtin_sphere_group([lower(3, 0.0)], 3, "cpu") is None                  # no such coordinate
    assert scu.builtin_sphere_group(cons + [lambda x: x[..., 0]], 3, "cpu") is None
    assert scu.builtin_sphere_group([lower(0, 0.0)] * 9, 3, "cpu") is None              # the kernels take 8
    assert scu.builtin_sphere_group([lower(0, 0.1)], 3, "cpu") == ([0], [0], [0.1], None)


@pytest.mark.parametrize("name,run", EQ_RUNS)
def test_library_equality_constraint_follows_the_reference_fp64_trace(golden, name, run):
    """as test_equality_constrained_iterates_follow_the_reference_fp64_trace, the great circle stated with the library function"""
    g, ge = golden("tr_traces.npz"), golden("tr_traces_eq.npz")
    cls, kw, x0, closures, fd = eq_run_setup(ge, name, run)
    cons = library_eq_constraints(run)
    assert torch.equal(cons[0](T(x0)), closures[0](T(x0)))
    prob = _problem(g, name, approx=fd)
    solver = cls(**kw)
    solver.trace = []
    x = solver.solve(prob, T(x0), eq_constraints=cons)
    res = compare_with_reference_trace(solver.trace, ge, f"{name}_{run}_f64", atol_x=1e-6)
    ok = ge[f"{name}_{run}_f64_ok"]
    for s, (agree, nit, worst, parted_at, drift) in enumerate(res):
        if ok[s]:
            assert agree == nit or (run == "eq_strict" and agree >= 30 and drift < 1e-6), (name, run, s, agree, nit, worst, parted_at, drift)
    np.testing.assert_allclose(x.numpy()[ok], ge[f"{name}_{run}_f64_x"][ok], rtol=0, atol=1e-6)
    np.testing.assert_allclose(prob.cost(x).numpy()[ok], ge[f"{name}_{run}_f64_f"][ok], rtol=1e-8, atol=1e-12)


@pytest.mark.parametrize("run", ["box", "box_strict", "box2", "box2_strict"])
def test_library_bound_constraints_follow_the_reference_fp64_trace(golden, run):
    """as test_five_bound_constraints_follow_the_reference_fp64_trace, the five bounds stated with the library functions"""
    g, gb = golden("tr_traces.npz"), golden("tr_traces_box.npz")
    cls, x0, closures = box_run_setup(gb, run)
    cons = library_box_constraints(run)
    for mine, theirs in zip(cons, closures):
        assert torch.equal(mine(T(x0)), theirs(T(x0)))
    prob = _problem(g, "sph3", approx=False)
    solver = cls(maxiter=100)
    solver.trace = []
    x = solver.solve(prob, T(x0), ineq_constraints=cons)
    res = compare_with_reference_trace(solver.trace, gb, f"sph3_{run}_f64", atol_x=1e-6)
    ok = gb[f"sph3_{run}_f64_ok"]
    for s, (agree, nit, worst, parted_at, drift) in enumerate(res):
        if ok[s]:
            assert agree == nit or (run.endswith("strict") and agree >= 30 and drift < 1e-6), (run, s, agree, nit, worst, parted_at, drift)
    np.testing.assert_allclose(prob.cost(x).numpy()[ok], gb[f"sph3_{run}_f64_f"][ok], rtol=1e-8, atol=1e-12)
