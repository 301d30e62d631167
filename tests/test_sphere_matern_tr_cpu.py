"""The lock-step solver on the CPU against tests/golden/sphere_matern_tr.npz: -EI of an exact GP with the Riemannian Matern kernel's zonal series
(plain fp64 torch, autograd), FD Hessian, exact Hessian and one built-in constraint.  The fixture's generator (tests/golden/
make_golden_sphere_matern_tr.py) accepted the problem because equally valid roundings of it agree on every iteration; this test re-runs its
solver and asks for the whole record.  The GPU twin is tests/test_gpu_sphere_matern_native.py."""
import importlib.util
import os

import numpy as np
import pytest

from tests._traces import compare_with_reference_trace


def generator():
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "make_golden_sphere_matern_tr.py")
    spec = importlib.util.spec_from_file_location("make_golden_sphere_matern_tr", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_fixture_holds_the_generators_settings(golden):
    g, gen = golden("sphere_matern_tr.npz"), generator()
    X, y, x0, con = gen.problem_data(int(g["seed"]))
    for name, want in (("X", X), ("y", y), ("x0", x0), ("con_x0", con)):
        np.testing.assert_array_equal(g[name], want)
    for k, v in gen.HYPER.items():
        assert float(g[k]) == float(v)
    assert g["x0"].shape == (8, 3) and int(g["maxiter"]) == gen.MAXIT
    np.testing.assert_allclose(np.linalg.norm(g["X"], axis=1), 1.0, atol=1e-15)
    assert (g["con_x0"][:, 0] > 0.3).all()
    for run in gen.RUNS:
        nit = g[f"{run}_nit"]
        assert nit.min() >= 2 and nit.max() < gen.MAXIT        # every restart moves and none runs into maxiter


@pytest.mark.parametrize("dim,levels", [(2, 1), (3, 2), (3, 24), (10, 128)])
def test_device_table_holds_the_three_series(dim, levels):
    """ops.sphere_zonal_table: what gabo_sphere_acq_params.series points to - order o holds the coefficients of sphere_matern_coefficients(order=o)
    and the factors B_k of series dimension dim - 1 + 2 o, zero-padded to the length of order 0"""
    from gabotorch_amd import ops
    from tests._cpu_sphere_zonal import recurrence_factors
    p, sd = ops.sphere_matern_coefficients(dim, 0.45, 2.5, levels)
    table = ops.sphere_zonal_table(p, sd)
    assert table.shape == (3, levels + 1, 2) and table.dtype == np.float64 and sd == dim - 1
    for order in range(3):
        co, sdo = ops.sphere_matern_coefficients(dim, 0.45, 2.5, levels, order)
        assert sdo == sd + 2 * order
        want = np.zeros(levels + 1)
        want[:max(levels + 1 - order, 0)] = co[:max(levels + 1 - order, 0)]
        np.testing.assert_array_equal(table[order, :, 0], want)
        rb = recurrence_factors(levels + 1, sdo)
        rb[:2] = 0.0
        np.testing.assert_array_equal(table[order, :, 1], rb)
    one = ops.sphere_zonal_table(np.ones(1), 1)              # a series of one term: the constant, its derivatives zero
    np.testing.assert_array_equal(one, np.array([[[1.0, 0.0]], [[0.0, 0.0]], [[0.0, 0.0]]]))
    with pytest.raises(ValueError):
        ops.sphere_zonal_table(np.ones(130), 2)


@pytest.mark.parametrize("rounding", [{}, {"descending": True}, {"cholesky": True}])
@pytest.mark.parametrize("run", ["fd", "exact", "con"])
def test_lock_step_solver_follows_the_record(golden, run, rounding):
    g, gen = golden("sphere_matern_tr.npz"), generator()
    hyper = {k: float(g[k]) for k in gen.HYPER}
    hyper["num_levels"] = int(g["num_levels"])
    cost = gen.neg_ei_cost(g["X"], g["y"], hyper, **rounding)
    trace, final = gen.solve_run(run, cost, g["con_x0"] if run == "con" else g["x0"])
    res = compare_with_reference_trace(trace, g, run, atol_x=1e-9)
    for s, (agree, nit, worst, parted_at, drift) in enumerate(res):
        assert agree == nit, (run, s, agree, nit, worst, parted_at, drift)
    last = g[f"{run}_xs"][np.arange(len(final)), g[f"{run}_nit"]]
    np.testing.assert_allclose(final, last, rtol=0, atol=1e-9)
