"""What conditioning the prediction cache decides on the host: gabo_gp_condition (csrc/gp_condition.hip) refuses malformed calls before any
HIP call, the plain-numpy statement of its bordered update stays within the tests' bound of a from-scratch reference in np.longdouble, and
sequential_optimize_manifold refuses what a believer batch cannot be built from - none of it needs a GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from gabotorch_amd import _lib, models
from gabotorch_amd.manifold_optimization import manifold_optimize
from tests import _cpu_gp_condition as cpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", autouse=True)
def _built_library():
    if not os.path.exists(_lib.LIB_PATH):
        from gabotorch_amd import _build
        _build.build()


def _p(a):
    return None if a is None else ctypes.c_void_p(a)


def _condition(lib, linv=8, alpha=16, kinv=24, n=5, kcross=32, knew=40, y_new=48, t=2, linv_out=56, linv_t_out=64, alpha_out=72, kinv_out=80,
               y_out=88, ws=96, ws_bytes=None, status=104):
    """made-up addresses that are never touched: the verdict on the arguments comes first"""
    if ws_bytes is None:
        ws_bytes = lib.gabo_gp_condition_workspace_bytes(n, t)
    return lib.gabo_gp_condition(_p(linv), _p(alpha), _p(kinv), n, _p(kcross), _p(knew), _p(y_new), t, 1.0, 1e-2, 0.0, _p(linv_out), _p(linv_t_out),
                                 _p(alpha_out), _p(kinv_out), _p(y_out), _p(ws), ws_bytes, _p(status), None)


def test_malformed_calls_are_refused_before_any_hip_call():
    lib = _lib.load()
    big = _lib.GABO_GP_MLL_LARGE_MAX_N
    assert _condition(lib, n=big - 1, t=2, ws_bytes=1 << 30) == _lib.GABO_ERR_DIM             # n + t = the limit + 1
    assert _condition(lib, n=big, t=1, ws_bytes=1 << 30) == _lib.GABO_ERR_DIM
    assert _condition(lib, n=big + 1, t=1, linv=None, ws_bytes=1 << 30) == _lib.GABO_ERR_DIM
    assert _condition(lib, t=_lib.GABO_GP_CONDITION_MAX_T + 1, ws_bytes=1 << 30) == _lib.GABO_ERR_DIM
    assert _lib.GABO_GP_CONDITION_MAX_T + 1 == 17
    for bad in (dict(linv=None), dict(alpha=None), dict(kcross=None), dict(knew=None), dict(linv_out=None), dict(alpha_out=None), dict(y_out=None),
                dict(ws=None), dict(status=None), dict(n=0, ws_bytes=1 << 20), dict(n=-3, ws_bytes=1 << 20), dict(t=0, ws_bytes=1 << 20),
                dict(t=-1, ws_bytes=1 << 20), dict(kinv_out=None), dict(kinv=None)):
        assert _condition(lib, **bad) == _lib.GABO_ERR_ARG, bad
    need = lib.gabo_gp_condition_workspace_bytes(5, 2)
    assert need == (2 * 7 + 8) * 8
    assert _condition(lib, ws_bytes=need - 1) == _lib.GABO_ERR_ARG
    assert _condition(lib, ws_bytes=0) == _lib.GABO_ERR_ARG


def test_workspace_of_a_refused_call_is_zero():
    lib = _lib.load()
    big = _lib.GABO_GP_MLL_LARGE_MAX_N
    for args in ((0, 1), (1, 0), (-1, 1), (big, 1), (big - 16, 17), (5, _lib.GABO_GP_CONDITION_MAX_T + 1)):
        assert lib.gabo_gp_condition_workspace_bytes(*args) == 0, args
    assert lib.gabo_gp_condition_workspace_bytes(big - 16, 16) == (2 * big + 8) * 8


def test_constants_match_the_header():
    text = open(os.path.join(ROOT, "include", "gabo_hip.h")).read()
    for name in ("GABO_GP_CONDITION_MAX_T", "GABO_GP_MLL_LARGE_MAX_N", "GABO_GP_FACTOR_MAX_N", "GABO_GP_MLL_MAX_N"):
        value = re.search(rf"#define {name} \(?(-?\d+)\)?", text)
        assert value is not None and int(value.group(1)) == getattr(_lib, name), name


@pytest.mark.parametrize("noise", cpu.GRID_NOISE)
@pytest.mark.parametrize("n", cpu.GRID_N)
def test_numpy_update_stays_within_the_bound_of_the_longdouble_reference(n, noise):
    for t in cpu.GRID_T:
        case, (linv, alpha, kinv), ref = cpu.grid_case(n, t, noise)
        cond = cpu.cond2(case)
        got = cpu.bordered_update(linv, alpha, kinv, case["kcross"], case["knew"], case["y"][n:], case["outputscale"], noise, case["mean"])
        for name, g, r in zip(("linv", "alpha", "kinv"), got, ref):
            err = float(np.max(np.abs(g - r)))
            print(f"n={n} t={t} noise={noise:g} cond={cond:.3g} {name}: err/max|ref|/eps = {err / float(np.max(np.abs(r))) / cpu.EPS:.3g}")
            assert err <= cpu.bound(cond, r), (n, t, noise, name, err, cpu.bound(cond, r))
        assert np.array_equal(got[3], case["y"][n:])
        assert np.array_equal(got[0], np.tril(got[0])) and np.array_equal(got[2], got[2].T)


def test_numpy_believer_keeps_alpha_and_reports_the_posterior_mean():
    case, (linv, alpha, kinv), _ = cpu.grid_case(65, 3, 1e-4)
    lo, al, a, y_used = cpu.bordered_update(linv, alpha, kinv, case["kcross"], case["knew"], None, case["outputscale"], 1e-4, case["mean"])
    assert np.array_equal(al[:65], alpha) and np.array_equal(al[65:], np.zeros(3))
    want = case["mean"] + case["outputscale"] * case["kcross"].astype(np.longdouble) @ alpha.astype(np.longdouble)
    scale = abs(case["mean"]) + case["outputscale"] * np.abs(case["kcross"]) @ np.abs(alpha)
    assert np.all(np.abs(y_used - want) <= (65 + 8) * cpu.EPS * scale)
    # the fantasy is consistent: conditioning on it with explicit targets changes nothing but rounding
    _, al2, _, _ = cpu.bordered_update(linv, alpha, kinv, case["kcross"], case["knew"], y_used, case["outputscale"], 1e-4, case["mean"])
    assert np.max(np.abs(al2 - al)) <= cpu.bound(cpu.cond2(case), al)


def test_numpy_update_reports_the_point_that_breaks_positive_definiteness():
    case, (linv, alpha, kinv), _ = cpu.grid_case(3, 2, 1e-2)
    kcross, knew = case["kcross"].copy(), case["knew"].copy()
    kcross[1] = case["kbase"][0, :3]              # the second new point repeats training point 0 ...
    knew[1, 0] = case["kbase"][0, 3]
    knew[1, 1] = 0.1                              # ... with a prior variance far below its covariance with it
    with pytest.raises(np.linalg.LinAlgError) as info:
        cpu.bordered_update(linv, alpha, kinv, kcross, knew, None, case["outputscale"], 1e-2, case["mean"])
    assert info.value.args[0] == 1


class _Foreign(torch.nn.Module):
    def forward(self, X):
        raise AssertionError("the acquisition must not be evaluated")


def test_sequential_optimize_refuses_what_it_cannot_condition_without_touching_the_device(monkeypatch):
    def no_sweep(*a, **k):
        raise AssertionError("no sweep may start")
    monkeypatch.setattr(manifold_optimize, "joint_optimize_manifold", no_sweep)
    x, y = torch.eye(3, dtype=torch.float64), torch.zeros(3, dtype=torch.float64)
    gp = models.ExactGP(x, y, base_kernel=None, mean=0.0)
    with pytest.raises(ValueError, match="posterior mean"):
        manifold_optimize.sequential_optimize_manifold(models.PosteriorMean(gp), None, None, 3, 4, 8, None)
    for acq in (_Foreign(), models.ExpectedImprovement(_Foreign(), best_f=0.0), (lambda X: X.sum(-1).sum(-1))):
        with pytest.raises(NotImplementedError, match="ExpectedImprovement over models.ExactGP or models.SingleTaskGP"):
            manifold_optimize.sequential_optimize_manifold(acq, None, None, 3, 4, 8, None)
    with pytest.raises(ValueError, match="q = 0"):
        manifold_optimize.sequential_optimize_manifold(models.ExpectedImprovement(gp, best_f=0.0), None, None, 0, 4, 8, None)


def test_python_wrapper_refuses_host_tensors():
    from gabotorch_amd import ops
    z = torch.zeros(3, 3, dtype=torch.float64)
    with pytest.raises(ValueError, match="HIP device"):
        ops.gp_condition(z, z[0], z[:1], z[:1, :1])


def test_condition_on_observations_is_part_of_both_models():
    assert callable(models.ExactGP.condition_on_observations) and callable(models.SingleTaskGP.condition_on_observations)
    gp = models.ExactGP(torch.eye(3, dtype=torch.float64), torch.zeros(3, dtype=torch.float64), base_kernel=None, mean=0.0)
    gp._cache = (torch.eye(3, dtype=torch.float64), torch.zeros(3, dtype=torch.float64))
    with pytest.raises(ValueError, match="HIP device"):        # a model on the host has no cache the device could extend
        gp.condition_on_observations(torch.ones(1, 3, dtype=torch.float64))
    with pytest.raises(ValueError, match="one set of new points"):
        gp.condition_on_observations(torch.ones(2, 1, 3, dtype=torch.float64))
