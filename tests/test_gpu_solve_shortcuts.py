"""The shortcuts of the single-launch trust-region solve (csrc/spd_tr_body.hpp, csrc/spd_tr_duo_body.hpp) against runs of the same problems with them switched
off (gabo_spd_tr_shortcuts, include/gabo_hip.h):

  * value first after a rejection - the proposal's acquisition value, its gradient only once the proposal is known to be accepted;
  * step reuse - the same step at the same iterate: the previous proposal and its value stand (tr_build_proposal / duo_same_step);
  * fast-forward over runs of rejections - the first tCG step does not change: one more iteration, the radius quartered, as scalars (tr_repeat_rejected).

Each is meant to leave every bit of the final state as the full iterations would.  A rejected iteration does not move x, so a fast-forward that counts
iterations wrongly or sets the wrong radius leaves the costs alone: the iteration counts and the final trust radii are compared too, bit for bit.  The
library's counters (gabo_spd_tr_shortcut_counters) prove which code ran: all zero with the switch off, in the same process right after a run in which
they moved; the cases below are chosen so that every shortcut runs in some named case (_EXPECT), and so that both the LDS-resident and the generic-
workspace form of the one-wave kernel and the two-wave kernel are covered."""
import contextlib
import ctypes
import functools
import os
import sys

import numpy as np
import pytest
import torch

from gabotorch_amd import _lib, manifolds, models, ops
from gabotorch_amd.kernel_utils.kernels_spd import (SpdAffineInvariantGaussianKernel, SpdFrobeniusGaussianKernel,
                                                    SpdLogEuclideanGaussianKernel)
from gabotorch_amd.manifold_optimization.batched_trust_regions import BatchedTrustRegions
from gabotorch_amd.manifold_optimization.manifold_optimize import gen_candidates_manifold
from gabotorch_amd.Riemannian_utils import spd_constraints_utils_torch as scut
from gabotorch_amd.Riemannian_utils.spd_utils_torch import (symmetric_matrix_to_vector_mandel_torch,
                                                            vector_to_symmetric_matrix_mandel_torch)
from oracle import spd as ospd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
pytestmark = pytest.mark.gpu
DEV = "cuda:0"
VALUE_FIRST, VALUE_FIRST_ACCEPTED, STEP_REUSED, FAST_FORWARDED, GENERIC_WORKSPACE = range(_lib.GABO_TR_SHORTCUT_COUNTERS)
SHORTCUT_SLOTS = (VALUE_FIRST, VALUE_FIRST_ACCEPTED, STEP_REUSED, FAST_FORWARDED)


def t(x):
    return torch.tensor(np.ascontiguousarray(x), dtype=torch.float64, device=DEV)


@contextlib.contextmanager
def switches(shortcuts, two_waves, counters=None):
    """gabo_spd_tr_shortcuts / gabo_spd_tr_two_waves set for the body, a counter buffer registered; all restored afterwards"""
    lib = _lib.load()
    before_sc, before_tw = lib.gabo_spd_tr_shortcuts(-1), lib.gabo_spd_tr_two_waves(-1)
    try:
        lib.gabo_spd_tr_shortcuts(int(shortcuts))
        lib.gabo_spd_tr_two_waves(int(two_waves))
        if counters is not None:
            counters.zero_()
            _lib.check(lib.gabo_spd_tr_shortcut_counters(ctypes.c_void_p(counters.data_ptr())), "gabo_spd_tr_shortcut_counters")
        yield
        torch.cuda.synchronize()
    finally:
        lib.gabo_spd_tr_shortcut_counters(None)
        lib.gabo_spd_tr_shortcuts(before_sc)
        lib.gabo_spd_tr_two_waves(before_tw)


def new_counters():
    return torch.zeros(_lib.GABO_TR_SHORTCUT_COUNTERS, dtype=torch.int64, device=DEV)


# ------------------------------------------------------------------------------------------------------------------------------------ problems
def _acquisition(surrogate, d, n_train, seed):
    rng = np.random.default_rng(seed)
    q = np.linalg.qr(rng.standard_normal((n_train, d, d)))[0]
    Xm = np.einsum("nab,nb,ncb->nac", q, rng.uniform(0.2, 3.0, (n_train, d)), q)
    X = ospd.symmetric_matrix_to_vector_mandel(0.5 * (Xm + Xm.transpose(0, 2, 1)))
    y = np.log(np.linalg.eigvalsh(Xm)).sum(1) ** 2 + 0.1 * rng.standard_normal(n_train)
    if surrogate == "ai":
        # (at d = 7, 8 the default beta leaves every start where the GP is its prior and EI flat to the gradient tolerance: no iteration at all)
        kern = SpdAffineInvariantGaussianKernel(beta_min=0.5 if d <= 6 else 0.05)
        if d > 6:
            kern.beta = torch.tensor(0.2, dtype=torch.float64)
    else:
        kern = (SpdLogEuclideanGaussianKernel if surrogate == "le" else SpdFrobeniusGaussianKernel)().double()
        kern.lengthscale = torch.tensor(1.4 if surrogate == "le" else 2.0, dtype=torch.float64)
    gp = models.ExactGP(t(X), t(y), kern, outputscale=1.0, noise=1e-2)
    return rng, models.ExpectedImprovement(gp, best_f=float(y.min()), maximize=False)


def _starts(rng, d, R, lo=0.4, hi=2.4):
    q = np.linalg.qr(rng.standard_normal((R, d, d)))[0]
    P = np.einsum("nab,nb,ncb->nac", q, rng.uniform(lo, hi, (R, d)), q)
    return 0.5 * (P + P.transpose(0, 2, 1))


def _bounds(case):
    """eigenvalue bounds built with functools.partial (evaluated inside the kernel): the EI optimum of many restarts lies beyond lambda_max = 2.5"""
    if case == "none":
        return None
    cons = [functools.partial(scut.max_eigenvalue_constraint_torch, maximum_eigenvalue=2.5)]
    if case.startswith("box"):
        cons.append(functools.partial(scut.min_eigenvalue_constraint_torch, minimum_eigenvalue=0.35))
    return cons


def solve(acq, x0, d, cons, strict, maxiter, shortcuts, two_waves, counters, rho_prime=0.1):
    """one single-launch solve; returns (final state as numpy arrays, counters)"""
    solver = BatchedTrustRegions(mingradnorm=1e-5, maxiter=maxiter, strict_constraints=strict, rho_prime=rho_prime)
    ops.set_error_checking(False)
    try:
        with switches(shortcuts, two_waves, counters):
            c, v = gen_candidates_manifold(x0, acq, manifolds.PositiveDefinite(d), solver, vector_to_symmetric_matrix_mandel_torch,
                                           symmetric_matrix_to_vector_mandel_torch, inequality_constraints=cons, approx_hessian=True, options={})
            cnt = counters.cpu().tolist()
    finally:
        ops.set_error_checking(True)
    log = solver.log
    assert log.get("one_launch_solve"), "the problem did not run in the single launch"
    state = {"candidate": c, "value": v, "final_cost": log["final_cost"], "final_gradnorm": log["final_gradnorm"],
             "final_radius": log["final_radius"], "per_restart_iterations": log["per_restart_iterations"]}
    return {k: v_.detach().cpu().numpy().copy() for k, v_ in state.items()}, cnt


def assert_same_state(on, off, what):
    assert on.keys() == off.keys()
    for k in on:
        np.testing.assert_array_equal(on[k], off[k], err_msg=f"{what}: {k}")


def on_and_off(acq, x0, d, cons, strict, maxiter, two_waves, generic, rho_prime=0.1):
    """the same problem with the shortcuts on, then off, in this process; returns the counters of the run with them on"""
    counters = new_counters()
    on, c_on = solve(acq, x0, d, cons, strict, maxiter, True, two_waves, counters, rho_prime)
    off, c_off = solve(acq, x0, d, cons, strict, maxiter, False, two_waves, counters, rho_prime)
    R = x0.shape[0]
    assert [c_off[s] for s in SHORTCUT_SLOTS] == [0] * 4, c_off                          # the switch is real: no shortcut ran
    assert c_on[GENERIC_WORKSPACE] == c_off[GENERIC_WORKSPACE] == (R if generic else 0), (c_on, c_off)
    assert c_on[VALUE_FIRST_ACCEPTED] <= c_on[VALUE_FIRST]
    assert_same_state(on, off, "shortcuts on / off")
    return on, c_on


# ------------------------------------------------------------------------------------------------------------------------------------ the matrix
# (surrogate, d, constraints, two waves, n_train, maxiter[, rho_prime]).  n_train = 90: the GP factor does not fit in LDS next to the workspace, so the
# generic-workspace instantiation of the one-wave kernel runs (LAT = false; counter slot 4); the two-wave form declines such problems.  rho_prime = 0.3:
# the fast-forward stands aside (it applies while a rejection quarters the radius, rho_prime < 1/4), and runs of rejections with an unchanged step go
# through the step reuse instead.
CASES = []
for _d in (2, 3, 5, 6, 7, 8):
    for _c in ("none", "max_eig", "box", "box_strict"):
        for _tw in ((1, 0) if _d <= 6 else (0,)):
            CASES.append(("ai", _d, _c, _tw, 20 if _d < 6 else 14, 100))
for _d in (2, 5, 6, 7, 8):
    for _c in ("none", "max_eig", "box", "box_strict"):
        CASES.append(("le", _d, _c, 0, 20 if _d < 6 else 14, 100))
for _d in (2, 5, 8):
    for _c in ("none", "max_eig", "box", "box_strict"):
        CASES.append(("frob", _d, _c, 0, 20, 100))
CASES += [("ai", 2, "max_eig", 0, 90, 100), ("ai", 6, "max_eig", 0, 90, 100), ("ai", 5, "max_eig", 0, 90, 250), ("ai", 3, "box_strict", 0, 90, 100),
          ("le", 6, "box", 0, 90, 100), ("le", 5, "box", 0, 90, 100), ("le", 7, "max_eig", 0, 90, 60), ("frob", 2, "max_eig", 0, 90, 100),
          ("frob", 8, "max_eig", 0, 90, 100), ("ai", 6, "max_eig", 1, 14, 250), ("ai", 6, "max_eig", 0, 14, 250),
          ("ai", 6, "max_eig", 1, 14, 100, 0.3), ("ai", 6, "max_eig", 0, 14, 100, 0.3), ("ai", 2, "box", 1, 20, 100, 0.3), ("le", 2, "max_eig", 0, 20, 100, 0.3)]


def case_id(c):
    rho = f"-rho{c[6]}" if len(c) > 6 else ""
    return f"{c[0]}-d{c[1]}-{c[2]}-{'two' if c[3] else 'one'}_wave{'s' if c[3] else ''}-n{c[4]}-it{c[5]}{rho}"


# counters the named cases must move with the shortcuts on: together every shortcut in every form of the kernel (test_the_matrix_reaches_every_shortcut).
# Every case checks slot 4 itself: the number of restarts in the n = 90 cases, 0 in the others (on_and_off).
_FF = {VALUE_FIRST, VALUE_FIRST_ACCEPTED, FAST_FORWARDED}
_REUSE = {VALUE_FIRST, VALUE_FIRST_ACCEPTED, STEP_REUSED}
_EXPECT = {
    "ai-d6-max_eig-one_wave-n14-it100": _FF, "ai-d6-max_eig-two_waves-n14-it100": _FF, "ai-d2-max_eig-one_wave-n20-it100": _FF,
    "ai-d7-box-one_wave-n14-it100": _FF, "le-d2-max_eig-one_wave-n20-it100": _FF, "le-d6-max_eig-one_wave-n14-it100": _FF,
    "frob-d2-max_eig-one_wave-n20-it100": _FF,
    "ai-d6-max_eig-one_wave-n14-it100-rho0.3": _REUSE, "ai-d6-max_eig-two_waves-n14-it100-rho0.3": _REUSE,
    "ai-d2-box-two_waves-n20-it100-rho0.3": _REUSE, "le-d2-max_eig-one_wave-n20-it100-rho0.3": _REUSE,
    "ai-d2-max_eig-one_wave-n90-it100": _FF | {GENERIC_WORKSPACE}, "frob-d2-max_eig-one_wave-n90-it100": _FF | {GENERIC_WORKSPACE},
}


def _generic(c):
    return c[4] == 90


@pytest.mark.parametrize("case", CASES, ids=[case_id(c) for c in CASES])
def test_shortcuts_do_not_change_a_bit(case):
    surrogate, d, cons_case, two_waves, n_train, maxiter = case[:6]
    rng, acq = _acquisition(surrogate, d, n_train, seed=1000 + 10 * d + n_train)
    R = 48
    x0 = ops.matrix_to_mandel(t(_starts(rng, d, R)))[:, None]
    _, cnt = on_and_off(acq, x0, d, _bounds(cons_case), cons_case.endswith("strict"), maxiter, two_waves, _generic(case), *case[6:])
    print(case_id(case), cnt)
    assert cnt[VALUE_FIRST] > 0, cnt                     # (every case has rejected proposals)
    for s in _EXPECT.get(case_id(case), ()):
        assert cnt[s] > 0, (s, cnt)


def test_the_matrix_reaches_every_shortcut():
    """(static) the named expectations cover every shortcut in some case, and name only cases of the matrix"""
    ids = {case_id(c) for c in CASES}
    assert set(_EXPECT) <= ids, set(_EXPECT) - ids
    assert set().union(*_EXPECT.values()) >= set(SHORTCUT_SLOTS)
    for slot in SHORTCUT_SLOTS:          # ... in each form of the kernel: one wave, two waves, the generic workspace
        assert any(slot in v for k, v in _EXPECT.items() if "one_wave" in k and "-n90-" not in k), slot
        assert any(slot in v for k, v in _EXPECT.items() if "two_waves" in k), slot
    assert any(FAST_FORWARDED in v and GENERIC_WORKSPACE in v for v in _EXPECT.values())


def test_nested_eigenvalue_bounds():
    """kinds 2 / 3: eigenvalue bounds of the iterate lifted to S^20_++ by a nested SPD mapping (config 5's latent sweep, log-Euclidean surrogate, strict)"""
    from gabotorch_amd.nested_mappings import nested_spd_constraints_utils as nscu
    D, d, R = 20, 2, 48
    rng, acq = _acquisition("le", d, 15, seed=43)
    m = D - d
    Rm = np.linalg.qr(rng.standard_normal((D, D)))[0]
    W, V = t(Rm[:, :d]), t(np.linalg.qr(Rm[:, d:] + 0.01 * rng.standard_normal((D, m)))[0])
    qc = np.linalg.qr(rng.standard_normal((m, m)))[0]
    C = t((qc * rng.uniform(0.6, 1.8, m)) @ qc.T)
    K0 = rng.standard_normal((d, m))
    K = t(0.5 * K0 / np.linalg.norm(K0))
    mapping = dict(projection_matrix=W, projection_complement_matrix=V, bottom_spd_matrix=C, contraction_matrix=K)
    P = _starts(rng, d, 4 * R, 0.5, 2.2)
    lam = np.linalg.eigvalsh(ospd.projection_from_nested_spd_to_spd(P, *(a.cpu().numpy() for a in (W, V, C, K))))
    hi, lo = float(np.quantile(lam[:, -1], 0.7)), float(np.quantile(lam[:, 0], 0.3))
    keep = np.flatnonzero((lam[:, -1] < hi - 0.02) & (lam[:, 0] > lo + 0.01))[:R]
    assert len(keep) >= 24
    x0 = ops.matrix_to_mandel(t(P[keep]))[:, None]
    cons = [functools.partial(nscu.max_eigenvalue_nested_spd_constraint, maximum_eigenvalue=hi, **mapping),
            functools.partial(nscu.min_eigenvalue_nested_spd_constraint, minimum_eigenvalue=lo, **mapping)]
    assert scut.builtin_constraint(cons[0])[0] == _lib.GABO_CONSTRAINT_MAX_EIGENVALUE_NESTED
    assert scut.builtin_constraint(cons[1])[0] == _lib.GABO_CONSTRAINT_MIN_EIGENVALUE_NESTED
    _, cnt = on_and_off(acq, x0, d, cons, True, 100, 0, False)
    print("nested", cnt)
    assert cnt[VALUE_FIRST] > 0, cnt


@pytest.mark.parametrize("two_waves", [0, 1])
def test_radius_underflow(two_waves):
    """600 iterations on the lambda_max bound: a restart that rejects every proposal quarters its radius through the subnormals to exactly 0
    (4^-537 ~ 5e-324) and goes on iterating there until maxiter.  Both forms must agree bit for bit, and nothing may turn non-finite."""
    maxiter = 600
    rng, acq = _acquisition("ai", 6, 14, seed=1074)          # (the problem of ai-d6-max_eig-*-n14-it100 above)
    x0 = ops.matrix_to_mandel(t(_starts(rng, 6, 48)))[:, None]
    on, cnt = on_and_off(acq, x0, 6, _bounds("max_eig"), False, maxiter, two_waves, False)
    print("underflow", two_waves, cnt, np.sort(on["final_radius"])[:6], np.sort(on["per_restart_iterations"])[-6:])
    for k in ("candidate", "final_cost", "final_gradnorm"):
        assert np.isfinite(on[k]).all(), k
    radius, iters = on["final_radius"], on["per_restart_iterations"]
    assert (radius == 0.0).any(), radius.min()                         # the edge is reached
    assert (iters[radius == 0.0] == maxiter).all()                     # ... by restarts on the bound, which iterate to maxiter
    assert cnt[FAST_FORWARDED] > 0, cnt


@pytest.mark.parametrize("two_waves", [0, 1])
def test_native_sweep(two_waves):
    """the sweep through the native driver (restarts started inside the launch from the raw-sample table, TrStart): candidate, value, final costs and
    iteration counts with the shortcuts on and off"""
    from tools.sweep_bench import run_sweep
    counters = new_counters()
    out = []
    for sc in (True, False):
        with switches(sc, two_waves, counters):
            _, best, val, log = run_sweep(DEV, num_restarts=64, raw_samples=256, device_rand=True, builtin_constraint=True, native_sweep=True,
                                          device_selection=False)
            cnt = counters.cpu().tolist()
        assert log.get("native_sweep") and log.get("one_launch_solve")
        out.append((best.cpu().numpy(), val, log["final_cost"].cpu().numpy(), log["per_restart_iterations"].cpu().numpy(), cnt))
    (b1, v1, f1, i1, c_on), (b2, v2, f2, i2, c_off) = out
    print("native", two_waves, c_on)
    np.testing.assert_array_equal(b1, b2)
    assert v1 == v2
    np.testing.assert_array_equal(f1, f2)
    np.testing.assert_array_equal(i1, i2)
    assert [c_off[s] for s in SHORTCUT_SLOTS] == [0] * 4, c_off
    assert c_on[VALUE_FIRST] > 0 and c_on[FAST_FORWARDED] > 0, c_on
