"""NestedSphereRiemannianMaternKernel and its one-call fit evaluation (gabo_nested_sphere_fit_evaluate_series) on the GPU, against the numpy
objective of tests/_cpu_nested_sphere_matern.py and against torch autograd through the level-by-level statement.

Shapes (D, latent, n, levels, nu) - the smallest at which each part can go wrong:
    (5, 3, 12, 32, 2.5)    the shape of examples/hd_gabo_sphere.py
    (4, 2, 7, 1, inf)      series dimension 1; f' is a one-term series
    (21, 3, 65, 8, 2.5)    one column past a wave
    (51, 4, 20, 32, 0.5)   47 projection levels
    (12, 2, 190, 16, inf)  the tiled likelihood above 160 points
    (5, 3, 1, 8, 2.5)      the diagonal term alone
"""
import ctypes
import functools
import math
import os
import sys

import numpy as np
import pytest
import torch

from gabotorch_amd import _lib, models, ops
from gabotorch_amd._compat import ScaleKernel
from gabotorch_amd.kernel_utils.kernels_nested_sphere import NestedSphereRiemannianMaternKernel
from tests import _cpu_nested_sphere_matern as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CASES = [(5, 3, 12, 32, 2.5), (4, 2, 7, 1, math.inf), (21, 3, 65, 8, 2.5), (51, 4, 20, 32, 0.5), (12, 2, 190, 16, math.inf), (5, 3, 1, 8, 2.5)]
SMALL = [c for c in CASES if c[2] <= 20]
_ids = lambda c: "D{}-lat{}-n{}-L{}-nu{}".format(*c)     # noqa: E731
HALF_PI = [math.pi / 2]
# data seeds, chosen on the CPU so that the numpy objective's own differences at h and h / 2 (test 3) agree within the cap along every direction
# (a training point close to the pole of a level makes its third derivative large: the first seed tried for the first case gave 3e-4)
SEEDS = dict(zip(CASES, (1, 4071, 21658, 51232, 13916, 5018)))


def _sphere(rng, n, dim):
    x = rng.standard_normal((n, dim))
    return x / np.linalg.norm(x, axis=1, keepdims=True)


@functools.lru_cache(maxsize=None)
def _data(case):
    """training set, packed unit axes and scalar hyper-parameters (kappa, outputscale, noise, mean) of a case; read-only"""
    D, lat, n, levels, nu = case
    rng = np.random.default_rng(SEEDS[case])
    x, y = _sphere(rng, n, D), rng.standard_normal(n)
    axes = np.concatenate([_sphere(rng, 1, D - k)[0] for k in range(D - lat)])
    scalars = np.array([0.6, 1.3, 0.1, 0.15])
    for a in (x, y, axes, scalars):
        a.setflags(write=False)
    return x, y, axes, scalars


def _numpy_ll(case, axes, scalars):
    D, lat, n, levels, nu = case
    x, y = _data(case)[:2]
    L = D - lat
    return ref.log_likelihood(x, y, ref.split_axes(axes, D, L), HALF_PI * L, scalars[0], scalars[1], scalars[2], scalars[3], nu, levels)


def _tangent(axes, v, D, L):
    """v (packed like the axes) with every level's block projected onto the tangent space of its axis"""
    out, off = np.array(v, dtype=np.float64), 0
    for k in range(L):
        a = axes[off:off + D - k]
        out[off:off + D - k] -= (out[off:off + D - k] @ a) * a
        off += D - k
    return out


@functools.lru_cache(maxsize=None)
def _directions(case):
    """5 seeded directions in (axes tangent spaces, kappa, outputscale, noise, mean), the axes part of unit length"""
    D, lat, n, levels, nu = case
    axes = _data(case)[2]
    rng = np.random.default_rng(77 + D + n)
    out = []
    for _ in range(5):
        ua = _tangent(axes, rng.standard_normal(axes.size), D, D - lat)
        out.append((ua / np.linalg.norm(ua), rng.standard_normal(4) * np.array([0.5, 0.5, 0.05, 0.5])))
    return out


@functools.lru_cache(maxsize=None)
def _reference_differences(case, h=1e-4):
    """central differences of the numpy objective along each direction at steps h and h / 2"""
    axes, scalars = _data(case)[2:]
    out = []
    for ua, us in _directions(case):
        d = [(_numpy_ll(case, axes + s * ua, scalars + s * us) - _numpy_ll(case, axes - s * ua, scalars - s * us)) / (2 * s) for s in (h, h / 2)]
        out.append(tuple(d))
    return out


def _entry(case, axes, scalars, want_grad=1):
    """gabo_nested_sphere_fit_evaluate_series called directly -> out_host (7 + packed axes)"""
    D, lat, n, levels, nu = case
    lib = _lib.load()
    x, y = _data(case)[:2]
    L = D - lat
    total = axes.size
    p, dp, sd = ops.sphere_matern_coefficients_and_derivative(lat, float(scalars[0]), nu, levels)
    assert sd == lat - 1 and p.size == levels + 1
    dev = torch.device(DEV)
    X, Y = torch.tensor(x, device=dev), torch.tensor(y, device=dev)
    ws = torch.empty(int(lib.gabo_nested_sphere_fit_series_workspace_bytes(n, D, L, p.size)), dtype=torch.uint8, device=dev)
    pinned = torch.empty(2 * total + L + 1 + 4 * p.size + 7, dtype=torch.float64).pin_memory()
    out = np.full(7 + total, np.nan)
    dists = np.full(L, math.pi / 2)
    axes = np.ascontiguousarray(axes, dtype=np.float64)
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)   # noqa: E731
    with torch.cuda.device(dev):
        _lib.check(lib.gabo_nested_sphere_fit_evaluate_series(
            X.data_ptr(), Y.data_ptr(), ptr(axes), ptr(dists), n, D, L, ptr(p), ptr(dp), int(p.size), float(scalars[1]), float(scalars[2]),
            float(scalars[3]), want_grad, ptr(out), ws.data_ptr(), ws.numel(), pinned.data_ptr(), pinned.numel(), ops._stream_ptr(dev)),
            "gabo_nested_sphere_fit_evaluate_series")
    return out


def _kernel(case, seed=4, lengthscale=0.7):
    D, lat, n, levels, nu = case
    torch.manual_seed(seed)
    k = NestedSphereRiemannianMaternKernel(D, lat, nu=nu, num_levels=levels).double()
    k.lengthscale = lengthscale
    return k


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_forward_against_numpy(case):
    """forward(x, x), forward(x1, x2) and diag=True against the numpy statement (projection of oracle/sphere.py, then the zonal series): the
    projection tolerance of test_gpu_gp_fit.py (rtol 1e-9, atol 1e-11 on entries of size <= 1) - the series adds a few ulp to it."""
    D, lat, n, levels, nu = case
    k = _kernel(case)
    x1 = _data(case)[0]
    x2 = _sphere(np.random.default_rng(D + n), 9, D)
    axes = [a.detach().numpy().reshape(-1) for a in k.axes]
    dists = [float(r) for r in k.distances_to_axis]
    kappa = float(k.lengthscale.detach())
    X1, X2 = torch.tensor(x1, device=DEV), torch.tensor(x2, device=DEV)
    with torch.no_grad():
        sym = k.forward(X1, X1).cpu().numpy()
        cross = k.forward(X1, X2).cpu().numpy()
        diag = k.forward(X1, X1, diag=True).cpu().numpy()
    want = ref.gram(x1, x1, axes, dists, kappa, nu, levels)
    assert sym.shape == (n, n) and cross.shape == (n, 9) and diag.shape == (n, 1)
    np.testing.assert_allclose(sym, want, rtol=1e-9, atol=1e-11)
    np.testing.assert_array_equal(sym, sym.T)
    np.testing.assert_allclose(cross, ref.gram(x1, x2, axes, dists, kappa, nu, levels), rtol=1e-9, atol=1e-11)
    np.testing.assert_allclose(diag[:, 0], np.diagonal(want), rtol=1e-9, atol=1e-11)


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_fit_objective_in_one_host_call_matches_autograd(case):
    """The comparison of test_nested_sphere_fit_objective_in_one_host_call_matches_autograd (test_gpu_gp_fit.py) for the Matern kernel, with its
    tolerances: value rtol 1e-9, scalar gradients 1e-7, axes 2e-5, atol = tol * max(1e-3, largest reference entry)."""
    from gabotorch_amd.manifold_optimization import manifold_gp_fit as mgf
    from gabotorch_amd.manifold_optimization.host_manifolds import Euclidean, PackedEuclideanSpheres, Product
    D, lat, n, levels, nu = case
    x, y = _data(case)[:2]
    rng = np.random.default_rng(D + n)
    torch.manual_seed(4)
    base = NestedSphereRiemannianMaternKernel(D, lat, nu=nu, num_levels=levels)
    gp = models.SingleTaskGP(torch.tensor(x, device=DEV), torch.tensor(y, device=DEV),
                             ScaleKernel(base, outputscale_prior=models.GammaPrior(2.0, 0.15)).double(), noise_prior=models.GammaPrior(1.1, 0.05))
    named = list(gp.named_parameters())
    params = [p for _, p in named]
    axis_ids = {id(a) for a in base.axes}
    factors = [getattr(base, nm.split(".")[-1] + "_manifold") if id(p) in axis_ids else Euclidean(int(p.numel())) for nm, p in named]
    manifold = Product(factors)
    fast = mgf._NestedSphereMllProblem.build(gp, [nm for nm, _ in named], params, manifold)
    assert fast is not None and fast.series == (lat, float(nu), levels)
    slow = mgf._MllProblem(gp, [nm for nm, _ in named], params, manifold)
    for trial in range(2):
        pt = [man.rand() if id(p) in axis_ids else rng.normal(0.3, 0.4, size=(int(p.numel()),)) for p, man in zip(params, factors)]
        fast.values_only = True
        c_values = fast.cost(pt)
        fast.values_only = False
        fast._recent = []
        c_fast, c_slow = fast.cost(pt), slow.cost(pt)
        print(f"trial {trial}: cost one call {c_fast:.15e}, autograd {c_slow:.15e}")
        np.testing.assert_allclose([c_values, c_fast], c_slow, rtol=1e-9)
        g_fast, g_slow = fast.egrad(pt), slow.egrad(pt)
        for a, b, (nm, p) in zip(g_fast, g_slow, named):
            tol = 2e-5 if id(p) in axis_ids else 1e-7
            gap = float(np.abs(np.ravel(a) - np.ravel(b)).max())
            print(f"  {nm}: largest gap {gap:.3e}, largest reference entry {float(np.abs(b).max()):.3e}")
            np.testing.assert_allclose(np.ravel(a), np.ravel(b), rtol=tol, atol=tol * max(1e-3, float(np.abs(b).max())), err_msg=nm)
        packed = PackedEuclideanSpheres(factors)
        fast.flat_layout(packed._bounds)
        fast._recent = []
        v = packed.pack(pt)
        assert fast.cost_flat(v) == c_fast
        np.testing.assert_array_equal(fast.egrad_flat(v), packed.pack(g_fast))


@pytest.mark.parametrize("case", SMALL, ids=_ids)
def test_entry_gradient_against_differences_of_the_numpy_objective(case):
    """The entry's gradient (axes projected onto their tangent spaces, kappa, outputscale, noise, mean) along 5 seeded directions against central
    differences of the numpy objective, fp64 on both sides.  The allowance is the reference's own: 10 x the disagreement of its differences at
    h = 1e-4 and h / 2, plus 1e-9 max(1, |D|); it may not exceed 1e-5 max(1, |D|) (the seeds were chosen on the CPU to stay under that cap)."""
    D, lat, n, levels, nu = case
    x, y, axes, scalars = _data(case)
    L = D - lat
    out = _entry(case, axes, scalars)
    want_ll = _numpy_ll(case, axes, scalars)
    print(f"ll: entry {out[0]:.15e}, numpy {want_ll:.15e}")
    np.testing.assert_allclose(out[0], want_ll, rtol=1e-9)
    assert out[1] == 0.0 and out[5] == 0.0
    g_axes = _tangent(axes, out[7:], D, L)
    g_scalars = np.array([out[6], out[2], out[3], out[4]])
    failures = []
    for k, ((ua, us), (d1, d2)) in enumerate(zip(_directions(case), _reference_differences(case))):
        got = float(g_axes @ ua + g_scalars @ us)
        scale = max(1.0, abs(d2))
        allowance = 10.0 * abs(d1 - d2) + 1e-9 * scale
        print(f"direction {k}: entry {got:.12e}, differences {d1:.12e} (h) {d2:.12e} (h/2), gap {abs(got - d2):.3e}, allowance {allowance:.3e}, "
              f"cap {1e-5 * scale:.3e}")
        if allowance > 1e-5 * scale:
            failures.append(f"direction {k}: the reference's own differences disagree by {abs(d1 - d2):.3e}: allowance {allowance:.3e} over the cap")
        elif abs(got - d2) > allowance:
            failures.append(f"direction {k}: {got:.12e} against {d2:.12e}, gap {abs(got - d2):.3e} > {allowance:.3e}")
    assert not failures, "\n".join(failures)
    # the value alone: the same first six numbers, zeros behind them
    values = _entry(case, axes, scalars, want_grad=0)
    assert values[:6].tobytes() == out[:6].tobytes()
    assert not values[6:].any()


@pytest.mark.parametrize("case", [c for c in CASES if c[2] in (65, 190)], ids=_ids)
def test_two_calls_return_the_same_bytes(case):
    """fixed summation order in the adjoint launch (lanes, then rows): no atomics on the numbers"""
    axes, scalars = _data(case)[2:]
    first = _entry(case, axes, scalars)
    second = _entry(case, axes, scalars)
    assert np.isfinite(first).all() and first[5] == 0.0 and np.abs(first[7:]).max() > 0.0 and first[6] != 0.0
    assert first.tobytes() == second.tobytes()


def test_fit_selects_the_one_call_problem_and_descends(monkeypatch):
    from gabotorch_amd.manifold_optimization import manifold_gp_fit as mgf
    from gabotorch_amd.manifold_optimization.conjugate_gradient import ConjugateGradient
    case = CASES[0]
    D, lat, n, levels, nu = case
    x, y = _data(case)[:2]
    built = []
    build = mgf._NestedSphereMllProblem.build
    monkeypatch.setattr(mgf._NestedSphereMllProblem, "build", staticmethod(lambda *a: built.append(build(*a)) or built[-1]))
    np.random.seed(3)
    torch.manual_seed(3)
    base = NestedSphereRiemannianMaternKernel(D, lat, nu=nu, num_levels=levels)
    gp = models.SingleTaskGP(torch.tensor(x, device=DEV), torch.tensor(y, device=DEV),
                             ScaleKernel(base, outputscale_prior=models.GammaPrior(2.0, 0.15)).double(), noise_prior=models.GammaPrior(1.1, 0.05))
    _, info = mgf.fit_gpytorch_manifold(gp, solver=ConjugateGradient(maxiter=15), nb_init_candidates=20)
    assert len(built) == 1 and isinstance(built[0], mgf._NestedSphereMllProblem) and built[0].series is not None
    print(f"fit: init cost {info['init_cost']:.9f} -> {info['fopt']:.9f} in {info['cost_evals']} cost evaluations")
    assert np.isfinite(info["fopt"]) and info["fopt"] <= info["init_cost"]
    for a in base.axes:
        assert abs(float(a.detach().double().norm()) - 1.0) < 1e-12
    assert float(base.lengthscale.detach()) > 0.0


def test_hd_gabo_sphere_loop_with_the_matern_kernel():
    """examples/hd_gabo_sphere.py with kernel="matern": no BETA_MIN anywhere on the path, and the fitted kernel's Gram matrices are positive
    semi-definite up to rounding (n eps lambda_max) wherever the fit left the axes and the lengthscale."""
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import hd_gabo_sphere
    state = {}
    x, y, best = hd_gabo_sphere.run(dim=5, latent=3, iters=3, kernel="matern", verbose=False, fit_iters=15, state=state)
    assert x.shape == (8, 5) and y.shape == (8,)
    np.testing.assert_allclose(np.linalg.norm(x.cpu().numpy(), axis=1), 1.0, atol=1e-12)
    assert all(b2 <= b1 + 1e-12 for b1, b2 in zip(best, best[1:])) and np.isfinite(best[-1])
    base = state["kernel"].base_kernel
    assert type(base) is NestedSphereRiemannianMaternKernel
    fresh = torch.tensor(_sphere(np.random.default_rng(8), 40, 5), device=x.device)
    with torch.no_grad():
        for pts in (x, fresh):
            gram = base.forward(pts, pts).cpu().numpy()
            lam = np.linalg.eigvalsh(gram)
            print(f"{gram.shape[0]} points: smallest eigenvalue {lam[0]:.3e}, largest {lam[-1]:.3e}")
            np.testing.assert_array_equal(gram, gram.T)
            assert lam[0] >= -16 * gram.shape[0] * np.finfo(np.float64).eps * lam[-1]
