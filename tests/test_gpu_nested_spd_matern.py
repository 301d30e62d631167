"""NestedSpdLogEuclideanMaternKernel, its fused Gram (gabo_nested_spd_matern_gram) and its one-call fit evaluation
(gabo_nested_spd_fit_evaluate_matern) on the GPU, against the numpy objective of tests/_cpu_nested_spd_matern.py and against torch autograd
through the separate launches.

Cases (D, d, n, nu) - the smallest at which each part can go wrong:
    (5, 2, 12, 2.5)     the shape of examples/hd_gabo_spd.py
    (5, 2, 12, 0.5)     the diagonal term of the adjoint launch (w(r_ii) eps is not small for nu = 1/2)
    (20, 2, 7, 1.5)     config 5's dimension
    (12, 3, 65, 2.5)    one column past a wave
    (9, 4, 20, 0.5)     the largest latent dimension of the fused Gram
    (6, 5, 10, 1.5)     latent dimension above 4: the composed forward, 15 features
    (32, 2, 9, 2.5)     D at its limit
    (10, 2, 190, 1.5)   the tiled likelihood above 160 points
    (6, 2, 260, 2.5)    a second 256-column chunk in the adjoint kernel
    (5, 2, 1, 2.5), (5, 2, 1, 0.5)   a single point
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from gabotorch_amd import _lib, models, ops
from gabotorch_amd._compat import ScaleKernel
from gabotorch_amd.kernel_utils.kernels_spd import NestedSpdLogEuclideanGaussianKernel, NestedSpdLogEuclideanMaternKernel
from tests import _cpu_flat_matern as fm
from tests import _cpu_nested_spd_matern as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES, SINGLE = ref.CASES, ref.SINGLE
_ids = lambda c: "D{}-d{}-n{}-nu{}".format(*c)     # noqa: E731
T = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device=DEV)     # noqa: E731


def _kernel(case):
    """the kernel at the case's W and lengthscale (parameters on the host, as the examples keep them)"""
    D, d, n, nu = case
    torch.manual_seed(4)
    k = NestedSpdLogEuclideanMaternKernel(D, d, nu=nu).double()
    k.projection_matrix = torch.tensor(np.array(ref.data(case)[2]))
    k.lengthscale = ref.SCALARS[0]
    return k


def _entry(case, w, scalars, want_grad=1):
    """gabo_nested_spd_fit_evaluate_matern called directly -> out_host (7 + D d)"""
    D, d, n, nu = case
    lib = _lib.load()
    x, y = ref.data(case)[:2]
    dev = torch.device(DEV)
    X, XM, Y = T(fm.to_mandel(x)), T(x), T(y)
    ws = torch.empty(int(lib.gabo_nested_spd_fit_workspace_bytes(n, D, d)), dtype=torch.uint8, device=dev)
    pinned = torch.empty(2 * D * d + 7, dtype=torch.float64).pin_memory()
    out = np.full(7 + D * d, np.nan)
    w = np.ascontiguousarray(w, dtype=np.float64)
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)   # noqa: E731
    with torch.cuda.device(dev):
        _lib.check(lib.gabo_nested_spd_fit_evaluate_matern(
            X.data_ptr(), XM.data_ptr(), Y.data_ptr(), ptr(w), n, D, d, float(scalars[0]), int(round(2 * nu)), float(scalars[1]), float(scalars[2]),
            float(scalars[3]), want_grad, ptr(out), ws.data_ptr(), ws.numel(), pinned.data_ptr(), pinned.numel(), ops._stream_ptr(dev)),
            "gabo_nested_spd_fit_evaluate_matern")
    return out


@pytest.mark.parametrize("case", CASES + SINGLE, ids=_ids)
def test_forward_against_numpy(case):
    """forward(x, x), forward(x1, x2) and the diagonal form against the numpy statement at the tolerance of test_gpu_nested_gram.py against the
    oracle (rtol 1e-9, atol 1e-12); exact symmetry; the fused path against the differentiable chain (rtol 1e-12, atol 1e-14, same file); the
    NaN rule of the Gaussian nested kernel; a batch of two point sets."""
    D, d, n, nu = case
    k = _kernel(case)
    x1, _, w, scalars = ref.data(case)
    x2 = fm.random_spd(np.random.default_rng(D + n), 9, D, 0.1, 4.0)
    X1, X2 = T(fm.to_mandel(x1)), T(fm.to_mandel(x2))
    with torch.no_grad():
        sym = k.forward(X1, X1)
        cross = k.forward(X1, X2)
        diag = k.forward(X1, X1, diagonal_distance=True)
    assert not sym.requires_grad and not cross.requires_grad
    assert sym.shape == (n, n) and cross.shape == (n, 9) and diag.shape == (n, 1)
    sym_np, cross_np = sym.cpu().numpy(), cross.cpu().numpy()
    want_sym, want_cross = ref.gram(x1, x1, w, scalars[0], nu), ref.gram(x1, x2, w, scalars[0], nu)
    print(f"largest gap to numpy: sym {np.abs(sym_np - want_sym).max():.3e}, cross {np.abs(cross_np - want_cross).max():.3e}")
    np.testing.assert_allclose(sym_np, want_sym, rtol=1e-9, atol=1e-12)
    np.testing.assert_array_equal(sym_np, sym_np.T)
    np.testing.assert_allclose(cross_np, want_cross, rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(diag.cpu().numpy()[:, 0], np.diagonal(want_sym), rtol=1e-9, atol=1e-12)
    # the parameters require a gradient: the differentiable chain
    graph_sym, graph_cross = k.forward(X1, X1), k.forward(X1, X2)
    assert graph_sym.requires_grad and graph_cross.requires_grad
    print(f"largest gap fused - chain: {np.abs(sym_np - graph_sym.detach().cpu().numpy()).max():.3e}")
    np.testing.assert_allclose(sym_np, graph_sym.detach().cpu().numpy(), rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(cross_np, graph_cross.detach().cpu().numpy(), rtol=1e-12, atol=1e-14)
    # a row of x2 that is not SPD: NaN where the Gaussian nested kernel has NaN
    bad = fm.to_mandel(x2)
    bad[3] = -bad[3]
    B = T(bad)
    torch.manual_seed(4)
    gauss = NestedSpdLogEuclideanGaussianKernel(D, d).double()
    gauss.projection_matrix = torch.tensor(np.array(w))
    with torch.no_grad():
        mask = torch.isnan(k.forward(X1, B)).cpu().numpy()
        mask_gauss = torch.isnan(gauss.forward(X1, B)).cpu().numpy()
    np.testing.assert_array_equal(mask, mask_gauss)
    assert mask[:, 3].all() and not np.delete(mask, 3, axis=1).any()
    # a batch of two point sets equals the two single calls
    if n >= 2:
        h = n // 2
        with torch.no_grad():
            both = k.forward(torch.stack([X1[:h], X1[h:2 * h]]), torch.stack([X2[:4], X2[4:8]])).cpu().numpy()
            one, two = k.forward(X1[:h], X2[:4]).cpu().numpy(), k.forward(X1[h:2 * h], X2[4:8]).cpu().numpy()
        np.testing.assert_allclose(both[0], one, rtol=1e-13, atol=1e-15)          # (the tolerance of the same check in test_gpu_nested_gram.py)
        np.testing.assert_allclose(both[1], two, rtol=1e-13, atol=1e-15)


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_fit_objective_in_one_host_call_matches_autograd(case):
    """The comparison of test_nested_spd_fit_objective_without_autograd_matches_the_autograd_objective (test_gpu_gp_fit.py) for the Matern
    kernel, with its tolerances (cost rtol 1e-10, gradients rtol 1e-7, atol 1e-9), against autograd (_MllProblem) and against the same chain
    launch by launch (native = False); a values-only call returns the same cost."""
    from gabotorch_amd.manifold_optimization import manifold_gp_fit as mgf
    from gabotorch_amd.manifold_optimization.host_manifolds import Euclidean, Product
    D, d, n, nu = case
    x, y = ref.data(case)[:2]
    rng = np.random.default_rng(D + n)
    torch.manual_seed(2)
    base = NestedSpdLogEuclideanMaternKernel(D, d, nu=nu)
    gp = models.SingleTaskGP(T(fm.to_mandel(x)), T(y), ScaleKernel(base, outputscale_prior=models.GammaPrior(2.0, 0.15)).double(),
                             noise_prior=models.GammaPrior(1.1, 0.05))
    named = list(gp.named_parameters())
    names, params = [nm for nm, _ in named], [p for _, p in named]
    factors = [base.raw_projection_matrix_manifold if p is base.raw_projection_matrix else Euclidean(int(p.numel())) for p in params]
    manifold = Product(factors)
    fast = mgf._NestedSpdMllProblem.build(gp, names, params, manifold)
    assert fast is not None and fast.matern == nu and fast.native and not fast.log_euclidean
    slow = mgf._MllProblem(gp, names, params, manifold)
    for trial in range(2):
        pt = [man.rand() if p is base.raw_projection_matrix else rng.normal(0.3, 0.5, size=(int(p.numel()),)) for p, man in zip(params, factors)]
        fast.values_only = True
        c_values = fast.cost(pt)
        fast.values_only = False
        fast._recent = []
        c_fast, c_slow = fast.cost(pt), slow.cost(pt)
        print(f"trial {trial}: cost one call {c_fast:.15e}, autograd {c_slow:.15e}, relative gap {abs(c_fast - c_slow) / abs(c_slow):.3e}")
        assert c_values == c_fast
        np.testing.assert_allclose(c_fast, c_slow, rtol=1e-10)
        g_fast, g_slow = fast.egrad(pt), slow.egrad(pt)
        assert fast._recent
        fast.native = False
        c_chain, g_chain = fast.cost(pt), fast.egrad(pt)
        fast.native = True
        np.testing.assert_allclose(c_fast, c_chain, rtol=1e-10)
        for a, b, c, nm in zip(g_fast, g_slow, g_chain, names):
            a, b, c = np.ravel(a), np.ravel(b), np.ravel(c)
            print(f"  {nm}: largest gap to autograd {np.abs(a - b).max():.3e}, to the launch-by-launch chain {np.abs(a - c).max():.3e}, "
                  f"largest reference entry {np.abs(b).max():.3e}")
            np.testing.assert_allclose(a, b, rtol=1e-7, atol=1e-9, err_msg=nm)
            np.testing.assert_allclose(a, c, rtol=1e-7, atol=1e-9, err_msg=nm)


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_entry_gradient_against_differences_of_the_numpy_objective(case):
    """The entry's gradient (W part along tangent directions of the Grassmannian, lengthscale, outputscale, noise, mean) along 5 seeded
    directions against central differences of the numpy objective, fp64 on both sides.  The allowance is the reference's own: 10 x the
    disagreement of its differences at h = 1e-4 and h / 2, plus 1e-9 max(1, |D|); it may not exceed 1e-5 max(1, |D|)
    (test_nested_spd_matern_cpu.py asserts that on the CPU; nu = 1/2 stays at n <= 20, where it holds)."""
    D, d, n, nu = case
    w, scalars = ref.data(case)[2:]
    out = _entry(case, w, scalars)
    want_ll = ref.objective(case, w, scalars)
    print(f"ll: entry {out[0]:.15e}, numpy {want_ll:.15e}, relative gap {abs(out[0] - want_ll) / abs(want_ll):.3e}")
    np.testing.assert_allclose(out[0], want_ll, rtol=1e-9)
    assert out[1] == 0.0 and out[5] == 0.0
    g_w = out[7:].reshape(D, d)
    g_scalars = np.array([out[6], out[2], out[3], out[4]])
    failures = []
    for k, ((uw, us), (d1, d2)) in enumerate(zip(ref.directions(case), ref.reference_differences(case))):
        got = float((g_w * uw).sum() + g_scalars @ us)
        allowance, cap = ref.allowance(d1, d2)
        print(f"direction {k}: entry {got:.12e}, differences {d1:.12e} (h) {d2:.12e} (h/2), gap {abs(got - d2):.3e}, allowance {allowance:.3e}, "
              f"cap {cap:.3e}")
        if allowance > cap:
            failures.append(f"direction {k}: the reference's own differences disagree by {abs(d1 - d2):.3e}: allowance {allowance:.3e} over the cap")
        elif not abs(got - d2) <= allowance:
            failures.append(f"direction {k}: {got:.12e} against {d2:.12e}, gap {abs(got - d2):.3e} > {allowance:.3e}")
    assert not failures, "\n".join(failures)
    # the value alone: the same first six numbers, zeros behind them
    values = _entry(case, w, scalars, want_grad=0)
    assert values[:6].tobytes() == out[:6].tobytes()
    assert not values[6:].any()


@pytest.mark.parametrize("case", SINGLE, ids=_ids)
def test_single_point(case):
    """k(x, x) does not depend on the features: the gradient with respect to W is exactly zero.  With nu = 1/2 the weight at r_ii = |eps| is
    a e^-x / r, of order a / d per entry: this fails unless the adjoint launch skips the pair j = i."""
    w, scalars = ref.data(case)[2:]
    out = _entry(case, w, scalars)
    print(f"ll {out[0]:.15e}, d ll / d lengthscale {out[6]:.3e}, largest |gW| {np.abs(out[7:]).max():.3e}")
    np.testing.assert_allclose(out[0], ref.objective(case, w, scalars), rtol=1e-9)
    assert np.isfinite(out).all() and out[5] == 0.0
    np.testing.assert_array_equal(out[7:], np.zeros(out.size - 7))


@pytest.mark.parametrize("case", [c for c in CASES if c[2] in (65, 190, 260)], ids=_ids)
def test_two_calls_return_the_same_bytes(case):
    """fixed summation order in the adjoint launch (columns in order, then rows in order): no atomics on the numbers"""
    w, scalars = ref.data(case)[2:]
    first = _entry(case, w, scalars)
    second = _entry(case, w, scalars)
    assert np.isfinite(first).all() and first[5] == 0.0 and np.abs(first[7:]).max() > 0.0 and first[6] != 0.0
    assert first.tobytes() == second.tobytes()


def test_fit_selects_the_one_call_problem_and_descends(monkeypatch):
    from gabotorch_amd.manifold_optimization import manifold_gp_fit as mgf
    from gabotorch_amd.manifold_optimization.conjugate_gradient import ConjugateGradient
    case = CASES[0]
    D, d, n, nu = case
    x, y = ref.data(case)[:2]
    built = []
    build = mgf._NestedSpdMllProblem.build
    monkeypatch.setattr(mgf._NestedSpdMllProblem, "build", staticmethod(lambda *a: built.append(build(*a)) or built[-1]))
    np.random.seed(3)
    torch.manual_seed(3)
    base = NestedSpdLogEuclideanMaternKernel(D, d, nu=nu)
    gp = models.SingleTaskGP(T(fm.to_mandel(x)), T(y), ScaleKernel(base, outputscale_prior=models.GammaPrior(2.0, 0.15)).double(),
                             noise_prior=models.GammaPrior(1.1, 0.05))
    _, info = mgf.fit_gpytorch_manifold(gp, solver=ConjugateGradient(maxiter=15), nb_init_candidates=20)
    assert len(built) == 1 and isinstance(built[0], mgf._NestedSpdMllProblem) and built[0].matern == nu
    print(f"fit: init cost {info['init_cost']:.9f} -> {info['fopt']:.9f} in {info['cost_evals']} cost evaluations")
    assert np.isfinite(info["fopt"]) and info["fopt"] <= info["init_cost"]
    w = base.projection_matrix.detach().double().cpu().numpy()
    np.testing.assert_allclose(w.T @ w, np.eye(d), rtol=0, atol=1e-10)
    assert float(base.lengthscale.detach()) > 0.0


def test_hd_gabo_spd_loop_with_the_matern_kernel(monkeypatch):
    """examples/hd_gabo_spd.py with kernel="matern52": the loop runs, and the fitted kernel's Gram matrices are symmetric and positive
    semi-definite up to rounding (16 n eps lambda_max) wherever the fit left the projection and the lengthscale."""
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import hd_gabo_spd
    fitted = []
    fit = hd_gabo_spd.fit_gpytorch_manifold
    monkeypatch.setattr(hd_gabo_spd, "fit_gpytorch_manifold", lambda model, **kw: fitted.append(model.covar_module) or fit(model, **kw))
    x, y, best = hd_gabo_spd.run(dim=5, latent=2, iters=3, rec_iters=2, verbose=False, kernel="matern52")
    assert x.shape == (8, 15) and y.shape == (8,)
    assert all(b2 <= b1 + 1e-12 for b1, b2 in zip(best, best[1:])) and np.isfinite(best[-1])
    assert len(fitted) == 3
    base = fitted[-1].base_kernel
    assert type(base) is NestedSpdLogEuclideanMaternKernel and base.nu == 2.5
    fresh = T(fm.to_mandel(fm.random_spd(np.random.default_rng(8), 40, 5, 0.1, 4.0)))
    with torch.no_grad():
        for pts in (x, fresh):
            gram = base.forward(pts, pts).cpu().numpy()
            lam = np.linalg.eigvalsh(gram)
            print(f"{gram.shape[0]} points: smallest eigenvalue {lam[0]:.3e}, largest {lam[-1]:.3e}")
            np.testing.assert_array_equal(gram, gram.T)
            assert lam[0] >= -16 * gram.shape[0] * np.finfo(np.float64).eps * lam[-1]
