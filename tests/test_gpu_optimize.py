"""Acquisition maximisation on the MI355X: HIP kernels + HIP manifold operations under the lock-step trust regions, against
(a) the reference solvers' optima (tests/golden/trust_regions.npz) and (b) the same pipeline on the torch-CPU stand-ins."""
import numpy as np
import pytest
import torch

from gabotorch_amd import _lib, manifolds, models, ops
from gabotorch_amd.kernel_utils.kernels_spd import SpdAffineInvariantGaussianKernel
from gabotorch_amd.kernel_utils.kernels_sphere import SphereGaussianKernel
from gabotorch_amd.manifold_optimization.batched_trust_regions import BatchedProblem, BatchedTrustRegions
from gabotorch_amd.manifold_optimization.manifold_optimize import joint_optimize_manifold
from gabotorch_amd.Riemannian_utils import spd_constraints_utils_torch as scut
from gabotorch_amd.Riemannian_utils.spd_utils_torch import (symmetric_matrix_to_vector_mandel_torch,
                                                            vector_to_symmetric_matrix_mandel_torch)
from oracle import spd as ospd
from tests._cpu_manifolds import CpuSpd, CpuSphere, _sym

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def t(x):
    return torch.tensor(np.ascontiguousarray(x), dtype=torch.float64, device=DEV)


@pytest.mark.parametrize("n", [3, 5])
@pytest.mark.parametrize("approx", [False, True])
def test_sphere_hip_path_matches_reference_optima(golden, n, approx):
    g = golden("trust_regions.npz")
    Y, w, beta = t(g[f"sph{n}_Y"]), t(g[f"sph{n}_w"]), float(g[f"sph{n}_beta"])
    cost = lambda x: -(ops.sphere_kernel(x, Y, beta) * w).sum(-1)      # noqa: E731  R x 12 kernel strip per call
    x = BatchedTrustRegions().solve(BatchedProblem(manifolds.Sphere(n), cost, approx_hessian=approx), t(g[f"sph{n}_x0"]))
    key = "fd" if approx else "exact"
    np.testing.assert_allclose(cost(x).cpu().numpy(), g[f"sph{n}_{key}_f"], rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(x.cpu().numpy(), g[f"sph{n}_{key}_x"], rtol=0, atol=1e-6)


@pytest.mark.parametrize("d", [2, 3])
def test_spd_hip_path_matches_reference_optima(golden, d):
    """SECONDARY check against the reference AS IT IS (trust_regions.npz: its solvers with the float32 eigenvalue buffer of
    spd_utils_torch.py:108, so its own costs / FD Hessians carry 1e-7 / 1e-3 relative noise - DESIGN 2): 2e-3 on the points and on the
    constrained costs is the reference's own f32-vs-f64 distance, not this solver's accuracy.  The primary, tight comparison is against the
    reference's float64 traces: tests/test_gpu_tr_traces.py (every iterate, 1e-6) and tests/test_gpu_ei_optimum.py (best-of-restarts, 1e-5)."""
    g = golden("trust_regions.npz")
    Ym = t(ospd.symmetric_matrix_to_vector_mandel(g[f"spd{d}_Y"]))
    w, beta = t(g[f"spd{d}_w"]), float(g[f"spd{d}_beta"])

    def cost(x):                                     # x: R x d x d matrices (the solver's representation)
        v = symmetric_matrix_to_vector_mandel_torch(x)
        return -(ops.spd_ai_kernel(v, Ym, beta) * w).sum(-1)
    man = manifolds.PositiveDefinite(d)
    ops.set_error_checking(False)
    try:
        x = BatchedTrustRegions(mingradnorm=1e-4, maxiter=100).solve(BatchedProblem(man, cost, approx_hessian=True), t(g[f"spd{d}_x0"]))
        np.testing.assert_allclose(cost(x).cpu().numpy(), g[f"spd{d}_fd_f"], rtol=1e-6)
        np.testing.assert_allclose(x.cpu().numpy(), g[f"spd{d}_fd_x"], rtol=0, atol=2e-3)
        mx = float(g[f"spd{d}_maxeig"])
        xc = BatchedTrustRegions(mingradnorm=1e-4, maxiter=100).solve(
            BatchedProblem(man, cost, approx_hessian=True), t(g[f"spd{d}_con_x0"]),
            ineq_constraints=[lambda x: scut.max_eigenvalue_constraint_torch(x, mx)])
        np.testing.assert_allclose(cost(xc).cpu().numpy(), g[f"spd{d}_con_f"], rtol=2e-3)
    finally:
        ops.set_error_checking(True)


class _CpuSpdKernel:
    """torch-CPU statement of exp(-beta d_AI^2) on Mandel inputs (test stand-in, differentiable by autograd)."""

    def __init__(self, beta):
        self.beta = beta

    def forward(self, x1, x2, **kw):
        a = torch.tensor(ospd.vector_to_symmetric_matrix_mandel(x1.detach().numpy())) if not x1.requires_grad else _mandel_to_mat(x1)
        b = torch.tensor(ospd.vector_to_symmetric_matrix_mandel(x2.detach().numpy())) if not x2.requires_grad else _mandel_to_mat(x2)
        L = torch.linalg.cholesky(a)
        Li = torch.linalg.inv(L)
        m = Li.unsqueeze(-3) @ b.unsqueeze(-4) @ Li.transpose(-1, -2).unsqueeze(-3)
        lam = torch.linalg.eigvalsh(_sym(m))
        return torch.exp(-self.beta * ((torch.log(lam) ** 2).sum(-1) + 1e-15))


def _mandel_to_mat(v):
    d = ospd.mandel_dim(v.shape[-1])
    r, c = ospd.mandel_index(d)
    scale = torch.tensor(np.where(r == c, 1.0, 1 / 2 ** 0.5))
    m = torch.zeros(v.shape[:-1] + (d, d), dtype=v.dtype)
    m[..., r, c] = v * scale
    m[..., c, r] = v * scale
    return m


def _mat_to_mandel(m):
    d = m.shape[-1]
    r, c = ospd.mandel_index(d)
    scale = torch.tensor(np.where(r == c, 1.0, 2 ** 0.5))
    return 0.5 * (m[..., r, c] + m[..., c, r]) * scale


def test_joint_optimize_spd_gp_ei_matches_cpu_pipeline():
    """Config-4-shaped sweep (GP + EI on S^3_++, max-eigenvalue constraint, FD Hessian, spd_sample as manifold.rand) on the HIP
    path vs the identical pipeline on torch-CPU stand-ins, same seeds => same initial conditions => same optimum."""
    d, n_train, R = 3, 12, 8
    rng = np.random.default_rng(0)
    q = np.linalg.qr(rng.standard_normal((n_train, d, d)))[0]
    Xm = np.einsum("nab,nb,ncb->nac", q, rng.uniform(0.2, 3.0, (n_train, d)), q)
    X = ospd.symmetric_matrix_to_vector_mandel(0.5 * (Xm + Xm.transpose(0, 2, 1)))
    y = np.log(np.linalg.eigvalsh(Xm)).sum(1) ** 2 + 0.1 * rng.standard_normal(n_train)
    beta = 0.5 + np.log(2)
    results = {}
    for where in ("hip", "cpu"):
        np.random.seed(7)
        torch.manual_seed(7)
        if where == "hip":
            man = manifolds.PositiveDefinite(d)
            kern = SpdAffineInvariantGaussianKernel(beta_min=0.5)
            assert abs(kern.beta.item() - beta) < 1e-6
            kern.beta = beta
            pre, post = vector_to_symmetric_matrix_mandel_torch, symmetric_matrix_to_vector_mandel_torch
            con = lambda x: scut.max_eigenvalue_constraint_torch(x, 3.5)        # noqa: E731
            tx, ty, opts = t(X), t(y), {"device": DEV}
        else:
            man = CpuSpd(d)
            kern = _CpuSpdKernel(kern_beta)
            pre, post = _mandel_to_mat, _mat_to_mandel
            con = lambda x: 3.5 - torch.linalg.eigvalsh(x)[..., -1]             # noqa: E731
            tx, ty, opts = torch.tensor(X), torch.tensor(y), {}
        kern_beta = float(kern.beta.item()) if where == "hip" else kern_beta
        man.min_eig, man.max_eig = 0.2, 3.0

        def rand(self=man):
            return ospd.spd_sample(d, self.min_eig, self.max_eig)
        man.rand = rand
        gp = models.ExactGP(tx, ty, kern, outputscale=1.0, noise=1e-2)
        acq = models.ExpectedImprovement(gp, best_f=float(y.min()), maximize=False)
        ops.set_error_checking(False)
        best = joint_optimize_manifold(acq, man, BatchedTrustRegions(mingradnorm=1e-4, maxiter=100), q=1, num_restarts=R,
                                       raw_samples=64, bounds=None, options=opts, inequality_constraints=[con],
                                       pre_processing_manifold=pre, post_processing_manifold=post, approx_hessian=True)
        ops.set_error_checking(True)
        results[where] = (best.detach().cpu().numpy(), float(acq(best[None].to(tx.device)).item()))
    (bh, vh), (bc, vc) = results["hip"], results["cpu"]
    assert bh.shape == (1, d * (d + 1) // 2)
    np.testing.assert_allclose(vh, vc, rtol=1e-5)                         # acquisition optimum: BASELINE.json tolerance
    np.testing.assert_allclose(bh, bc, rtol=0, atol=2e-3)
    assert np.linalg.eigvalsh(ospd.vector_to_symmetric_matrix_mandel(bh[0])).min() > 0


def test_joint_optimize_sphere_gp_ei_exact_hessian():
    """Config-1-shaped sweep on S^2 (stock trust regions, exact Hessian-vector products through the double-differentiable
    sphere kernel): the returned candidate is on the sphere and at least as good as every initial condition."""
    rng = np.random.default_rng(1)
    X = rng.standard_normal((20, 3)); X /= np.linalg.norm(X, axis=1, keepdims=True)
    y = np.arccos(np.clip(X[:, 0], -1, 1)) ** 2 + 0.05 * rng.standard_normal(20)
    kern = SphereGaussianKernel(beta_min=6.5)
    gp = models.ExactGP(t(X), t(y), kern, outputscale=1.0, noise=1e-2)
    acq = models.ExpectedImprovement(gp, best_f=float(y.min()), maximize=False)
    np.random.seed(3)
    torch.manual_seed(3)
    solver = BatchedTrustRegions()
    best = joint_optimize_manifold(acq, manifolds.Sphere(3), solver, q=1, num_restarts=16, raw_samples=200, bounds=None,
                                   options={"device": DEV})
    assert best.shape == (1, 3) and abs(best.norm().item() - 1) < 1e-12
    raw = torch.tensor(np.stack([manifolds.Sphere(3).rand() for _ in range(500)]), device=DEV)[:, None]
    assert acq(best[None]).item() >= acq(raw).max().item() - 1e-12


def test_hip_graph_evaluations_match_eager():
    """options={"hip_graphs": True}: the acquisition value / gradient evaluations are captured once and replayed; same optimum."""
    from tools.sweep_bench import run_sweep
    _, best_e, val_e, log_e = run_sweep(DEV, num_restarts=32, raw_samples=256)
    _, best_g, val_g, log_g = run_sweep(DEV, num_restarts=32, raw_samples=256, hip_graphs=True)
    np.testing.assert_allclose(best_g.cpu().numpy(), best_e.cpu().numpy(), rtol=0, atol=1e-9)
    np.testing.assert_allclose(val_g, val_e, rtol=1e-10)
    assert int(log_g["iterations"]) == int(log_e["iterations"])          # same trust-region trajectory


# ------------------------------------------------------------------------------------------- fused acquisition chain
def _spd_gp(d=4, n_train=23, seed=5):
    rng = np.random.default_rng(seed)
    q = np.linalg.qr(rng.standard_normal((n_train, d, d)))[0]
    Xm = np.einsum("nab,nb,ncb->nac", q, rng.uniform(0.2, 3.0, (n_train, d)), q)
    X = ospd.symmetric_matrix_to_vector_mandel(0.5 * (Xm + Xm.transpose(0, 2, 1)))
    y = np.log(np.linalg.eigvalsh(Xm)).sum(1) ** 2 + 0.1 * rng.standard_normal(n_train)
    return rng, X, y


@pytest.mark.parametrize("which", ["ei_min", "ei_max", "mean_min", "laplace_ei_min"])
def test_fused_spd_acquisition_matches_autograd(which):
    from gabotorch_amd.fused_acquisition import FusedAcquisition
    from gabotorch_amd.kernel_utils.kernels_spd import SpdAffineInvariantLaplaceKernel
    d = 4
    rng, X, y = _spd_gp(d)
    kern = (SpdAffineInvariantLaplaceKernel if which.startswith("laplace") else SpdAffineInvariantGaussianKernel)(beta_min=0.4)
    gp = models.ExactGP(t(X), t(y), kern, outputscale=1.7, noise=1e-2)
    if "ei" in which:
        acq = models.ExpectedImprovement(gp, best_f=float(y.min()), maximize=which.endswith("max"))
    else:
        acq = models.PosteriorMean(gp, maximize=False)
    post = symmetric_matrix_to_vector_mandel_torch
    fused = FusedAcquisition.build(acq, post, torch.device(DEV))
    assert fused is not None and fused.single_launch
    R = 70
    q = np.linalg.qr(rng.standard_normal((R, d, d)))[0]
    P = np.einsum("nab,nb,ncb->nac", q, rng.uniform(0.2, 3.0, (R, d)), q)
    if not which.startswith("laplace"):      # (exp(-beta d) has a kink at d = 0: no gradient to compare there)
        P[:5] = ospd.vector_to_symmetric_matrix_mandel(X[:5])      # candidates ON training points (variance clamp region)
    x = t(0.5 * (P + P.transpose(0, 2, 1)))
    xx = x.clone().requires_grad_(True)
    f_ref = -acq(post(xx)[:, None])
    (g_ref,) = torch.autograd.grad(f_ref.sum(), xx)
    f, g = fused.cost_egrad(x)
    scale = max(1.0, float(g_ref.abs().max()))
    np.testing.assert_allclose(f.cpu().numpy(), f_ref.detach().cpu().numpy(), rtol=1e-10, atol=1e-14)
    # autograd also differentiates k(x, x), which is constant: for exp(-beta d) that adds rounding noise of logm(I) amplified by
    # 1/d(x, x) = 3e7 (~5e-9 absolute); the fused chain treats k(x, x) as the constant it is
    atol = 1e-7 if which.startswith("laplace") else 1e-11
    np.testing.assert_allclose(g.cpu().numpy(), g_ref.cpu().numpy(), rtol=1e-8, atol=atol * scale)
    np.testing.assert_allclose(fused.cost(x).cpu().numpy(), f.cpu().numpy(), rtol=0, atol=0)
    # the single launch was handed the symmetric inverse A = L^-T L^-1 in place of the two factors (round 6: one product per training point
    # instead of two); with the factors themselves it computes the same posterior
    assert fused.kinv is not None
    held, fused.kinv = fused.kinv, None
    f_lt, g_lt = fused.cost_egrad(x)
    fused.kinv = held
    np.testing.assert_allclose(f_lt.cpu().numpy(), f.cpu().numpy(), rtol=1e-11, atol=1e-14)
    np.testing.assert_allclose(g_lt.cpu().numpy(), g.cpu().numpy(), rtol=1e-9, atol=1e-12 * scale)
    # the separate-launch chain (strip -> gabo_gp_acquisition -> kernel backward) serves d > 12; same numbers
    fused.single_launch = False
    f2, g2 = fused.cost_egrad(x)
    np.testing.assert_allclose(f2.cpu().numpy(), f_ref.detach().cpu().numpy(), rtol=1e-10, atol=1e-14)
    np.testing.assert_allclose(g2.cpu().numpy(), g_ref.cpu().numpy(), rtol=1e-8, atol=atol * scale)
    np.testing.assert_allclose(fused.egrad_mandel(ops.matrix_to_mandel(x)).cpu().numpy(), ops.matrix_to_mandel(g2).cpu().numpy(),
                               rtol=1e-12, atol=1e-14 * scale)


def test_fused_sphere_acquisition_matches_autograd():
    from gabotorch_amd.fused_acquisition import FusedAcquisition
    rng = np.random.default_rng(2)
    X = rng.standard_normal((150, 5)); X /= np.linalg.norm(X, axis=1, keepdims=True)       # n_train > 128: 256-thread blocks
    y = np.arccos(np.clip(X[:, 0], -1, 1)) ** 2 + 0.05 * rng.standard_normal(150)
    gp = models.ExactGP(t(X), t(y), SphereGaussianKernel(beta_min=1.2), outputscale=0.8, noise=1e-2)
    acq = models.ExpectedImprovement(gp, best_f=float(y.min()), maximize=False)
    fused = FusedAcquisition.build(acq, None, torch.device(DEV))
    assert fused is not None
    P = rng.standard_normal((40, 5)); P /= np.linalg.norm(P, axis=1, keepdims=True)
    x = t(P)
    xx = x.clone().requires_grad_(True)
    f_ref = -acq(xx[:, None])
    (g_ref,) = torch.autograd.grad(f_ref.sum(), xx)
    f, g = fused.cost_egrad(x)
    np.testing.assert_allclose(f.cpu().numpy(), f_ref.detach().cpu().numpy(), rtol=1e-10, atol=1e-14)
    np.testing.assert_allclose(g.cpu().numpy(), g_ref.cpu().numpy(), rtol=1e-8, atol=1e-11 * max(1.0, float(g_ref.abs().max())))


def test_fused_path_declines_what_it_does_not_know():
    from gabotorch_amd.fused_acquisition import FusedAcquisition
    _, X, y = _spd_gp()
    gp = models.ExactGP(t(X), t(y), SpdAffineInvariantGaussianKernel(beta_min=0.4), outputscale=1.0, noise=1e-2)
    acq = models.ExpectedImprovement(gp, best_f=0.0, maximize=False)
    assert FusedAcquisition.build(acq, lambda m: symmetric_matrix_to_vector_mandel_torch(m), torch.device(DEV)) is None   # user callable
    assert FusedAcquisition.build(lambda X_: X_.sum((-1, -2)), symmetric_matrix_to_vector_mandel_torch, torch.device(DEV)) is None


def test_sweep_with_fused_chain_matches_autograd_sweep():
    from tools.sweep_bench import run_sweep
    _, best_a, val_a, log_a = run_sweep(DEV, num_restarts=32, raw_samples=256, fused=False)
    _, best_f, val_f, log_f = run_sweep(DEV, num_restarts=32, raw_samples=256, fused=True)
    _, best_g, val_g, log_g = run_sweep(DEV, num_restarts=32, raw_samples=256, fused=True, hip_graphs=True)
    # two different evaluation orders stopped by |grad| < 1e-4: the optimum's coordinates agree to rounding noise / curvature ~ 1e-8
    np.testing.assert_allclose(best_f.cpu().numpy(), best_a.cpu().numpy(), rtol=0, atol=5e-8)
    np.testing.assert_allclose(val_f, val_a, rtol=1e-9)
    np.testing.assert_allclose(val_g, val_a, rtol=1e-9)
    assert int(log_f["iterations"]) == int(log_a["iterations"]) == int(log_g["iterations"])


def test_device_tcg_matches_torch_tcg():
    """csrc/spd_tcg.hip (whitened-coordinate tCG, one wave per restart) against the torch lock-step tCG on the same constrained
    sweep: same trust-region trajectory, same optimum."""
    from tools.sweep_bench import run_sweep
    _, best_t, val_t, log_t = run_sweep(DEV, num_restarts=48, raw_samples=256, device_tcg=False)
    _, best_d, val_d, log_d = run_sweep(DEV, num_restarts=48, raw_samples=256, device_tcg=True)
    _, best_g, val_g, log_g = run_sweep(DEV, num_restarts=48, raw_samples=256, device_tcg=True, hip_graphs=True)
    _, best_i, val_i, log_i = run_sweep(DEV, num_restarts=48, raw_samples=256, device_tcg=True, device_outer=False)   # tCG only
    np.testing.assert_allclose(val_i, val_t, rtol=1e-9)
    np.testing.assert_array_equal(log_i["per_restart_iterations"].cpu().numpy(), log_t["per_restart_iterations"].cpu().numpy())
    np.testing.assert_array_equal(log_g["per_restart_iterations"].cpu().numpy(), log_t["per_restart_iterations"].cpu().numpy())
    np.testing.assert_allclose(val_d, val_t, rtol=1e-9)
    np.testing.assert_allclose(val_g, val_t, rtol=1e-9)
    np.testing.assert_allclose(best_d.cpu().numpy(), best_t.cpu().numpy(), rtol=0, atol=1e-7)
    assert int(log_d["iterations"]) == int(log_t["iterations"]) == int(log_g["iterations"])
    np.testing.assert_array_equal(log_d["per_restart_iterations"].cpu().numpy(), log_t["per_restart_iterations"].cpu().numpy())
    # (two evaluation orders - the device kernels use the Householder/QL eigen-solver - stopped by |grad| < 1e-4: values agree to
    # |grad|^2 / curvature, ~1e-10 absolute)
    np.testing.assert_allclose(log_d["final_cost"].cpu().numpy(), log_t["final_cost"].cpu().numpy(), rtol=1e-9, atol=1e-12)


@pytest.mark.parametrize("constraint", [True, False])
def test_use_rand_on_the_device_tcg_plan_follows_the_torch_path(constraint):
    """use_rand=True (robust_trust_regions.py:173-219, 407-452): random tCG start (torch's generator, the same draws on both sides),
    no preconditioner, comparison with the Cauchy point.  The plan of device-resident tCG launches (gabo_spd_tcg_begin_rand + the steps
    without the preconditioner) against the generic torch lock-step statement of the same solver: same trajectory restart for restart."""
    from tools.sweep_bench import run_sweep
    from gabotorch_amd.manifold_optimization.batched_trust_regions import BatchedTrustRegions
    kw = dict(num_restarts=40, raw_samples=256, use_rand=True, constraint=constraint)
    taken = []
    real = BatchedTrustRegions._solve_device

    def spy(self, *a, **k):
        taken.append(self.use_rand)
        return real(self, *a, **k)
    _, best_t, val_t, log_t = run_sweep(DEV, device_tcg=False, **kw)
    BatchedTrustRegions._solve_device = spy
    try:
        _, best_d, val_d, log_d = run_sweep(DEV, **kw)
    finally:
        BatchedTrustRegions._solve_device = real
    assert taken == [True]                                   # (the device plan ran, with use_rand)
    assert "one_launch_solve" not in log_d
    np.testing.assert_array_equal(log_d["per_restart_iterations"].cpu().numpy(), log_t["per_restart_iterations"].cpu().numpy())
    np.testing.assert_allclose(val_d, val_t, rtol=1e-9)
    np.testing.assert_allclose(best_d.cpu().numpy(), best_t.cpu().numpy(), rtol=0, atol=1e-7)
    np.testing.assert_allclose(log_d["final_cost"].cpu().numpy(), log_t["final_cost"].cpu().numpy(), rtol=1e-9, atol=1e-12)
    # and the random start changes nothing about where the sweep ends (the plain solver, same seeds)
    _, _, val_p, log_p = run_sweep(DEV, num_restarts=40, raw_samples=256, constraint=constraint)
    np.testing.assert_allclose(val_d, val_p, rtol=1e-6)
    # The reference's start is 1e-6 of a unit vector - a device plan that ignored it would pass the comparison above.  With the draw
    # amplified to 0.05 on both sides the start decides the first steps.  (a) one tCG call, same inputs: the device launches against
    # the generic torch statement - step, Hessian applied to it, stop reason; (b) whole sweeps: the plans end where the generic one does.
    from gabotorch_amd.manifold_optimization import batched_trust_regions as btr
    real_rv, real_tcg = btr._randvec, BatchedTrustRegions._tcg
    seen = {}

    def spy_tcg(self, problem, x, g, Delta, active, mininner, maxinner, fc, gc, neq, Delta_cons, eta0=None):
        if not seen:
            seen.update(solver=self, problem=problem, eta0=eta0,
                        args=(x.clone(), g.clone(), Delta.clone(), active.clone(), mininner, maxinner, None if fc is None else fc.clone(),
                              [c.clone() for c in gc], neq, Delta_cons))
        return real_tcg(self, problem, x, g, Delta, active, mininner, maxinner, fc, gc, neq, Delta_cons, eta0=eta0)
    btr._randvec = lambda man, x: 5e4 * real_rv(man, x)
    BatchedTrustRegions._tcg = spy_tcg
    try:
        _, _, val_i5, log_i5 = run_sweep(DEV, device_outer=False, **kw)          # generic outer loop around the device tCG
        BatchedTrustRegions._tcg = real_tcg
        _, _, val_t5, log_t5 = run_sweep(DEV, device_tcg=False, **kw)
        _, _, val_d5, log_d5 = run_sweep(DEV, **kw)
    finally:
        btr._randvec, BatchedTrustRegions._tcg = real_rv, real_tcg
    prob, eta0 = seen["problem"], seen["eta0"]
    assert eta0 is not None and 0.04 < float(prob.manifold.norm(seen["args"][0], eta0).max()) < 0.06
    out = {}
    for name, flag in (("torch", False), ("device", True)):
        prob.device_tcg = flag
        out[name] = real_tcg(seen["solver"], prob, *seen["args"], eta0=eta0.clone())
    (eta_t, heta_t, stop_t), (eta_d, heta_d, stop_d) = out["torch"], out["device"]
    np.testing.assert_array_equal(stop_d.cpu().numpy(), stop_t.cpu().numpy())
    # (finite differences of the gradient at c = 2^-14 / |delta| amplify the rounding difference of the two evaluation orders by 1 / c:
    # 2e-10 / 4e-10 measured.  This comparison is what found the 2^-13 the device kernels had carried as their step since round 2 -
    # 1e-4 of H delta, invisible in optima and iteration counts)
    def rel_err(a_d, a_t):
        return ((a_d - a_t).flatten(1).abs().amax(1) / a_t.flatten(1).abs().amax(1).clamp(min=1e-300)).cpu().numpy()
    for a_d, a_t in ((eta_d, eta_t), (heta_d, heta_t)):
        assert rel_err(a_d, a_t).max() < 2e-8, rel_err(a_d, a_t).max()
    assert float((eta_t - eta0).abs().max()) > 1e-3                         # (tCG moved away from its start)
    prob.device_tcg = False
    plain = real_tcg(seen["solver"], prob, *seen["args"], eta0=None)
    assert float((plain[0] - eta_t).abs().max()) > 1e-3                     # (and the start matters at this size)
    prob.device_tcg = True
    plain_d = real_tcg(seen["solver"], prob, *seen["args"], eta0=None)      # the same for the zero start: step and H step of the device tCG
    np.testing.assert_array_equal(plain_d[2].cpu().numpy(), plain[2].cpu().numpy())
    assert rel_err(plain_d[0], plain[0]).max() < 2e-8 and rel_err(plain_d[1], plain[1]).max() < 2e-8
    it_t5 = log_t5["per_restart_iterations"].cpu().numpy()
    for log5, val5 in ((log_d5, val_d5), (log_i5, val_i5)):
        # (iteration counts: a restart whose gradient norm passes 1e-4 within rounding of an iteration boundary may stop one later)
        it5 = log5["per_restart_iterations"].cpu().numpy()
        assert np.abs(it5 - it_t5).max() <= 1 and (it5 == it_t5).mean() >= 0.9
        np.testing.assert_allclose(val5, val_t5, rtol=1e-8)


@pytest.mark.parametrize("strict", [False, True])
def test_device_solve_graph_plans_match_torch_path(strict):
    """Every execution plan of the device-resident solve (eager; graphs with the constraint callables between replays; graphs
    with the callables captured) follows the torch lock-step solver restart for restart."""
    from tools.sweep_bench import run_sweep
    kw = dict(num_restarts=40, raw_samples=256, strict=strict)
    _, _, val_t, log_t = run_sweep(DEV, device_tcg=False, **kw)
    ref_iters = log_t["per_restart_iterations"].cpu().numpy()
    for extra in (dict(), dict(hip_graphs=True), dict(hip_graphs=True, capture_constraints=True),
                  dict(device_iteration=False), dict(device_iteration=False, hip_graphs=True)):
        _, _, val, log = run_sweep(DEV, **kw, **extra)
        np.testing.assert_allclose(val, val_t, rtol=1e-9)
        np.testing.assert_array_equal(log["per_restart_iterations"].cpu().numpy(), ref_iters)
        np.testing.assert_allclose(log["final_cost"].cpu().numpy(), log_t["final_cost"].cpu().numpy(), rtol=1e-9, atol=1e-12)   # (stopped by |grad| < 1e-4: |grad|^2 / curvature)


def test_fused_acquisition_on_trainable_surrogate():
    """SingleTaskGP(ScaleKernel(SpdAffineInvariantGaussianKernel)) - the surrogate of the reference examples (gabo_spd.py:165-176) -
    takes the same fused chain once fitted."""
    from gabotorch_amd._compat import ScaleKernel
    from gabotorch_amd.fused_acquisition import FusedAcquisition
    d = 3
    rng, X, y = _spd_gp(d, n_train=15, seed=9)
    kern = ScaleKernel(SpdAffineInvariantGaussianKernel(beta_min=0.5), outputscale_prior=models.GammaPrior(2.0, 0.15))
    gp = models.SingleTaskGP(t(X), t((y - y.mean()) / y.std()), kern, noise_prior=models.GammaPrior(1.1, 0.05))
    models.fit_gpytorch_model(gp, maxiter=20)
    acq = models.ExpectedImprovement(gp, best_f=float(gp.train_y.min()), maximize=False)
    post = symmetric_matrix_to_vector_mandel_torch
    fused = FusedAcquisition.build(acq, post, torch.device(DEV))
    assert fused is not None and fused.single_launch
    q = np.linalg.qr(rng.standard_normal((33, d, d)))[0]
    P = np.einsum("nab,nb,ncb->nac", q, rng.uniform(0.2, 3.0, (33, d)), q)
    x = t(0.5 * (P + P.transpose(0, 2, 1)))
    xx = x.clone().requires_grad_(True)
    f_ref = -acq(post(xx)[:, None])
    (g_ref,) = torch.autograd.grad(f_ref.sum(), xx)
    f, g = fused.cost_egrad(x)
    np.testing.assert_allclose(f.cpu().numpy(), f_ref.detach().cpu().numpy(), rtol=1e-9, atol=1e-14)
    np.testing.assert_allclose(g.cpu().numpy(), g_ref.cpu().numpy(), rtol=1e-7, atol=1e-10 * max(1.0, float(g_ref.abs().max())))


def test_gp_acquisition_kernel_against_the_numpy_oracle():
    """gabo_gp_acquisition (value and d/dK*) against oracle/gp.py: posterior by dense solves, EI by scipy.stats.norm, gradient by
    central differences of the oracle."""
    from oracle import gp as ogp
    rng = np.random.default_rng(12)
    n, r = 37, 9
    a = rng.standard_normal((n, 3))
    ktr = np.exp(-0.5 * ((a[:, None] - a[None]) ** 2).sum(-1))
    b = rng.standard_normal((r, 3))
    ks = np.exp(-0.5 * ((b[:, None] - a[None]) ** 2).sum(-1))
    y = rng.standard_normal(n)
    mean, osc, noise, best = 0.3, 1.7, 1e-2, float(y.min())
    L = np.linalg.cholesky(osc * ktr + noise * np.eye(n))
    linv = np.linalg.inv(L)
    alpha = np.linalg.solve(L.T, np.linalg.solve(L, y - mean))
    for kind, maximize in ((_lib.GABO_ACQ_EXPECTED_IMPROVEMENT, False), (_lib.GABO_ACQ_EXPECTED_IMPROVEMENT, True),
                           (_lib.GABO_ACQ_POSTERIOR_MEAN, False)):
        def oracle_value(k):
            mu, var = ogp.gp_posterior(ktr, k, np.ones(len(k)), y, mean, osc, noise)
            if kind == _lib.GABO_ACQ_POSTERIOR_MEAN:
                return mu if maximize else -mu
            return ogp.expected_improvement(mu, var, best, maximize)
        val, grad = ops.gp_acquisition(t(ks), t(alpha), t(linv), t(np.ascontiguousarray(linv.T)), mean, osc, 1.0, best, kind, maximize)
        np.testing.assert_allclose(val.cpu().numpy(), oracle_value(ks), rtol=1e-9, atol=1e-13)
        num = np.zeros_like(ks)
        h = 1e-6
        for idx in np.ndindex(ks.shape):
            kp, km = ks.copy(), ks.copy()
            kp[idx] += h
            km[idx] -= h
            num[idx] = (oracle_value(kp)[idx[0]] - oracle_value(km)[idx[0]]) / (2 * h)
        np.testing.assert_allclose(grad.cpu().numpy(), num, rtol=1e-5, atol=1e-8)


@pytest.mark.parametrize("d", [2, 5, 8])
@pytest.mark.parametrize("flavour", ["le", "frob"])
def test_fused_chain_for_log_euclidean_and_frobenius_kernels(flavour, d):
    """The latent surrogate of config 5 (SpdLogEuclideanGaussianKernel, hd_gabo_spd.py:166) takes the fused chain too."""
    from gabotorch_amd.fused_acquisition import FusedAcquisition
    from gabotorch_amd.kernel_utils.kernels_spd import SpdFrobeniusGaussianKernel, SpdLogEuclideanGaussianKernel
    rng, X, y = _spd_gp(d, n_train=70 if d == 5 else 17, seed=4)
    kern = (SpdLogEuclideanGaussianKernel if flavour == "le" else SpdFrobeniusGaussianKernel)().double()
    kern.lengthscale = torch.tensor(1.3, dtype=torch.float64)
    gp = models.ExactGP(t(X), t(y), kern, outputscale=1.2, noise=1e-2)
    acq = models.ExpectedImprovement(gp, best_f=float(y.min()), maximize=False)
    post = symmetric_matrix_to_vector_mandel_torch
    fused = FusedAcquisition.build(acq, post, torch.device(DEV))
    assert fused is not None and fused.flavour == flavour
    assert fused.single_launch                           # d <= 8: one launch per evaluation for both (Frobenius: round 5)
    q = np.linalg.qr(rng.standard_normal((50, d, d)))[0]
    P = np.einsum("nab,nb,ncb->nac", q, rng.uniform(0.2, 3.0, (50, d)), q)
    x = t(0.5 * (P + P.transpose(0, 2, 1)))
    xx = x.clone().requires_grad_(True)
    f_ref = -acq(post(xx)[:, None])
    (g_ref,) = torch.autograd.grad(f_ref.sum(), xx)
    f, g = fused.cost_egrad(x)
    np.testing.assert_allclose(f.cpu().numpy(), f_ref.detach().cpu().numpy(), rtol=1e-10, atol=1e-14)
    np.testing.assert_allclose(g.cpu().numpy(), g_ref.cpu().numpy(), rtol=1e-8, atol=1e-11 * max(1.0, float(g_ref.abs().max())))
    np.testing.assert_allclose(fused.cost(x).cpu().numpy(), f.cpu().numpy(), rtol=0, atol=0)
    np.testing.assert_allclose(fused.egrad_mandel(ops.matrix_to_mandel(x)).cpu().numpy(), ops.matrix_to_mandel(g).cpu().numpy(),
                               rtol=1e-12, atol=1e-14)
    # the separate-launch chain (d > 8) gives the same numbers
    fused.single_launch = False
    f2, g2 = fused.cost_egrad(x)
    np.testing.assert_allclose(f2.cpu().numpy(), f.cpu().numpy(), rtol=1e-10, atol=1e-14)
    np.testing.assert_allclose(g2.cpu().numpy(), g.cpu().numpy(), rtol=1e-8, atol=1e-11 * max(1.0, float(g.abs().max())))


def test_single_launch_acquisition_at_the_lds_limits():
    """d = 12 is the largest register-resident dimension (120 KB of static LDS in the fused kernels) and gabo_spd_acq_max_train(12)
    the largest training set that still fits the 160 KB of a CU: the single launch must agree with the separate-launch chain."""
    from gabotorch_amd.fused_acquisition import FusedAcquisition
    d = 12
    n_max = int(_lib.load().gabo_spd_acq_max_train(d))
    assert 1500 < n_max <= 2048
    rng = np.random.default_rng(77)
    q = np.linalg.qr(rng.standard_normal((n_max, d, d)))[0]
    Xm = np.einsum("nab,nb,ncb->nac", q, rng.uniform(0.5, 2.0, (n_max, d)), q)
    X = ospd.symmetric_matrix_to_vector_mandel(0.5 * (Xm + Xm.transpose(0, 2, 1)))
    y = rng.standard_normal(n_max)
    gp = models.ExactGP(t(X), t(y), SpdAffineInvariantGaussianKernel(beta_min=0.16), outputscale=1.0, noise=0.5)
    acq = models.ExpectedImprovement(gp, best_f=float(y.min()), maximize=False)
    fused = FusedAcquisition.build(acq, symmetric_matrix_to_vector_mandel_torch, torch.device(DEV))
    assert fused is not None and fused.single_launch
    x = t(Xm[:5] + 0.05 * np.eye(d))
    f1, g1 = fused.cost_egrad(x)
    fused.single_launch = False
    f2, g2 = fused.cost_egrad(x)
    np.testing.assert_allclose(f1.cpu().numpy(), f2.cpu().numpy(), rtol=1e-9, atol=1e-14)
    np.testing.assert_allclose(g1.cpu().numpy(), g2.cpu().numpy(), rtol=1e-7, atol=1e-12 * max(1.0, float(g2.abs().max())))
    # one more training point: the fused kernels decline, the chain takes over
    gp2 = models.ExactGP(t(np.concatenate([X, X[:1]])), t(np.concatenate([y, y[:1]])), SpdAffineInvariantGaussianKernel(beta_min=0.16),
                         outputscale=1.0, noise=0.5)
    fused2 = FusedAcquisition.build(models.ExpectedImprovement(gp2, best_f=0.0, maximize=False), symmetric_matrix_to_vector_mandel_torch,
                                    torch.device(DEV))
    assert fused2 is not None and not fused2.single_launch


def test_device_trust_region_iteration_at_d12():
    """the propose/update kernels at the largest supported dimension against the torch lock-step solver: three and six iterations (at
    d = 12 the tCG runs up to 78 inner iterations on a finite-difference Hessian) agree to 1e-9.  (Rounds 2-4 compared the six-iteration
    run at 1e-4 and blamed the amplification of the last bits by 1 / c; it was the kernels' step, 2^-13 instead of 2^-14: DESIGN 0.)"""
    from tools.sweep_bench import run_sweep
    for maxiter, tol in ((3, 1e-9), (6, 1e-9)):
        kw = dict(num_restarts=12, raw_samples=64, d=12, n_train=30, maxiter=maxiter)
        _, _, val_t, log_t = run_sweep(DEV, device_tcg=False, **kw)
        _, _, val_d, log_d = run_sweep(DEV, **kw)
        np.testing.assert_allclose(val_d, val_t, rtol=tol)
        np.testing.assert_array_equal(log_d["per_restart_iterations"].cpu().numpy(), log_t["per_restart_iterations"].cpu().numpy())
        np.testing.assert_allclose(log_d["final_cost"].cpu().numpy(), log_t["final_cost"].cpu().numpy(), rtol=tol, atol=1e-11)


@pytest.mark.parametrize("case", ["unconstrained_ei", "posterior_mean", "laplace_ei_3_iterations", "tiny_training_set_two_constraints"])
def test_device_solve_variants_match_torch_path(case):
    """Corners of the device-resident solve: no constraints, PosteriorMean, the Laplace kernel (its surrogate has kinks at the
    training points, so trajectories are only compared over the first iterations), d = 2 with 3 training points and an eigenvalue box
    (two inequality constraints) - all against the torch lock-step solver from the same initial points."""
    from gabotorch_amd.kernel_utils.kernels_spd import SpdAffineInvariantLaplaceKernel
    from gabotorch_amd.manifold_optimization.manifold_optimize import gen_candidates_manifold
    d, n_train, R = (2, 3, 37) if case.startswith("tiny") else (3, 20, 70)
    rng, X, y = _spd_gp(d, n_train=n_train, seed=31)
    maxiter = 25
    if case == "posterior_mean":
        gp = models.ExactGP(t(X), t(y), SpdAffineInvariantGaussianKernel(beta_min=0.5), outputscale=1.0, noise=1e-2)
        acq = models.PosteriorMean(gp, maximize=False)
    elif case.startswith("laplace"):
        gp = models.ExactGP(t(X), t(y), SpdAffineInvariantLaplaceKernel(beta_min=0.5), outputscale=1.0, noise=1e-2)
        acq = models.ExpectedImprovement(gp, best_f=float(y.min()), maximize=False)
        maxiter = 3
    else:
        gp = models.ExactGP(t(X), t(y), SpdAffineInvariantGaussianKernel(beta_min=0.5), outputscale=1.0, noise=1e-2)
        acq = models.ExpectedImprovement(gp, best_f=float(y.min()), maximize=False)
    cons = None
    if case.startswith("tiny"):
        cons = [lambda m: scut.max_eigenvalue_constraint_torch(m, 3.5), lambda m: scut.min_eigenvalue_constraint_torch(m, 0.1)]
    q = np.linalg.qr(rng.standard_normal((R, d, d)))[0]
    P = np.einsum("nab,nb,ncb->nac", q, rng.uniform(0.3, 3.0, (R, d)), q)
    x0 = ops.matrix_to_mandel(t(0.5 * (P + P.transpose(0, 2, 1))))[:, None]
    man = manifolds.PositiveDefinite(d)
    out = {}
    ops.set_error_checking(False)
    for name, opts in (("torch", {"device_tcg": False}), ("device", {}), ("graphs", {"hip_graphs": True}), ("two_launch_off", {"device_iteration": False})):
        solver = BatchedTrustRegions(mingradnorm=1e-5, maxiter=maxiter)
        c, v = gen_candidates_manifold(x0, acq, man, solver, vector_to_symmetric_matrix_mandel_torch, symmetric_matrix_to_vector_mandel_torch,
                                       inequality_constraints=cons, approx_hessian=True, options=opts)
        out[name] = (c.cpu().numpy(), v.cpu().numpy(), solver.log["per_restart_iterations"].cpu().numpy())
    ops.set_error_checking(True)
    # (until round 5 the constrained and Laplace cases were compared at 2e-5, attributed to rounding-decided branches: it was the
    # finite-difference step of the device kernels)
    tol = 1e-7 if case in ("unconstrained_ei", "posterior_mean") else 1e-9
    for name in ("device", "graphs", "two_launch_off"):
        np.testing.assert_array_equal(out[name][2], out["torch"][2])
        np.testing.assert_allclose(out[name][1], out["torch"][1], rtol=tol, atol=1e-12)
        np.testing.assert_allclose(out[name][0], out["torch"][0], rtol=0, atol=1e-6 if tol < 1e-6 else 1e-3)
    np.testing.assert_allclose(out["graphs"][1], out["device"][1], rtol=1e-12, atol=0)      # the execution plans are the same arithmetic


@pytest.mark.parametrize("case", ["ai_unconstrained", "ai_max_eig", "ai_box_strict", "le_box_strict"])
def test_single_launch_solve_matches_torch_path(case):
    """gabo_spd_tr_solve (every wave iterates its restart to the end; the eigenvalue bounds - functools.partial objects as in the
    reference examples - are evaluated on the device) against the torch lock-step solver, and against the same constraints given
    as opaque lambdas (which take the propose/update plan)."""
    import functools
    from gabotorch_amd.kernel_utils.kernels_spd import SpdLogEuclideanGaussianKernel
    from gabotorch_amd.manifold_optimization.manifold_optimize import gen_candidates_manifold
    d, n_train, R = (2, 15, 90) if case.startswith("le") else (3, 20, 90)
    rng, X, y = _spd_gp(d, n_train=n_train, seed=41)
    if case.startswith("le"):
        kern = SpdLogEuclideanGaussianKernel().double()
        kern.lengthscale = torch.tensor(1.4, dtype=torch.float64)
    else:
        kern = SpdAffineInvariantGaussianKernel(beta_min=0.5)
    gp = models.ExactGP(t(X), t(y), kern, outputscale=1.0, noise=1e-2)
    acq = models.ExpectedImprovement(gp, best_f=float(y.min()), maximize=False)
    strict = case.endswith("strict")
    if case.endswith("unconstrained"):
        partials = lambdas = None
    else:
        partials = [functools.partial(scut.max_eigenvalue_constraint_torch, maximum_eigenvalue=2.5)]
        lambdas = [lambda m: scut.max_eigenvalue_constraint_torch(m, 2.5)]
        if "box" in case:
            partials.append(functools.partial(scut.min_eigenvalue_constraint_torch, minimum_eigenvalue=0.35))
            lambdas.append(lambda m: scut.min_eigenvalue_constraint_torch(m, 0.35))
    q = np.linalg.qr(rng.standard_normal((R, d, d)))[0]
    P = np.einsum("nab,nb,ncb->nac", q, rng.uniform(0.4, 2.4, (R, d)), q)
    x0 = ops.matrix_to_mandel(t(0.5 * (P + P.transpose(0, 2, 1))))[:, None]
    man = manifolds.PositiveDefinite(d)
    out = {}
    ops.set_error_checking(False)
    for name, cons, opts in (("torch", lambdas, {"device_tcg": False}), ("plan", lambdas, {}), ("solve", partials, {}),
                             ("solve_off", partials, {"device_solve": False})):
        solver = BatchedTrustRegions(mingradnorm=1e-5, maxiter=20, strict_constraints=strict)
        c, v = gen_candidates_manifold(x0, acq, man, solver, vector_to_symmetric_matrix_mandel_torch, symmetric_matrix_to_vector_mandel_torch,
                                       inequality_constraints=cons, approx_hessian=True, options=opts)
        out[name] = (c.cpu().numpy(), v.cpu().numpy(), solver.log["per_restart_iterations"].cpu().numpy())
    ops.set_error_checking(True)
    for name in ("plan", "solve", "solve_off"):
        np.testing.assert_array_equal(out[name][2], out["torch"][2])
        np.testing.assert_allclose(out[name][1], out["torch"][1], rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(out["solve"][1], out["plan"][1], rtol=1e-9, atol=1e-13)       # same device arithmetic, two drivers
    # (with constraints the two drivers evaluate lambda_max/min with different eigen-solvers - the wave's register solver against
    # the torch callable's launch - and a restart that sits on the bound can end a rounding error apart along a flat direction: 9e-8)
    # (round 6, other rounding in the GP factor and the whitened gradient: a restart of 90 that stops on the bound ends 2.5e-5 away along a flat
    # direction, its value equal to 1e-9 above; the solver stops at |grad| < 1e-5, which pins x to ~1e-5 / curvature)
    np.testing.assert_allclose(out["solve"][0], out["plan"][0], rtol=0, atol=1e-8 if lambdas is None else 5e-5)
    assert scut.builtin_constraint(lambdas[0]) is None if lambdas else True


@pytest.mark.parametrize("d,n_train", [(8, 47), (7, 60), (8, 20)])
def test_log_euclidean_sweep_at_d7_d8_beyond_the_lds_resident_solve(d, n_train):
    """Two instantiations of the trust-region kernels for the log-Euclidean surrogate were wrong as compiled until round 5 (found by
    tools/soak_tr.py): the generic-workspace single-launch solve at d = 7, 8 faulted on a null address, the propose kernel at d = 8 returned
    wrong proposals - 512-register functions with ~4 k spilled registers.  The evaluation's adjoint is now shared by the wave through LDS
    (233 registers at d = 8, bit-identical results) and both are right; the library says what it has (gabo_spd_tr_solve_supported,
    gabo_spd_tr_propose_supported: a build with -DGABO_LE_MAX_GENERIC_DIM=6 leaves them out) and the sweep takes the best plan there is -
    every choice with the torch path's results.  The sizes here are the ones that crashed or went wrong."""
    import ctypes
    import functools
    from gabotorch_amd.fused_acquisition import FusedAcquisition
    from gabotorch_amd.kernel_utils.kernels_spd import SpdLogEuclideanGaussianKernel
    from gabotorch_amd.manifold_optimization.manifold_optimize import gen_candidates_manifold
    rng, X, y = _spd_gp(d, n_train=n_train, seed=47)
    kern = SpdLogEuclideanGaussianKernel().double()
    kern.lengthscale = torch.tensor(1.4, dtype=torch.float64)
    gp = models.ExactGP(t(X), t(y), kern, outputscale=1.0, noise=1e-2)
    acq = models.ExpectedImprovement(gp, best_f=float(y.min()), maximize=False)
    R = 24
    q = np.linalg.qr(rng.standard_normal((R, d, d)))[0]
    P = np.einsum("nab,nb,ncb->nac", q, rng.uniform(0.5, 2.2, (R, d)), q)
    x0 = ops.matrix_to_mandel(t(0.5 * (P + P.transpose(0, 2, 1))))[:, None]
    cons = [functools.partial(scut.max_eigenvalue_constraint_torch, maximum_eigenvalue=2.6),
            functools.partial(scut.min_eigenvalue_constraint_torch, minimum_eigenvalue=0.3)]
    fused = FusedAcquisition.build(acq, symmetric_matrix_to_vector_mandel_torch, torch.device(DEV))
    supported = bool(_lib.load().gabo_spd_tr_solve_supported(ctypes.byref(fused.acq_params()), R, d, 2, 0))
    proposes = bool(_lib.load().gabo_spd_tr_propose_supported(int(fused.mode) | int(fused.metric), d))
    assert supported and proposes                 # (the default build has every instantiation)
    out = {}
    ops.set_error_checking(False)
    try:
        for name, opts in (("torch", {"device_tcg": False}), ("device", {}), ("no_solve", {"device_solve": False}), ("graphs", {"hip_graphs": True})):
            solver = BatchedTrustRegions(mingradnorm=1e-5, maxiter=12, strict_constraints=True)
            c, v = gen_candidates_manifold(x0, acq, manifolds.PositiveDefinite(d), solver, vector_to_symmetric_matrix_mandel_torch,
                                           symmetric_matrix_to_vector_mandel_torch, inequality_constraints=cons, approx_hessian=True, options=opts)
            out[name] = (v.cpu().numpy(), solver.log["per_restart_iterations"].cpu().numpy(), "one_launch_solve" in solver.log)
    finally:
        ops.set_error_checking(True)
    assert out["device"][2] == supported and out["graphs"][2] == supported and not out["torch"][2] and not out["no_solve"][2]
    for name in ("device", "no_solve", "graphs"):
        np.testing.assert_array_equal(out[name][1], out["torch"][1])
        np.testing.assert_allclose(out[name][0], out["torch"][0], rtol=1e-8, atol=1e-12)


@pytest.mark.parametrize("d", [2, 3])
def test_device_solve_matches_reference_solver_optima(golden, d):
    """The golden trust-region problems (tests/golden/make_golden_tr.py: the REFERENCE's TrustRegions / ConstrainedTrustRegions /
    StrictConstrainedTrustRegions run on cost(x) = -sum_j w_j exp(-beta d_AI(x, Y_j)^2) with get_hessianfd) are posterior-mean
    acquisitions of a GP with alpha = w: the device-resident solve - propose/update plan and gabo_spd_tr_solve - must land on the
    reference's optima from the same starting points.  SECONDARY check: these fixtures are the reference as it is (float32 eigenvalue
    buffer), hence the 2e-3 on the constrained costs (its own f32-vs-f64 distance); the float64 traces of
    tests/test_gpu_tr_traces.py and the EI optimum of tests/test_gpu_ei_optimum.py are the tight ones."""
    import functools
    from gabotorch_amd.manifold_optimization.manifold_optimize import gen_candidates_manifold
    g = golden("trust_regions.npz")
    Y = ospd.symmetric_matrix_to_vector_mandel(g[f"spd{d}_Y"])
    w, beta, mx = g[f"spd{d}_w"], float(g[f"spd{d}_beta"]), float(g[f"spd{d}_maxeig"])
    kern = SpdAffineInvariantGaussianKernel(beta_min=0.1).double()
    kern.beta = torch.tensor(beta, dtype=torch.float64)
    gp = models.ExactGP(t(Y), t(np.zeros(len(w))), kern, outputscale=1.0, noise=1.0, mean=0.0)
    gp._cache = (torch.eye(len(w), dtype=torch.float64, device=DEV), t(w))          # posterior mean = sum_j w_j k(x, Y_j)
    acq = models.PosteriorMean(gp, maximize=True)                                      # cost = -acq = the golden cost
    man = manifolds.PositiveDefinite(d)
    pre, post = vector_to_symmetric_matrix_mandel_torch, symmetric_matrix_to_vector_mandel_torch
    partial = [functools.partial(scut.max_eigenvalue_constraint_torch, maximum_eigenvalue=mx)]
    opaque = [lambda m: scut.max_eigenvalue_constraint_torch(m, mx)]
    ops.set_error_checking(False)
    try:
        for cons, opts in ((None, {}), (None, {"device_solve": False})):
            x0 = ops.matrix_to_mandel(t(g[f"spd{d}_x0"]))[:, None]
            c, v = gen_candidates_manifold(x0, acq, man, BatchedTrustRegions(mingradnorm=1e-4, maxiter=100), pre, post,
                                           inequality_constraints=cons, approx_hessian=True, options=opts)
            np.testing.assert_allclose(-v.cpu().numpy(), g[f"spd{d}_fd_f"], rtol=1e-6)
            np.testing.assert_allclose(ospd.vector_to_symmetric_matrix_mandel(c[:, 0].cpu().numpy()), g[f"spd{d}_fd_x"], rtol=0, atol=2e-3)
        x0c = ops.matrix_to_mandel(t(g[f"spd{d}_con_x0"]))[:, None]
        for cons in (partial, opaque):
            c, v = gen_candidates_manifold(x0c, acq, man, BatchedTrustRegions(mingradnorm=1e-4, maxiter=100), pre, post,
                                           inequality_constraints=cons, approx_hessian=True)
            np.testing.assert_allclose(-v.cpu().numpy(), g[f"spd{d}_con_f"], rtol=2e-3)
            strict = BatchedTrustRegions(mingradnorm=2e-4, maxiter=100, minstepsize=1e-4, strict_constraints=True)
            c, v = gen_candidates_manifold(x0c, acq, man, strict, pre, post, inequality_constraints=cons, approx_hessian=True)
            np.testing.assert_allclose(-v.cpu().numpy(), g[f"spd{d}_strict_f"], rtol=2e-3)
            lam = np.linalg.eigvalsh(ospd.vector_to_symmetric_matrix_mandel(c[:, 0].cpu().numpy()))
            assert lam.max() <= mx + 1e-9                                            # the strict solver never leaves the feasible set
    finally:
        ops.set_error_checking(True)


def test_fused_acquisition_cache_follows_the_surrogate():
    """FusedAcquisition.build is cached on the acquisition object; new data / a refit (a new prediction cache) must rebuild it."""
    from gabotorch_amd.fused_acquisition import FusedAcquisition
    rng, X, y = _spd_gp(3, n_train=10, seed=3)
    gp = models.ExactGP(t(X), t(y), SpdAffineInvariantGaussianKernel(beta_min=0.5), outputscale=1.0, noise=1e-2)
    acq = models.ExpectedImprovement(gp, best_f=float(y.min()), maximize=False)
    post = symmetric_matrix_to_vector_mandel_torch
    f1 = FusedAcquisition.build(acq, post, torch.device(DEV))
    assert FusedAcquisition.build(acq, post, torch.device(DEV)) is f1                 # cache hit
    x = vector_to_symmetric_matrix_mandel_torch(t(X[:4]) * 1.1)
    v1 = f1.cost(x).clone()
    gp.train_y = gp.train_y * 2.0 + 1.0          # change the surrogate: a new prediction cache
    gp.mean = float(gp.train_y.mean())
    gp._cache = None
    f2 = FusedAcquisition.build(acq, post, torch.device(DEV))
    assert f2 is not f1
    np.testing.assert_allclose(f2.cost(x).cpu().numpy(), -acq(post(x)[:, None]).detach().cpu().numpy(), rtol=1e-10, atol=1e-14)
    assert float((f2.cost(x) - v1).abs().max()) > 1e-6
    acq.best_f = acq.best_f - 0.5                 # a different incumbent also rebuilds
    assert FusedAcquisition.build(acq, post, torch.device(DEV)) is not f2


def test_single_launch_solve_properties_at_scale():
    """4096 restarts through gabo_spd_tr_solve (strict eigenvalue box): size-independent properties - every restart ends no worse than
    it started (the solver only accepts decreasing steps), never leaves the feasible set, stays SPD, respects the iteration limit,
    and the result does not depend on how many restarts share the launch."""
    import functools
    from gabotorch_amd.manifold_optimization.manifold_optimize import gen_candidates_manifold
    d, R = 4, 4096
    rng, X, y = _spd_gp(d, n_train=40, seed=77)
    gp = models.ExactGP(t(X), t(y), SpdAffineInvariantGaussianKernel(beta_min=0.4), outputscale=1.0, noise=1e-2)
    acq = models.ExpectedImprovement(gp, best_f=float(y.min()), maximize=False)
    cons = [functools.partial(scut.max_eigenvalue_constraint_torch, maximum_eigenvalue=3.2),
            functools.partial(scut.min_eigenvalue_constraint_torch, minimum_eigenvalue=0.15)]
    x0m = ops.spd_sample(R, d, 0.2, 3.0, seed=99, device=DEV)
    x0 = ops.matrix_to_mandel(x0m)[:, None]
    man = manifolds.PositiveDefinite(d)
    pre, post = vector_to_symmetric_matrix_mandel_torch, symmetric_matrix_to_vector_mandel_torch
    ops.set_error_checking(False)
    try:
        solver = BatchedTrustRegions(mingradnorm=1e-4, maxiter=30, strict_constraints=True)
        c, v = gen_candidates_manifold(x0, acq, man, solver, pre, post, inequality_constraints=cons, approx_hessian=True)
        s2 = BatchedTrustRegions(mingradnorm=1e-4, maxiter=30, strict_constraints=True)
        c2, v2 = gen_candidates_manifold(x0[:100], acq, man, s2, pre, post, inequality_constraints=cons, approx_hessian=True)
    finally:
        ops.set_error_checking(True)
    with torch.no_grad():
        v0 = acq(x0)
    assert torch.isfinite(c).all() and torch.isfinite(v).all()
    assert bool((v >= v0 - 1e-12).all())                                  # acquisition never decreases (cost never increases)
    lam = np.linalg.eigvalsh(ospd.vector_to_symmetric_matrix_mandel(c[:, 0].cpu().numpy()))
    assert lam.min() >= 0.15 - 1e-9 and lam.max() <= 3.2 + 1e-9
    it = solver.log["per_restart_iterations"].cpu().numpy()
    assert it.min() >= 1 and it.max() <= 30
    np.testing.assert_array_equal(c2.cpu().numpy(), c[:100].cpu().numpy())    # restarts are independent: bit-identical in a smaller launch
    assert float(v.max()) > float(v0.max()) - 1e-12


@pytest.mark.parametrize("case", ["unconstrained", "bound_constraint", "laplace_mean", "exact_hessian", "exact_hessian_bound", "exact_hessian_mean"])
def test_sphere_device_solve_matches_torch_path(case):
    """csrc/sphere_tr.hip (single-launch acquisition on the sphere, tCG with the FD Hessian, propose / update / solve) against the
    torch lock-step solver from the same initial points."""
    from gabotorch_amd.fused_acquisition import FusedAcquisition
    from gabotorch_amd.kernel_utils.kernels_sphere import SphereLaplaceKernel
    from gabotorch_amd.manifold_optimization.manifold_optimize import gen_candidates_manifold
    dim, n_train, R = 6, 70, 150
    rng = np.random.default_rng(14)
    X = rng.standard_normal((n_train, dim)); X /= np.linalg.norm(X, axis=1, keepdims=True)
    y = np.arccos(np.clip(X[:, 0], -1, 1)) ** 2 + 0.05 * rng.standard_normal(n_train)
    approx = not case.startswith("exact")
    if case == "exact_hessian_mean":
        gp = models.ExactGP(t(X), t(y), SphereGaussianKernel(beta_min=1.0), outputscale=1.3, noise=1e-2)
        acq = models.PosteriorMean(gp, maximize=False)
    elif case == "laplace_mean":
        kern = SphereLaplaceKernel().double()
        kern.lengthscale = torch.tensor(0.9, dtype=torch.float64)
        gp = models.ExactGP(t(X), t(y), kern, outputscale=1.0, noise=1e-2)
        acq = models.PosteriorMean(gp, maximize=False)
    else:
        gp = models.ExactGP(t(X), t(y), SphereGaussianKernel(beta_min=1.0), outputscale=1.3, noise=1e-2)
        acq = models.ExpectedImprovement(gp, best_f=float(y.min()), maximize=False)
    # the fused single launch against autograd through the generic path
    fused = FusedAcquisition.build(acq, None, torch.device(DEV))
    assert fused is not None and fused.single_launch
    P = rng.standard_normal((R, dim)); P /= np.linalg.norm(P, axis=1, keepdims=True)
    x = t(P)
    xx = x.clone().requires_grad_(True)
    f_ref = -acq(xx[:, None])
    (g_ref,) = torch.autograd.grad(f_ref.sum(), xx)
    f, g = fused.cost_egrad(x)
    np.testing.assert_allclose(f.cpu().numpy(), f_ref.detach().cpu().numpy(), rtol=1e-10, atol=1e-14)
    np.testing.assert_allclose(g.cpu().numpy(), g_ref.cpu().numpy(), rtol=1e-8, atol=1e-11 * max(1.0, float(g_ref.abs().max())))
    cons = [lambda p: p[..., 0] + 0.3] if case.endswith("bound_constraint") or case.endswith("_bound") else None
    man = manifolds.Sphere(dim)
    out = {}
    maxiter = 1 if case == "laplace_mean" else 40        # (the Laplace surrogate has kinks: only the first iteration is comparable)
    for name, opts in (("torch", {"device_tcg": False}), ("device", {}), ("graphs", {"hip_graphs": True}),
                       ("graphs_captured", {"hip_graphs": True, "capture_constraints": True})):
        solver = BatchedTrustRegions(mingradnorm=1e-6, maxiter=maxiter)
        c, v = gen_candidates_manifold(x[:, None], acq, man, solver, inequality_constraints=cons, approx_hessian=approx, options=opts)
        out[name] = (c.cpu().numpy(), v.cpu().numpy(), solver.log["per_restart_iterations"].cpu().numpy())
    tol = 1e-9 if cons is not None else 1e-7
    for name in ("device", "graphs", "graphs_captured"):
        np.testing.assert_array_equal(out[name][2], out["torch"][2])
        np.testing.assert_allclose(out[name][1], out["torch"][1], rtol=tol, atol=1e-12)
        np.testing.assert_allclose(np.linalg.norm(out[name][0][:, 0], axis=1), 1.0, atol=1e-12)
    np.testing.assert_allclose(out["graphs"][1], out["device"][1], rtol=1e-12, atol=0)


@pytest.mark.parametrize("n", [3, 5])
def test_sphere_device_solve_matches_reference_solver_optima(golden, n):
    """The golden sphere problems (the REFERENCE's TrustRegions with exact and FD Hessians, ConstrainedTrustRegions and
    StrictConstrainedTrustRegions on cost(x) = -sum_j w_j exp(-beta d(x, Y_j)^2)) are posterior-mean acquisitions with alpha = w: the
    device-resident sphere solve (closed-form exact Hessian, FD Hessian, constraint lambdas, strict) must land on the reference's optima."""
    from gabotorch_amd.manifold_optimization.manifold_optimize import gen_candidates_manifold
    g = golden("trust_regions.npz")
    Y, w, beta = g[f"sph{n}_Y"], g[f"sph{n}_w"], float(g[f"sph{n}_beta"])
    kern = SphereGaussianKernel(beta_min=0.1).double()
    kern.beta = torch.tensor(beta, dtype=torch.float64)
    gp = models.ExactGP(t(Y), t(np.zeros(len(w))), kern, outputscale=1.0, noise=1.0, mean=0.0)
    gp._cache = (torch.eye(len(w), dtype=torch.float64, device=DEV), t(w))
    acq = models.PosteriorMean(gp, maximize=True)                  # cost = -acq = the golden cost
    man = manifolds.Sphere(n)
    for approx, key in ((False, "exact"), (True, "fd")):
        c, v = gen_candidates_manifold(t(g[f"sph{n}_x0"])[:, None], acq, man, BatchedTrustRegions(), approx_hessian=approx)
        np.testing.assert_allclose(-v.cpu().numpy(), g[f"sph{n}_{key}_f"], rtol=1e-6, atol=1e-9)
        np.testing.assert_allclose(c[:, 0].cpu().numpy(), g[f"sph{n}_{key}_x"], rtol=0, atol=1e-4)
    # (constrained runs: a restart that ends on the bound x_0 = 0.3 stops where its last accepted step happened to land along the bound; the
    # reference's own runs differ by this much between float32 and float64 eigen-buffers - a secondary check, the tight one is
    # tests/test_gpu_tr_traces.py against the float64 traces)
    cons = [lambda p: p[..., 0] - 0.3]
    x0c = t(g[f"sph{n}_con_x0"])[:, None]
    c, v = gen_candidates_manifold(x0c, acq, man, BatchedTrustRegions(mingradnorm=1e-6, maxiter=200), inequality_constraints=cons)
    np.testing.assert_allclose(-v.cpu().numpy(), g[f"sph{n}_con_f"], rtol=2e-3, atol=1e-6)
    c, v = gen_candidates_manifold(x0c, acq, man, BatchedTrustRegions(mingradnorm=1e-6, maxiter=200, strict_constraints=True),
                                   inequality_constraints=cons)
    np.testing.assert_allclose(-v.cpu().numpy(), g[f"sph{n}_strict_f"], rtol=2e-3, atol=1e-6)
    assert float(c[:, 0, 0].min()) >= 0.3 - 1e-9


def test_device_solvers_at_the_smallest_sizes():
    """One restart, one training point, the smallest manifolds (S^2_++ and the circle S^1): the device solvers against the torch path."""
    from gabotorch_amd.manifold_optimization.manifold_optimize import gen_candidates_manifold
    # SPD: d = 2, n = 1, R = 1
    xtr = ospd.symmetric_matrix_to_vector_mandel(np.array([[[1.5, 0.2], [0.2, 0.8]]]))
    gp = models.ExactGP(t(xtr), t(np.array([0.3])), SpdAffineInvariantGaussianKernel(beta_min=0.5), outputscale=1.0, noise=1e-2, mean=0.0)
    acq = models.PosteriorMean(gp, maximize=True)                    # peaks at the training point (a flat EI tail would be ill-posed)
    x0 = ops.matrix_to_mandel(t(np.array([[[0.9, -0.1], [-0.1, 1.7]]])))[:, None]
    man = manifolds.PositiveDefinite(2)
    res = {}
    ops.set_error_checking(False)
    try:
        for name, opts in (("torch", {"device_tcg": False}), ("device", {}), ("plan", {"device_solve": False})):
            s_ = BatchedTrustRegions(mingradnorm=1e-7, maxiter=15)
            c, v = gen_candidates_manifold(x0, acq, man, s_, vector_to_symmetric_matrix_mandel_torch, symmetric_matrix_to_vector_mandel_torch,
                                           approx_hessian=True, options=opts)
            res[name] = (c.cpu().numpy(), v.cpu().numpy())
    finally:
        ops.set_error_checking(True)
    for name in ("device", "plan"):
        np.testing.assert_allclose(res[name][1], res["torch"][1], rtol=1e-7, atol=1e-13)
        np.testing.assert_allclose(res[name][0], res["torch"][0], rtol=0, atol=1e-6)
        np.testing.assert_allclose(res[name][0][0, 0], xtr[0], atol=1e-5)
    # circle S^1: dim = 2, n = 1, R = 1, exact and FD Hessian
    gp = models.ExactGP(t(np.array([[0.6, 0.8]])), t(np.array([0.1])), SphereGaussianKernel(beta_min=1.0), outputscale=1.0, noise=1e-2, mean=0.0)
    acq = models.PosteriorMean(gp, maximize=True)
    x0 = t(np.array([[1.0, 0.0]]))[:, None]
    for approx in (False, True):
        out = []
        for opts in ({"device_tcg": False}, {}):
            c, v = gen_candidates_manifold(x0, acq, manifolds.Sphere(2), BatchedTrustRegions(mingradnorm=1e-9, maxiter=30), approx_hessian=approx,
                                           options=opts)
            out.append((c.cpu().numpy(), v.cpu().numpy()))
        np.testing.assert_allclose(out[1][1], out[0][1], rtol=1e-8)
        np.testing.assert_allclose(out[1][0], out[0][0], atol=1e-6)
        np.testing.assert_allclose(out[1][0][0, 0], [0.6, 0.8], atol=1e-5)          # the posterior mean peaks at the training point


@pytest.mark.parametrize("case", ["D20_d2_strict", "D12_d3", "D20_d2_max_only_strict"])
def test_single_launch_solve_with_nested_eigenvalue_constraints(case):
    """Config 5's latent sweep: log-Euclidean surrogate on S^d_++, eigenvalue bounds stated in the original space S^D_++ of a nested SPD mapping
    (functools.partial over max/min_eigenvalue_nested_spd_constraint with the mapping bound by keyword, hd_gabo_spd.py:244-257).  The
    single-launch solve evaluates them inside the kernel (nested_extremes_body: lift, both extreme eigenpairs from one Householder
    reduction, gradient through sqrtm); checked against the same constraints as opaque callables on the torch lock-step solver and on the
    propose / update plan."""
    import functools
    from gabotorch_amd.kernel_utils.kernels_spd import SpdLogEuclideanGaussianKernel
    from gabotorch_amd.manifold_optimization.manifold_optimize import gen_candidates_manifold
    from gabotorch_amd.nested_mappings import nested_spd_constraints_utils as nscu
    D, d = (12, 3) if case.startswith("D12") else (20, 2)
    strict = case.endswith("strict")
    n_train, R = 15, 64
    rng, X, y = _spd_gp(d, n_train=n_train, seed=43)
    kern = SpdLogEuclideanGaussianKernel().double()
    kern.lengthscale = torch.tensor(1.4, dtype=torch.float64)
    gp = models.ExactGP(t(X), t(y), kern, outputscale=1.0, noise=1e-2)
    acq = models.ExpectedImprovement(gp, best_f=float(y.min()), maximize=False)
    m = D - d
    Rm = np.linalg.qr(rng.standard_normal((D, D)))[0]
    W, V = t(Rm[:, :d]), t(np.linalg.qr(Rm[:, d:] + 0.01 * rng.standard_normal((D, m)))[0])
    qc = np.linalg.qr(rng.standard_normal((m, m)))[0]
    C = t((qc * rng.uniform(0.6, 1.8, m)) @ qc.T)
    K0 = rng.standard_normal((d, m))
    K = t(0.5 * K0 / np.linalg.norm(K0))
    mapping = dict(projection_matrix=W, projection_complement_matrix=V, bottom_spd_matrix=C, contraction_matrix=K)
    lift = lambda mats: np.linalg.eigvalsh(ospd.projection_from_nested_spd_to_spd(mats, *(a.cpu().numpy() for a in (W, V, C, K))))   # noqa: E731
    q = np.linalg.qr(rng.standard_normal((4 * R, d, d)))[0]
    P = np.einsum("nab,nb,ncb->nac", q, rng.uniform(0.5, 2.2, (4 * R, d)), q)
    P = 0.5 * (P + P.transpose(0, 2, 1))
    man = manifolds.PositiveDefinite(d)
    ops.set_error_checking(False)
    # bounds that the unconstrained optimum of a good part of the restarts violates, starts that satisfy them
    free = BatchedTrustRegions(mingradnorm=1e-5, maxiter=25)
    c_free, v_free = gen_candidates_manifold(ops.matrix_to_mandel(t(P))[:, None], acq, man, free, vector_to_symmetric_matrix_mandel_torch,
                                        symmetric_matrix_to_vector_mandel_torch, approx_hessian=True)
    lam_free, lam_start = lift(ospd.vector_to_symmetric_matrix_mandel(c_free.cpu().numpy()[:, 0])), lift(P)
    steer = case.startswith("D20")             # (at D = 12 -> 3 the unconstrained optima move inwards: the bounds are evaluated but rarely bind)
    if steer:
        hi, lo = float(np.quantile(lam_free[:, -1], 0.5)), float(np.quantile(lam_free[:, 0], 0.3))
    else:
        hi, lo = float(np.quantile(lam_start[:, -1], 0.8)), float(np.quantile(lam_start[:, 0], 0.2))
    ok = (lam_start[:, -1] < hi - 0.05) & (lam_start[:, 0] > lo + 0.02)
    keep = np.concatenate([np.flatnonzero(ok & (lam_free[:, -1] > hi + 0.05))[:R // 2], np.flatnonzero(ok & (lam_free[:, -1] <= hi + 0.05))])[:R]
    assert len(keep) >= 24 and (not steer or (lam_free[keep, -1] > hi + 0.05).sum() >= 5), (hi, lo, len(keep))
    x0 = ops.matrix_to_mandel(t(P[keep]))[:, None]
    partials = [functools.partial(nscu.max_eigenvalue_nested_spd_constraint, maximum_eigenvalue=hi, **mapping)]
    lambdas = [lambda z: nscu.max_eigenvalue_nested_spd_constraint(z, hi, W, V, C, K)]
    if "max_only" not in case:
        partials.append(functools.partial(nscu.min_eigenvalue_nested_spd_constraint, minimum_eigenvalue=lo, **mapping))
        lambdas.append(lambda z: nscu.min_eigenvalue_nested_spd_constraint(z, lo, W, V, C, K))
    b = scut.builtin_constraint(partials[0])
    assert b is not None and b[0] == _lib.GABO_CONSTRAINT_MAX_EIGENVALUE_NESTED and b[1] == hi and scut.builtin_constraint(lambdas[0]) is None
    out = {}
    for maxiter in (1, 25):
        for name, cons, opts in (("torch", lambdas, {"device_tcg": False}), ("plan", lambdas, {}), ("solve", partials, {})):
            solver = BatchedTrustRegions(mingradnorm=1e-5, maxiter=maxiter, strict_constraints=strict)
            c, v = gen_candidates_manifold(x0, acq, man, solver, vector_to_symmetric_matrix_mandel_torch, symmetric_matrix_to_vector_mandel_torch,
                                           inequality_constraints=cons, approx_hessian=True, options=opts)
            out[name, maxiter] = (c.cpu().numpy(), v.cpu().numpy(), solver.log["per_restart_iterations"].cpu().numpy())
    ops.set_error_checking(True)
    # ONE trust-region iteration (constraint values, whitened gradients, tCG with the constraint stop, proposal, strict feasibility test,
    # rho test): the three drivers agree restart by restart
    for name in ("plan", "solve"):
        np.testing.assert_allclose(out[name, 1][1], out["torch", 1][1], rtol=1e-10, atol=1e-13)       # (device tCG vs torch tCG)
    np.testing.assert_allclose(out["solve", 1][1], out["plan", 1][1], rtol=1e-9, atol=1e-14)         # same device arithmetic, two drivers
    np.testing.assert_allclose(out["solve", 1][0], out["plan", 1][0], rtol=0, atol=1e-9)
    # The whole solve: nine restarts in ten end on the torch path's value to 1e-8, all of them within 1e-6 (a restart that crawls along a
    # bound takes accept / reject decisions that rounding can flip: the drivers whiten the constraint gradients in different orders), none
    # of them outside the bounds (strict), and the bounds did steer restarts whose unconstrained optimum lies outside.
    lam = lift(ospd.vector_to_symmetric_matrix_mandel(out["solve", 25][0][:, 0]))
    if strict:
        assert lam[:, -1].max() < hi + 1e-9 and ("max_only" in case or lam[:, 0].min() > lo - 1e-9), (hi, lo, lam[:, -1].max(), lam[:, 0].min())
    assert not steer or (np.abs(out["solve", 25][1] - v_free.cpu().numpy()[keep]) > 1e-6 * np.abs(out["solve", 25][1])).sum() >= 5
    for name in ("plan", "solve"):
        rel = np.abs(out[name, 25][1] - out["torch", 25][1]) / np.maximum(np.abs(out["torch", 25][1]), 1e-12)
        assert (rel < 1e-8).mean() >= 0.9 and rel.max() < 1e-6, (name, np.sort(rel)[-8:])


@pytest.mark.parametrize("n_train", [12, 60])
@pytest.mark.parametrize("flavour,d", [(f, d) for f in ("ai", "le") for d in range(2, 9)] + [("ai", d) for d in (9, 10, 11, 12)]
                         + [("frob", d) for d in range(2, 9)])
def test_every_trust_region_kernel_instantiation_against_the_torch_solver(flavour, d, n_train):
    """One small constrained (eigenvalue box, strict) EI sweep per surrogate metric and dimension, on every execution plan the library offers
    for it - the single launch (LDS-resident with 12 training points; generic workspace with 60, whose GP factors do not fit beside it), the
    propose / update launches, the tCG launches - against the torch lock-step solver: same iteration counts, same values.  Every
    (dimension, metric, workspace) instantiation of the trust-region kernels is launched here once; two of them were wrong as compiled
    until round 5 and no test had run them."""
    import functools
    from gabotorch_amd.kernel_utils.kernels_spd import SpdFrobeniusGaussianKernel, SpdLogEuclideanGaussianKernel
    from gabotorch_amd.manifold_optimization.manifold_optimize import gen_candidates_manifold
    if n_train > int(_lib.load().gabo_spd_acq_max_train(d)):
        pytest.skip("more training points than the fused evaluation holds at this dimension")
    rng, X, y = _spd_gp(d, n_train=n_train, seed=100 + d)
    if flavour == "ai":
        kern = SpdAffineInvariantGaussianKernel(beta_min=0.5)
    else:
        kern = (SpdLogEuclideanGaussianKernel if flavour == "le" else SpdFrobeniusGaussianKernel)().double()
        kern.lengthscale = torch.tensor(1.4, dtype=torch.float64)
    R = 16
    q = np.linalg.qr(rng.standard_normal((R, d, d)))[0]
    P = np.einsum("nab,nb,ncb->nac", q, rng.uniform(0.5, 2.2, (R, d)), q)
    x0 = ops.matrix_to_mandel(t(0.5 * (P + P.transpose(0, 2, 1))))[:, None]
    # Guard: the solves must move on an EI that is not ~0.  u = (best_f - mu) / sigma at the 16 starts, from the CPU reference of the acquisition
    # (tests/_cpu_acquisition.py, nothing from the device): at least half of the starts within |u| <= 6.  Where the (sum log lambda)^2 targets with
    # best_f = min y do not give that (every d >= 7 at 12 training points: no start within |u| <= 6 at d >= 8, the EI comparison there was one of
    # values ~0), the targets are standardised and best_f is their median.
    from tests import _cpu_acquisition as cpu_ref
    ref_kernel, ref_beta = ("ai_gaussian", kern.beta_float()) if flavour == "ai" else (flavour + "_gaussian", 1.0 / 1.4 ** 2)
    starts = x0[:, 0].cpu().numpy()

    def starts_in_range(targets, best):
        u = cpu_ref.acquisition(ref_kernel, starts, X, targets, ref_beta, float(targets.mean()), 1.0, 1e-2, best, "ei", False)["u"]
        return int((np.abs(u) <= 6.0).sum())
    best_f = float(y.min())
    if starts_in_range(y, best_f) < R // 2:
        y = (y - y.mean()) / y.std()
        best_f = float(np.median(y))
    assert starts_in_range(y, best_f) >= R // 2
    gp = models.ExactGP(t(X), t(y), kern, outputscale=1.0, noise=1e-2)
    acq = models.ExpectedImprovement(gp, best_f=best_f, maximize=False)
    cons = [functools.partial(scut.max_eigenvalue_constraint_torch, maximum_eigenvalue=2.6),
            functools.partial(scut.min_eigenvalue_constraint_torch, minimum_eigenvalue=0.3)]
    out = {}
    ops.set_error_checking(False)
    try:
        for name, opts in (("torch", {"device_tcg": False}), ("default", {}), ("no_solve", {"device_solve": False}),
                           ("tcg_launches", {"device_iteration": False})):
            solver = BatchedTrustRegions(mingradnorm=1e-5, maxiter=8, strict_constraints=True)
            c, v = gen_candidates_manifold(x0, acq, manifolds.PositiveDefinite(d), solver, vector_to_symmetric_matrix_mandel_torch,
                                           symmetric_matrix_to_vector_mandel_torch, inequality_constraints=cons, approx_hessian=True, options=opts)
            out[name] = (v.cpu().numpy(), solver.log["per_restart_iterations"].cpu().numpy(), "one_launch_solve" in solver.log)
    finally:
        ops.set_error_checking(True)
    assert not out["torch"][2] and not out["no_solve"][2] and not out["tcg_launches"][2]
    if d <= 6:
        assert out["default"][2]                     # (a single launch exists for every metric and size up to d = 6)
    for name in ("default", "no_solve", "tcg_launches"):
        np.testing.assert_array_equal(out[name][1], out["torch"][1], err_msg=name)
        np.testing.assert_allclose(out[name][0], out["torch"][0], rtol=1e-7, atol=1e-12, err_msg=name)
