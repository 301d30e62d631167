"""Candidates of seeded acquisition sweeps with the GEODESIC sphere kernels (SphereGaussianKernel, SphereLaplaceKernel) through the single-launch
solve and the native sweep drivers, recorded on an MI355X at the commit BEFORE csrc/sphere_tr.hip learnt the series kernels:

    python tests/golden/make_golden_sphere_native_pin.py [OUT.npz]        (default: tests/golden/sphere_native_pin.npz)

tests/test_gpu_sphere_matern_native.py re-runs `cases()` and demands the same bits: the geodesic instantiations of the kernels are the ones they
were.  Data only: per case the candidate, the final costs and the per-restart iteration counts."""
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

DEV = "cuda:0"


def _surrogate(kernel_name, dim, n):
    from gabotorch_amd import models
    from gabotorch_amd.kernel_utils.kernels_sphere import SphereGaussianKernel, SphereLaplaceKernel
    rng = np.random.RandomState(11 + dim)
    X = rng.randn(n, dim)
    X /= np.linalg.norm(X, axis=1, keepdims=True)
    y = np.sin(3.0 * X[:, 0]) + X[:, 1] * X[:, -1] + 0.5 * X[:, -1]
    if kernel_name == "gaussian":
        kern = SphereGaussianKernel(beta_min=0.1).double()
        kern.beta = torch.tensor(6.5 if dim == 3 else 1.5, dtype=torch.float64)
    else:
        kern = SphereLaplaceKernel().double()
        kern.lengthscale = 0.8
    t = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device=DEV)      # noqa: E731
    gp = models.ExactGP(t(X), t(y), kern, outputscale=1.0, noise=1e-2)
    return models.ExpectedImprovement(gp, best_f=float(y.min()), maximize=False)


# (kernel, dim, training points, FD Hessian, constrained, restarts, raw samples, options)
CASES = [("gaussian", 3, 20, False, False, 16, 64, {}), ("gaussian", 3, 20, True, True, 16, 64, {}),
         ("gaussian", 10, 50, True, False, 64, 256, {}), ("gaussian", 10, 50, False, False, 16, 64, {"device_selection": True, "device_rand": True}),
         ("gaussian", 3, 20, False, False, 16, 64, {"native_sweep": False}), ("gaussian", 3, 20, True, False, 8, 32, {"native_sweep": False, "device_solve": False}),
         ("laplace", 3, 20, False, False, 16, 64, {}), ("laplace", 3, 20, True, True, 16, 64, {}),
         ("laplace", 10, 50, True, False, 64, 256, {}), ("laplace", 3, 20, False, True, 7, 50, {"native_sweep": False})]


def run_case(case):
    """-> dict of numpy arrays: candidate, final costs, per-restart iterations"""
    import functools

    from gabotorch_amd import manifolds
    from gabotorch_amd.manifold_optimization.constrained_trust_regions import ConstrainedTrustRegions
    from gabotorch_amd.manifold_optimization.manifold_optimize import joint_optimize_manifold
    from gabotorch_amd.manifold_optimization.robust_trust_regions import TrustRegions
    from gabotorch_amd.Riemannian_utils import sphere_constraints_utils_torch as scu
    kernel_name, dim, n, approx, constrained, R, raw, options = case
    acq = _surrogate(kernel_name, dim, n)
    np.random.seed(21)
    torch.manual_seed(21)
    man = manifolds.Sphere(dim)
    if constrained:
        solver = ConstrainedTrustRegions(maxiter=100)
        cons = [functools.partial(scu.coordinate_lower_bound_constraint_torch, index=0, lower_bound=-0.2)]
    else:
        solver, cons = TrustRegions(maxiter=100), None
    best = joint_optimize_manifold(acq, man, solver, q=1, num_restarts=R, raw_samples=raw, bounds=None, inequality_constraints=cons,
                                   approx_hessian=approx, options=dict(options, device=DEV))
    log = solver.log
    return {"best": best.cpu().numpy(), "final_cost": log["final_cost"].cpu().numpy(),
            "iterations": log["per_restart_iterations"].cpu().numpy(),
            "plan": np.array([bool(log.get("native_sweep")), bool(log.get("one_launch_solve")), bool(log.get("device_selection"))])}


def main(out):
    store = {}
    for i, case in enumerate(CASES):
        res = run_case(case)
        print(i, case, "plan (native, one launch, device selection)", res["plan"].tolist(), "iterations max", int(res["iterations"].max()),
              "candidate", res["best"].ravel()[:3])
        assert math.isfinite(float(res["final_cost"].min()))
        for k, v in res.items():
            store[f"case{i}_{k}"] = v
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    np.savez(out, **store)
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "sphere_native_pin.npz"))
