"""Generator of tests/golden/sweep_pins.npz: what twelve tiny native sweeps (gabotorch_amd/manifold_optimization/native_sweep.py, csrc/spd_sweep.hip)
returned BEFORE the drivers moved into that module, and the cases themselves (tests/test_gpu_sweep_pins.py runs them again and compares exactly).
Needs an MI355X.

    python tests/golden/make_golden_sweep_pins.py            (writes the fixture)

The fixture in the repository was written on the commit before the move, where the one name this file takes from native_sweep (the sphere
driver, which holds the flag of the exhausted-sampler warning) lived in manifold_optimize.

8 training points, 5 restarts among 12 raw samples, 10 trust-region iterations: the smallest shapes at which the drivers' bookkeeping (rows of the
tables, picks, retries, the fall-backs, the log) can go wrong.  Every case is run three times; a case whose device bytes differ between those runs
keeps only its host-side record (generators, log keys and flags, warnings), and with more than two such cases no fixture is written."""
import functools
import math
import os
import sys
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

DEV = "cuda:0"
N_TRAIN, RESTARTS, RAW, MAXITER = 8, 5, 12, 10
DEVICE_KEYS = ("candidate", "final_cost", "per_restart_iterations", "iterations", "final_constraints", "picks")
HOST_KEYS = ("log_keys", "log_true", "log_false", "warnings", "next_numpy", "next_torch")


def _spd_problem(best_shift=0.0):
    from gabotorch_amd import manifolds, models
    from gabotorch_amd.kernel_utils.kernels_spd import SpdAffineInvariantGaussianKernel
    from gabotorch_amd.Riemannian_utils import spd_constraints_utils_torch as scut
    from oracle import spd as ospd
    rng = np.random.default_rng(3)
    d = 3
    q = np.linalg.qr(rng.standard_normal((N_TRAIN, d, d)))[0]
    X = np.einsum("nab,nb,ncb->nac", q, rng.uniform(0.3, 3.0, (N_TRAIN, d)), q)
    xv = torch.tensor(ospd.symmetric_matrix_to_vector_mandel(0.5 * (X + X.transpose(0, 2, 1))), device=DEV)
    y = torch.tensor(rng.standard_normal(N_TRAIN), device=DEV)
    gp = models.ExactGP(xv, y, SpdAffineInvariantGaussianKernel(beta_min=0.3), outputscale=1.0, noise=1e-2)
    acq = models.ExpectedImprovement(gp, best_f=float(y.min()) - best_shift, maximize=False)
    man = manifolds.PositiveDefinite(d)
    man.min_eig, man.max_eig = 0.1, 4.0

    def rand():          # (the reference's spd_sample: numpy's global stream)
        lam = man.min_eig + (man.max_eig - man.min_eig) * np.random.rand(d)
        u, _ = np.linalg.qr(np.random.randn(d, d))
        return u @ np.diag(lam) @ u.T
    man.rand = rand
    cons = [functools.partial(scut.max_eigenvalue_constraint_torch, maximum_eigenvalue=4.0)]
    return acq, man, cons


def _spd_case(options, restarts=RESTARTS, raw=RAW, best_shift=0.0):
    def run():
        from gabotorch_amd.manifold_optimization.batched_trust_regions import BatchedTrustRegions
        from gabotorch_amd.manifold_optimization.manifold_optimize import joint_optimize_manifold
        from gabotorch_amd.Riemannian_utils.spd_utils_torch import symmetric_matrix_to_vector_mandel_torch as to_vec
        from gabotorch_amd.Riemannian_utils.spd_utils_torch import vector_to_symmetric_matrix_mandel_torch as to_mat
        acq, man, cons = _spd_problem(best_shift)
        solver = BatchedTrustRegions(mingradnorm=1e-4, maxiter=MAXITER)
        return solver, lambda: joint_optimize_manifold(acq, man, solver, q=1, num_restarts=restarts, raw_samples=raw, bounds=None,
                                                       options=dict(options, device=DEV, log_picked=True), inequality_constraints=cons,
                                                       pre_processing_manifold=to_mat, post_processing_manifold=to_vec, approx_hessian=True)
    return run


def _sphere_acq(matern_levels=None):
    from gabotorch_amd import models
    from gabotorch_amd.kernel_utils.kernels_sphere import SphereGaussianKernel, SphereRiemannianMaternKernel
    rng = np.random.default_rng(4)
    X = rng.standard_normal((N_TRAIN, 3))
    X /= np.linalg.norm(X, axis=1, keepdims=True)
    y = np.arccos(np.clip(X[:, 0], -1, 1)) ** 2 + 0.05 * rng.standard_normal(N_TRAIN)
    if matern_levels is None:
        kern = SphereGaussianKernel(beta_min=6.5)
    else:
        kern = SphereRiemannianMaternKernel(nu=2.5, num_levels=matern_levels).double()
        kern.lengthscale = torch.tensor(0.6, dtype=torch.float64)
    gp = models.ExactGP(torch.tensor(X, device=DEV), torch.tensor(y, device=DEV), kern, outputscale=1.0, noise=1e-2)
    return models.ExpectedImprovement(gp, best_f=float(y.min()), maximize=False)


def _sphere_case(options, approx, constrained=False, matern_levels=None):
    def run():
        from gabotorch_amd import manifolds
        from gabotorch_amd.manifold_optimization import native_sweep
        from gabotorch_amd.manifold_optimization.constrained_trust_regions import ConstrainedTrustRegions
        from gabotorch_amd.manifold_optimization.manifold_optimize import joint_optimize_manifold
        from gabotorch_amd.manifold_optimization.robust_trust_regions import TrustRegions
        from gabotorch_amd.Riemannian_utils import sphere_constraints_utils_torch as scu
        acq = _sphere_acq(matern_levels)
        man = manifolds.Sphere(3)
        cons = None
        solver = TrustRegions(maxiter=MAXITER)
        if constrained:
            centre = torch.tensor([1.0, 0.0, 0.0], dtype=torch.float64)
            cons = [functools.partial(scu.coordinate_lower_bound_constraint_torch, index=1, lower_bound=-0.3),
                    functools.partial(scu.geodesic_ball_constraint_torch, center=centre, angle=1.0)]

            def feasible():          # (what the reference's constrained examples bind to manifold.rand: rejection on numpy's global stream)
                while True:
                    p = np.random.randn(3)
                    p /= np.linalg.norm(p)
                    if p[1] > -0.3 and math.acos(p[0]) < 1.0:
                        return p
            man.rand = feasible
            solver = ConstrainedTrustRegions(maxiter=MAXITER)
            native_sweep._native_sweep_sphere._warned_exhausted = False          # (the warning of an exhausted device sampler is raised once per process)
        return solver, lambda: joint_optimize_manifold(acq, man, solver, q=1, num_restarts=RESTARTS, raw_samples=RAW, bounds=None,
                                                       inequality_constraints=cons, approx_hessian=approx,
                                                       options=dict(options, device=DEV, log_picked=True))
    return run


CASES = {
    "spd_device_rand": _spd_case({"device_rand": True}),
    "spd_device_rand_host_selection": _spd_case({"device_rand": True, "device_selection": False}),
    "spd_host_rand_host_selection": _spd_case({"device_selection": False}),
    "spd_batched_rand": _spd_case({"batched_rand": True}),
    "spd_restarts_equal_raw": _spd_case({"device_rand": True}, restarts=5, raw=5),
    "spd_selection_flag_fallback": _spd_case({"device_rand": True}, best_shift=1e4),
    "sphere_one_call_host_sampler_fd": _sphere_case({}, approx=True),
    "sphere_one_call_device_rand_exact": _sphere_case({"device_rand": True}, approx=False),
    "sphere_two_calls": _sphere_case({"device_selection": False}, approx=False),
    "sphere_constrained_two_calls": _sphere_case({}, approx=False, constrained=True),
    "sphere_constrained_one_call_device_rand": _sphere_case({"device_selection": True, "device_rand": True}, approx=False, constrained=True),
    "sphere_matern_one_call": _sphere_case({}, approx=False, matern_levels=16),
}


def run_case(name):
    """One seeded sweep of case `name` -> {key: numpy array} of what the fixture records"""
    solver, sweep = CASES[name]()
    seed = 100 + list(CASES).index(name)
    np.random.seed(seed)
    torch.manual_seed(seed)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        best = sweep()
    next_numpy, next_torch = int(np.random.randint(2 ** 31)), int(torch.randint(2 ** 31, (1,)))
    log = solver.log
    picks = log.get("picked_samples", log.get("picked"))
    fc = log.get("final_constraints")
    return {"candidate": best.detach().cpu().numpy(), "final_cost": log["final_cost"].cpu().numpy(),
            "per_restart_iterations": log["per_restart_iterations"].cpu().numpy(), "iterations": np.array(log["iterations"]),
            "final_constraints": np.zeros(0) if fc is None else fc.cpu().numpy(), "picks": np.zeros(0, dtype=np.int64) if picks is None else np.asarray(picks),
            "log_keys": np.array(sorted(log)), "log_true": np.array(sorted(k for k, v in log.items() if v is True), dtype=str),
            "log_false": np.array(sorted(k for k, v in log.items() if v is False), dtype=str),
            "warnings": np.array(sorted(w.category.__name__ for w in caught), dtype=str),
            "next_numpy": np.array(next_numpy), "next_torch": np.array(next_torch)}


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def main(out):
    record, host_only = {}, []
    for name in CASES:
        runs = [run_case(name) for _ in range(3)]
        for key in HOST_KEYS:
            assert all(same(runs[0][key], r[key]) for r in runs[1:]), f"{name}: the host-side record {key} differs between runs"
        differing = [key for key in DEVICE_KEYS if not all(same(runs[0][key], r[key]) for r in runs[1:])]
        if differing:
            host_only.append(name)
            print(f"{name}: device bytes differ between runs of the same code in {differing}: host-side record only")
        for key in HOST_KEYS + (() if differing else DEVICE_KEYS):
            record[f"{name}/{key}"] = runs[0][key]
        print(name, {k: (v.tolist() if v.size <= 12 else v.shape) for k, v in runs[0].items()}, flush=True)
    if len(host_only) > 2:
        raise SystemExit(f"{len(host_only)} of {len(CASES)} cases are not reproducible on the device ({host_only}): no fixture written")
    record["host_only"] = np.array(host_only, dtype=str)
    np.savez_compressed(out, **record)
    print(f"wrote {out}: {len(CASES)} cases, host-side record only for {host_only}")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.abspath(__file__)), "sweep_pins.npz"))
