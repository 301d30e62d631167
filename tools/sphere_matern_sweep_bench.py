"""Acquisition sweeps with a SphereRiemannianMaternKernel surrogate: the native plan (one-call sweep driver, single-launch solve, the ZONAL
instantiations of csrc/sphere_tr.hip) against the lock-step plan this kernel ran before it had them (strip by sphere_zonal_from_inner +
gabo_gp_acquisition per evaluation, the solver's arithmetic in torch), with SphereGaussianKernel's native sweep on the same problem as the yardstick.

  * S^9, the gabo_sphere setting of tools/sphere_sweep_bench.py (50 training points, EI, FD Hessian, no constraints): 64 restarts of 256 raw samples and
    512 of 2048, L = 32;
  * S^2, 64 restarts of 256 raw samples, L = 16 / 32 / 64.

Wall time around whole sweeps (synchronised before and after), the three sides in turn in one process, median of 20 alternating repetitions after 2
warm-up rounds.    python tools/sphere_matern_sweep_bench.py [--reps 20] [--out FILE.json]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from gabotorch_amd import manifolds, models, ops  # noqa: E402
from gabotorch_amd.fused_acquisition import FusedAcquisition  # noqa: E402
from gabotorch_amd.kernel_utils.kernels_sphere import SphereGaussianKernel, SphereRiemannianMaternKernel  # noqa: E402
from gabotorch_amd.manifold_optimization.batched_trust_regions import BatchedTrustRegions  # noqa: E402
from gabotorch_amd.manifold_optimization.manifold_optimize import joint_optimize_manifold  # noqa: E402

LOCK_STEP = {"native_sweep": False}


def surrogate(kernel, dim, n_train, device):
    rng = np.random.default_rng(3)
    X = rng.standard_normal((n_train, dim))
    X /= np.linalg.norm(X, axis=1, keepdims=True)
    y = np.arccos(np.clip(X[:, 0], -1, 1)) ** 2 + 0.05 * rng.standard_normal(n_train)
    gp = models.ExactGP(torch.tensor(X, device=device), torch.tensor(y, device=device), kernel, outputscale=1.0, noise=1e-2)
    return models.ExpectedImprovement(gp, best_f=float(y.min()), maximize=False)


def matern(levels):
    kern = SphereRiemannianMaternKernel(nu=2.5, num_levels=levels).double()
    kern.lengthscale = torch.tensor(0.7, dtype=torch.float64)
    return kern


def sweep(acq, dim, R, raw, device, options):
    np.random.seed(5)
    torch.manual_seed(5)
    solver = BatchedTrustRegions(mingradnorm=1e-5, maxiter=50)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    best = joint_optimize_manifold(acq, manifolds.Sphere(dim), solver, q=1, num_restarts=R, raw_samples=raw, bounds=None,
                                   options=dict(options, device=str(device), batched_rand=True), approx_hessian=True)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, best, solver.log


def measure(dim, levels, R, raw, device, reps):
    native, lock, gauss = (surrogate(matern(levels), dim, 50, device), surrogate(matern(levels), dim, 50, device),
                           surrogate(SphereGaussianKernel(beta_min=0.6), dim, 50, device))
    # the plan of the parent commit: no series evaluator, so no device-resident plan applies (the object is cached on the acquisition)
    FusedAcquisition.build(lock, None, device).series_launch = False
    sides = (("native", native, {}), ("lock-step", lock, LOCK_STEP), ("gaussian native", gauss, {}))
    times = {name: [] for name, _, _ in sides}
    plans, values = {}, {}
    for rep in range(reps + 2):
        for name, acq, options in sides:
            dt, best, log = sweep(acq, dim, R, raw, device, options)
            if rep >= 2:
                times[name].append(dt * 1e3)
            plans[name] = (bool(log.get("native_sweep")), bool(log.get("one_launch_solve")), int(log["iterations"]))
            values[name] = float(acq(best[None]).item())
    assert plans["native"][:2] == (True, True) and plans["gaussian native"][:2] == (True, True) and plans["lock-step"][:2] == (False, False), plans
    row = {"dim": dim, "levels": levels, "restarts": R, "raw": raw}
    for name in times:
        v = np.array(times[name])
        row[name] = {"median_ms": float(np.median(v)), "min_ms": float(v.min()), "max_ms": float(v.max()), "iterations": plans[name][2], "ei": values[name]}
    row["speedup"] = row["lock-step"]["median_ms"] / row["native"]["median_ms"]
    return row


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    device = torch.device("cuda", torch.cuda.current_device())
    ops.set_error_checking(False)
    rows = []
    for dim, levels, R, raw in ((10, 32, 64, 256), (10, 32, 512, 2048), (3, 16, 64, 256), (3, 32, 64, 256), (3, 64, 64, 256)):
        row = measure(dim, levels, R, raw, device, args.reps)
        rows.append(row)
        fmt = lambda s: f"{s['median_ms']:.3f} [{s['min_ms']:.3f}, {s['max_ms']:.3f}]"      # noqa: E731
        print(f"S^{dim - 1} L = {levels} {R} restarts of {raw}: native {fmt(row['native'])} ms, lock-step {fmt(row['lock-step'])} ms "
              f"({row['speedup']:.1f} x), SphereGaussianKernel native {fmt(row['gaussian native'])} ms; TR iterations "
              f"{row['native']['iterations']} / {row['lock-step']['iterations']} / {row['gaussian native']['iterations']}, EI at the candidate "
              f"{row['native']['ei']:.6e} / {row['lock-step']['ei']:.6e}", flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(rows, fh, indent=1)
