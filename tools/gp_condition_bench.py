"""Conditioning the GP on the device against rebuilding its prediction cache, and the q-point believer batch against the same batch with a
rebuild between its sweeps.  Device events around whole chains (kernel strips included), the two sides alternating in one process after a
warm-up; medians in microseconds.

  (a) model.condition_on_observations(one point, its target)   vs   the training set replaced by the concatenated one and the cache rebuilt
      (gabo_spd_gp_prepare / gabo_gp_factor up to GABO_GP_FACTOR_MAX_N points, torch.linalg.cholesky + solves with their host wait beyond)
  (b) sequential_optimize_manifold(q = 4)   vs   four joint_optimize_manifold sweeps with posterior mean + rebuild in between

usage: python tools/gp_condition_bench.py [--reps 20] [--out FILE.json]"""
import argparse
import functools
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from gabotorch_amd import manifolds, models, ops
from gabotorch_amd.kernel_utils.kernels_spd import SpdAffineInvariantGaussianKernel
from gabotorch_amd.kernel_utils.kernels_sphere import SphereGaussianKernel
from gabotorch_amd.manifold_optimization.batched_trust_regions import BatchedTrustRegions
from gabotorch_amd.manifold_optimization.manifold_optimize import joint_optimize_manifold, sequential_optimize_manifold
from gabotorch_amd.Riemannian_utils import spd_constraints_utils_torch as scut
from gabotorch_amd.Riemannian_utils.spd_utils_torch import symmetric_matrix_to_vector_mandel_torch as to_vec, vector_to_symmetric_matrix_mandel_torch as to_mat

DEV = "cuda:0"
SIZES = (20, 96, 97, 160, 512, 2047)


def data(kind, count, seed=0):
    rng = np.random.default_rng(seed)
    if kind == "spd3":
        q = np.linalg.qr(rng.standard_normal((count, 3, 3)))[0]
        X = np.einsum("nab,nb,ncb->nac", q, rng.uniform(0.1, 4.0, (count, 3)), q)
        x = to_vec(torch.tensor(0.5 * (X + X.transpose(0, 2, 1))))
        y = torch.tensor((np.log(np.linalg.eigvalsh(X) / 2.0) ** 2).sum(1))
    else:
        X = rng.standard_normal((count, 4))
        X /= np.linalg.norm(X, axis=1, keepdims=True)
        x, y = torch.tensor(X), torch.tensor(np.arccos(np.clip(X[:, 0], -1, 1)) ** 2 + 0.05 * rng.standard_normal(count))
    return x.to(DEV), y.to(DEV)


def model(kind, x, y):
    kern = SpdAffineInvariantGaussianKernel(beta_min=0.25) if kind == "spd3" else SphereGaussianKernel(beta_min=0.6)
    return models.ExactGP(x, y, kern, outputscale=1.0, noise=1e-2, mean=float(y.mean()))


def rebuild(gp, x, y):
    """what a caller without condition_on_observations does: new training set, cache from scratch"""
    gp.train_x, gp.train_y, gp._cache = x, y, None
    return gp._train_cache()


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3


def alternate(sides, reps, warmup=3):
    for _ in range(warmup):
        for fn in sides:
            fn()
    torch.cuda.synchronize()
    times = [[] for _ in sides]
    for _ in range(reps):
        for i, fn in enumerate(sides):
            times[i].append(timed(fn))
            ops.check_deferred()          # (outside the timed window: the status words of the launches just timed)
    return [(statistics.median(t), min(t), max(t)) for t in times]


def bench_condition(kind, n, reps):
    x, y = data(kind, n + 1)
    src = model(kind, x[:n], y[:n])
    src._train_cache()
    other = model(kind, x[:n], y[:n])
    ops.check_deferred()

    def conditioned():
        src.condition_on_observations(x[n:], y[n:])

    def rebuilt():
        rebuild(other, x, y)
    (c, cmin, cmax), (r, rmin, rmax) = alternate((conditioned, rebuilt), reps)
    ops.check_deferred()
    return dict(model=kind, n=n, condition_us=c, condition_min_us=cmin, condition_max_us=cmax, rebuild_us=r, rebuild_min_us=rmin, rebuild_max_us=rmax)


def bench_batch(kind, n, reps, q=4, restarts=64, raw=256):
    x, y = data(kind, n, seed=1)
    if kind == "spd3":
        man = manifolds.PositiveDefinite(3)
        man.min_eig, man.max_eig = 0.05, 5.0
        kw = dict(inequality_constraints=[functools.partial(scut.max_eigenvalue_constraint_torch, maximum_eigenvalue=5.0),
                                          functools.partial(scut.min_eigenvalue_constraint_torch, minimum_eigenvalue=0.05)],
                  pre_processing_manifold=to_mat, post_processing_manifold=to_vec, approx_hessian=True)
    else:
        man, kw = manifolds.Sphere(4), dict(approx_hessian=True)
    best = float(y.min())
    native = []

    def sweep(fn, acq, **more):
        solver = BatchedTrustRegions(mingradnorm=1e-5, maxiter=40)
        out = fn(acq, man, solver, num_restarts=restarts, raw_samples=raw, bounds=None, options={"device": DEV}, **kw, **more)
        native.append(bool(solver.log.get("native_sweep")))
        return out

    def sequential():
        np.random.seed(3)
        torch.manual_seed(3)
        sweep(sequential_optimize_manifold, models.ExpectedImprovement(model(kind, x, y), best_f=best, maximize=False), q=q)

    def host_loop():
        np.random.seed(3)
        torch.manual_seed(3)
        gp = model(kind, x, y)
        acq = models.ExpectedImprovement(gp, best_f=best, maximize=False)
        for k in range(q):
            row = sweep(joint_optimize_manifold, acq, q=1).reshape(1, -1)
            if k + 1 < q:
                mu, _ = gp.posterior(row)
                rebuild(gp, torch.cat([gp.train_x, row]), torch.cat([gp.train_y, mu.reshape(-1)]))
    (s, smin, smax), (h, hmin, hmax) = alternate((sequential, host_loop), reps, warmup=2)
    return dict(model=kind, n=n, q=q, restarts=restarts, raw_samples=raw, native_sweeps=all(native), sequential_us=s, sequential_min_us=smin,
                sequential_max_us=smax, host_rebuild_us=h, host_rebuild_min_us=hmin, host_rebuild_max_us=hmax)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gp_condition_bench needs an MI355X: nothing is measured without one")
    rows_a, rows_b = [], []
    print("(a) one point: condition_on_observations vs rebuild, median [min, max] us")
    for kind in ("spd3", "sphere3"):
        for n in SIZES:
            r = bench_condition(kind, n, args.reps)
            rows_a.append(r)
            print(f"  {kind:8s} n {n:5d}: condition {r['condition_us']:9.1f} [{r['condition_min_us']:.1f}, {r['condition_max_us']:.1f}]   "
                  f"rebuild {r['rebuild_us']:9.1f} [{r['rebuild_min_us']:.1f}, {r['rebuild_max_us']:.1f}]   ratio {r['rebuild_us'] / r['condition_us']:.2f}", flush=True)
    print("(b) q = 4 batch: sequential_optimize_manifold vs four sweeps with a host rebuild in between, median [min, max] us")
    for kind in ("spd3", "sphere3"):
        for n in (50, 160):
            r = bench_batch(kind, n, max(args.reps // 2, 3))
            rows_b.append(r)
            print(f"  {kind:8s} n {n:5d}: sequential {r['sequential_us']:10.1f} [{r['sequential_min_us']:.1f}, {r['sequential_max_us']:.1f}]   "
                  f"host rebuild {r['host_rebuild_us']:10.1f} [{r['host_rebuild_min_us']:.1f}, {r['host_rebuild_max_us']:.1f}]   "
                  f"ratio {r['host_rebuild_us'] / r['sequential_us']:.2f}   native sweeps {r['native_sweeps']}", flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"condition": rows_a, "batch": rows_b}, f, indent=1)


if __name__ == "__main__":
    main()
