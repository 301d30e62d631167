"""The constrained trust-region solve on the sphere, single launch against the propose / update launches: S^2, 50 training points, EI, the
five bound constraints of gabo_sphere_bound_constraints.py:94-121, ConstrainedTrustRegions, 64 and 512 restarts from feasible starts.

  one launch            the library's constraint functions, evaluated by the wave (gabo_sphere_tr_solve_constrained)
  two launches, eval    the same constraints, propose / update launches with one gabo_sphere_constraints_eval launch between them
  two launches, lambdas opaque callables: a Python call and an autograd pass per constraint and iteration (the only plan there was
                        for a constrained sphere problem before the library functions existed)

The plans are run in turn, `--repeats` rounds of them after `--warmup` rounds, each solve timed on the host around a device synchronise;
reported: the median and the quartiles of every plan, and the final iterates' largest difference between the plans."""
import argparse
import functools
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np                                                                                       # noqa: E402
import torch                                                                                             # noqa: E402
from gabotorch_amd import manifolds, models, ops                                                         # noqa: E402
from gabotorch_amd.kernel_utils.kernels_sphere import SphereGaussianKernel                              # noqa: E402
from gabotorch_amd.manifold_optimization.constrained_trust_regions import ConstrainedTrustRegions       # noqa: E402
from gabotorch_amd.manifold_optimization.manifold_optimize import gen_candidates_manifold               # noqa: E402
from gabotorch_amd.Riemannian_utils import sphere_constraints_utils_torch as scu                        # noqa: E402

BOX = dict(xl=0.0, yl=-0.6, yu=0.6, zl=-0.6, zu=0.6)


def library_constraints(b=BOX):
    lo = lambda i, v: functools.partial(scu.coordinate_lower_bound_constraint_torch, index=i, lower_bound=v)      # noqa: E731
    up = lambda i, v: functools.partial(scu.coordinate_upper_bound_constraint_torch, index=i, upper_bound=v)      # noqa: E731
    return [lo(0, b["xl"]), lo(1, b["yl"]), up(1, b["yu"]), lo(2, b["zl"]), up(2, b["zu"])]


def lambda_constraints(b=BOX):
    return [lambda x: x[..., 0] - b["xl"], lambda x: x[..., 1] - b["yl"], lambda x: b["yu"] - x[..., 1], lambda x: x[..., 2] - b["zl"],
            lambda x: b["zu"] - x[..., 2]]


def feasible_points(rng, count, b=BOX):
    out = []
    while len(out) < count:
        p = np.array([rng.uniform(b["xl"], 1.0), rng.uniform(b["yl"], b["yu"]), rng.uniform(b["zl"], b["zu"])])
        p /= np.linalg.norm(p)
        if p[0] > b["xl"] and b["yl"] < p[1] < b["yu"] and b["zl"] < p[2] < b["zu"]:
            out.append(p)
    return np.stack(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--restarts", type=int, nargs="+", default=[64, 512])
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--maxiter", type=int, default=200)
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args()
    dev = torch.device(a.device)
    ops.set_error_checking(False)
    rng = np.random.default_rng(3)
    X = feasible_points(rng, 50)
    y = np.arccos(np.clip(X[:, 0], -1, 1)) ** 2 + np.sin(4.0 * X[:, 1]) * X[:, 2] + 0.05 * rng.standard_normal(50)
    kern = SphereGaussianKernel(beta_min=0.1).double()
    kern.beta = torch.tensor(6.5, dtype=torch.float64)
    gp = models.ExactGP(torch.tensor(X, device=dev), torch.tensor(y, device=dev), kern, outputscale=1.0, noise=1e-2)
    acq = models.ExpectedImprovement(gp, best_f=float(y.min()), maximize=False)
    plans = (("one launch", library_constraints(), {}),
             ("two launches, eval", library_constraints(), {"device_solve": False}),
             ("two launches, lambdas", lambda_constraints(), {"device_solve": False}))
    for R in a.restarts:
        x0 = torch.tensor(feasible_points(np.random.default_rng(7), R), device=dev)[:, None]
        times = {name: [] for name, _, _ in plans}
        ends, logs = {}, {}
        for rep in range(a.warmup + a.repeats):
            for name, cons, options in plans:
                solver = ConstrainedTrustRegions(maxiter=a.maxiter)
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                x, _ = gen_candidates_manifold(x0, acq, manifolds.Sphere(3), solver, inequality_constraints=cons, approx_hessian=False, options=options)
                torch.cuda.synchronize(dev)
                if rep >= a.warmup:
                    times[name].append(time.perf_counter() - t0)
                ends[name], logs[name] = x, solver.log
        assert logs["one launch"].get("one_launch_solve") and not logs["two launches, lambdas"].get("one_launch_solve")
        for name, _, _ in plans:
            ms = np.sort(np.array(times[name])) * 1e3
            q1, med, q3 = np.percentile(ms, [25, 50, 75])
            print(f"S^2 n=50 EI five bounds R={R} {name:22s}: median {med:8.3f} ms  quartiles [{q1:.3f}, {q3:.3f}]  min {ms[0]:.3f} max {ms[-1]:.3f}  "
                  f"outer iterations {logs[name]['iterations']}  |x - x(one launch)| {float((ends[name] - ends['one launch']).abs().max()):.1e}", flush=True)


if __name__ == "__main__":
    main()
