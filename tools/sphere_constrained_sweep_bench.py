"""One constrained acquisition sweep on the sphere, Python path against the native sweep drivers: S^9, 50 training points, EI, the library's bound
x[0] >= 0.1 (functools.partial over coordinate_lower_bound_constraint_torch), ConstrainedTrustRegions, 2048 raw samples, 512 and 64 restarts, FD
Hessian (--exact: the closed-form one).  `manifold.rand_batch` is replaced by a sampler of feasible points, as the reference's constrained examples
replace `manifold.rand`.

  (a) python path          options["native_sweep"] = False: draw, upload, score, read back, select, gather, evaluate, project, norm, then the one launch
  (b) native, two calls    the default with constraints: gabo_sphere_sweep_score, select_rows on the host, gabo_sphere_sweep_solve_constrained
  (c) native, one call     options["device_selection"] = True: gabo_sphere_sweep_run_constrained on the host sampler's points, one host wait
  (d) native, device rand  ... and options["device_rand"] = True: the raw samples drawn inside the constraint on the device, no host sampling

The forms are run in turn, `--repeats` rounds of them after `--warmup` rounds, each sweep timed on the host between two device synchronisations;
reported: the median and the range of every form.  On a checkout without the constrained drivers only (a) runs: the baseline."""
import argparse
import functools
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np                                                                                       # noqa: E402
import torch                                                                                             # noqa: E402
from gabotorch_amd import _lib, manifolds, models, ops                                                   # noqa: E402
from gabotorch_amd.kernel_utils.kernels_sphere import SphereGaussianKernel                              # noqa: E402
from gabotorch_amd.manifold_optimization.constrained_trust_regions import ConstrainedTrustRegions       # noqa: E402
from gabotorch_amd.manifold_optimization.manifold_optimize import joint_optimize_manifold               # noqa: E402
from gabotorch_amd.Riemannian_utils import sphere_constraints_utils_torch as scu                        # noqa: E402

BOUND = 0.1
FORMS = (("(a) python path", {"native_sweep": False}), ("(b) native, two calls", {}), ("(c) native, one call", {"device_selection": True}),
         ("(d) native, device rand", {"device_selection": True, "device_rand": True}))


def feasible_batch(dim, count):
    """count points uniform on the part x[0] > BOUND of S^(dim-1): numpy's global stream, by rejection (acceptance ~0.38 on S^9)"""
    out = np.empty((0, dim))
    while out.shape[0] < count:
        x = np.random.standard_normal((2 * (count - out.shape[0]) + 64, dim))
        x /= np.linalg.norm(x, axis=1, keepdims=True)
        out = np.concatenate([out, x[x[:, 0] > BOUND]])
    return out[:count]


def setting(dim, n_train, dev):
    rng = np.random.default_rng(3)
    X = rng.standard_normal((n_train, dim))
    X /= np.linalg.norm(X, axis=1, keepdims=True)
    y = np.arccos(np.clip(X[:, 0], -1, 1)) ** 2 + 0.05 * rng.standard_normal(n_train)
    gp = models.ExactGP(torch.tensor(X, device=dev), torch.tensor(y, device=dev), SphereGaussianKernel(beta_min=0.6), outputscale=1.0, noise=1e-2)
    acq = models.ExpectedImprovement(gp, best_f=float(y.min()), maximize=False)
    man = manifolds.Sphere(dim)
    man.rand_batch = functools.partial(feasible_batch, dim)
    man.rand = lambda: feasible_batch(dim, 1)[0]
    return acq, man


def sweep(acq, man, dev, R, raw, approx, maxiter, options, seed):
    np.random.seed(seed)
    torch.manual_seed(seed)
    cons = [functools.partial(scu.coordinate_lower_bound_constraint_torch, index=0, lower_bound=BOUND)]
    solver = ConstrainedTrustRegions(mingradnorm=1e-5, maxiter=maxiter)
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    best = joint_optimize_manifold(acq, man, solver, q=1, num_restarts=R, raw_samples=raw, bounds=None, inequality_constraints=cons,
                                   approx_hessian=approx, options=dict(options, device=str(dev), batched_rand=True))
    torch.cuda.synchronize(dev)
    return time.perf_counter() - t0, best, solver.log


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--restarts", type=int, nargs="+", default=[512, 64])
    ap.add_argument("--raw", type=int, default=2048)
    ap.add_argument("--dim", type=int, default=10)
    ap.add_argument("--n-train", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--maxiter", type=int, default=50)
    ap.add_argument("--exact", action="store_true", help="the exact Hessian instead of the finite-difference one")
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args()
    dev = torch.device(a.device)
    ops.set_error_checking(False)
    forms = FORMS if "gabo_sphere_sweep_run_constrained" in _lib.SIGNATURES else FORMS[:1]
    acq, man = setting(a.dim, a.n_train, dev)
    for R in a.restarts:
        times = {name: [] for name, _ in forms}
        last = {}
        for rep in range(a.warmup + a.repeats):
            for name, options in forms:
                dt, best, log = sweep(acq, man, dev, R, a.raw, not a.exact, a.maxiter, options, 5 + rep)
                if rep >= a.warmup:
                    times[name].append(dt)
                last[name] = (best, log)
        for name, options in forms:
            best, log = last[name]
            assert bool(log.get("native_sweep")) == (options.get("native_sweep", True)) and log.get("one_launch_solve"), (name, log)
            assert bool(log.get("device_selection")) == bool(options.get("device_selection")), (name, log.get("device_selection"))
            ms = np.sort(np.array(times[name])) * 1e3
            row = {"form": name, "restarts": R, "raw": a.raw, "dim": a.dim, "n_train": a.n_train, "sweeps": len(ms), "median_ms": float(np.median(ms)),
                   "min_ms": float(ms[0]), "max_ms": float(ms[-1]), "EI": float(acq(best[None]).item()), "x0": float(best[0, 0]),
                   "outer_iterations": int(log["iterations"])}
            print(f"S^{a.dim - 1} n={a.n_train} EI x[0]>={BOUND} raw={a.raw} R={R:4d} {name:24s}: median {row['median_ms']:7.3f} ms  range [{row['min_ms']:.3f}, "
                  f"{row['max_ms']:.3f}] over {len(ms)} sweeps  EI*={row['EI']:.4e} x[0]={row['x0']:.4f} outer iterations {row['outer_iterations']}", flush=True)
            print("JSON " + json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
