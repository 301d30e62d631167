#!/usr/bin/env python3
"""Surrogate fit of HD-GaBO on the sphere with ScaleKernel(NestedSphereRiemannianMaternKernel): the one-call problem
(_NestedSphereMllProblem: gabo_nested_sphere_fit_evaluate_series per evaluation) against the generic one (_MllProblem: torch autograd through
the level-by-level projection, the GEMM, the element-wise series and the likelihood launch), for fit_gpytorch_manifold as a whole and for one
objective-and-gradient evaluation.

    python tools/nested_sphere_matern_fit_bench.py [--reps 20] [--shapes 5,3 21,3 51,4] [--sizes 5 20 50 160 300] [--levels 32]
                                                   [--fit-iters 10] [--candidates 10]

Both are host-bound, so the figure is wall time around a call that ends in a device synchronise: the median of `reps` repetitions, the two
sides taking turns inside one process, after a warm-up of each.  Every fit starts from the same seeded model and candidates.  Prints one table
row per shape and one JSON line at the end."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gabotorch_amd import models                                                                           # noqa: E402
from gabotorch_amd._compat import ScaleKernel                                                              # noqa: E402
from gabotorch_amd.kernel_utils.kernels_nested_sphere import NestedSphereRiemannianMaternKernel            # noqa: E402
from gabotorch_amd.manifold_optimization import manifold_gp_fit as mgf                                     # noqa: E402
from gabotorch_amd.manifold_optimization.conjugate_gradient import ConjugateGradient                       # noqa: E402
from gabotorch_amd.manifold_optimization.host_manifolds import Euclidean, Product                          # noqa: E402

DEV = "cuda:0"


def _model(x, y, D, lat, levels):
    torch.manual_seed(4)
    base = NestedSphereRiemannianMaternKernel(D, lat, nu=2.5, num_levels=levels)
    kern = ScaleKernel(base, outputscale_prior=models.GammaPrior(2.0, 0.15)).double()
    return models.SingleTaskGP(x, y, kern, noise_prior=models.GammaPrior(1.1, 0.05)), base


def _timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def _alternate(variants, reps):
    """median wall time of each callable, the callables taking turns"""
    for fn in variants:
        fn()                                   # warm-up: code objects, workspaces, the pinned buffers
    times = [[] for _ in variants]
    for _ in range(reps):
        for k, fn in enumerate(variants):
            times[k].append(_timed(fn))
    return [statistics.median(ts) for ts in times]


def _fit(x, y, D, lat, levels, one_call, fit_iters, candidates):
    gp, _ = _model(x, y, D, lat, levels)
    np.random.seed(7)
    build = mgf._NestedSphereMllProblem.build
    if not one_call:
        mgf._NestedSphereMllProblem.build = staticmethod(lambda *a: None)
    try:
        _, info = mgf.fit_gpytorch_manifold(gp, solver=ConjugateGradient(maxiter=fit_iters), nb_init_candidates=candidates)
    finally:
        mgf._NestedSphereMllProblem.build = staticmethod(build)
    return info


def _problems(x, y, D, lat, levels):
    gp, base = _model(x, y, D, lat, levels)
    named = list(gp.named_parameters())
    params = [p for _, p in named]
    for p in params:
        p.requires_grad_(True)
    axis_ids = {id(a) for a in base.axes}
    factors = [getattr(base, nm.split(".")[-1] + "_manifold") if id(p) in axis_ids else Euclidean(int(p.numel())) for nm, p in named]
    manifold = Product(factors)
    names = [nm for nm, _ in named]
    fast = mgf._NestedSphereMllProblem.build(gp, names, params, manifold)
    if fast is None:
        raise SystemExit("nested_sphere_matern_fit_bench: the one-call problem was not selected")
    rng = np.random.default_rng(D)
    pt = [man.rand() if id(p) in axis_ids else rng.normal(0.3, 0.4, size=(int(p.numel()),)) for p, man in zip(params, factors)]
    return fast, mgf._MllProblem(gp, names, params, manifold), pt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--shapes", nargs="+", default=["5,3", "21,3", "51,4"], help="D,latent pairs")
    ap.add_argument("--sizes", type=int, nargs="+", default=[5, 20, 50, 160, 300])
    ap.add_argument("--levels", type=int, default=32)
    ap.add_argument("--fit-iters", type=int, default=10)
    ap.add_argument("--candidates", type=int, default=10)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("nested_sphere_matern_fit_bench: no HIP device is visible; there is nothing to measure without one")
    rows = []
    for shape in a.shapes:
        D, lat = (int(v) for v in shape.split(","))
        for n in a.sizes:
            rng = np.random.default_rng(1000 * D + n)
            xs = rng.standard_normal((n, D))
            xs /= np.linalg.norm(xs, axis=1, keepdims=True)
            x = torch.tensor(xs, device=DEV)
            y = torch.tensor(np.arccos(np.clip(xs[:, 0], -1, 1)) ** 2 + 0.05 * rng.standard_normal(n), device=DEV)
            fast, slow, pt = _problems(x, y, D, lat, a.levels)

            def eval_fast():
                fast._recent = []              # (the recent-result cache would answer the repetition)
                fast.cost(pt)
                fast.egrad(pt)

            def eval_slow():
                slow.cost(pt)
                slow.egrad(pt)

            ev_fast, ev_slow = _alternate([eval_fast, eval_slow], a.reps)
            gap = abs(fast.cost(pt) - slow.cost(pt))
            fit_fast, fit_slow = _alternate([lambda: _fit(x, y, D, lat, a.levels, True, a.fit_iters, a.candidates),
                                             lambda: _fit(x, y, D, lat, a.levels, False, a.fit_iters, a.candidates)], a.reps)
            row = {"D": D, "latent": lat, "n": n, "levels": a.levels, "eval_one_call_ms": ev_fast * 1e3, "eval_autograd_ms": ev_slow * 1e3,
                   "eval_cost_gap": gap, "fit_one_call_ms": fit_fast * 1e3, "fit_autograd_ms": fit_slow * 1e3}
            rows.append(row)
            print(f"D={D:3d} latent={lat} n={n:4d}  objective + gradient: one call {row['eval_one_call_ms']:8.3f} ms  autograd "
                  f"{row['eval_autograd_ms']:9.2f} ms ({ev_slow / ev_fast:6.1f}x; cost gap {gap:.1e})   fit: one call "
                  f"{row['fit_one_call_ms']:9.2f} ms  autograd {row['fit_autograd_ms']:10.2f} ms ({fit_slow / fit_fast:6.1f}x)", flush=True)
    print(json.dumps({"tool": "nested_sphere_matern_fit_bench", "reps": a.reps, "fit_iters": a.fit_iters, "candidates": a.candidates,
                      "rows": rows}))


if __name__ == "__main__":
    main()
