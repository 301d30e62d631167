#!/usr/bin/env python3
"""Surrogate fit of HD-GaBO on the SPD manifold with ScaleKernel(NestedSpdLogEuclideanMaternKernel): the one-call problem
(_NestedSpdMllProblem: gabo_nested_spd_fit_evaluate_matern per evaluation) against the generic one (_MllProblem: torch autograd through the
projection, logm, the Matern Gram and the likelihood launch), for fit_gpytorch_manifold as a whole and for one objective-and-gradient
evaluation; and the Gaussian one-call entry (gabo_nested_spd_fit_evaluate, NestedSpdLogEuclideanGaussianKernel) at the same shape, as the
yardstick for what the Matern chain should cost.

    python tools/nested_spd_matern_fit_bench.py [--reps 20] [--shapes 5,2 10,3 20,2] [--sizes 5 20 50 160 300] [--fit-iters 10] [--candidates 10]

All are host-bound, so the figure is wall time around a call that ends in a device synchronise: the median of `reps` repetitions, the sides
taking turns inside one process, after a warm-up of each.  Every fit starts from the same seeded model and candidates.  Prints one table row
per shape and one JSON line at the end."""
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
from gabotorch_amd.kernel_utils.kernels_spd import NestedSpdLogEuclideanGaussianKernel, NestedSpdLogEuclideanMaternKernel   # noqa: E402
from gabotorch_amd.manifold_optimization import manifold_gp_fit as mgf                                     # noqa: E402
from gabotorch_amd.manifold_optimization.conjugate_gradient import ConjugateGradient                       # noqa: E402
from gabotorch_amd.manifold_optimization.host_manifolds import Euclidean, Product                          # noqa: E402
from gabotorch_amd.Riemannian_utils.spd_utils import symmetric_matrix_to_vector_mandel                     # noqa: E402

DEV = "cuda:0"


def _model(x, y, D, d, matern=True):
    torch.manual_seed(4)
    base = NestedSpdLogEuclideanMaternKernel(D, d, nu=2.5) if matern else NestedSpdLogEuclideanGaussianKernel(D, d)
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


def _fit(x, y, D, d, one_call, fit_iters, candidates):
    gp, _ = _model(x, y, D, d)
    np.random.seed(7)
    build = mgf._NestedSpdMllProblem.build
    if not one_call:
        mgf._NestedSpdMllProblem.build = staticmethod(lambda *a: None)
    try:
        _, info = mgf.fit_gpytorch_manifold(gp, solver=ConjugateGradient(maxiter=fit_iters), nb_init_candidates=candidates)
    finally:
        mgf._NestedSpdMllProblem.build = staticmethod(build)
    return info


def _problems(x, y, D, d, matern=True):
    gp, base = _model(x, y, D, d, matern)
    named = list(gp.named_parameters())
    names, params = [nm for nm, _ in named], [p for _, p in named]
    for p in params:
        p.requires_grad_(True)
    factors = [base.raw_projection_matrix_manifold if p is base.raw_projection_matrix else Euclidean(int(p.numel())) for p in params]
    manifold = Product(factors)
    fast = mgf._NestedSpdMllProblem.build(gp, names, params, manifold)
    if fast is None:
        raise SystemExit("nested_spd_matern_fit_bench: the one-call problem was not selected")
    rng = np.random.default_rng(D)
    pt = [man.rand() if p is base.raw_projection_matrix else rng.normal(0.3, 0.4, size=(int(p.numel()),)) for p, man in zip(params, factors)]
    return fast, mgf._MllProblem(gp, names, params, manifold), pt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--shapes", nargs="+", default=["5,2", "10,3", "20,2"], help="D,latent pairs")
    ap.add_argument("--sizes", type=int, nargs="+", default=[5, 20, 50, 160, 300])
    ap.add_argument("--fit-iters", type=int, default=10)
    ap.add_argument("--candidates", type=int, default=10)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("nested_spd_matern_fit_bench: no HIP device is visible; there is nothing to measure without one")
    rows = []
    for shape in a.shapes:
        D, d = (int(v) for v in shape.split(","))
        for n in a.sizes:
            rng = np.random.default_rng(1000 * D + n)
            q = np.linalg.qr(rng.standard_normal((n, D, D)))[0]
            mats = np.einsum("nab,nb,ncb->nac", q, rng.uniform(0.1, 4.0, (n, D)), q)          # spectra uniform in [0.1, 4]
            x = torch.tensor(np.stack([symmetric_matrix_to_vector_mandel(0.5 * (m + m.T)) for m in mats]), device=DEV)
            y = torch.tensor(rng.standard_normal(n), device=DEV)
            fast, slow, pt = _problems(x, y, D, d)
            gauss = _problems(x, y, D, d, matern=False)[0]

            def eval_fast():
                fast._recent = []              # (the recent-result cache would answer the repetition)
                fast.cost(pt)
                fast.egrad(pt)

            def eval_slow():
                slow.cost(pt)
                slow.egrad(pt)

            def eval_gauss():
                gauss._recent = []
                gauss.cost(pt)
                gauss.egrad(pt)

            ev_fast, ev_slow, ev_gauss = _alternate([eval_fast, eval_slow, eval_gauss], a.reps)
            gap = abs(fast.cost(pt) - slow.cost(pt))
            fit_fast, fit_slow = _alternate([lambda: _fit(x, y, D, d, True, a.fit_iters, a.candidates),
                                             lambda: _fit(x, y, D, d, False, a.fit_iters, a.candidates)], a.reps)
            row = {"D": D, "latent": d, "n": n, "eval_one_call_ms": ev_fast * 1e3, "eval_autograd_ms": ev_slow * 1e3,
                   "eval_gaussian_one_call_ms": ev_gauss * 1e3, "eval_cost_gap": gap, "fit_one_call_ms": fit_fast * 1e3,
                   "fit_autograd_ms": fit_slow * 1e3}
            rows.append(row)
            print(f"D={D:3d} latent={d} n={n:4d}  objective + gradient: one call {row['eval_one_call_ms']:8.3f} ms  autograd "
                  f"{row['eval_autograd_ms']:9.2f} ms ({ev_slow / ev_fast:6.1f}x; cost gap {gap:.1e})  Gaussian one call "
                  f"{row['eval_gaussian_one_call_ms']:8.3f} ms ({ev_fast / ev_gauss:5.2f}x)   fit: one call {row['fit_one_call_ms']:9.2f} ms  "
                  f"autograd {row['fit_autograd_ms']:10.2f} ms ({fit_slow / fit_fast:6.1f}x)", flush=True)
    print(json.dumps({"tool": "nested_spd_matern_fit_bench", "reps": a.reps, "fit_iters": a.fit_iters, "candidates": a.candidates, "rows": rows}))


if __name__ == "__main__":
    main()
