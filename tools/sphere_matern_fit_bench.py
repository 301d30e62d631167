#!/usr/bin/env python3
"""Surrogate fit with the sphere Matern kernel: one gabo_gp_mll_series launch per L-BFGS evaluation (fit_gpytorch_model(fast=True)) against
the autograd route (fast=False: GEMM, element-wise series, gabo_gp_mll_gram, W, a second series launch, a reduction), and one
ops.gp_mll_series evaluation against one ops.gp_mll evaluation at the same size - what the series costs over exp(-theta E).

    python tools/sphere_matern_fit_bench.py [--reps 20] [--sizes 20 50 100 160 512] [--dims 3 10] [--levels 32]

The fit is host-bound, so the figure is wall time around a call that ends in a device synchronise: the median of `reps` repetitions, the two
variants alternating inside one process, after a warm-up of each.  Prints one table row per (dim, n) and one JSON line at the end."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gabotorch_amd import models, ops                                                                  # noqa: E402
from gabotorch_amd._compat import ScaleKernel                                                          # noqa: E402
from gabotorch_amd.kernel_utils.kernels_sphere import SphereRiemannianMaternKernel                     # noqa: E402

DEV = "cuda:0"


def _model(x, y, levels):
    kern = ScaleKernel(SphereRiemannianMaternKernel(nu=2.5, num_levels=levels).double(), outputscale_prior=models.GammaPrior(2.0, 0.15)).double()
    return models.SingleTaskGP(x, y, kern, noise_prior=models.GammaPrior(1.1, 0.05))


def _timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def _alternate(variants, reps):
    """median wall time of each callable, the callables taking turns"""
    for fn in variants:
        fn()                                   # warm-up: code objects, workspaces, the pinned result buffer
    times = [[] for _ in variants]
    for _ in range(reps):
        for k, fn in enumerate(variants):
            times[k].append(_timed(fn))
    return [statistics.median(ts) for ts in times]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--sizes", type=int, nargs="+", default=[20, 50, 100, 160, 512])
    ap.add_argument("--dims", type=int, nargs="+", default=[3, 10])
    ap.add_argument("--levels", type=int, default=32)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sphere_matern_fit_bench: no HIP device is visible; there is nothing to measure without one")
    rows = []
    for dim in a.dims:
        for n in a.sizes:
            rng = np.random.default_rng(1000 * dim + n)
            xs = rng.standard_normal((n, dim))
            xs /= np.linalg.norm(xs, axis=1, keepdims=True)
            x = torch.tensor(xs, device=DEV)
            y = torch.tensor(np.arccos(np.clip(xs[:, 0], -1, 1)) ** 2 + 0.05 * rng.standard_normal(n), device=DEV)
            fit_fast, fit_auto = _alternate([lambda: models.fit_gpytorch_model(_model(x, y, a.levels), fast=True),
                                             lambda: models.fit_gpytorch_model(_model(x, y, a.levels), fast=False)], a.reps)
            a_, b_ = _model(x, y, a.levels), _model(x, y, a.levels)
            models.fit_gpytorch_model(a_, fast=True)
            models.fit_gpytorch_model(b_, fast=False)
            for m in (a_, b_):
                for p in m.parameters():
                    p.requires_grad_(True)
            gap = abs(float(a_.marginal_log_likelihood()) - float(b_.marginal_log_likelihood()))
            # one evaluation: the series launch on C = X X^T against the exp launch on E = d^2 at the same n
            c = (x @ x.T).contiguous()
            e = (2.0 - 2.0 * c).clamp_min(0.0).contiguous()
            p, dp, sd = ops.sphere_matern_coefficients_and_derivative(dim, 0.5, 2.5, a.levels)
            ev_series, ev_coeff, ev_exp = _alternate(
                [lambda: ops.gp_mll_series(c, y, p, dp, sd, 1.7, 0.03, -0.2),
                 lambda: ops.gp_mll_series(c, y, *ops.sphere_matern_coefficients_and_derivative(dim, 0.5, 2.5, a.levels), 1.7, 0.03, -0.2),
                 lambda: ops.gp_mll(e, y, 0.4, 1.7, 0.03, -0.2)], 10 * a.reps)
            row = {"dim": dim, "n": n, "levels": a.levels, "fit_fast_ms": fit_fast * 1e3, "fit_autograd_ms": fit_auto * 1e3,
                   "fit_likelihood_gap": gap, "eval_series_us": ev_series * 1e6, "eval_series_with_coefficients_us": ev_coeff * 1e6,
                   "eval_exp_us": ev_exp * 1e6}
            rows.append(row)
            print(f"S^{dim - 1} n={n:4d}  fit fast {row['fit_fast_ms']:8.2f} ms  autograd {row['fit_autograd_ms']:8.2f} ms  "
                  f"({fit_auto / fit_fast:5.1f}x; likelihood gap {gap:.1e})   evaluation: series {row['eval_series_us']:7.1f} us "
                  f"(+ coefficients {row['eval_series_with_coefficients_us']:7.1f} us), exp {row['eval_exp_us']:7.1f} us", flush=True)
    print(json.dumps({"tool": "sphere_matern_fit_bench", "reps": a.reps, "rows": rows}))


if __name__ == "__main__":
    main()
