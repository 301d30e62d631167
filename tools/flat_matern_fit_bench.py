#!/usr/bin/env python3
"""Surrogate fit with the log-Euclidean Matern kernel: one gabo_gp_mll_matern launch per L-BFGS evaluation (fit_gpytorch_model(fast=True))
against the autograd route (fast=False: logm, Gram launch, gabo_gp_mll_gram, W, the backward launches), and one ops.gp_mll_matern
evaluation against one ops.gp_mll evaluation at the same size - what the Matern function costs over exp(-theta E).

    python tools/flat_matern_fit_bench.py [--reps 20] [--sizes 20 50 100 160 512] [--d 3] [--nu 2.5]

The fit is host-bound, so the figure is wall time around a call that ends in a device synchronise: the median of `reps` repetitions, the two
variants alternating inside one process, after a warm-up of each.  Prints one table row per n and one JSON line at the end."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gabotorch_amd import _lib, models, ops                                                            # noqa: E402
from gabotorch_amd._compat import ScaleKernel                                                          # noqa: E402
from gabotorch_amd.kernel_utils.kernels_spd import SpdLogEuclideanMaternKernel                         # noqa: E402

DEV = "cuda:0"


def _model(x, y, nu):
    kern = ScaleKernel(SpdLogEuclideanMaternKernel(nu=nu).double(), outputscale_prior=models.GammaPrior(2.0, 0.15)).double()
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


def _spd_mandel(rng, n, d):
    q = np.linalg.qr(rng.standard_normal((n, d, d)))[0]
    m = np.einsum("nab,nb,ncb->nac", q, rng.uniform(0.5, 2.0, (n, d)), q)
    m = 0.5 * (m + m.transpose(0, 2, 1))
    y = np.log(np.linalg.det(m)) + 0.3 * np.trace(m, axis1=-2, axis2=-1) + 0.05 * rng.standard_normal(n)
    return ops.matrix_to_mandel(torch.tensor(m, device=DEV)), torch.tensor(y, device=DEV)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--sizes", type=int, nargs="+", default=[20, 50, 100, 160, 512])
    ap.add_argument("--d", type=int, default=3)
    ap.add_argument("--nu", type=float, default=2.5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("flat_matern_fit_bench: no HIP device is visible; there is nothing to measure without one")
    rows = []
    for n in a.sizes:
        x, y = _spd_mandel(np.random.default_rng(1000 * a.d + n), n, a.d)
        fit_fast, fit_auto = _alternate([lambda: models.fit_gpytorch_model(_model(x, y, a.nu), fast=True),
                                         lambda: models.fit_gpytorch_model(_model(x, y, a.nu), fast=False)], a.reps)
        a_, b_ = _model(x, y, a.nu), _model(x, y, a.nu)
        models.fit_gpytorch_model(a_, fast=True)
        models.fit_gpytorch_model(b_, fast=False)
        for m in (a_, b_):
            for p in m.parameters():
                p.requires_grad_(True)
        gap = abs(float(a_.marginal_log_likelihood()) - float(b_.marginal_log_likelihood()))
        # one evaluation: the Matern launch on the distances against the exp launch on E = r^2 at the same n
        feat = ops.spd_logm_mandel(x)
        r = ops.frobenius_pairwise(feat, feat, 1.0, _lib.GABO_OUT_DISTANCE).contiguous()
        e = (r * r).contiguous()
        ev_matern, ev_exp = _alternate([lambda: ops.gp_mll_matern(r, y, 0.9, a.nu, 1.7, 0.03, -0.2),
                                        lambda: ops.gp_mll(e, y, 0.6, 1.7, 0.03, -0.2)], 10 * a.reps)
        row = {"d": a.d, "n": n, "nu": a.nu, "fit_fast_ms": fit_fast * 1e3, "fit_autograd_ms": fit_auto * 1e3, "fit_likelihood_gap": gap,
               "eval_matern_us": ev_matern * 1e6, "eval_exp_us": ev_exp * 1e6}
        rows.append(row)
        print(f"S^{a.d}_++ n={n:4d}  fit fast {row['fit_fast_ms']:8.2f} ms  autograd {row['fit_autograd_ms']:8.2f} ms  "
              f"({fit_auto / fit_fast:5.1f}x; likelihood gap {gap:.1e})   evaluation: matern {row['eval_matern_us']:7.1f} us, "
              f"exp {row['eval_exp_us']:7.1f} us", flush=True)
    print(json.dumps({"tool": "flat_matern_fit_bench", "reps": a.reps, "rows": rows}))


if __name__ == "__main__":
    main()
