#!/usr/bin/env python3
"""Surrogate fit with the affine-invariant SPD Matern kernel: one gabo_gp_mll_spd_ai_spectral call per L-BFGS evaluation
(fit_gpytorch_model(fast=True)) against the autograd route (fast=False: element-wise torch on the log-diagonals, the feature product,
gabo_gp_mll_gram, W and the backward pass through all of it), and one ops.gp_mll_spd_ai_spectral evaluation against one ops.gp_mll evaluation
at the same n - what 2 L random phase features cost over exp(-theta E) on a stored distance matrix.

    python tools/spd_ai_matern_fit_bench.py [--reps 20] [--sizes 20 50 100 160 512] [--dims 3 10] [--features 1024] [--nu 2.5]

The fit is host-bound, so the figure is wall time around a call that ends in a device synchronise: the median of `reps` repetitions, the two
variants alternating inside one process, after a warm-up of each.  Both fits include the one ops.spd_ai_logdiag launch of their point set.
Prints one table row per (d, n) and one JSON line at the end."""
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
from gabotorch_amd.kernel_utils.kernels_spd import SpdAffineInvariantMaternKernel                      # noqa: E402

DEV = "cuda:0"


def _model(x, y, d, nu, features):
    base = SpdAffineInvariantMaternKernel(d, nu=nu, num_features=features, seed=1)
    kern = ScaleKernel(base, outputscale_prior=models.GammaPrior(2.0, 0.15))
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
    ap.add_argument("--dims", type=int, nargs="+", default=[3, 10])
    ap.add_argument("--features", type=int, default=1024)
    ap.add_argument("--nu", type=float, default=2.5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("spd_ai_matern_fit_bench: no HIP device is visible; there is nothing to measure without one")
    rows = []
    for d in a.dims:
        for n in a.sizes:
            x, y = _spd_mandel(np.random.default_rng(1000 * d + n), n, d)
            make = lambda: _model(x, y, d, a.nu, a.features)                                              # noqa: E731
            fit_fast, fit_auto = _alternate([lambda: models.fit_gpytorch_model(make(), fast=True),
                                             lambda: models.fit_gpytorch_model(make(), fast=False)], a.reps)
            a_, b_ = make(), make()
            models.fit_gpytorch_model(a_, fast=True)
            models.fit_gpytorch_model(b_, fast=False)
            for m in (a_, b_):
                for p in m.parameters():
                    p.requires_grad_(True)
            gap = abs(float(a_.marginal_log_likelihood().detach()) - float(b_.marginal_log_likelihood().detach()))
            # one evaluation: the chain on the stored log-diagonals against the exp launch on a distance matrix at the same n
            base = a_.covar_module.base_kernel
            logdiag = ops.spd_ai_logdiag(x, base._phases_on(x.device)).contiguous()
            e = ops.spd_ai_pairwise(x, x, 1.0, return_dist=True)[1].contiguous() ** 2
            ev_spec, ev_exp = _alternate([lambda: ops.gp_mll_spd_ai_spectral(logdiag, y, base.spectral_base, 0.9, a.nu, 1.7, 0.03, -0.2),
                                          lambda: ops.gp_mll(e, y, 0.6, 1.7, 0.03, -0.2)], 10 * a.reps)
            row = {"d": d, "n": n, "nu": a.nu, "features": a.features, "fit_fast_ms": fit_fast * 1e3, "fit_autograd_ms": fit_auto * 1e3,
                   "fit_likelihood_gap": gap, "eval_spectral_us": ev_spec * 1e6, "eval_exp_us": ev_exp * 1e6}
            rows.append(row)
            print(f"S^{d}_++ n={n:4d}  fit fast {row['fit_fast_ms']:8.2f} ms  autograd {row['fit_autograd_ms']:8.2f} ms  "
                  f"({fit_auto / fit_fast:5.1f}x; likelihood gap {gap:.1e})   evaluation: spectral {row['eval_spectral_us']:7.1f} us, "
                  f"exp {row['eval_exp_us']:7.1f} us", flush=True)
    print(json.dumps({"tool": "spd_ai_matern_fit_bench", "reps": a.reps, "rows": rows}))


if __name__ == "__main__":
    main()
