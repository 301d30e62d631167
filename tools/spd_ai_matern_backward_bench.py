#!/usr/bin/env python3
"""The x-gradient of SpdAffineInvariantMaternKernel by the backward launch (x_grad="launch": the fused features launch forward,
gabo_spd_ai_spectral_features_backward backward) against the plain torch composition (x_grad="torch": einsum H^T X H, torch.linalg.cholesky on
N L matrices and the autograd tape through both), with a lengthscale that does not require grad - the acquisition maximiser's situation.
Timed per (d, N1), N1 candidates against --train training points:
  * value plus x1-gradient of a weighted sum of the kernel matrix, under either route;
  * the backward launch pair alone, and the forward features launch at the same shape as the yardstick.
One more row: wall time of one joint_optimize_manifold call (expected improvement on a fitted d = 2 model of 10 points, 128 features, 3 restarts
from 12 raw samples, 5 trust-region iterations: the problem of tests/test_gpu_spd_ai_spectral.py) under either route.

    python tools/spd_ai_matern_backward_bench.py [--candidates 64 512] [--train 50] [--features 1024] [--dims 3 10] [--reps 20]

Device events, the median of `reps` repetitions, the variants taking turns inside one process after a warm-up of each (the maximiser: wall
time around calls that end in a device synchronise, median of --opt-reps).  Prints one table row per measurement and one JSON line at the end."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gabotorch_amd import manifolds, models, ops                                                       # noqa: E402
from gabotorch_amd._compat import ScaleKernel                                                          # noqa: E402
from gabotorch_amd.kernel_utils.kernels_spd import SpdAffineInvariantMaternKernel                      # noqa: E402
from gabotorch_amd.manifold_optimization.batched_trust_regions import BatchedTrustRegions              # noqa: E402
from gabotorch_amd.manifold_optimization.manifold_optimize import joint_optimize_manifold              # noqa: E402
from gabotorch_amd.Riemannian_utils.spd_utils_torch import (symmetric_matrix_to_vector_mandel_torch,   # noqa: E402
                                                            vector_to_symmetric_matrix_mandel_torch)

DEV = "cuda:0"


def _event_time(fn):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1e-3


def _wall_time(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def _alternate(variants, reps, clock=_event_time):
    for fn in variants.values():
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(reps):
        for k, fn in variants.items():
            times[k].append(clock(fn))
    return {k: statistics.median(v) for k, v in times.items()}


def _spd(rng, n, d, lo=0.5, hi=2.0):
    q = np.linalg.qr(rng.standard_normal((n, d, d)))[0]
    m = np.einsum("nab,nb,ncb->nac", q, rng.uniform(lo, hi, (n, d)), q)
    return 0.5 * (m + m.transpose(0, 2, 1))


def _points(rng, n, d):
    return ops.matrix_to_mandel(torch.tensor(_spd(rng, n, d), device=DEV))


def _kernel(d, nu, features, route):
    k = SpdAffineInvariantMaternKernel(d, nu=nu, num_features=features, seed=0, x_grad=route).double()
    k.lengthscale = torch.tensor(0.9, dtype=torch.float64)
    k = k.to(DEV)
    k.raw_lengthscale.requires_grad_(False)
    return k


def _maximiser_problem():
    """the fitted model of the end-to-end test, its parameters frozen afterwards"""
    rng = np.random.default_rng(9)
    d, n = 2, 10
    mats = _spd(rng, n, d)
    x = ops.matrix_to_mandel(torch.tensor(mats, device=DEV))
    y = torch.tensor(np.log(np.linalg.det(mats)) + 0.05 * rng.standard_normal(n), device=DEV)
    base = SpdAffineInvariantMaternKernel(d, nu=2.5, num_features=128, seed=1)
    gp = models.SingleTaskGP(x, y, ScaleKernel(base, outputscale_prior=models.GammaPrior(2.0, 0.15)), noise_prior=models.GammaPrior(1.1, 0.05))
    models.fit_gpytorch_model(gp)
    for p in gp.parameters():
        p.requires_grad_(False)
    acq = models.ExpectedImprovement(gp, best_f=float(y.min()), maximize=False)
    man = manifolds.PositiveDefinite(2)
    man.min_eig, man.max_eig = 0.5, 2.0

    def rand():
        lam = man.min_eig + (man.max_eig - man.min_eig) * np.random.rand(2)
        q = np.linalg.qr(np.random.randn(2, 2))[0]
        m = q @ np.diag(lam) @ q.T
        return 0.5 * (m + m.T)
    man.rand = rand

    def run(route):
        base.x_grad = route
        np.random.seed(0)
        torch.manual_seed(0)
        return joint_optimize_manifold(acq, man, BatchedTrustRegions(mingradnorm=1e-5, maxiter=5), q=1, num_restarts=3, raw_samples=12, bounds=None,
                                       options={"device": DEV}, pre_processing_manifold=vector_to_symmetric_matrix_mandel_torch,
                                       post_processing_manifold=symmetric_matrix_to_vector_mandel_torch, approx_hessian=True)
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--candidates", type=int, nargs="+", default=[64, 512])
    ap.add_argument("--train", type=int, default=50)
    ap.add_argument("--features", type=int, default=1024)
    ap.add_argument("--dims", type=int, nargs="+", default=[3, 10])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--opt-reps", type=int, default=3)
    ap.add_argument("--nu", type=float, default=2.5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("spd_ai_matern_backward_bench: no HIP device is visible; there is nothing to measure without one")
    rows = []

    def report(d, n1, name, sec, over, train=None, features=None):
        train, features = train or a.train, features or a.features
        rows.append({"d": d, "n1": n1, "train": train, "features": features, "variant": name, "ms": sec * 1e3, "over_launch_route": over})
        print(f"d={d:2d} N1={n1:4d} n={train} L={features}  {name:46s} {sec * 1e3:10.3f} ms  {over:8.2f} x the launch route", flush=True)

    for d in a.dims:
        rng = np.random.default_rng(d)
        kernels = {route: _kernel(d, a.nu, a.features, route) for route in ("launch", "torch")}
        x2 = _points(rng, a.train, d)
        with torch.no_grad():
            k0 = kernels["launch"]
            h = k0._phases_on(torch.device(DEV))
            lam, w = ops.spd_ai_spectral_points(k0.spectral_base, k0.lengthscale.double().reshape(()), a.nu)
        for n1 in a.candidates:
            x1 = _points(rng, n1, d).requires_grad_(True)
            c = torch.tensor(rng.standard_normal((n1, a.train)), device=DEV)
            gbar = torch.tensor(rng.standard_normal((n1, 2 * a.features)), device=DEV)
            with torch.no_grad():
                fhat = ops.spd_ai_spectral_features(x1, h, lam, w)

            def value_and_gradient(route):
                k = kernels[route].forward(x1, x2)
                return torch.autograd.grad((c * k).sum(), x1)[0]

            variants = {"value + x1-gradient, x_grad='launch'": lambda: value_and_gradient("launch"),
                        "value + x1-gradient, x_grad='torch'": lambda: value_and_gradient("torch"),
                        "backward launch pair alone": lambda: ops.spd_ai_spectral_features_backward(x1, h, lam, fhat, gbar),
                        "forward features launch alone": lambda: ops.spd_ai_spectral_features(x1.detach(), h, lam, w)}
            got = _alternate(variants, a.reps)
            g_l, g_t = value_and_gradient("launch"), value_and_gradient("torch")
            for name, sec in got.items():
                report(d, n1, name, sec, sec / got["value + x1-gradient, x_grad='launch'"])
            print(f"d={d:2d} N1={n1:4d}  max |gradient by launch - by torch| = {float((g_l - g_t).abs().max()):.2e} "
                  f"(largest entry {float(g_t.abs().max()):.2e});  backward pair / forward launch = "
                  f"{got['backward launch pair alone'] / got['forward features launch alone']:.2f}", flush=True)
    run = _maximiser_problem()
    got = _alternate({"launch": lambda: run("launch"), "torch": lambda: run("torch")}, a.opt_reps, clock=_wall_time)
    same = float((run("launch") - run("torch")).abs().max())
    for route, sec in got.items():
        report(2, 3, f"joint_optimize_manifold, x_grad='{route}' (wall)", sec, sec / got["launch"], train=10, features=128)
    print(f"maximiser: max |candidate by launch - by torch| = {same:.2e}", flush=True)
    print(json.dumps({"tool": "spd_ai_matern_backward_bench", "reps": a.reps, "opt_reps": a.opt_reps, "rows": rows}))


if __name__ == "__main__":
    main()
