#!/usr/bin/env python3
"""Times the Gram matrix of the Riemannian Matern kernel on the sphere (csrc/sphere_zonal.hip) at N = 4096, dim in {3, 10},
num_levels in {16, 32, 64}:

  (a) the fused launch                       ops.sphere_zonal_pairwise: inner products and series in one kernel
  (b) torch.matmul + the element-wise series ops.sphere_zonal_from_inner on x x^T (the route autograd takes)
  (c) the recurrence in plain torch operations on x x^T: what a user writes without the library's kernel - the baseline
  (d) SphereGaussianKernel's Gram at the same shape (beta = 1.3, table built beforehand): the write-floor yardstick

Device events around each call, all sides in turn within every repetition, in one process, after warm-up; reported: the median of the
repetitions [min, max].  The coefficients are computed on the host once (they are launch arguments, not part of the timed region of (a) - (c)).

    python tools/sphere_matern_bench.py [--n 4096] [--reps 20] [--warmup 3]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gabotorch_amd import ops                                                                          # noqa: E402

DEV = "cuda:0"


def torch_series(c, coeff, series_dim):
    """(c): sum_k coeff[k] P_k(c) as one writes it from the recurrence, a handful of element-wise launches per level"""
    d, coeff = series_dim, [float(v) for v in coeff]
    p0, p1 = torch.ones_like(c), c
    f = coeff[0] + coeff[1] * c
    for k in range(2, len(coeff)):
        p = ((2 * k + d - 3) * c * p1 - (k - 1) * p0) / (k + d - 2)
        f = f + coeff[k] * p
        p0, p1 = p1, p
    return f


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def bench(n, dim, levels, reps, warmup):
    rng = np.random.default_rng(dim * 1000 + levels)
    x = rng.standard_normal((n, dim))
    x = torch.tensor(x / np.linalg.norm(x, axis=1, keepdims=True), device=DEV)
    coeff, sd = ops.sphere_matern_coefficients(dim, 0.3, 2.5, levels)
    sides = {
        "a_fused": lambda: ops.sphere_zonal_pairwise(x, x, coeff, sd),
        "a_fused_symmetric": lambda: ops.sphere_zonal_pairwise(x, x, coeff, sd, symmetric=True),
        "b_matmul_from_inner": lambda: ops.sphere_zonal_from_inner(x @ x.t(), coeff, sd),
        "c_torch_ops": lambda: torch_series(x @ x.t(), coeff, sd),
        "d_gaussian_gram": lambda: ops.sphere_pairwise(x, x, 1.3),
    }
    for _ in range(warmup):
        for fn in sides.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in sides}
    last = {}
    for _ in range(reps):
        for k, fn in sides.items():
            ms, last[k] = event_ms(fn)
            times[k].append(ms * 1e3)
    res = {"n": n, "dim": dim, "num_levels": levels, "reps": reps,
           **{k: {"median_us": float(np.median(v)), "min_us": float(np.min(v)), "max_us": float(np.max(v))} for k, v in times.items()},
           "max_abs_b_minus_a": float((last["b_matmul_from_inner"] - last["a_fused"]).abs().max()),
           "max_abs_c_minus_a": float((last["c_torch_ops"] - last["a_fused"]).abs().max()),
           "symmetric_equals_plain": bool(torch.equal(last["a_fused_symmetric"], last["a_fused"]))}
    print(f"N = {n}, dim = {dim}, num_levels = {levels}")
    for k in sides:
        s = res[k]
        print(f"  {k:22s} {s['median_us']:10.1f} us  [{s['min_us']:.1f}, {s['max_us']:.1f}]")
    print("RESULT " + json.dumps(res), flush=True)
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sphere_matern_bench.py needs an MI355X: there is nothing to time without one")
    with torch.no_grad():
        for dim in (3, 10):
            for levels in (16, 32, 64):
                bench(a.n, dim, levels, a.reps, a.warmup)
