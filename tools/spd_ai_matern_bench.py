#!/usr/bin/env python3
"""Gram matrix of SpdAffineInvariantMaternKernel on N points: the fused features launch (gabo_spd_ai_spectral_features, N L Cholesky
factorisations of order d in registers) plus the N x 2L product, against
  * the plain torch composition of the same features (einsum H^T X H, torch.linalg.cholesky on N L matrices, element-wise work) plus the same
    product, at N = --n, and
  * the Gram matrix of SpdAffineInvariantGaussianKernel (gabo_spd_ai_pairwise) at the same N: the library's yardstick on this metric.
The fused side is also timed alone at --n-large.

    python tools/spd_ai_matern_bench.py [--n 1024] [--n-large 4096] [--features 1024] [--dims 3 10] [--reps 20]

Device events, the median of `reps` repetitions, the variants taking turns inside one process after a warm-up of each.  Prints one table row
per (d, N, variant) and one JSON line at the end."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gabotorch_amd import _lib, ops                                                                    # noqa: E402

DEV = "cuda:0"


def _event_time(fn):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1e-3


def _alternate(variants, reps):
    for fn in variants.values():
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(reps):
        for k, fn in variants.items():
            times[k].append(_event_time(fn))
    return {k: statistics.median(v) for k, v in times.items()}


def _points(n, d, seed):
    rng = np.random.default_rng(seed)
    q = np.linalg.qr(rng.standard_normal((n, d, d)))[0]
    m = np.einsum("nab,nb,ncb->nac", q, rng.uniform(0.5, 2.0, (n, d)), q)
    return ops.matrix_to_mandel(torch.tensor(0.5 * (m + m.transpose(0, 2, 1)), device=DEV))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--n-large", type=int, default=4096)
    ap.add_argument("--features", type=int, default=1024)
    ap.add_argument("--dims", type=int, nargs="+", default=[3, 10])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--nu", type=float, default=2.5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("spd_ai_matern_bench: no HIP device is visible; there is nothing to measure without one")
    rows = []
    for d in a.dims:
        base = ops.spd_ai_spectral_base(d, a.features, a.nu, 0)
        h = torch.tensor(base[2], device=DEV)
        lam, w = ops.spd_ai_spectral_points(base, torch.tensor(0.9, dtype=torch.float64, device=DEV), a.nu)

        def fused(x):
            f = ops.spd_ai_spectral_features(x, h, lam, w)
            return torch.mm(f, f.t())

        def composed(x):
            f = ops._spectral_features_torch(ops._spectral_logdiag_torch(x, h), lam, w)
            return torch.mm(f, f.t())

        for n, with_torch in ((a.n, True), (a.n_large, False)):
            x = _points(n, d, d)
            other = x.clone()
            variants = {"fused features + product": lambda: fused(x), "features launch alone": lambda: ops.spd_ai_spectral_features(x, h, lam, w)}
            if with_torch:
                variants["torch composition + product"] = lambda: composed(x)
            variants["gaussian gram (gabo_spd_ai_pairwise)"] = lambda: ops.spd_ai_pairwise(x, other, 1.0, _lib.GABO_OUT_GAUSSIAN)
            got = _alternate(variants, a.reps)
            err = float((fused(x) - composed(x)).abs().max()) if with_torch else float("nan")
            for name, sec in got.items():
                rows.append({"d": d, "n": n, "features": a.features, "variant": name, "ms": sec * 1e3,
                             "factorisations_per_s": n * a.features / sec if "gaussian" not in name else None,
                             "over_fused": sec / got["fused features + product"]})
                print(f"d={d:2d} N={n:5d} L={a.features}  {name:40s} {sec * 1e3:10.3f} ms  {rows[-1]['over_fused']:8.2f} x fused", flush=True)
            if with_torch:
                print(f"d={d:2d} N={n:5d}  max |fused - torch composition| = {err:.2e}", flush=True)
    print(json.dumps({"tool": "spd_ai_matern_bench", "reps": a.reps, "rows": rows}))


if __name__ == "__main__":
    main()
