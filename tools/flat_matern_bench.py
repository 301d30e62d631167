#!/usr/bin/env python3
"""Gram matrix of the log-Euclidean Matern kernels (gabo_flat_matern_pairwise) on N x N pairs of given features, against
  * the Gaussian Gram of SpdLogEuclideanGaussianKernel on the same features (gabo_frobenius_pairwise, GABO_OUT_GAUSSIAN): the kernel that sits
    on the write floor of 8 bytes per pair, and
  * torch.cdist plus the Matern formula in torch operations (nu = 5/2).

    python tools/flat_matern_bench.py [--n 4096] [--dims 3 10] [--reps 20] [--inner 20]

Device events around `inner` back-to-back launches, the median of `reps` repetitions, all variants taking turns inside one process after a
warm-up of each.  Prints one table row per (d, variant), the bytes-per-pair rate each time implies, and one JSON line at the end."""
import argparse
import json
import math
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gabotorch_amd import _lib, ops                                                                    # noqa: E402

DEV = "cuda:0"


def _event_time(fn, inner):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(inner):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1e-3 / inner


def _alternate(variants, reps, inner):
    for fn in variants.values():
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(reps):
        for k, fn in variants.items():
            times[k].append(_event_time(fn, inner))
    return {k: statistics.median(v) for k, v in times.items()}


def _torch_matern52(f, ls):
    x = torch.cdist(f, f) * (math.sqrt(5.0) / ls)
    return (1.0 + x + x * x / 3.0) * torch.exp(-x)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--dims", type=int, nargs="+", default=[3, 10])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--inner", type=int, default=20)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("flat_matern_bench: no HIP device is visible; there is nothing to measure without one")
    rows = []
    ls = 0.9
    for d in a.dims:
        rng = np.random.default_rng(d)
        q = np.linalg.qr(rng.standard_normal((a.n, d, d)))[0]
        m = np.einsum("nab,nb,ncb->nac", q, rng.uniform(0.5, 2.0, (a.n, d)), q)
        feat = ops.spd_logm_mandel(ops.matrix_to_mandel(torch.tensor(0.5 * (m + m.transpose(0, 2, 1)), device=DEV)))
        other = feat.clone()          # two sets: the general launch, as the Gaussian yardstick runs it
        variants = {f"matern nu={nu}": (lambda nu=nu: ops.flat_matern_pairwise(feat, other, ls, nu)) for nu in (0.5, 1.5, 2.5)}
        variants["gaussian"] = lambda: ops.frobenius_pairwise(feat, other, 1.0 / (ls * ls), _lib.GABO_OUT_GAUSSIAN)
        variants["torch cdist + formula (nu=2.5)"] = lambda: _torch_matern52(feat, ls)
        got = _alternate(variants, a.reps, a.inner)
        err = float((ops.flat_matern_pairwise(feat, other, ls, 2.5) - _torch_matern52(feat, ls)).abs().max())
        for name, sec in got.items():
            rows.append({"d": d, "n": a.n, "variant": name, "us": sec * 1e6, "gb_per_s_written": 8.0 * a.n * a.n / sec * 1e-9,
                         "over_gaussian": sec / got["gaussian"]})
            print(f"d={d:2d} N={a.n}  {name:32s} {sec * 1e6:9.1f} us  {rows[-1]['gb_per_s_written']:7.0f} GB/s written  "
                  f"{rows[-1]['over_gaussian']:5.2f} x gaussian", flush=True)
        print(f"d={d:2d}  max |matern 5/2 - torch formula| = {err:.2e}", flush=True)
    print(json.dumps({"tool": "flat_matern_bench", "reps": a.reps, "inner": a.inner, "rows": rows}))


if __name__ == "__main__":
    main()
