#!/usr/bin/env python3
"""Times the joint GP posterior over a test set (ops.gp_posterior_joint: projection + fused covariance, two launches) and, at the demo size,
the chain on to posterior samples (ops.mvn_sample: one more launch) against the torch composition a user writes without them:

  (a) the new chain, from k* and k** resident on the device to Sigma (and on to 10 samples where m <= GABO_MVN_SAMPLE_MAX_M)
  (b) V = (os k*) @ linv^T;  Sigma = os k** - V @ V^T;  then torch.linalg.cholesky_ex with the jitter ladder and a matmul for the samples
  (b') the same with the product and the subtraction in one torch.addmm (beta = os, alpha = -1)

All forms run in one process, in turn within every round, after warm-up rounds of every form at every shape; a form's time is the time between two
device events around its launches (the inputs are resident; the copy of k** that (a) consumes is made outside the window).  Reported: median
[min, max] over the rounds.  For the covariance the compulsory HBM traffic - one read of the lower 64 x 64 tiles of k** and one write of the
whole matrix - over the time of (a) is given as a fraction of the 8.0 TB/s peak of the MI355X: a chain-level figure (it includes the
projection launch); the kernel's own time is what `rocprofv3 --kernel-trace --stats` reports for gp_posterior_cov_kernel in a run of its own.

    python tools/gp_posterior_bench.py [--rounds 20] [--warmup 3] [--shapes 79x100,96x1024,96x4096]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gabotorch_amd import _lib, ops                                                                      # noqa: E402

DEV = "cuda:0"
HBM_PEAK = 8.0e12
SAMPLES = 10


def problem(n, m, seed=0):
    """kernel matrices of points on a curve (a smooth, badly conditioned posterior like the letters problem) and the prediction cache"""
    rng = np.random.default_rng(seed)
    xs = np.sort(rng.uniform(0.0, 4.0, m))
    xt = np.sort(rng.uniform(0.0, 4.0, n))
    k = lambda a, b: np.exp(-1.3 * (a[:, None] - b[None, :]) ** 2)                   # noqa: E731
    os_, noise = 2000.0, 2.0
    linv = np.linalg.inv(np.linalg.cholesky(os_ * k(xt, xt) + noise * np.eye(n)))
    alpha = linv.T @ (linv @ np.sin(xt))
    t = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device=DEV)    # noqa: E731
    return t(k(xs, xt)), t(k(xs, xs)), t(np.tril(linv)), t(alpha), 0.0, os_


def ladder_samples(mean, cov, z):
    eye = torch.eye(cov.shape[0], dtype=cov.dtype, device=cov.device)
    for jitter in _lib.GABO_MVN_JITTER_LADDER:
        L, info = torch.linalg.cholesky_ex(cov if jitter == 0.0 else cov + jitter * eye)
        if int(info.item()) == 0:
            return mean + z @ L.T
    raise RuntimeError("not positive definite")


def chain_new(kstar, kss, linv, alpha, mean, os_, sample):
    mu, var, cov = ops.gp_posterior_joint(kstar, kss, linv, alpha, mean, os_)
    return (cov, ops.mvn_sample(mu, cov, (SAMPLES,), seed=1)) if sample else (cov, None)


def chain_torch(kstar, kss, linv, alpha, mean, os_, sample, z, fused_update):
    ks = os_ * kstar
    v = ks @ linv.T
    mu = mean + ks @ alpha
    cov = torch.addmm(kss, v, v.T, beta=os_, alpha=-1.0) if fused_update else os_ * kss - v @ v.T
    return (cov, ladder_samples(mu, cov, z)) if sample else (cov, None)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e-3, out


def summary(times):
    return {"median_s": float(np.median(times)), "min_s": float(np.min(times)), "max_s": float(np.max(times)), "rounds": len(times)}


def fmt(s):
    return f"{s['median_s'] * 1e6:10.1f} us  [{s['min_s'] * 1e6:.1f}, {s['max_s'] * 1e6:.1f}]"


def bench(n, m, rounds, warmup):
    kstar, kss, linv, alpha, mean, os_ = problem(n, m)
    sample = m <= _lib.GABO_MVN_SAMPLE_MAX_M
    z = ops.mvn_base_samples(SAMPLES, m, 1, device=DEV)
    forms = {
        "new_chain": lambda k: chain_new(kstar, k, linv, alpha, mean, os_, sample),
        "torch_composed": lambda k: chain_torch(kstar, k, linv, alpha, mean, os_, sample, z, False),
        "torch_addmm": lambda k: chain_torch(kstar, k, linv, alpha, mean, os_, sample, z, True),
    }
    times = {k: [] for k in forms}
    last = {}
    for r in range(warmup + rounds):
        for name, fn in forms.items():
            work = kss.clone()                                       # (a) consumes its k**: every form gets a fresh copy, outside the window
            torch.cuda.synchronize()
            dt, out = timed(lambda: fn(work))
            if r >= warmup:
                times[name].append(dt)
            last[name] = out[0]
            del out, work
    tiles = (m + 63) // 64
    traffic = (tiles * (tiles + 1) // 2 * 64 * 64 + m * m) * 8       # lower tiles read (padded to whole tiles: an upper bound of <= 2 %), all written
    res = {"n": n, "m": m, "with_samples": sample, **{k: summary(v) for k, v in times.items()},
           "max_abs_difference_to_torch_composed": float((last["new_chain"] - last["torch_composed"]).abs().max()),
           "covariance_scale": float(last["torch_composed"].abs().max()), "compulsory_bytes": traffic}
    res["new_chain_fraction_of_hbm_peak"] = traffic / res["new_chain"]["median_s"] / HBM_PEAK
    print(f"n = {n}, m = {m}{', then 10 samples' if sample else ''}:")
    print(f"  (a)  gp_posterior_joint{' + mvn_sample' if sample else ''}     {fmt(res['new_chain'])}")
    print(f"  (b)  torch: product, subtraction{', ladder' if sample else ''}   {fmt(res['torch_composed'])}")
    print(f"  (b') torch: addmm{', ladder' if sample else ''}                  {fmt(res['torch_addmm'])}")
    print(f"  compulsory traffic {traffic / 1e6:.1f} MB over (a): {res['new_chain_fraction_of_hbm_peak'] * 100:.1f} % of {HBM_PEAK / 1e12:.1f} TB/s; "
          f"max |Sigma(a) - Sigma(b)| {res['max_abs_difference_to_torch_composed']:.2e} at scale {res['covariance_scale']:.1f}")
    print("RESULT " + json.dumps(res), flush=True)
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shapes", default="79x100,96x1024,96x4096", help="comma-separated n x m")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gp_posterior_bench.py needs an MI355X: there is nothing to time without one")
    for shape in a.shapes.split(","):
        n_, m_ = (int(v) for v in shape.split("x"))
        bench(n_, m_, a.rounds, a.warmup)
