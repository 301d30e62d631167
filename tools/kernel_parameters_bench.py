#!/usr/bin/env python3
"""Times the kernel-parameter study (kernel_utils.kernel_parameters.min_eigenvalues: one distance launch, one gabo_gram_extreme_eig launch and
one copy per call) at the shapes of the reference's two scripts against the loop a user writes without it:

  (a) per set and per beta: kernel.forward, copy to the host, np.linalg.eig             (the reference's loop on this library's kernels)
  (b) the same loop with torch.linalg.eigvalsh on the device instead of the copy and np.linalg.eig, if this torch build provides it

All three run in one process, in turn within every round, after warm-up rounds; the time of a round is host time between two device
synchronisations.  Reported: median [min, max] over the rounds.  (a) costs minutes per round at the full shapes, so it has its own, smaller
round count and may be restricted to the first sets (--host-sets; its time is then that of those sets alone).  The minimum eigenvalues of the three are compared at the end.

    python tools/kernel_parameters_bench.py [--study spd|sphere|both] [--rounds 5] [--warmup 2] [--host-rounds 1] [--host-sets N] [--samples 500]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))
from gabotorch_amd.kernel_utils import kernel_parameters                                                # noqa: E402
from gabotorch_amd.kernel_utils.kernels_sphere import SphereGaussianKernel                              # noqa: E402
from gabotorch_amd.kernel_utils.kernels_spd import SpdAffineInvariantGaussianKernel                     # noqa: E402
import sphere_gaussian_kernel_parameters as sphere_study                                                # noqa: E402
import spd_gaussian_kernel_parameters as spd_study                                                      # noqa: E402

DEV = "cuda:0"


def one_call(kind, sets, betas):
    return np.atleast_2d(kernel_parameters.min_eigenvalues(kind, sets, betas))


def loop_host_eig(kind, sets, betas):
    """baseline (a)"""
    out = np.empty((len(sets), len(betas)))
    for t, x in enumerate(sets):
        for p, b in enumerate(betas):
            k = kind(beta_min=0.0)
            k.beta = float(b)
            gram = k.forward(x, x).detach().cpu().numpy()
            out[t, p] = np.min(np.real(np.linalg.eig(gram)[0]))
    return out


def loop_device_eigvalsh(kind, sets, betas):
    """baseline (b): the minimum eigenvalues stay on the device until the end (one copy)"""
    rows = []
    for x in sets:
        for b in betas:
            k = kind(beta_min=0.0)
            k.beta = float(b)
            rows.append(torch.linalg.eigvalsh(k.forward(x, x).detach())[0])
    return torch.stack(rows).reshape(len(sets), len(betas)).cpu().numpy()


def timed(fn, *args):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn(*args)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def summary(times):
    return None if not times else {"median_s": float(np.median(times)), "min_s": float(np.min(times)), "max_s": float(np.max(times)), "rounds": len(times)}


def fmt(s):
    return "not run" if s is None else f"{s['median_s'] * 1e3:12.2f} ms  [{s['min_s'] * 1e3:.2f}, {s['max_s'] * 1e3:.2f}]  ({s['rounds']} rounds)"


def bench(name, kind, sets, betas, rounds, warmup, host_rounds, host_sets):
    sets = [torch.as_tensor(s, dtype=torch.float64, device=DEV) for s in sets]
    have_b = True
    try:
        torch.linalg.eigvalsh(torch.eye(8, dtype=torch.float64, device=DEV))
    except Exception as exc:                          # this torch build has no symmetric eigensolver for HIP tensors
        have_b = False
        print(f"{name}: torch.linalg.eigvalsh is not available on the device ({type(exc).__name__}: {exc}); baseline (b) not run")
    for _ in range(warmup):
        one_call(kind, sets, betas)
        if have_b:
            loop_device_eigvalsh(kind, sets[:1], betas)
    if host_rounds:
        loop_host_eig(kind, sets[:1], betas[:2])
    times = {"one_call": [], "loop_device_eigvalsh": [], "loop_host_eig": []}
    last = {}
    for r in range(rounds):
        dt, last["one_call"] = timed(one_call, kind, sets, betas)
        times["one_call"].append(dt)
        if have_b:
            dt, last["loop_device_eigvalsh"] = timed(loop_device_eigvalsh, kind, sets, betas)
            times["loop_device_eigvalsh"].append(dt)
        if r < host_rounds:
            dt, last["loop_host_eig"] = timed(loop_host_eig, kind, sets[:host_sets], betas)
            times["loop_host_eig"].append(dt)
    res = {"study": name, "sets": len(sets), "sets_of_loop_host_eig": len(sets[:host_sets]), "points": [int(len(s)) for s in sets], "params": len(betas),
           **{k: summary(v) for k, v in times.items()}}
    for k in ("loop_device_eigvalsh", "loop_host_eig"):
        if k in last:
            res[f"max_abs_difference_of_lambda_min_to_{k}"] = float(np.max(np.abs(last[k] - last["one_call"][:len(last[k])])))
    print(f"{name}: {len(sets)} sets of {min(res['points'])} ... {max(res['points'])} points, {len(betas)} parameters")
    print(f"  one call (min_eigenvalues)                  {fmt(res['one_call'])}")
    print(f"  (b) loop: forward + torch.linalg.eigvalsh   {fmt(res['loop_device_eigvalsh'])}")
    print(f"  (a) loop: forward + copy + np.linalg.eig    {fmt(res['loop_host_eig'])}  on {len(sets[:host_sets])} of the {len(sets)} sets")
    print("RESULT " + json.dumps(res), flush=True)
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--study", choices=("spd", "sphere", "both"), default="both")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host-rounds", type=int, default=1)
    ap.add_argument("--host-sets", type=int, default=None, help="baseline (a) on the first N sets only (default: all)")
    ap.add_argument("--samples", type=int, default=500)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("kernel_parameters_bench.py needs an MI355X: there is nothing to time without one")
    np.random.seed(1234)
    if a.study in ("spd", "both"):            # spd_gaussian_kernel_parameters.py: d = 3, 500 samples, 10 trials, 30 beta
        bench("spd", SpdAffineInvariantGaussianKernel, spd_study.sample_sets(3, a.samples, 10), spd_study.betas_for(3), a.rounds, a.warmup,
              a.host_rounds, a.host_sets)
    if a.study in ("sphere", "both"):         # sphere_gaussian_kernel_parameters.py: dim 3, 500 samples, 20 trials, 30 beta
        bench("sphere", SphereGaussianKernel, list(sphere_study.sample_sets(3, a.samples, 20)), sphere_study.betas_for(3), a.rounds, a.warmup,
              a.host_rounds, a.host_sets)
