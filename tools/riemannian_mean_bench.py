#!/usr/bin/env python3
"""Times the Frechet / Karcher means, 10 iterations, device events around the whole enqueued chain (needs the GPU; there is no CPU path).

    python tools/riemannian_mean_bench.py [--reps 15] [--json out.json]

Three ways to the same mean:
  fused      ops.spd_frechet_mean / ops.sphere_karcher_mean: the kernels of csrc/riemannian_mean.hip
  composed   ops.spd_frechet_mean(fused=False): torch whitening + one batched logm launch + weighted sum + one expm launch per iteration
  user       the loop a user writes from this package's Riemannian_utils logmap / expmap (numpy in, numpy out: a broadcast base point and
             two device round trips per iteration) - what the package offered before the mean existed.  Host clock: it ends on the host.
Each shape is warmed up, then the three are timed alternately `reps` times; the table gives medians (and minima).  The reference itself
takes 1.46 s on a build machine's CPU at N = 1024, d = 10 (20 k calls of the non-symmetric numpy eig); it is not run here."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from gabotorch_amd import ops  # noqa: E402
from gabotorch_amd.Riemannian_utils import spd_utils, sphere_utils  # noqa: E402

DEV = "cuda:0"
ITERS = 10


def rand_spd_mandel(rng, b, n, d, c=10.0):
    q = np.linalg.qr(rng.standard_normal((b * n, d, d)))[0]
    lam = 0.1 * np.exp(rng.uniform(0.0, np.log(c), (b * n, d)))
    m = np.einsum("nab,nb,ncb->nac", q, lam, q)
    return spd_utils.symmetric_matrix_to_vector_mandel(0.5 * (m + m.transpose(0, 2, 1))).reshape(b, n, -1)


def rand_sphere(rng, n, dim):
    c = rng.standard_normal(dim)
    c /= np.linalg.norm(c)
    x = c[None] + 0.4 * rng.standard_normal((n, dim))
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def host_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def user_spd_mean(X):
    """the reference's loop (spd_utils.py:248-259) on this package's batched logmap / expmap"""
    m = X[0]
    for _ in range(ITERS):
        t = spd_utils.logmap(X, np.broadcast_to(m, X.shape)).mean(axis=0)
        m = spd_utils.expmap(t, m)
    return m


def user_sphere_mean(xT):
    m = xT[:, 0]
    for _ in range(ITERS):
        t = sphere_utils.logmap(xT, np.broadcast_to(m[:, None], xT.shape)).mean(axis=1)
        m = sphere_utils.expmap(t, m)[:, 0]
    return m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--user-reps", type=int, default=3)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("riemannian_mean_bench needs an MI355X")
    ops.set_error_checking(False)            # (no status read-back inside the timed window)
    rng = np.random.default_rng(0)
    rows = []
    shapes = [("spd", d, n, 1) for d in (5, 10) for n in (64, 1024, 4096)] + [("spd", 5, 64, 256), ("spd", 10, 64, 256), ("sphere", 10, 4096, 1)]
    for kind, d, n, b in shapes:
        if kind == "spd":
            xh = rand_spd_mandel(rng, b, n, d)
            x = torch.tensor(xh, device=DEV)
            paths = {"fused": lambda x=x: ops.spd_frechet_mean(x, iters=ITERS, fused=True),
                     "composed": lambda x=x: ops.spd_frechet_mean(x, iters=ITERS, fused=False)}
            Xm = spd_utils.vector_to_symmetric_matrix_mandel(xh[0])
            user = (lambda Xm=Xm: user_spd_mean(Xm)) if b == 1 else None
        else:
            xh = rand_sphere(rng, n, d)
            x = torch.tensor(xh, device=DEV)
            paths = {"fused": lambda x=x: ops.sphere_karcher_mean(x, iters=ITERS)}
            xT = np.ascontiguousarray(xh.T)
            user = lambda xT=xT: user_sphere_mean(xT)   # noqa: E731
        outs = {k: f() for k, f in paths.items()}           # warm-up (code objects, allocator) and agreement
        for f in paths.values():
            f()
        torch.cuda.synchronize()
        agree = None
        if "composed" in outs:
            agree = float((outs["fused"] - outs["composed"]).norm() / outs["composed"].norm())
        times = {k: [] for k in paths}
        for _ in range(args.reps):
            for k, f in paths.items():
                times[k].append(event_ms(f))
        row = {"kind": kind, "d": d, "n": n, "batch": b, "iters": ITERS, "fused_vs_composed": agree}
        for k, v in times.items():
            row[k + "_ms_median"], row[k + "_ms_min"] = float(np.median(v)), float(np.min(v))
        if user is not None:
            user()
            tu = [host_ms(user) for _ in range(args.user_reps)]
            row["user_ms_median"], row["user_ms_min"] = float(np.median(tu)), float(np.min(tu))
        rows.append(row)
        print(json.dumps(row), flush=True)
    print("\n| manifold | d / dim | N | sets | fused ms | composed ms | logmap/expmap loop ms |")
    print("|---|---|---|---|---|---|---|")
    for r in rows:
        f = lambda k: "-" if k not in r else f"{r[k]:.3f}"   # noqa: E731
        print(f"| {r['kind']} | {r['d']} | {r['n']} | {r['batch']} | {f('fused_ms_median')} | {f('composed_ms_median')} | {f('user_ms_median')} |")
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
