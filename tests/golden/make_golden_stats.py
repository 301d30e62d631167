#!/usr/bin/env python3
"""Golden Frechet means and parallel-transport operators from the reference's numpy functions (development container only; it imports the reference).

    python -W ignore tests/golden/make_golden_stats.py

Reference functions called, unmodified:  BoManifolds/Riemannian_utils/spd_utils.py  mean (:235-259), mean_mandel_vector (:262-287),
parallel_transport_operator (:200-213), parallel_transport_operator_mandel_vector (:216-232);  sphere_utils.py  karcher_mean_sphere (:126-149),
parallel_transport_operator (:93-123).  Real parts are taken where numpy / scipy hand back a complex dtype.

Inputs (tests/_cpu_riemannian_stats.py: stats_spd_pool, stats_sphere_pool - seeded, one stream per dimension, NOT stored).  SPD: Q diag(lam) Q^T with Q
from qr(randn) and lam = 0.1 exp(U[0, ln c]), c = 10 or 1e3 per dimension.  Sphere: a random unit centre plus 0.4 randn, normalised.  One pool of 129
points per dimension; the case with N points is the pool's first N, N = 1, 2, 63, 64, 65, 129 at every dimension.  Stored: the reference's outputs and,
as a check of the random stream, each pool's first point.  Output: tests/golden/riemannian_stats.npz (arrays only)."""
import os
import sys

import numpy as np

REF = os.environ.get("GABO_REFERENCE", "/root/reference")
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REF)
sys.path.insert(0, os.path.dirname(HERE))

from BoManifolds.Riemannian_utils import spd_utils as ref_spd  # noqa: E402
from BoManifolds.Riemannian_utils import sphere_utils as ref_sph  # noqa: E402
import _cpu_riemannian_stats as cpu  # noqa: E402


def real(a):
    a = np.asarray(a)
    return np.ascontiguousarray(a.real if np.iscomplexobj(a) else a, dtype=np.float64)


def main():
    out = {}
    worst = worst_pt = 0.0
    for d in sorted(cpu.STATS_SPD_C):
        pool = cpu.stats_spd_pool(d)
        X = cpu.from_mandel(pool)
        out[f"spd{d}_first"] = pool[0]
        for n in cpu.STATS_NS:
            m = real(ref_spd.mean(X[:n].copy(), nb_iter=10))
            out[f"spd{d}_mean_n{n}"] = m
            worst = max(worst, np.linalg.norm(cpu.spd_mean(X[:n]) - m) / np.linalg.norm(m))
        if d in cpu.STATS_SPD_TRANSPORT_DIMS:
            out[f"spd{d}_pt"] = real(ref_spd.parallel_transport_operator(X[0], X[1]))
            out[f"spd{d}_pt_mandel"] = real(ref_spd.parallel_transport_operator_mandel_vector(pool[0], pool[1]))
            worst_pt = max(worst_pt, np.abs(cpu.spd_transport(X[0], X[1]) - out[f"spd{d}_pt"]).max())
    # the Mandel-vector form of the mean, points in columns (one case: it is the same loop on vectors)
    out["spd3_mean_mandel_n5"] = real(ref_spd.mean_mandel_vector(np.ascontiguousarray(cpu.stats_spd_pool(3)[:5].T), nb_iter=10))
    print(f"SPD: restatement vs reference, mean worst relative Frobenius {worst:.2e}, transport worst entry {worst_pt:.2e}")
    worst = worst_pt = 0.0
    for dim in cpu.STATS_SPHERE_DIMS:
        x = cpu.stats_sphere_pool(dim)
        out[f"sph{dim}_first"] = x[0]
        for n in cpu.STATS_NS:
            m = real(ref_sph.karcher_mean_sphere(np.ascontiguousarray(x[:n].T), nb_iter=10))
            assert m.shape == (dim, 1)
            out[f"sph{dim}_mean_n{n}"] = m
            worst = max(worst, np.abs(cpu.sphere_mean(x[:n]) - m[:, 0]).max())
        if dim in cpu.STATS_SPHERE_TRANSPORT_DIMS:
            out[f"sph{dim}_pt"] = real(ref_sph.parallel_transport_operator(x[0].copy(), x[1].copy()))
            worst_pt = max(worst_pt, np.abs(cpu.sphere_transport(x[0], x[1]) - out[f"sph{dim}_pt"]).max())
    print(f"sphere: restatement vs reference, mean worst component {worst:.2e}, transport worst entry {worst_pt:.2e}")
    path = os.path.join(HERE, "riemannian_stats.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
