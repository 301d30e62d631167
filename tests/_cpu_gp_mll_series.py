"""Plain numpy fp64 reference of gabo_gp_mll_series: the exact-GP marginal log likelihood of Ky = outputscale * K + noise * I with
K = sum_k p_k(kappa) P_k(C) the Riemannian Matern series on the inner products C, and its derivatives in kappa, outputscale, noise and mean.
K and dK / dkappa come from tests/_cpu_sphere_zonal.zonal_series with the host's coefficients; the algebra is numpy's.

Every output is a sum; next to it the reference returns the sum of the ABSOLUTE values of its terms - the scale rounding errors are relative
to when the terms cancel (the lengthscale gradient does, by orders of magnitude, for short series) - and cond_2(Ky), which amplifies them."""
import math

import numpy as np

from tests._cpu_sphere_zonal import zonal_series


def series_matrices(c, dim, kappa, nu, num_levels):
    """(K, dK / dkappa) on the inner products c"""
    from gabotorch_amd import ops
    p, sd = ops.sphere_matern_coefficients(dim, kappa, nu, num_levels)
    dp, _ = ops.sphere_matern_coefficients(dim, kappa, nu, num_levels, wrt_lengthscale=True)
    return zonal_series(c, p, sd), zonal_series(c, dp, sd)


def reference(c, y, dim, kappa, nu, num_levels, outputscale, noise, mean):
    """-> (out, scale, cond): out = [ll, dll/dkappa, dll/doutputscale, dll/dnoise, dll/dmean], scale = the sums of absolute terms of the five,
    cond = cond_2(Ky).  The pivots of the sweep operator are the squared diagonal of the Cholesky factor."""
    c, y = np.asarray(c, dtype=np.float64), np.asarray(y, dtype=np.float64)
    n = len(y)
    k, dk = series_matrices(c, dim, kappa, nu, num_levels)
    k, dk = np.tril(k) + np.tril(k, -1).T, np.tril(dk) + np.tril(dk, -1).T          # (the launch reads the lower triangle)
    ky = outputscale * k + noise * np.eye(n)
    r = y - mean
    kinv = np.linalg.inv(ky)
    alpha = np.linalg.solve(ky, r)
    w = np.outer(alpha, alpha) - kinv
    logpiv = 2.0 * np.log(np.diagonal(np.linalg.cholesky(ky)))
    out = np.array([-0.5 * r @ alpha - 0.5 * logpiv.sum() - 0.5 * n * math.log(2.0 * math.pi),
                    0.5 * outputscale * (w * dk).sum(),
                    0.5 * (w * k).sum(),
                    0.5 * np.trace(w),
                    alpha.sum()])
    scale = np.array([0.5 * abs(r @ alpha) + 0.5 * np.abs(logpiv).sum() + 0.5 * n * math.log(2.0 * math.pi),
                      0.5 * outputscale * np.abs(w * dk).sum(),
                      0.5 * np.abs(w * k).sum(),
                      0.5 * np.abs(np.diagonal(w)).sum(),
                      np.abs(alpha).sum()])
    return out, scale, float(np.linalg.cond(ky))


def sphere_points(rng, n, dim):
    x = rng.standard_normal((n, dim))
    return x / np.linalg.norm(x, axis=1, keepdims=True)
