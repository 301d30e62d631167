"""Plain numpy fp64 statement of the surrogate-fit objective of ScaleKernel(NestedSphereRiemannianMaternKernel), from three pieces that are
each tested on their own: the level-by-level projection of oracle/sphere.py, the zonal series of tests/_cpu_sphere_zonal.py on the projected
points, and slogdet / solve for the likelihood.  The GPU tests compare the one-call fit evaluation with it and with its central differences."""
import math

import numpy as np

from oracle import sphere as osph
from tests._cpu_sphere_zonal import matern_gram


def split_axes(packed, dim, levels):
    """the packed axes (level k has dimension dim - k) as a list"""
    out, off = [], 0
    for k in range(levels):
        out.append(np.asarray(packed[off:off + dim - k], dtype=np.float64))
        off += dim - k
    return out


def project(x, axes, dists):
    return osph.projection_from_sphere_to_subsphere(x, axes, dists)[-1]


def gram(x1, x2, axes, dists, lengthscale, nu, num_levels):
    return matern_gram(project(x1, axes, dists), project(x2, axes, dists), lengthscale, nu, num_levels)


def log_likelihood(x, y, axes, dists, lengthscale, outputscale, noise, mean, nu, num_levels):
    """log N(y | mean, outputscale K + noise I), K the nested Matern Gram matrix of x (no priors, not divided by n)"""
    n = x.shape[0]
    ky = outputscale * gram(x, x, axes, dists, lengthscale, nu, num_levels) + noise * np.eye(n)
    r = np.asarray(y, dtype=np.float64) - mean
    sign, logdet = np.linalg.slogdet(ky)
    if sign <= 0:
        return float("nan")
    return float(-0.5 * (r @ np.linalg.solve(ky, r)) - 0.5 * logdet - 0.5 * n * math.log(2.0 * math.pi))
