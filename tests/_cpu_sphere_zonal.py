"""Plain numpy fp64 restatement of the zonal series of csrc/sphere_zonal.hip: the same recurrence P_k = t + B_k (t - P_{k-2}), t = c P_{k-1},
the same factors B_k (one IEEE division each), the same ascending order of summation, with separate multiplications and additions where the
device uses fma.  Its own
error against the 50-digit golden values is what the GPU tests derive their tolerances from."""
import numpy as np


def recurrence_factors(n_coeff, series_dim):
    """B_k = (k - 1) / (k + d - 2), k = 0 ... n_coeff - 1 (entries 0, 1 unused)"""
    k = np.arange(n_coeff, dtype=np.float64)
    den = k + float(series_dim) - 2.0
    den[:2] = 1.0
    return (k - 1.0) / den


def zonal_series(c, coeff, series_dim):
    """sum_k coeff[k] P_k^(series_dim)(c), element-wise"""
    c = np.asarray(c, dtype=np.float64)
    coeff = np.asarray(coeff, dtype=np.float64)
    rb = recurrence_factors(len(coeff), series_dim)
    p0, p1 = np.ones_like(c), c.copy()
    f = coeff[0] + (coeff[1] if len(coeff) > 1 else 0.0) * c
    for k in range(2, len(coeff)):
        t = c * p1
        p = rb[k] * (t - p0) + t
        f = f + coeff[k] * p
        p0, p1 = p1, p
    return f


def matern_gram(x1, x2, lengthscale, nu, num_levels, order=0, wrt_lengthscale=False):
    """the kernel matrix (or the derivative `order` in c / in the lengthscale of its entries) from the host's coefficients"""
    from gabotorch_amd import ops
    coeff, sd = ops.sphere_matern_coefficients(x1.shape[-1], lengthscale, nu, num_levels, order, wrt_lengthscale)
    return zonal_series(x1 @ np.swapaxes(x2, -1, -2), coeff, sd)
