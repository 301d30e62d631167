"""Plain numpy fp64 reference of the Matern kernels on the flat SPD metrics (csrc/flat_matern.hip, csrc/gp_mll_matern.hip), written from the
formulas and not from the device code:

    r_ij = sqrt(sum_e (x1_ie - x2_je + eps_e)^2),  eps_e = 1e-15 on the d diagonal Mandel entries, sqrt(2) 1e-15 on the others
    a = sqrt(2 nu) / l,  x = a r
    k      = m(x) exp(-x)            m = 1 | 1 + x | 1 + x + x^2 / 3        (nu = 1/2 | 3/2 | 5/2)
    dk/dl  = x^2 q(x) exp(-x) / l    q = 1/x | 1 | (1 + x) / 3
    2 dk/d(r^2) = -a^2 q(x) exp(-x)  (the weight of the x-gradient)

and the exact-GP marginal log likelihood of Ky = outputscale * k(R) + noise * I with its four derivatives, each next to the sum of the
absolute values of its terms and cond_2(Ky) (as tests/_cpu_gp_mll_series.py).  U = 2^-53 is the unit roundoff the tolerances are stated in."""
import math

import numpy as np

U = 2.0 ** -53
NUS = (0.5, 1.5, 2.5)


def mandel_dim(dv):
    d = int(round((math.sqrt(8 * dv + 1) - 1) / 2))
    assert d * (d + 1) // 2 == dv
    return d


def eps_vector(dv, sign=1.0):
    d = mandel_dim(dv)
    return sign * np.where(np.arange(dv) < d, 1e-15, math.sqrt(2.0) * 1e-15)


def to_mandel(mats):
    """(..., d, d) symmetric -> (..., d(d+1)/2): the diagonal, then the k-th sub-diagonals times sqrt(2) (the library's layout)"""
    mats = np.asarray(mats, dtype=np.float64)
    d = mats.shape[-1]
    parts = [np.diagonal(mats, axis1=-2, axis2=-1)]
    for k in range(1, d):
        parts.append(math.sqrt(2.0) * np.diagonal(mats, offset=-k, axis1=-2, axis2=-1))
    return np.concatenate(parts, axis=-1)


def logm_mandel(mats):
    lam, v = np.linalg.eigh(np.asarray(mats, dtype=np.float64))
    return to_mandel(np.einsum("...ab,...b,...cb->...ac", v, np.log(lam), v))


def random_spd(rng, n, d, lo=0.3, hi=3.0):
    q = np.linalg.qr(rng.standard_normal((n, d, d)))[0]
    x = np.einsum("nab,nb,ncb->nac", q, rng.uniform(lo, hi, (n, d)), q)
    return 0.5 * (x + x.transpose(0, 2, 1))


def differences(x1, x2, sign=1.0):
    """(..., n1, n2, dv): x1_i - x2_j + sign * eps"""
    x1, x2 = np.asarray(x1, dtype=np.float64), np.asarray(x2, dtype=np.float64)
    return (x1[..., :, None, :] - x2[..., None, :, :]) + eps_vector(x1.shape[-1], sign)


def distance(x1, x2):
    diff = differences(x1, x2)
    return np.sqrt((diff * diff).sum(-1))


def _poly(x, nu):
    if nu == 0.5:
        return np.ones_like(x)
    if nu == 1.5:
        return 1.0 + x
    if nu == 2.5:
        return 1.0 + x + x * x / 3.0
    raise ValueError(nu)


def _q(x, nu):
    if nu == 0.5:
        return 1.0 / x
    if nu == 1.5:
        return np.ones_like(x)
    if nu == 2.5:
        return (1.0 + x) / 3.0
    raise ValueError(nu)


def value(r, lengthscale, nu):
    x = math.sqrt(2.0 * nu) / lengthscale * np.asarray(r, dtype=np.float64)
    return _poly(x, nu) * np.exp(-x)


def dlengthscale(r, lengthscale, nu):
    x = math.sqrt(2.0 * nu) / lengthscale * np.asarray(r, dtype=np.float64)
    return x * x * _q(x, nu) * np.exp(-x) / lengthscale


def weight(r, lengthscale, nu):
    a = math.sqrt(2.0 * nu) / lengthscale
    x = a * np.asarray(r, dtype=np.float64)
    return -a * a * _q(x, nu) * np.exp(-x)


def gram(x1, x2, lengthscale, nu):
    return value(distance(x1, x2), lengthscale, nu)


def backward(x1, x2, grad_out, lengthscale, nu, wrt=1):
    """gradient of sum(grad_out * gram(x1, x2)) in x1 (wrt = 1) or x2 (wrt = 2), and the sum of the absolute values of its terms"""
    diff = differences(x1, x2)
    terms = (np.asarray(grad_out, dtype=np.float64) * weight(np.sqrt((diff * diff).sum(-1)), lengthscale, nu))[..., None] * diff
    axis, sign = (-2, 1.0) if wrt == 1 else (-3, -1.0)
    return sign * terms.sum(axis), np.abs(terms).sum(axis)


def likelihood(r, y, lengthscale, nu, outputscale, noise, mean):
    """-> (out, scale, cond): out = [ll, dll/dlengthscale, dll/doutputscale, dll/dnoise, dll/dmean], scale = the sums of absolute terms of the
    five, cond = cond_2(Ky).  r: the n x n distance matrix (its lower triangle is what the launch reads)."""
    r, y = np.asarray(r, dtype=np.float64), np.asarray(y, dtype=np.float64)
    n = len(y)
    r = np.tril(r) + np.tril(r, -1).T
    k, dk = value(r, lengthscale, nu), dlengthscale(r, lengthscale, nu)
    ky = outputscale * k + noise * np.eye(n)
    res = y - mean
    kinv = np.linalg.inv(ky)
    alpha = np.linalg.solve(ky, res)
    w = np.outer(alpha, alpha) - kinv
    logpiv = 2.0 * np.log(np.diagonal(np.linalg.cholesky(ky)))
    out = np.array([-0.5 * res @ alpha - 0.5 * logpiv.sum() - 0.5 * n * math.log(2.0 * math.pi),
                    0.5 * outputscale * (w * dk).sum(),
                    0.5 * (w * k).sum(),
                    0.5 * np.trace(w),
                    alpha.sum()])
    scale = np.array([0.5 * abs(res @ alpha) + 0.5 * np.abs(logpiv).sum() + 0.5 * n * math.log(2.0 * math.pi),
                      0.5 * outputscale * np.abs(w * dk).sum(),
                      0.5 * np.abs(w * k).sum(),
                      0.5 * np.abs(np.diagonal(w)).sum(),
                      np.abs(alpha).sum()])
    return out, scale, float(np.linalg.cond(ky))
