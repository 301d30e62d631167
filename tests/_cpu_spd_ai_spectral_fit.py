"""Plain numpy statement of the one-call surrogate fit of the affine-invariant SPD Matern / heat kernels (csrc/spd_ai_spectral_fit.hip,
ops.gp_mll_spd_ai_spectral), written from the formulas and on top of tests/_cpu_spd_ai_spectral.py.  With rho_k = (d + 1 - 2k) / 4:

    lam_l   = e_l g(kappa),   c = g' / g = -1 / kappa (heat),  -nu / (kappa (nu + b kappa^2)), b = d (d^2 - 1) / 96 (Matern):  d lam / d kappa = c lam
    q_l     = (d log w_l / d kappa) / 2 = c sum_{i<j} pi |D_ij| / sinh(2 pi |D_ij|),  D_ij = lam_li - lam_lj      (each term -> 1/2 at D = 0)
    u_il    = sqrt(w_l) exp(-rho . a_il),  theta_il = lam_l . a_il,  f_i = [u cos theta | u sin theta],  s_i = sum_l u_il^2,  Fh_i = f_i / sqrt(s_i)
    df_cos  = u (q cos theta - c theta sin theta),  df_sin = u (q sin theta + c theta cos theta)
    Gd_i    = d Fh_i / d kappa = df_i / sqrt(s_i) - Fh_i (sum_l u_il^2 q_l) / s_i
    K_ij    = Fh_i . Fh_j (K_ii = 1),   dK_ij = Gd_i . Fh_j + Fh_i . Gd_j (dK_ii = 0)
    d ll / d kappa = outputscale sum_ij W_ij dK_ij / 2,   W = alpha alpha^T - Ky^-1,   Ky = outputscale K + noise I

Every function takes the element type (np.float64 or np.longdouble) from its `dtype` argument: the long-double evaluation is the yardstick of
the fp64 one."""
import collections
import math

import numpy as np

from tests import _cpu_gp_dense as dense
from tests import _cpu_spd_ai_spectral as ref

U = ref.U
LD = np.longdouble


def _pi(dtype):
    return 4 * np.arctan(dtype(1))


def log_derivative_factor(d, kappa, nu, dtype=np.float64):
    """c with d lam / d kappa = c lam"""
    kappa = dtype(kappa)
    if math.isinf(nu):
        return -1 / kappa
    b = dtype(d * (d * d - 1)) / 96
    return -dtype(nu) / (kappa * (dtype(nu) + b * kappa * kappa))


def points_and_derivative(base, kappa, nu, dtype=np.float64):
    """-> (lam (L, d), w (L,), q (L,), c, q_scale (L,)): lam and w by the formulas of ref.spectral_points in `dtype`; q_scale = the sum of the
    absolute values of q's terms"""
    e, gamma, _ = base
    d = e.shape[1]
    e = np.asarray(e, dtype=np.float64).astype(dtype)
    kappa_t = dtype(kappa)
    if math.isinf(nu):
        lam = e / kappa_t
    else:
        g = np.asarray(gamma, dtype=np.float64).astype(dtype)
        lam = e * np.sqrt((dtype(nu) / (kappa_t * kappa_t) + dtype(0.5) * dtype(ref.rho_norm2(d))) / g)[:, None]
    c = log_derivative_factor(d, kappa, nu, dtype)
    pi = _pi(dtype)
    w = np.ones(len(e), dtype=dtype)
    s = np.zeros(len(e), dtype=dtype)
    for i in range(d):
        for j in range(i + 1, d):
            x = pi * np.abs(lam[:, i] - lam[:, j])
            w = w * np.tanh(x)
            with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
                term = np.where(x > 0, x / np.sinh(2 * x), dtype(0.5))
            s = s + term
    return lam, w, c * s, c, np.abs(c) * s


def features_and_derivative(a, lam, w, q, c, dtype=np.float64):
    """a (n, L, d) -> (Fh (n, 2 L), Gd (n, 2 L))"""
    d = a.shape[-1]
    a, lam, w, q = (np.asarray(v).astype(dtype) for v in (a, lam, w, q))
    c = dtype(c)
    u = np.sqrt(w) * np.exp(-(a * ref.rho(d).astype(dtype)).sum(-1))
    theta = (a * lam).sum(-1)
    cs, sn = np.cos(theta), np.sin(theta)
    s = (u * u).sum(-1, keepdims=True)
    root = np.sqrt(s)
    fh = np.concatenate([u * cs, u * sn], axis=-1) / root
    df = np.concatenate([u * (q * cs - c * theta * sn), u * (q * sn + c * theta * cs)], axis=-1)
    return fh, df / root - fh * ((u * u * q).sum(-1, keepdims=True) / s)


def gdot_tolerance(a, lam, w, q, c):
    """The bound on the error of an fp64 evaluation of Gd (n, 2 L), from the rounding of the phase and the log-amplitude, two chains of d
    multiply-adds: eps_i = max_l (d + 1) u sum_k (|lam_lk a_ilk| + |rho_k a_ilk|) + 16 u (the 16 u: sqrt, exp, sincos and the products) is the
    relative error of a raw feature of row i and, through the two row sums, of the row's normalisation.  An entry is
    uh_il [(q_l - r_i) (cos | sin) -+ c theta_il (sin | cos)] with uh = u / sqrt(s) and |r_i| <= max |q|; a phase error turns (cos, sin) and moves
    c theta, so the amplification is 1 + |c| sum_k |lam_k a_k| + |q_l| + max |q| (the sum bounds |c theta| and the rounding of c theta alike).
    The factor 4 is tol_K's (tests/test_gpu_spd_ai_spectral.py): the entry's own error, the two row sums and the final products.
    Deliberately wider than the bare sketch (d + 1) u sum_k |lam_k a_k| (1 + |c theta| + |q|): it adds the rho . a chain, the 16 u floor, max |q| for
    the normalisation term, the factor 4 and the row maximum of eps, each for the reason above."""
    d = a.shape[-1]
    phase = np.abs(a * lam).sum(-1)
    eps = ((d + 1) * U * (phase + np.abs(a * ref.rho(d)).sum(-1))).max(-1, keepdims=True) + 16.0 * U
    u = np.sqrt(w) * np.exp(-(a * ref.rho(d)).sum(-1))
    uh = u / np.sqrt((u * u).sum(-1, keepdims=True))
    tol = 4.0 * uh * (1.0 + abs(c) * phase + np.abs(q) + np.abs(q).max()) * eps
    return np.concatenate([tol, tol], axis=-1)


def gram_and_derivative(fh, gd):
    """-> (K, dK / d kappa), the diagonals set to 1 (NaN for a NaN row) and 0"""
    k = fh @ fh.T
    m = gd @ fh.T
    dk = m + m.T
    dg = np.diagonal(k)
    with np.errstate(invalid="ignore"):
        np.fill_diagonal(k, dg / dg)
    np.fill_diagonal(dk, 0)
    return k, dk


Likelihood = collections.namedtuple("Likelihood", "out scale cond k dk w")
NAMES = ("ll", "d kappa", "d outputscale", "d noise", "d mean")


def likelihood(a, y, base, kappa, nu, outputscale, noise, mean):
    """The five numbers [ll, d/d kappa, d/d outputscale, d/d noise, d/d mean] of the chain on the log-diagonals a (n, L, d), with the sum of the
    absolute values of each output's terms as its scale and cond_2(Ky): features, Gram matrix and its derivative in long double (rounded to
    fp64 for K, the matrix the likelihood reference reads), the likelihood through _cpu_gp_dense.reference(..., gram=True),
    d/d kappa = outputscale sum W o dK / 2 with that reference's long-double W."""
    lam, w, q, c, _ = points_and_derivative(base, kappa, nu, LD)
    fh, gd = features_and_derivative(a, lam, w, q, c, LD)
    k, dk = gram_and_derivative(fh, gd)
    k64 = k.astype(np.float64)
    r = dense.reference(k64, y, 0.0, outputscale, noise, mean, gram=True)
    terms = LD(0.5) * LD(outputscale) * r.W * dk
    out = np.array(r.out, dtype=LD)
    out[1] = terms.sum()
    scale = np.array(r.scale, dtype=np.float64)
    scale[1] = float(np.abs(terms).sum())
    return Likelihood(out.astype(np.float64), scale, r.cond, k64, dk.astype(np.float64), r.W)


def numpy_route_d_kappa(a, y, base, kappa, nu, outputscale, noise, mean):
    """d ll / d kappa in plain fp64 through LAPACK, the route _cpu_gp_dense.numpy_route takes for the other outputs: the yardstick of the constant
    in front of cond_2(Ky) in that output's tolerance"""
    lam, w, q, c, _ = points_and_derivative(base, kappa, nu)
    fh, gd = features_and_derivative(a, lam, w, q, c)
    k, dk = gram_and_derivative(fh, gd)
    n = len(y)
    ky = outputscale * k + noise * np.eye(n)
    alpha = np.linalg.solve(ky, np.asarray(y, dtype=np.float64) - mean)
    return 0.5 * outputscale * ((np.outer(alpha, alpha) - np.linalg.inv(ky)) * dk).sum()
