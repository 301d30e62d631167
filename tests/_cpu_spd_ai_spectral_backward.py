"""Plain numpy statement of the x-gradient of the normalised random phase features of the affine-invariant Matern / heat kernels
(csrc/spd_ai_spectral_backward.hip, ops.spd_ai_spectral_features_backward), written from the closed form and not from the device code.
Notation of tests/_cpu_spd_ai_spectral.py; Fh (n, 2L) the normalised features, Gb (n, 2L) their upstream gradient:

    X_i = G G^T (G lower),  M = H_l^T G,  v_0 .. v_{d-1} = the rows of M made orthogonal to the rows before them,  a_k = log |v_k|^2
    s_i  = <Gb_i, Fh_i>
    P_il = (Gb_c - s Fh_c) Fh_c + (Gb_s - s Fh_s) Fh_s,   R_il = Gb_s Fh_c - Gb_c Fh_s       (c, s: the entries l and L + l of row i)
    gb_ilk = -rho_k P_il + lam_lk R_il                                                        (the adjoint of a_ilk)
    S_i  = sum_l sum_k gb_ilk v_ilk v_ilk^T / |v_ilk|^2,   Gamma_i = G^-T S_i G^-1
    grad_x_i = mandel(Gamma_i): the diagonal, then the k-th sub-diagonals times sqrt 2

(d a_k / d X = G^-T v_k v_k^T G^-1 / |v_k|^2: a_k is the difference of the log-determinants of two leading minors of H^T X H.)  Every step is
written with explicit loops over d, so that it runs in np.float64 and in np.longdouble alike: numpy.linalg has no long double."""
import numpy as np

from tests import _cpu_spd_ai_spectral as ref

U = ref.U


def cholesky(x):
    """(n, d, d) -> lower factors, in x's dtype; a pivot that is not > 0 gives NaN"""
    d = x.shape[-1]
    g = np.zeros_like(x)
    for r in range(d):
        for c in range(r + 1):
            s = x[:, r, c] - (g[:, r, :c] * g[:, c, :c]).sum(-1)
            if r == c:
                with np.errstate(invalid="ignore"):
                    g[:, r, r] = np.where(s > 0, np.sqrt(np.where(s > 0, s, 1)), np.nan)
            else:
                g[:, r, c] = s / g[:, c, c]
    return g


def lower_inverse(g):
    """(n, d, d) lower -> their inverses by forward substitution"""
    d = g.shape[-1]
    w = np.zeros_like(g)
    for c in range(d):
        w[:, c, c] = 1 / g[:, c, c]
        for r in range(c + 1, d):
            w[:, r, c] = -(g[:, r, c:r] * w[:, c:r, c]).sum(-1) / g[:, r, r]
    return w


def orthogonal_rows(g, h):
    """g (n, d, d), h (L, d, d) -> (v (n, L, d, d): row k of H_l^T G_i orthogonal to rows 0 .. k-1, nn (n, L, d) = |v_k|^2)"""
    m = np.einsum("lrk,nrj->nlkj", h, g)
    d = g.shape[-1]
    v = np.zeros_like(m)
    nn = np.zeros(m.shape[:-1], dtype=m.dtype)
    for k in range(d):
        row = m[:, :, k, :].copy()
        for p in range(k):
            row = row - ((row * v[:, :, p]).sum(-1) / nn[:, :, p])[..., None] * v[:, :, p]
        v[:, :, k] = row
        nn[:, :, k] = (row * row).sum(-1)
    return v, nn


def to_mandel(mats):
    """ref.to_mandel in the dtype of `mats`"""
    d = mats.shape[-1]
    parts = [np.diagonal(mats, axis1=-2, axis2=-1)]
    for k in range(1, d):
        parts.append(np.sqrt(mats.dtype.type(2)) * np.diagonal(mats, offset=-k, axis1=-2, axis2=-1))
    return np.concatenate(parts, axis=-1)


def log_diagonal_adjoint(fhat, gbar, lam):
    """-> gb (n, L, d), the adjoint of the log-diagonals"""
    L, d = lam.shape
    s = (gbar * fhat).sum(-1, keepdims=True)
    fc, fs, gc, gs = fhat[:, :L], fhat[:, L:], gbar[:, :L], gbar[:, L:]
    p = (gc - s * fc) * fc + (gs - s * fs) * fs
    r = gs * fc - gc * fs
    return -p[..., None] * ref.rho(d).astype(fhat.dtype) + r[..., None] * lam


def backward(v_mandel, h, lam, fhat, gbar, dtype=np.float64):
    """v_mandel (n, dv) fp64 Mandel vectors, h (L, d, d), lam (L, d), fhat and gbar (n, 2L) -> dict(grad (n, dv), scale (n,)) in `dtype`;
    scale_i = sqrt 2 |G_i^-1|_F^2 sum_lk |gb_ilk| bounds the sum of the magnitudes of the terms of Gamma_i.  The matrices factored are
    ref.from_mandel(v_mandel): to the bit those of the launch."""
    x = ref.from_mandel(v_mandel).astype(dtype)
    h, lam, fhat, gbar = (np.asarray(t, dtype=np.float64).astype(dtype) for t in (h, lam, fhat, gbar))
    g = cholesky(x)
    v, nn = orthogonal_rows(g, h)
    gb = log_diagonal_adjoint(fhat, gbar, lam)
    s = np.einsum("nlk,nlkr,nlkc->nrc", gb / nn, v, v)
    w = lower_inverse(g)
    gamma = np.einsum("nar,nab,nbc->nrc", w, s, w)
    scale = np.sqrt(dtype(2)) * (w * w).sum((-1, -2)) * np.abs(gb).sum((-1, -2))
    return dict(grad=to_mandel(gamma), scale=scale)


def backward_with_tolerance(v_mandel, h, lam, fhat, gbar, terms):
    """-> (grad fp64 (n, dv), tol (n,), usual (n,), ref_err (n,)):  ref_err_i = max|grad_fp64 - grad_longdouble|_i, the reference against its
    more precise evaluation;  tol_i = max(8 ref_err_i, terms u scale_i), the second the worst-case rounding of a sum of `terms` terms;
    usual_i = 64 u scale_i, the project's usual mark"""
    lo = backward(v_mandel, h, lam, fhat, gbar, np.float64)
    hi = backward(v_mandel, h, lam, fhat, gbar, np.longdouble)
    ref_err = np.abs(lo["grad"] - hi["grad"]).max(-1).astype(np.float64)
    return lo["grad"], np.maximum(8.0 * ref_err, terms * U * lo["scale"]), 64.0 * U * lo["scale"], ref_err
