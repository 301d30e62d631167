"""Plain numpy statement of the random phase features of the Riemannian Matern / heat kernels of the affine-invariant metric on S^d_++
(csrc/spd_ai_spectral.hip, ops.spd_ai_*, SpdAffineInvariantMaternKernel), written from the formulas and not from the device code:

    a(Z)      = 2 log diag chol(Z)                 (lower Cholesky factor)
    rho_k     = (d + 1 - 2k) / 4, k = 1 .. d       |rho|^2 = d (d^2 - 1) / 48,   D = d (d + 1) / 2
    a_il      = a(H_l^T X_i H_l)
    lam_l     = e_l / kappa                                            (heat, nu = inf)
              = e_l sqrt((nu / kappa^2 + |rho|^2 / 2) / gamma_l)       (Matern)
    w_l       = prod_{i<j} tanh(pi |lam_li - lam_lj|)
    F_i       = [sqrt(w_l) exp(-rho . a_il) cos(lam_l . a_il) | sqrt(w_l) exp(-rho . a_il) sin(lam_l . a_il)],   k(X_i, Y_j) = <F_i, F_j> / (|F_i| |F_j|)

with the base draw (e, gamma, H) of numpy.random.Generator(PCG64(seed)) in this order: standard normals (L, d, d) whose symmetric parts give
e = eigvalsh; Generator.permuted of e along its rows; gamma (shape nu, L values; finite nu only); standard normals (L, d, d) whose QR gives H
(columns multiplied by the sign of diag R).  Also a 50-digit mpmath version of `a`, and the truth at d = 2: the heat kernel in closed form
(McKean) and the spectral integral of either family by quadrature.  U = 2^-53 is the unit roundoff the tolerances are stated in."""
import math

import numpy as np

from tests import _cpu_flat_matern as fm

U = 2.0 ** -53
to_mandel, random_spd = fm.to_mandel, fm.random_spd


def from_mandel(v):
    """(..., d(d+1)/2) -> (..., d, d): the diagonal, then the k-th sub-diagonals DIVIDED by sqrt(2) - the operation of the launches, so that the
    matrices the references factor are to the bit the ones the device factors"""
    v = np.asarray(v, dtype=np.float64)
    d = fm.mandel_dim(v.shape[-1])
    m = np.zeros(v.shape[:-1] + (d, d))
    pos = 0
    for k in range(d):
        for c in range(d - k):
            m[..., c + k, c] = m[..., c, c + k] = v[..., pos] if k == 0 else v[..., pos] / math.sqrt(2.0)
            pos += 1
    return m


def rho(d):
    return (d - 1 - 2.0 * np.arange(d)) / 4.0


def rho_norm2(d):
    return d * (d * d - 1) / 48.0


def base_draw(dim, num_features, nu, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    g = rng.standard_normal((num_features, dim, dim))
    e = np.linalg.eigvalsh(0.5 * (g + g.transpose(0, 2, 1)))
    e = rng.permuted(e, axis=1)
    gamma = None if math.isinf(nu) else rng.gamma(nu, 1.0, num_features)
    q, r = np.linalg.qr(rng.standard_normal((num_features, dim, dim)))
    h = q * np.sign(np.diagonal(r, axis1=-2, axis2=-1))[:, None, :]
    return e, gamma, h


def spectral_points(base, kappa, nu):
    e, gamma, _ = base
    d = e.shape[1]
    lam = e / kappa if math.isinf(nu) else e * np.sqrt((nu / kappa ** 2 + 0.5 * rho_norm2(d)) / gamma)[:, None]
    w = np.ones(len(e))
    for i in range(d):
        for j in range(i + 1, d):
            w = w * np.tanh(math.pi * np.abs(lam[:, i] - lam[:, j]))
    return lam, w


def logdiag(x, h):
    """x (n, d, d) SPD, h (L, d, d) -> a (n, L, d)"""
    s = np.einsum("lba,nbc,lcd->nlad", h, x, h)
    return 2.0 * np.log(np.diagonal(np.linalg.cholesky(0.5 * (s + s.transpose(0, 1, 3, 2))), axis1=-2, axis2=-1))


def logdiag_mp(x, h, pairs):
    """the same at 50 digits for the (i, l) in `pairs` -> (len(pairs), d) rounded to fp64"""
    import mpmath
    out = []
    with mpmath.workdps(50):
        for i, l in pairs:
            hm = mpmath.matrix(h[l].tolist())
            c = mpmath.cholesky(hm.T * mpmath.matrix(x[i].tolist()) * hm)
            out.append([float(2 * mpmath.log(c[k, k])) for k in range(x.shape[-1])])
    return np.array(out)


def features(a, lam, w):
    """a (n, L, d) -> normalised features (n, 2 L)"""
    d = a.shape[-1]
    amp = np.sqrt(w) * np.exp(-(a * rho(d)).sum(-1))
    theta = (a * lam).sum(-1)
    f = np.concatenate([amp * np.cos(theta), amp * np.sin(theta)], axis=-1)
    return f / np.sqrt((f * f).sum(-1, keepdims=True))


def kernel_from_logdiag(a1, a2, lam, w):
    """the estimator as the issue writes it: the raw Gram matrix divided by sqrt(k(X, X) k(Y, Y)); a2 None: one point set"""
    d = a1.shape[-1]

    def raw(a):
        amp = np.sqrt(w) * np.exp(-(a * rho(d)).sum(-1))
        theta = (a * lam).sum(-1)
        return np.concatenate([amp * np.cos(theta), amp * np.sin(theta)], axis=-1)
    f1 = raw(a1)
    if a2 is None:          # k(X, X) is the raw matrix's own diagonal: the ratio on the diagonal is 1 to the rounding of one sqrt and one division
        g = f1 @ f1.T
        n1 = np.diagonal(g)
        return g / np.sqrt(n1[:, None] * n1[None, :])
    f2 = raw(a2)
    n1, n2 = (f1 * f1).sum(-1), (f2 * f2).sum(-1)
    return (f1 @ f2.T) / np.sqrt(n1[:, None] * n2[None, :])


def kernel(x1, x2, base, kappa, nu):
    lam, w = spectral_points(base, kappa, nu)
    return kernel_from_logdiag(logdiag(x1, base[2]), None if x2 is None else logdiag(x2, base[2]), lam, w)


# ---------------------------------------------------------------------------------------------------- the truth at d = 2
D2_POINTS = ((0.3, -0.5), (1.0, 0.2), (1.5, -1.0))
# (kappa, (t1, t2)) -> the normalised heat kernel k(I, Y), Y = R(0.7) diag(e^t1, e^t2) R(0.7)^T.  McKean's closed form (heat_truth_d2) and the
# quadrature of the spectral integral (spectral_truth_d2) give these digits alike (they differ by 2e-16)
HEAT_D2 = {(0.7, (0.3, -0.5)): 0.697607160535, (0.7, (1.0, 0.2)): 0.341507767087, (0.7, (1.5, -1.0)): 0.032081767172,
           (1.5, (0.3, -0.5)): 0.915386502157, (1.5, (1.0, 0.2)): 0.783515486394, (1.5, (1.5, -1.0)): 0.430556485714}
# (nu, (t1, t2)) -> the normalised Matern kernel at kappa = 1: spectral_truth_d2 at s_max = 400, ds = 0.005, 720 angles; doubling s_max and
# the angles and halving ds moves none of them by more than 4e-16
MATERN_D2 = {(2.5, (0.3, -0.5)): 0.763490487056, (2.5, (1.0, 0.2)): 0.496718076146, (2.5, (1.5, -1.0)): 0.157431533104,
             (0.5, (0.3, -0.5)): 0.526299898319, (0.5, (1.0, 0.2)): 0.328697768464, (0.5, (1.5, -1.0)): 0.126988479259}


def d2_point(t1, t2, angle=0.7):
    c, s = math.cos(angle), math.sin(angle)
    r = np.array([[c, -s], [s, c]])
    return r @ np.diag([math.exp(t1), math.exp(t2)]) @ r.T


def heat_truth_d2(kappa, t1, t2):
    """S^2_++ = R x H^2 (curvature -1/2): exp(-u^2 / (2 kappa^2)) p_tau(r / sqrt 2) / p_tau(0), u = (t1 + t2) / sqrt 2, r = |t1 - t2| / sqrt 2,
    tau = kappa^2 / 4, p_tau(x) = int_x^inf s exp(-s^2 / 4 tau) / sqrt(cosh s - cosh x) ds (McKean).  Needs scipy."""
    from scipy.integrate import quad
    tau = kappa ** 2 / 4.0

    def p(x):
        # s = x + v^2: cosh s - cosh x = 2 sinh((s + x) / 2) sinh((s - x) / 2), finite integrand at v = 0
        def f(v):
            s = x + v * v
            den = 2.0 * math.sinh(0.5 * (s + x)) * math.sinh(0.5 * v * v) if v > 0 else 0.0
            if den <= 0.0:
                return 2.0 * x * math.exp(-x * x / (4 * tau)) / math.sqrt(math.sinh(x)) if x > 0 else 2.0 * math.sqrt(2.0)
            return 2.0 * v * s * math.exp(-s * s / (4 * tau)) / math.sqrt(den)
        return quad(f, 0.0, math.sqrt(40.0 * math.sqrt(tau) + 40.0), epsabs=1e-14, epsrel=1e-13, limit=400)[0]
    u, r = (t1 + t2) / math.sqrt(2.0), abs(t1 - t2) / math.sqrt(2.0)
    return math.exp(-u * u / (2 * kappa ** 2)) * p(r / math.sqrt(2.0)) / p(0.0)


def _bessel_k(order, x):
    """K_order(x) = int_0^inf exp(-x cosh u) cosh(order u) du, trapezoid (exponentially convergent); x > 0 array"""
    u = np.linspace(0.0, 12.0, 2401)
    f = np.exp(-x[:, None] * np.cosh(u)[None, :]) * np.cosh(order * u)[None, :]
    return (f.sum(-1) - 0.5 * (f[:, 0] + f[:, -1])) * (u[1] - u[0])


def spectral_truth_d2(kappa, nu, t1, t2, s_max=400.0, ds=0.005, angles=720):
    """k(I, Y) by quadrature of the spectral integral, in s = lam_1 - lam_2, t = lam_1 + lam_2 (|lam|^2 = (s^2 + t^2) / 2, |c|^-2 = |s| tanh(pi |s|)):
    a_1 + a_2 = log det Y for every H, so the integral over t is the Fourier transform of Phi at omega = (t1 + t2) / 2 - a Gaussian (heat) or
    2 sqrt(pi) / Gamma(p) (|omega| / 2 sqrt B)^(p - 1/2) K_(p - 1/2)(sqrt(B) |omega|), B = 2 (2 nu / kappa^2 + 1/8) + s^2, p = nu + 3/2 (Matern) -
    and what is left is  int_0^inf s tanh(pi s) T(s) Re psi_s ds  over the same with psi = 1, omega = 0;  psi_s = E_H exp(-(a_1 - a_2)(1/4 + i s / 2)),
    E_H by the trapezoid rule over the rotation angle (reflections do not change diag chol).  Simpson in s on [0, s_max]; the tail of the
    denominator beyond s_max, where tanh = 1, in closed form."""
    y = d2_point(t1, t2)
    phi = 2.0 * math.pi * np.arange(angles) / angles
    c, sn = np.cos(phi), np.sin(phi)
    s11 = c * c * y[0, 0] + 2 * c * sn * y[0, 1] + sn * sn * y[1, 1]           # (H^T Y H)_11, H = R(phi)
    a1 = np.log(s11)
    delta = 2.0 * a1 - math.log(np.linalg.det(y))                             # a_1 - a_2
    omega = abs(0.5 * (t1 + t2))
    s = np.arange(0.0, s_max + 0.5 * ds, ds)
    if len(s) % 2 == 0:
        s = s[:-1]
    simpson = np.ones(len(s))
    simpson[1:-1:2], simpson[2:-1:2] = 4.0, 2.0
    simpson *= (s[1] - s[0]) / 3.0
    re_psi = np.empty(len(s))
    for lo in range(0, len(s), 4096):
        blk = s[lo:lo + 4096]
        re_psi[lo:lo + 4096] = (np.exp(-0.25 * delta)[None, :] * np.cos(0.5 * blk[:, None] * delta[None, :])).mean(-1)
    plancherel = s * np.tanh(math.pi * s)
    if math.isinf(nu):
        t_num = np.exp(-kappa ** 2 * s * s / 4.0) * math.exp(-omega ** 2 / kappa ** 2)
        t_den = np.exp(-kappa ** 2 * s * s / 4.0)
        tail = 0.0
    else:
        p = nu + 1.5
        c0 = 2.0 * (2.0 * nu / kappa ** 2 + 0.125)
        b = c0 + s * s
        t_den = math.sqrt(math.pi) * math.gamma(p - 0.5) / math.gamma(p) * b ** (0.5 - p)
        if omega == 0.0:
            t_num = t_den
        else:
            sb = np.sqrt(b)
            t_num = 2.0 * math.sqrt(math.pi) / math.gamma(p) * (omega / (2.0 * sb)) ** (p - 0.5) * _bessel_k(p - 0.5, sb * omega)
        tail = math.sqrt(math.pi) * math.gamma(p - 0.5) / math.gamma(p) * (c0 + s[-1] ** 2) ** (-nu) / (2.0 * nu)
    return float((simpson * plancherel * t_num * re_psi).sum() / ((simpson * plancherel * t_den).sum() + tail))
