"""Host side of the tests of the GP dense-algebra launches (gabo_gp_mll, gabo_gp_mll_gram, gabo_gp_mll_large, gabo_gp_factor) on nearly
singular training covariances: seeded cases of clustered points whose near-duplicates and small noise give cond_2(Ky) up to 1e12, a reference
of everything those launches return in np.longdouble, the same in mpmath at 50 digits (the check of the longdouble one), the plain fp64
LAPACK route (the yardstick of the tolerances) and a construction that makes a chosen pivot negative.  No GPU, no library.

Ky = outputscale * exp(-theta E) + noise I (or outputscale * K + noise I for a given base Gram matrix K), r = y - mean, alpha = Ky^-1 r,
W = alpha alpha^T - Ky^-1; the five outputs are those of csrc/gp_mll.hip,
    [ll, dll/dtheta, dll/doutputscale, dll/dnoise, dll/dmean],
each a sum, and `scale` is the sum of the absolute values of its terms exactly as tests/_cpu_gp_mll_series.reference defines it."""
import collections
import functools
import math

import numpy as np

LD = np.longdouble
U = 2.0 ** -53                      # unit roundoff of fp64
U_LD = 2.0 ** -64                   # ... of the x87 extended format behind np.longdouble
THETA, OUTPUTSCALE, MEAN = 0.8, 1.3, 0.2
LEVELS = {"benign": (None, 0.05), "mid": (1e-3, 1e-7), "hard": (1e-4, 1e-10)}       # level -> (distance of the near-duplicates, noise)
# (n, level) -> the noise used instead of the level's: the smallest power of ten above it at which every pivot of the case stays beyond the
# rounding of an fp64 elimination (tests/test_gp_dense_reference_cpu.py asserts the condition for every case).  None needed so far.
NOISE_RAISED = {}
NAMES = ("ll", "d theta", "d outputscale", "d noise", "d mean")

# The case tables of tests/test_gpu_gp_ill_conditioned.py (the smallest sizes at which each body and edge exists)
MLL_SIZES = (5, 30, 31, 39, 40, 42, 160)      # packed body and its limit; one-wave tiled body (n + 1 = 0 mod 4 twice); several waves with
#                                               n + 1 = 1 and 3 mod 4; the tiled limit
LARGE_SIZES = (161, 192, 193, 512)            # 32 x 32 tiles: 31 padded rows, none, one live row in the last block, 16 pivot blocks
FACTOR_SIZES = (5, 16, 17, 64, 96)
MLL_CASES = [(n, level) for n in MLL_SIZES for level in LEVELS] + [(n, level) for n in LARGE_SIZES for level in ("benign", "mid")]
FACTOR_CASES = [(n, level) for n in FACTOR_SIZES for level in LEVELS]
FLAG_POSITIONS = {20: (0, 1, 10, 19), 39: (0, 4, 37, 38), 160: (0, 3, 4, 80, 156, 159), 161: (0, 31, 32, 100, 160), 512: (0, 33, 300, 511)}
ZERO_POSITIONS = {20: (10,), 39: (37,), 160: (4, 159), 161: (0, 32, 160), 512: (300,)}       # an exactly zero pivot (zero_pivot_at)
LIMIT_SIZES = (2017, 2048)                   # the large path at its limit (level benign, against the fp64 oracle)
REPEAT_CASE = (200, "mid")


def clustered_case(n, level, seed=0):
    """-> (e, y, theta, outputscale, noise, mean): ceil(n / 2) standard-normal points of R^3 and a copy of them displaced by delta * N(0, I)
    (benign: fresh points instead), the first n of the stacked array; e their squared distances, y = sin(x_0) + 0.05 N(0, 1)"""
    delta, noise = LEVELS[level]
    noise = NOISE_RAISED.get((n, level), noise)
    rng = np.random.default_rng([seed, n])
    half = (n + 1) // 2
    p = rng.standard_normal((half, 3))
    q = rng.standard_normal((half, 3))
    x = np.concatenate([p, q if delta is None else p + delta * q])[:n]
    e = np.zeros((n, n))
    for c in range(3):
        d = x[:, c, None] - x[None, :, c]
        e += d * d
    y = np.sin(x[:, 0]) + 0.05 * rng.standard_normal(n)
    return e, y, THETA, OUTPUTSCALE, noise, MEAN


Reference = collections.namedtuple("Reference", "out scale W alpha linv kinv pivots cond")


def _base(e_or_gram, theta, gram, dtype):
    """(K, dK / dtheta) in `dtype` from the fp64 input, the lower triangle mirrored (the launches read the lower triangle)"""
    a = np.asarray(e_or_gram, dtype=np.float64)
    a = (np.tril(a) + np.tril(a, -1).T).astype(dtype)
    if gram:
        return a, np.zeros_like(a)
    k = np.exp(-dtype(theta) * a)
    return k, -a * k


def ld_cholesky(ky):
    """lower Cholesky factor of the longdouble matrix ky, right-looking, one vectorised rank-one update per column; a pivot that is not
    positive raises LinAlgError(its index)"""
    a = np.array(ky, dtype=LD)
    n = a.shape[0]
    L = np.zeros((n, n), dtype=LD)
    for j in range(n):
        if not a[j, j] > 0:
            raise np.linalg.LinAlgError(j)
        L[j, j] = np.sqrt(a[j, j])
        if j + 1 < n:
            col = a[j + 1:, j] / L[j, j]
            L[j + 1:, j] = col
            a[j + 1:, j + 1:] -= col[:, None] * col[None, :]
    return L


def ld_lower_inverse(L):
    """L^-1 by forward substitution, row by row"""
    n = L.shape[0]
    linv = np.zeros((n, n), dtype=LD)
    for i in range(n):
        row = -(L[i, :i] @ linv[:i, :])
        row[i] += 1.0
        linv[i] = row / L[i, i]
    return linv


def _outputs(k, dk, r, alpha, w, logpiv, outputscale):
    n = len(r)
    half_log_2pi_n = 0.5 * n * math.log(2.0 * math.pi)
    if k.dtype == LD:
        half_log_2pi_n = LD(0.5) * n * np.log(8 * np.arctan(LD(1)))       # (pi to the precision of the format)
    out = np.array([-0.5 * (r @ alpha) - 0.5 * logpiv.sum() - half_log_2pi_n,
                    0.5 * outputscale * (w * dk).sum(),
                    0.5 * (w * k).sum(),
                    0.5 * np.trace(w),
                    alpha.sum()])
    scale = np.array([0.5 * abs(r @ alpha) + 0.5 * np.abs(logpiv).sum() + half_log_2pi_n,
                      0.5 * outputscale * np.abs(w * dk).sum(),
                      0.5 * np.abs(w * k).sum(),
                      0.5 * np.abs(np.diagonal(w)).sum(),
                      np.abs(alpha).sum()])
    return out, scale


def reference(e_or_gram, y, theta, outputscale, noise, mean, gram=False):
    """Everything the launches return, in np.longdouble from the fp64 inputs -> Reference(out (5,), scale (5,), W, alpha, linv, kinv,
    pivots = diag(L)^2 (the Schur complements the sweeps meet), cond = cond_2(Ky) from fp64 numpy).  gram: the first argument is the base
    Gram matrix K itself; the theta derivative and its scale are then 0."""
    k, dk = _base(e_or_gram, theta, gram, LD)
    n = len(y)
    ky = LD(outputscale) * k + LD(noise) * np.eye(n, dtype=LD)
    L = ld_cholesky(ky)
    linv = ld_lower_inverse(L)
    kinv = np.einsum("mi,mj->ij", linv, linv)          # L^-T L^-1 (rows of L^-1 read contiguously: half the time of linv.T @ linv at n = 512)
    r = np.asarray(y, dtype=np.float64).astype(LD) - LD(mean)
    alpha = linv.T @ (linv @ r)
    w = alpha[:, None] * alpha[None, :] - kinv
    pivots = np.diagonal(L) ** 2
    out, scale = _outputs(k, dk, r, alpha, w, np.log(pivots), LD(outputscale))
    return Reference(out, scale.astype(np.float64), w, alpha, linv, kinv, pivots, float(np.linalg.cond(ky.astype(np.float64))))


def numpy_route(e_or_gram, y, theta, outputscale, noise, mean, gram=False):
    """the five outputs in plain fp64 through LAPACK (np.linalg.cholesky / solve / inv): the formulas of tests/_cpu_gp_mll_series.reference"""
    k, dk = _base(e_or_gram, theta, gram, np.float64)
    n = len(y)
    ky = outputscale * k + noise * np.eye(n)
    r = np.asarray(y, dtype=np.float64) - mean
    kinv = np.linalg.inv(ky)
    alpha = np.linalg.solve(ky, r)
    w = np.outer(alpha, alpha) - kinv
    logpiv = 2.0 * np.log(np.diagonal(np.linalg.cholesky(ky)))
    return _outputs(k, dk, r, alpha, w, logpiv, outputscale)[0]


def mp_to_longdouble(v):
    """an mpmath number rounded to np.longdouble (through its two leading fp64 pieces: 106 bits)"""
    hi = float(v)
    return LD(hi) + LD(float(v - hi))


def reference_mp(e_or_gram, y, theta, outputscale, noise, mean, gram=False, digits=50):
    """the five outputs and alpha with mpmath at `digits` digits from the same fp64 inputs -> (out, alpha), lists of mpmath numbers.
    For n <= 40: n = 40 takes half a second."""
    import mpmath as mp
    with mp.workdps(digits):
        n = len(y)
        a = np.asarray(e_or_gram, dtype=np.float64)
        a = np.tril(a) + np.tril(a, -1).T
        src = [[mp.mpf(float(a[i, j])) for j in range(n)] for i in range(n)]
        th, os_, nz, mu = (mp.mpf(float(v)) for v in (theta, outputscale, noise, mean))
        zero = mp.mpf(0)
        if gram:
            k, dk = src, [[zero] * n for _ in range(n)]
        else:
            k = [[mp.exp(-th * v) for v in row] for row in src]
            dk = [[-src[i][j] * k[i][j] for j in range(n)] for i in range(n)]
        ky = [[os_ * k[i][j] + (nz if i == j else zero) for j in range(n)] for i in range(n)]
        L = [[zero] * n for _ in range(n)]
        for j in range(n):
            s = ky[j][j] - mp.fdot(L[j][:j], L[j][:j])
            if not s > 0:
                raise np.linalg.LinAlgError(j)
            L[j][j] = mp.sqrt(s)
            for i in range(j + 1, n):
                L[i][j] = (ky[i][j] - mp.fdot(L[i][:j], L[j][:j])) / L[j][j]
        linv = [[zero] * n for _ in range(n)]
        for i in range(n):
            for c in range(i + 1):
                s = (1 if c == i else 0) - mp.fsum(L[i][m] * linv[m][c] for m in range(c, i))
                linv[i][c] = s / L[i][i]
        kinv = [[zero] * n for _ in range(n)]
        for i in range(n):
            for j in range(i + 1):
                kinv[i][j] = kinv[j][i] = mp.fsum(linv[m][i] * linv[m][j] for m in range(i, n))
        r = [mp.mpf(float(v)) - mu for v in np.asarray(y, dtype=np.float64)]
        alpha = [mp.fdot(kinv[i], r) for i in range(n)]
        w = [[alpha[i] * alpha[j] - kinv[i][j] for j in range(n)] for i in range(n)]
        logdet = 2 * mp.fsum(mp.log(L[j][j]) for j in range(n))
        out = [-mp.fdot(r, alpha) / 2 - logdet / 2 - n * mp.log(2 * mp.pi) / 2,
               os_ * mp.fsum(w[i][j] * dk[i][j] for i in range(n) for j in range(n)) / 2,
               mp.fsum(w[i][j] * k[i][j] for i in range(n) for j in range(n)) / 2,
               mp.fsum(w[i][i] for i in range(n)) / 2,
               mp.fsum(alpha)]
        return out, alpha


def indefinite_at(k, y, outputscale, noise, pos):
    """A base Gram matrix that is not positive definite, from one that is: k - ((pivots[pos] + 0.1) / outputscale) e_pos e_pos^T.  The leading
    block before pos is untouched, so the pivots 0 .. pos-1 are those of k; pivot pos becomes -0.1."""
    k = np.array(k, dtype=np.float64)
    n = k.shape[0]
    ky = LD(outputscale) * k.astype(LD) + LD(noise) * np.eye(n, dtype=LD)
    L = ld_cholesky(ky[:pos + 1, :pos + 1])
    k[pos, pos] -= (float(L[pos, pos] ** 2) + 0.1) / outputscale
    return k


def zero_pivot_at(k, outputscale, pos):
    """-> (k', noise'): point pos decoupled from the others (row and column pos of k' are zero) with Ky'[pos, pos] = outputscale * -2^-5 +
    noise' = 0 EXACTLY for noise' = outputscale * 2^-5, with or without a fused multiply-add.  Pivot pos of outputscale k' + noise' I is the
    exact zero whatever the elimination order (nothing but zeros is ever subtracted from it) - the case `pivot > 0` fails on without any
    negative number, NaN or logarithm of one to give it away; the other pivots are those of a positive definite matrix."""
    k = np.array(k, dtype=np.float64)
    k[pos, :] = 0.0
    k[:, pos] = 0.0
    k[pos, pos] = -2.0 ** -5
    return k, outputscale * 2.0 ** -5


# ---- shared, read-only: one computation per case and session ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def case(n, level):
    return clustered_case(n, level, 0)


@functools.lru_cache(maxsize=None)
def gram_of(n, level):
    """the fp64 base Gram matrix exp(-theta e) of the case, as the host hands it to gabo_gp_mll_gram and gabo_gp_factor"""
    e, _, theta = case(n, level)[:3]
    return np.exp(-theta * e)


@functools.lru_cache(maxsize=None)
def case_reference(n, level, gram=False):
    """Reference of the case: of the distance form (gram=False) or of the fp64 Gram matrix gram_of(n, level)"""
    e, y, theta, outputscale, noise, mean = case(n, level)
    return reference(gram_of(n, level) if gram else e, y, theta, outputscale, noise, mean, gram=gram)


def numpy_route_constant(cases):
    """the largest |numpy_route - reference| / (cond 2^-53 scale) over the cases, both forms and the five outputs"""
    worst = 0.0
    for n, level in cases:
        e, y, theta, outputscale, noise, mean = case(n, level)
        for gram in (False, True):
            ref = case_reference(n, level, gram)
            got = numpy_route(gram_of(n, level) if gram else e, y, theta, outputscale, noise, mean, gram=gram)
            err = np.abs(got.astype(LD) - ref.out).astype(np.float64)
            for i in range(5):
                if ref.scale[i] > 0.0:
                    worst = max(worst, err[i] / (ref.cond * U * ref.scale[i]))
    return worst
