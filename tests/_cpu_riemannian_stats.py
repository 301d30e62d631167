"""Plain numpy fp64 restatements of the Riemannian statistics the device code implements: the SPD Frechet mean (affine-invariant metric, with
weights and a start point), the sphere Karcher mean and both parallel-transport operators.  Written from the formulas, with symmetric
eigen-decompositions (`eigh`) where the reference runs the non-symmetric `eig` on S^-1 X.  Test infrastructure: the library has no CPU path."""
import numpy as np


def mandel_index(d):
    r, c = [], []
    for k in range(d):
        for i in range(d - k):
            r.append(i)
            c.append(i + k)
    return np.array(r), np.array(c)


def to_mandel(M):
    M = np.asarray(M, dtype=float)
    r, c = mandel_index(M.shape[-1])
    return M[..., r, c] * np.where(r == c, 1.0, 2.0 ** 0.5)


def from_mandel(v):
    v = np.asarray(v, dtype=float)
    d = int((-1.0 + (1.0 + 8.0 * v.shape[-1]) ** 0.5) / 2.0)
    r, c = mandel_index(d)
    s = np.where(r == c, 1.0, 0.5 ** 0.5)
    M = np.zeros(v.shape[:-1] + (d, d))
    M[..., r, c] = v * s
    M[..., c, r] = v * s
    return M


def sym_fun(S, fun):
    """fun applied to the eigenvalues of the symmetric matrices S (..., d, d)"""
    lam, V = np.linalg.eigh(0.5 * (S + np.swapaxes(S, -1, -2)))
    return np.einsum("...ik,...k,...jk->...ij", V, fun(lam), V)


def spd_mean(X, weights=None, start=None, iters=10, return_residual=False):
    """m <- L expm(sum_j w_j logm(L^-1 X_j L^-T)) L^T, L = chol(m); X: N x d x d; weights normalised by their sum; start: default X[0]."""
    X = np.asarray(X, dtype=float)
    n = X.shape[0]
    w = np.full(n, 1.0 / n) if weights is None else np.asarray(weights, dtype=float) / np.sum(weights)
    m = np.array(X[0] if start is None else start, dtype=float)
    resid = []
    for _ in range(iters):
        L = np.linalg.cholesky(m)
        Li = np.linalg.inv(L)
        S = np.einsum("n,nij->ij", w, sym_fun(Li @ X @ Li.T, np.log))
        resid.append(np.linalg.norm(S))
        m = L @ sym_fun(S, np.exp) @ L.T
        m = 0.5 * (m + m.T)
    return (m, np.array(resid)) if return_residual else m


def sphere_log(x, m):
    """Log_m of the rows of x (N x dim): (x - m cos t) t / sin t, t = acos(clip(<m, x>)); 0 where t < 1e-16"""
    t = np.arccos(np.clip(x @ m, -1.0, 1.0))
    with np.errstate(invalid="ignore", divide="ignore"):
        u = (x - m[None] * np.cos(t)[:, None]) * (t / np.sin(t))[:, None]
    u[t < 1e-16] = 0.0
    return u


def sphere_exp(u, m):
    nu = np.sqrt(np.sum(u * u))
    return m.copy() if nu < 1e-16 else m * np.cos(nu) + u * np.sin(nu) / nu


def sphere_mean(x, weights=None, start=None, iters=10, return_residual=False):
    """m <- Exp_m(sum_j w_j Log_m(x_j)); x: N x dim unit rows."""
    x = np.asarray(x, dtype=float)
    n = x.shape[0]
    w = np.full(n, 1.0 / n) if weights is None else np.asarray(weights, dtype=float) / np.sum(weights)
    m = np.array(x[0] if start is None else start, dtype=float)
    resid = []
    for _ in range(iters):
        u = w @ sphere_log(x, m)
        resid.append(np.sqrt(np.sum(u * u)))
        m = sphere_exp(u, m)
    return (m, np.array(resid)) if return_residual else m


def spd_transport(S1, S2):
    """(S2 S1^-1)^(1/2) = L sqrtm(L^-1 S2 L^-T) L^-1, L = chol(S1)"""
    L = np.linalg.cholesky(np.asarray(S1, dtype=float))
    Li = np.linalg.inv(L)
    return L @ sym_fun(Li @ np.asarray(S2, dtype=float) @ Li.T, np.sqrt) @ Li


def sphere_transport(x1, x2):
    """-x1 sin|u| v^T + v cos|u| v^T + I - v v^T, u = Log_x1(x2), v = u / |u|; the identity when sum(x1 - x2) == 0"""
    x1, x2 = np.asarray(x1, dtype=float).reshape(-1), np.asarray(x2, dtype=float).reshape(-1)
    if np.sum(x1 - x2) == 0.0:
        return np.eye(x1.size)
    u = sphere_log(x2[None], x1)[0]
    nu = np.sqrt(np.sum(u * u))
    v = u / nu
    return -np.sin(nu) * np.outer(x1, v) + np.cos(nu) * np.outer(v, v) + np.eye(x1.size) - np.outer(v, v)


def rand_spd(rng, n, d, c):
    """Q diag(lam) Q^T, Q from qr(randn), lam = 0.1 exp(U[0, ln c])"""
    q = np.linalg.qr(rng.standard_normal((n, d, d)))[0]
    lam = 0.1 * np.exp(rng.uniform(0.0, np.log(c), (n, d)))
    m = np.einsum("nab,nb,ncb->nac", q, lam, q)
    return 0.5 * (m + m.transpose(0, 2, 1))


def rand_sphere(rng, n, dim, spread=0.4):
    """a random unit centre plus spread * randn, normalised"""
    c = rng.standard_normal(dim)
    c /= np.linalg.norm(c)
    x = c[None] + spread * rng.standard_normal((n, dim))
    return x / np.linalg.norm(x, axis=1, keepdims=True)


# ---- the inputs of tests/golden/riemannian_stats.npz: derived from a seed here and in make_golden_stats.py, not stored ------------------------------
# dimension -> c of the SPD recipe; 9 is the first fused instantiation with one wave per SIMD, 12 and 16 are served by the composed path only
STATS_SPD_C = {2: 10.0, 3: 1e3, 5: 10.0, 8: 1e3, 9: 10.0, 10: 1e3, 12: 10.0, 16: 1e3}
STATS_SPHERE_DIMS = (2, 3, 10, 64, 65, 130, 512)
STATS_NS = (1, 2, 63, 64, 65, 129)          # the case with N points is the pool's first N
STATS_SPD_TRANSPORT_DIMS = (2, 3, 5, 10)
STATS_SPHERE_TRANSPORT_DIMS = (2, 3, 10)


def stats_spd_pool(d):
    """129 SPD matrices (as Mandel vectors) of the fixture's recipe at dimension d.  A stream of its own per dimension; the fixture stores the pool's
    first vector so that a numpy whose Generator draws differently is noticed (the QR's last bits may differ between LAPACK builds: 1e-16 of the input)."""
    return to_mandel(rand_spd(np.random.default_rng(20261018 + d), max(STATS_NS), d, STATS_SPD_C[d]))


def stats_sphere_pool(dim):
    return rand_sphere(np.random.default_rng(20270000 + dim), max(STATS_NS), dim, 0.4)
