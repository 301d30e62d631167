"""Host side of the tests of gabo_gp_condition (csrc/gp_condition.hip): seeded cases on a sphere, a from-scratch reference of the
prediction cache in np.longdouble, a plain-numpy fp64 statement of the bordered update the kernels perform, and the error bound the
tests hold both to.  No GPU, no library."""
import functools

import numpy as np

EPS = 2.0 ** -53


def bound(cond, ref):
    """max |got - ref| allowed: the Cholesky forward-error form cond * eps, with a floor for well-conditioned matrices"""
    return (8.0 + 4.0 * cond) * EPS * float(np.max(np.abs(np.asarray(ref, dtype=np.float64))))


def sphere_points(rng, count, dim):
    x = rng.standard_normal((count, dim))
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def base_kernel(x1, x2, beta):
    """exp(-beta acos(<x, y>)^2), the library's Gaussian kernel on the sphere"""
    return np.exp(-beta * np.arccos(np.clip(x1 @ x2.T, -1.0, 1.0)) ** 2)


def make_case(n, t, noise, seed=0, dim=3, beta=2.0, outputscale=1.3, mean=0.4):
    """n old and t new points on S^(dim-1); the points, targets and base kernel matrix of a smaller t are a prefix of those of a larger one"""
    rng = np.random.default_rng([seed, n, dim])
    x = sphere_points(rng, n + 16, dim)[:n + t]
    y = (np.arccos(np.clip(x[:, 0], -1.0, 1.0)) ** 2 + 0.05 * rng.standard_normal(n + 16)[:n + t])
    kb = base_kernel(x, x, beta)
    np.fill_diagonal(kb, 1.0)
    return dict(n=n, t=t, x=x, y=y, kbase=kb, beta=beta, outputscale=outputscale, noise=noise, mean=mean,
                kcross=np.ascontiguousarray(kb[n:, :n]), knew=np.ascontiguousarray(kb[n:, n:]))


def covariance(case, m=None):
    m = case["n"] + case["t"] if m is None else m
    return case["outputscale"] * case["kbase"][:m, :m] + case["noise"] * np.eye(m)


def cond2(case):
    return float(np.linalg.cond(covariance(case)))


def ld_factor(k):
    """(L, L^-1) of the fp64 matrix k in np.longdouble: column Cholesky, then forward substitution row by row"""
    k = np.asarray(k, dtype=np.longdouble)
    m = k.shape[0]
    L = np.zeros((m, m), dtype=np.longdouble)
    for j in range(m):
        s = k[j, j] - L[j, :j] @ L[j, :j]
        if not s > 0:
            raise np.linalg.LinAlgError(f"pivot {j}")
        L[j, j] = np.sqrt(s)
        if j + 1 < m:
            L[j + 1:, j] = (k[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    linv = np.zeros((m, m), dtype=np.longdouble)
    for i in range(m):
        row = -(L[i, :i] @ linv[:i, :])
        row[i] += 1.0
        linv[i] = row / L[i, i]
    return L, linv


def ld_cache(linv_full, y, mean, m):
    """(linv, alpha, kinv) of the leading m points from the longdouble L^-1 of a superset: L^-1 of a leading block is the leading block"""
    linv = linv_full[:m, :m]
    r = np.asarray(y[:m], dtype=np.longdouble) - np.longdouble(mean)
    return linv, linv.T @ (linv @ r), linv.T @ linv


def reference(case, m=None):
    """from scratch in longdouble for the first m points (default: all n + t) -> (linv, alpha, kinv)"""
    m = case["n"] + case["t"] if m is None else m
    _, linv = ld_factor(covariance(case, m))
    return ld_cache(linv, case["y"], case["mean"], m)


def reference_fp64(case, m=None):
    """the same with numpy's fp64 Cholesky (for sizes at which the longdouble loops take minutes)"""
    import scipy.linalg
    m = case["n"] + case["t"] if m is None else m
    L = np.linalg.cholesky(covariance(case, m))
    linv = np.tril(scipy.linalg.solve_triangular(L, np.eye(m), lower=True))
    r = case["y"][:m] - case["mean"]
    return linv, linv.T @ (linv @ r), linv.T @ linv


def bordered_update(linv, alpha, kinv, kcross, knew, y_new, outputscale, noise, mean):
    """What gabo_gp_condition computes, in plain fp64 numpy (its sums in numpy's order) -> (linv, alpha, kinv or None, y_used).
    Raises LinAlgError(j) where the library sets status = {GABO_ERR_NOT_SPD, j}."""
    n, t = linv.shape[0], kcross.shape[0]
    m = n + t
    lo = np.zeros((m, m))
    lo[:n, :n] = np.tril(linv)
    al = np.zeros(m)
    al[:n] = alpha
    a = None
    if kinv is not None:
        a = np.zeros((m, m))
        a[:n, :n] = kinv
    y_used = np.zeros(t)
    for j in range(t):
        N = n + j
        c = outputscale * np.concatenate([kcross[j], knew[j, :j]])
        kappa = outputscale * knew[j, j] + noise
        l = lo[:N, :N] @ c
        lam2 = kappa - l @ l
        if not (lam2 > 0.0 and np.isfinite(lam2)):
            raise np.linalg.LinAlgError(j)
        u = lo[:N, :N].T @ l
        lam = np.sqrt(lam2)
        lo[N, :N] = -u / lam
        lo[N, N] = 1.0 / lam
        s = c @ al[:N]
        if y_new is None:
            y_used[j], gamma = mean + s, 0.0
        else:
            y_used[j] = y_new[j]
            gamma = ((y_new[j] - mean) - s) / lam2
            al[:N] -= gamma * u
        al[N] = gamma
        if a is not None:
            a[:N, :N] += np.outer(u, u) / lam2
            a[N, :N] = a[:N, N] = -u / lam2
            a[N, N] = 1.0 / lam2
    return lo, al, a, y_used


# the cases of the CPU test of the bound: every (n, t, noise) of the grid
GRID_N, GRID_T, GRID_NOISE = (1, 3, 65, 161, 400), (1, 2, 3, 5), (1e-2, 1e-4, 1e-6)


@functools.lru_cache(maxsize=None)
def grid_factor(n, noise):
    """the longdouble L^-1 of the n + max(GRID_T) points of a grid case, shared by its four values of t"""
    case = make_case(n, max(GRID_T), noise)
    return case, ld_factor(covariance(case))[1]


@functools.lru_cache(maxsize=None)
def grid_old(n, noise):
    """the cache of the n old points of a grid case: the longdouble reference rounded to fp64 (treat as read-only)"""
    full, linv_full = grid_factor(n, noise)
    return tuple(np.asarray(v, dtype=np.float64) for v in ld_cache(linv_full, full["y"], full["mean"], n))


def grid_case(n, t, noise):
    """-> (case, fp64 inputs (linv, alpha, kinv) of the n old points, longdouble reference (linv, alpha, kinv) of the n + t)"""
    full, linv_full = grid_factor(n, noise)
    return make_case(n, t, noise), grid_old(n, noise), ld_cache(linv_full, full["y"], full["mean"], n + t)
