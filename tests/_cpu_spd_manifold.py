"""CPU side of the SPD-manifold grid tests: the seeded families of point pairs, two independent fp64 evaluations of the two-operand operations,
the error measure and the tolerance rule.  Shared by tests/golden/make_golden_spd_manifold_grid.py (which adds the 50-digit truth), by
test_spd_manifold_grid_cpu.py and by test_gpu_spd_manifold_grid.py.  numpy and the oracle only: no mpmath, no GPU.

Families (four cases per order d, one of each): X = Q diag(lambda) Q^T symmetrised, L its Cholesky factor, Y = L M L^T symmetrised, so the spectrum
of the whitened matrix L^-1 Y L^-T is that of M up to rounding.
  A  well-conditioned     lambda(X) uniform in [0.5, 2];                     M: eigenvalues uniform in [0.5, 2], random frame
  B  ill-conditioned base lambda(X) = 10^linspace(-4, 4, d)  (cond 1e8);     M as A
  C  a hair apart         lambda(X) as A;                                    M = I + 1e-6 S, S symmetric standard normal
  D  far apart            lambda(X) as A;                                    M: eigenvalues exp(uniform(-6, 6)), random frame; for d >= 2 the draw
                                                                             is repeated until max/min >= 1e3 (the condition the CPU test asserts)
"""
import numpy as np

from oracle import spd as ospd

ORDERS = tuple(range(1, 13)) + (13, 16, 17, 24, 31, 32)
FAMILIES = ("A", "B", "C", "D")
OPS = ("log", "exp", "dist", "inner", "norm")          # the operations with a 50-digit truth in the fixture; the order of the eref table's rows
SEED = 20261020
FIXTURE = "spd_manifold_grid.npz"
POLY_TOL = 1e-11                                       # egrad2rgrad / ehess2rhess against their longdouble values, relative to max|truth|
TOL_FLOOR = 1e-12
TOL_CAP = 1e-7
D_MIN_RATIO = 1e3


def sym(a):
    return 0.5 * (a + np.swapaxes(a, -1, -2))


def _frame(rng, d):
    return np.linalg.qr(rng.standard_normal((d, d)))[0]


def _from_spectrum(rng, lam):
    q = _frame(rng, len(lam))
    return sym((q * lam) @ q.T)


def build_case(rng, d, family):
    """(X, Y, M) of one family at order d, drawn from rng"""
    lam = 10.0 ** np.linspace(-4.0, 4.0, d) if family == "B" else rng.uniform(0.5, 2.0, d)
    x = _from_spectrum(rng, lam)
    if family in ("A", "B"):
        m = _from_spectrum(rng, rng.uniform(0.5, 2.0, d))
    elif family == "C":
        g = rng.standard_normal((d, d))
        m = np.eye(d) + 1e-6 * (g + g.T) / np.sqrt(2.0)
    else:
        while True:
            mu = np.exp(rng.uniform(-6.0, 6.0, d))
            if d == 1 or mu.max() / mu.min() >= D_MIN_RATIO:
                break
        m = _from_spectrum(rng, mu)
    L = np.linalg.cholesky(x)
    return x, sym(L @ m @ L.T), m


def build_order(d):
    """X, Y, M (4, d, d): the four cases of order d in the order of FAMILIES"""
    rng = np.random.default_rng([SEED, d])
    cases = [build_case(rng, d, f) for f in FAMILIES]
    return tuple(np.stack([c[k] for c in cases]) for k in range(3))


def whitened(x, y):
    """sym(L^-1 Y L^-T) in fp64, L the Cholesky factor of X"""
    w = np.linalg.inv(np.linalg.cholesky(x))
    return sym(w @ y @ np.swapaxes(w, -1, -2))


def rel_err(got, truth):
    """max|got - truth| / max|truth|: for a matrix over its entries, for a scalar the plain relative error"""
    got, truth = np.asarray(got, dtype=np.float64), np.asarray(truth, dtype=np.float64)
    return float(np.max(np.abs(got - truth)) / np.max(np.abs(truth)))


def route_oracle(x, y, u):
    """The five operations on one case (d x d arrays) by the oracle's functions: {op: value}"""
    dist = ospd.affine_invariant_distance(x[None], y[None])[0, 0]
    return {"log": ospd.spd_log(x, y), "exp": ospd.spd_exp(x, u), "dist": np.sqrt(max(dist * dist - 1e-15, 0.0)),     # (its 1e-15 removed)
            "inner": ospd.spd_inner(x, u, y), "norm": ospd.spd_norm(x, u)}


def route_whiten(x, y, u):
    """The same by Cholesky whitening in plain numpy - the device's algorithm: cholesky, inv, eigh"""
    L = np.linalg.cholesky(x)
    w = np.linalg.inv(L)
    my, mu = w @ y @ w.T, w @ u @ w.T
    lam, v = np.linalg.eigh(sym(my))
    lg = np.log(lam)
    el, ev = np.linalg.eigh(sym(mu))
    return {"log": sym(L @ ((v * lg) @ v.T) @ L.T), "exp": sym(L @ ((ev * np.exp(el)) @ ev.T) @ L.T), "dist": np.sqrt(np.sum(lg * lg)),
            "inner": np.sum(mu * my.T), "norm": np.sqrt(max(np.sum(mu * mu.T), 0.0))}


ROUTES = {"oracle": route_oracle, "whiten": route_whiten}


def route_errors(g, d):
    """{route: (5 ops, 4 families)} relative errors of the two fp64 routes against the fixture's truth at order d"""
    out = {}
    for name, route in ROUTES.items():
        err = np.zeros((len(OPS), len(FAMILIES)))
        for f in range(len(FAMILIES)):
            got = route(g[f"X_{d}"][f], g[f"Y_{d}"][f], g[f"log_{d}"][f])
            for o, op in enumerate(OPS):
                err[o, f] = rel_err(got[op], g[f"{op}_{d}"][f])
        out[name] = err
    return out


def tol(g, op, family):
    """max(10 x eref(op, family), 1e-12): 10 is the project's margin over a reference's own fp64 uncertainty, 1e-12 the bar the eigen-solver's logm
    is held to.  eref (in the fixture) is the worst error of the two CPU routes over all orders; nothing in it comes from the device."""
    return max(10.0 * float(g["eref"][OPS.index(op), FAMILIES.index(family)]), TOL_FLOOR)


# ------------------------------------------------------------------------------ the two polynomial operations, 64-bit mantissa
def _ld(a):
    assert np.finfo(np.longdouble).nmant >= 63, "np.longdouble has no 64-bit mantissa on this platform"      # (x87: 63 stored + the explicit bit)
    return np.asarray(a, dtype=np.longdouble)


def egrad2rgrad_ld(x, g):
    """X sym(G) X in longdouble (np.matmul on longdouble arrays: plain loops, no LAPACK)"""
    x, g = _ld(x), _ld(g)
    return np.matmul(np.matmul(x, sym(g)), x)


def ehess2rhess_ld(x, eg, eh, u):
    """X sym(H) X + sym(U sym(G) X) in longdouble"""
    x, eg, eh, u = _ld(x), _ld(eg), _ld(eh), _ld(u)
    return np.matmul(np.matmul(x, sym(eh)), x) + sym(np.matmul(np.matmul(u, sym(eg)), x))


def poly_inputs(d, n):
    """G, H (n, d, d): seeded standard-normal, non-symmetric Euclidean gradient / Hessian-vector product"""
    rng = np.random.default_rng([SEED, d, 1])
    return rng.standard_normal((n, d, d)), rng.standard_normal((n, d, d))
