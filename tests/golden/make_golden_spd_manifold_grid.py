"""Golden data of the two-operand SPD-manifold operations on a grid of orders and regimes: 50-digit mpmath, written to
tests/golden/spd_manifold_grid.npz.

    python tests/golden/make_golden_spd_manifold_grid.py

Runs on the CPU; the GPU tests read the file only (mpmath is not needed where they run).  The cases come from the family builders of
tests/_cpu_spd_manifold.py (see its docstring): four per order, A well-conditioned, B ill-conditioned base point, C a hair apart, D far apart.

Truth, from the fp64 inputs as stored and rounded once, by the symmetric route: L = chol(X), W = L^-1, eigsy of the whitened matrices
  My = sym(W Y W^T) = Q diag(mu) Q^T     Log_X(Y) = L Q diag(log mu) Q^T L^T     dist(X, Y) = sqrt(sum log^2 mu)
  U := Log_X(Y) rounded to fp64 (the tangent handed to exp: family D brings a large one)
  Mu = sym(W U W^T) = P diag(t) P^T      Exp_X(U) = L P diag(exp t) P^T L^T
  inner(X, U, Y) = tr(X^-1 U X^-1 Y) = sum(Mu o My)   (Y as a second symmetric tangent)          norm(X, U) = sqrt(sum(Mu o Mu))

Layout, per order d (every array float64, first axis = the four families in the order A, B, C, D):
  X_d, Y_d, log_d (= U), exp_d (4, d, d);  dist_d, inner_d, norm_d (4,)
  orders (18,)
  err_oracle, err_whiten (18 orders, 5 ops, 4 families): relative error (max|got - truth| / max|truth|) of two independent fp64 CPU evaluations -
      the oracle's functions, and plain-numpy Cholesky whitening - against the truth; ops in the order log, exp, dist, inner, norm
  eref (5, 4): their maximum over both routes and all orders: the reference error the tests' tolerances are derived from
"""
import os
import sys

import mpmath as mp
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))                       # tests/: the helper module
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))      # the repository root: the oracle
import _cpu_spd_manifold as cpu  # noqa: E402

mp.mp.dps = 50


def to_mp(a):
    return mp.matrix(np.asarray(a, dtype=np.float64).tolist())     # (a Python float converts exactly)


def to_f64(m):
    return np.array([[float(m[i, j]) for j in range(m.cols)] for i in range(m.rows)], dtype=np.float64)


def msym(m):
    return (m + m.T) / 2


def fun_of_sym(m, f):
    """(eigenvalues, Q diag(f(eigenvalues)) Q^T) of a symmetric matrix"""
    lam, q = mp.eigsy(m)
    fl = [f(lam[k]) for k in range(m.rows)]
    scaled = q.copy()
    for i in range(m.rows):
        for k in range(m.rows):
            scaled[i, k] = q[i, k] * fl[k]
    return lam, scaled * q.T


def truth(x64, y64):
    """{name: fp64-rounded 50-digit value} for one case"""
    x, y = to_mp(x64), to_mp(y64)
    d = x.rows
    L = mp.cholesky(x)
    w = mp.inverse(L)
    my = msym(w * y * w.T)
    mu_, logm = fun_of_sym(my, mp.log)
    log = msym(L * logm * L.T)
    dist = mp.sqrt(mp.fsum(mp.log(mu_[k]) ** 2 for k in range(d)))
    u64 = to_f64(log)
    assert np.array_equal(u64, u64.T)
    u = to_mp(u64)
    mu = msym(w * u * w.T)
    _, expm = fun_of_sym(mu, mp.exp)
    exp = msym(L * expm * L.T)
    inner = mp.fsum(mu[i, j] * my[i, j] for i in range(d) for j in range(d))
    norm = mp.sqrt(mp.fsum(mu[i, j] ** 2 for i in range(d) for j in range(d)))
    return {"log": u64, "exp": to_f64(exp), "dist": float(dist), "inner": float(inner), "norm": float(norm)}


def main():
    out = {"orders": np.array(cpu.ORDERS, dtype=np.float64)}
    for d in cpu.ORDERS:
        X, Y, _ = cpu.build_order(d)
        rows = [truth(X[f], Y[f]) for f in range(len(cpu.FAMILIES))]
        out[f"X_{d}"], out[f"Y_{d}"] = X, Y
        for op in cpu.OPS:
            out[f"{op}_{d}"] = np.array([r[op] for r in rows], dtype=np.float64)
        print(f"order {d}", flush=True)
    errs = {name: np.stack([cpu.route_errors(out, d)[name] for d in cpu.ORDERS]) for name in cpu.ROUTES}
    for name, e in errs.items():
        out[f"err_{name}"] = e
    out["eref"] = np.maximum(errs["oracle"], errs["whiten"]).max(axis=0)
    path = os.path.join(HERE, cpu.FIXTURE)
    np.savez(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes")
    print("eref (rows " + ", ".join(cpu.OPS) + "; columns " + ", ".join(cpu.FAMILIES) + ")")
    for op, row in zip(cpu.OPS, out["eref"]):
        print(f"  {op:6s}" + "".join(f" {v:9.2e}" for v in row) + "   tol" + "".join(f" {cpu.tol(out, op, f):8.1e}" for f in cpu.FAMILIES))
    for name, e in errs.items():
        print(f"worst order per (op, family), route {name}:")
        for o, op in enumerate(cpu.OPS):
            print(f"  {op:6s}" + "".join(f" d={cpu.ORDERS[int(np.argmax(e[:, o, f]))]:<2d} {e[:, o, f].max():8.1e}" for f in range(4)))


if __name__ == "__main__":
    main()
