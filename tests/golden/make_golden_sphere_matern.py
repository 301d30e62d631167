"""Golden data of the Riemannian Matern / heat kernels on the sphere: 50-digit mpmath, written to tests/golden/sphere_matern.npz.

    python tests/golden/make_golden_sphere_matern.py

Everything is formed from the definition (Borovitskiy et al. 2020), independently of the package:
  d = dim - 1, lambda_n = n (n + d - 1), m_n = (2n + d - 1) Gamma(n + d - 1) / (Gamma(d) Gamma(n + 1))  (d = 1: 1, 2, 2, ...),
  Phi = (2 nu / kappa^2 + lambda)^(-nu - d/2)  or  exp(-kappa^2 lambda / 2),  p_n = Phi(lambda_n) m_n / sum_k Phi(lambda_k) m_k,
  f(c) = sum_n p_n P_n(c),  (n + d - 2) P_n = (2n + d - 3) c P_{n-1} - (n - 1) P_{n-2}.
f' and f'' come from the DIFFERENTIATED recurrence of P_n (not from the identity d/dc P_n^(d) = [n (n + d - 1) / d] P_{n-1}^(d+2) the package
uses; the stored coefficients of orders 1, 2 do use it, and the generator asserts that both routes agree).  d p_n / d kappa uses the closed form
of Phi' and is asserted against a 50-digit central difference.

Layout (arrays are packed: one zip member per quantity, not per case):
  cases (ncase, 4): dim, kappa, nu (inf: heat), L      - only cases whose largest p_n is below 0.9 (a near-constant kernel tests nothing)
  c (nc,): 100 seeded points of [-1, 1], then -1, 1, 1 - 1e-15, 1 + 2^-52       vals (ncase, 4, nc): f, f', f'', df/dkappa at c
  coef0 / coef1 / coef2 / coefk: the coefficients of orders 0, 1, 2 and of d/dkappa, concatenated over the cases; case i owns
      coefX[offX[i]:offX[i + 1]]
  per dim in GRAM_DIMS: x1_d (65, dim), x2_d (130, dim) seeded unit vectors (as fp64), gram_d (65, 130) = f(<x1_i, x2_j>) with the exact
      inner products of those fp64 rows, for the case gram_case_d; gram1_d, gram2_d, gramk_d (7, 33): f', f'', df/dkappa on the leading block
"""
import os

import mpmath as mp
import numpy as np

mp.mp.dps = 50
HERE = os.path.dirname(os.path.abspath(__file__))

DIMS, KAPPAS, NUS, LEVELS = (2, 3, 10, 17), (0.05, 0.3, 1.0), (0.5, 2.5, float("inf")), (1, 32, 128)
GRAM_DIMS, GRAM_CASE = (2, 3, 10, 17), (0.3, 2.5, 32)        # (kappa, nu, L) of the stored Gram matrices


def multiplicity(n, d):
    if d == 1:
        return mp.mpf(1 if n == 0 else 2)
    return (2 * n + d - 1) * mp.gamma(n + d - 1) / (mp.gamma(d) * mp.gamma(n + 1))


def phi(lam, d, kappa, nu):
    if nu == float("inf"):
        return mp.exp(-kappa * kappa * lam / 2)
    return (2 * mp.mpf(nu) / kappa ** 2 + lam) ** (-mp.mpf(nu) - mp.mpf(d) / 2)


def dphi(lam, d, kappa, nu):
    if nu == float("inf"):
        return -kappa * lam * phi(lam, d, kappa, nu)
    nu = mp.mpf(nu)
    return (nu + mp.mpf(d) / 2) * (4 * nu / kappa ** 3) * (2 * nu / kappa ** 2 + lam) ** (-nu - mp.mpf(d) / 2 - 1)


def coefficients(d, kappa, nu, L):
    lam = [mp.mpf(n * (n + d - 1)) for n in range(L + 1)]
    m = [multiplicity(n, d) for n in range(L + 1)]
    w = [phi(l, d, kappa, nu) * mm for l, mm in zip(lam, m)]
    s = mp.fsum(w)
    return [x / s for x in w]


def dcoefficients(d, kappa, nu, L):
    lam = [mp.mpf(n * (n + d - 1)) for n in range(L + 1)]
    m = [multiplicity(n, d) for n in range(L + 1)]
    w = [phi(l, d, kappa, nu) * mm for l, mm in zip(lam, m)]
    dw = [dphi(l, d, kappa, nu) * mm for l, mm in zip(lam, m)]
    s, ds = mp.fsum(w), mp.fsum(dw)
    return [(b * s - a * ds) / (s * s) for a, b in zip(w, dw)]


def derivative_map(coef, d):
    out = [coef[n] * n * (n + d - 1) / mp.mpf(d) for n in range(1, len(coef))]
    return (out if out else [mp.mpf(0)]), d + 2


def value(coef, d, c):
    p = [mp.mpf(1), c]
    for n in range(2, len(coef)):
        p.append(((2 * n + d - 3) * c * p[n - 1] - (n - 1) * p[n - 2]) / (n + d - 2))
    return mp.fsum(x * y for x, y in zip(coef, p[:len(coef)]))


def series(coef, d, c):
    """sum_n coef[n] P_n(c) and its first two derivatives in c, the latter from the differentiated recurrence"""
    p = [mp.mpf(1), c]
    p1 = [mp.mpf(0), mp.mpf(1)]
    p2 = [mp.mpf(0), mp.mpf(0)]
    for n in range(2, len(coef)):
        a, b, den = 2 * n + d - 3, n - 1, n + d - 2
        p.append((a * c * p[n - 1] - b * p[n - 2]) / den)
        p1.append((a * (p[n - 1] + c * p1[n - 1]) - b * p1[n - 2]) / den)
        p2.append((a * (2 * p1[n - 1] + c * p2[n - 1]) - b * p2[n - 2]) / den)
    k = len(coef)
    return (mp.fsum(x * y for x, y in zip(coef, p[:k])), mp.fsum(x * y for x, y in zip(coef, p1[:k])),
            mp.fsum(x * y for x, y in zip(coef, p2[:k])))


def to_f64(v):
    return np.array([float(x) for x in v], dtype=np.float64)


def main():
    rng = np.random.default_rng(20201206)
    c64 = np.concatenate([rng.uniform(-1.0, 1.0, 100), [-1.0, 1.0, 1.0 - 1e-15, 1.0 + 2.0 ** -52]])
    cmp_ = [mp.mpf(float(x)) for x in c64]
    out = {"c": c64}
    cases, vals = [], []
    packed = {k: [] for k in ("coef0", "coef1", "coef2", "coefk")}
    for dim in DIMS:
        d = dim - 1
        for kap in KAPPAS:
            kappa = mp.mpf(float(kap))          # (the fp64 value the package is handed)
            for nu in NUS:
                for L in LEVELS:
                    p = coefficients(d, kappa, nu, L)
                    if max(p) >= mp.mpf("0.9"):
                        continue
                    dp = dcoefficients(d, kappa, nu, L)
                    h = mp.mpf(10) ** -20
                    fd = [(a - b) / (2 * h) for a, b in zip(coefficients(d, kappa + h, nu, L), coefficients(d, kappa - h, nu, L))]
                    assert max(abs(a - b) for a, b in zip(dp, fd)) < mp.mpf(10) ** -30 * (1 + max(abs(x) for x in dp))
                    q1, d1 = derivative_map(p, d)
                    q2, d2 = derivative_map(q1, d1)
                    row = [[], [], [], []]
                    for idx, c in enumerate(cmp_):
                        f0, f1, f2 = series(p, d, c)
                        row[0].append(f0), row[1].append(f1), row[2].append(f2)
                        row[3].append(value(dp, d, c))
                        if idx % 8 == 0 or idx >= 100:
                            # the identity the package relies on, against the differentiated recurrence
                            g1, g2 = value(q1, d1, c), value(q2, d2, c)
                            assert abs(g1 - f1) < mp.mpf(10) ** -35 * (1 + abs(f1)) and abs(g2 - f2) < mp.mpf(10) ** -35 * (1 + abs(f2))
                    cases.append([dim, float(kap), nu, L])
                    vals.append([to_f64(r) for r in row])
                    for key, v in zip(("coef0", "coef1", "coef2", "coefk"), (p, q1, q2, dp)):
                        packed[key].append(to_f64(v))
                    print(f"case dim {dim} kappa {kap} nu {nu} L {L}: max p {float(max(p)):.3f}", flush=True)
    out["cases"] = np.array(cases, dtype=np.float64)
    out["vals"] = np.array(vals, dtype=np.float64)
    for key, chunks in packed.items():
        out[key] = np.concatenate(chunks)
        out["off" + key[4:]] = np.concatenate([[0], np.cumsum([len(x) for x in chunks])]).astype(np.int64)
    kap, nu, L = GRAM_CASE
    kappa = mp.mpf(float(kap))
    for dim in GRAM_DIMS:
        d = dim - 1
        x1 = rng.standard_normal((65, dim))
        x2 = rng.standard_normal((130, dim))
        x1 /= np.linalg.norm(x1, axis=1, keepdims=True)
        x2 /= np.linalg.norm(x2, axis=1, keepdims=True)
        x2[5] = x1[3]            # an inner product next to 1 ...
        x2[6] = -x1[4]           # ... and one next to -1
        p, dp = coefficients(d, kappa, nu, L), dcoefficients(d, kappa, nu, L)
        m1 = [[mp.mpf(float(v)) for v in r] for r in x1]
        m2 = [[mp.mpf(float(v)) for v in r] for r in x2]
        g = np.zeros((65, 130))
        g1, g2, gk = np.zeros((7, 33)), np.zeros((7, 33)), np.zeros((7, 33))
        for i in range(65):
            for j in range(130):
                c = mp.fsum(a * b for a, b in zip(m1[i], m2[j]))
                f0, f1, f2 = series(p, d, c)
                g[i, j] = float(f0)
                if i < 7 and j < 33:
                    g1[i, j], g2[i, j], gk[i, j] = float(f1), float(f2), float(value(dp, d, c))
        out[f"x1_{dim}"], out[f"x2_{dim}"], out[f"gram_{dim}"] = x1, x2, g
        out[f"gram1_{dim}"], out[f"gram2_{dim}"], out[f"gramk_{dim}"] = g1, g2, gk
        out[f"gram_case_{dim}"] = np.array([dim, float(kap), nu, L], dtype=np.float64)
        print(f"gram dim {dim}", flush=True)
    path = os.path.join(HERE, "sphere_matern.npz")
    np.savez(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes, {len(cases)} cases")


if __name__ == "__main__":
    main()
