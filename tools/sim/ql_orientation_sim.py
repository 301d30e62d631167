#!/usr/bin/env python3
"""CPU simulation: which end of the Householder tridiagonal should sit at the QL iteration's deflation index (0), as a COMPILE-TIME fact?

csrc/spd_eig.hpp reverses (dg, e2) per lane when |dg[0]| > |dg[D-1]| (~40 selects per pair).  The tridiagonal that the reduction produces is
the Lanczos tridiagonal of M started at a unit vector and is systematically graded, so a fixed orientation can replace the per-lane rule.
This script counts, at WAVE granularity (64 consecutive columns share the instruction stream, as in ql_lookahead_sim.py whose generator and
reduction it imports), the sweep steps and sweeps of the QL with the kernel's Gaussian-only settings (eps2 = 1e-14, look-ahead window 1, floor
on p, the f^2 t form) for six orientations:

    col0/rule   elimination from column 0 of M, per-lane reversal rule                     (the strict path; the parent of this study)
    col0/first  elimination from column 0, entries produced FIRST at the deflation index   (never reversed)
    col0/last   elimination from column 0, entries produced LAST at the deflation index    (always reversed)
    last/rule   elimination from the last column of M towards the first, per-lane rule
    last/last   elimination from the last column, entries produced last at the deflation index
    last/first  elimination from the last column, entries produced first at the deflation index

for every D that has a Gaussian-only instantiation (3 ... 20 without 12) and three input families restated from
tests/test_gpu_pairwise_gauss_finish.py: the benchmark generator (rows 5, 100, 2000, 3000 of an N = 4096 set against all its columns, seed
1234), nearly identical pairs and eigenvalue ratio 1e6 (40 x 300 pairs each, the test's seeds; the partial last wave recomputes the last
column as the kernel's clamped lanes do).  Per case: steps and sweeps per wave, the QL's VALU per wave-row at 16 per step + 25 per sweep, the
LARGEST sweep count of any stage of any wave (the kernel caps a stage at 60) and the worst absolute error of sum log^2 lambda against LAPACK.

    python tools/sim/ql_orientation_sim.py [D ...] > profiles/orient_sim.txt
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ql_lookahead_sim as base  # noqa: E402

EPS2 = 1e-14          # GABO_QL_EPS2_GAUSS
CAP = 60              # sweeps per stage in tridiag_eigenvalues
WAVE = 64
DIMS = tuple(d for d in range(3, 21) if d != 12)
ORIENTATIONS = ("col0/rule", "col0/first", "col0/last", "last/rule", "last/last", "last/first")
FAMILIES = ("bench", "near", "ratio1e6")
BENCH_ROWS = (5, 100, 2000, 3000)
N1, N2 = 40, 300


def ql(dg, e2, rule):
    """Wave-level model of tridiag_eigenvalues (look-ahead window 1, deflated e2[l] zeroed, p floored, f^2 t form).  rule: apply the per-lane
    reversal first.  Returns (eigenvalues, sweep steps, sweeps, largest sweep count of a stage of a wave)."""
    dg, e2 = dg.copy(), e2.copy()
    n, D = dg.shape
    assert n % WAVE == 0
    if rule and D >= 3:
        flip = np.abs(dg[:, 0]) > np.abs(dg[:, D - 1])
        dg[flip] = dg[flip, ::-1]
        e2[flip, :D - 1] = e2[flip, D - 2::-1]
    steps = sweeps = worst_stage = 0
    lanes = np.arange(n)

    def conv(k):
        return e2[:, k] <= EPS2 * np.abs(dg[:, k] * dg[:, k + 1])

    for l in range(D - 2):
        per_wave = np.zeros(n // WAVE, dtype=int)
        for it in range(CAP):
            c_l = conv(l)
            wave_active = (~c_l).reshape(-1, WAVE).any(1)
            if not wave_active.any():
                break
            per_wave += wave_active
            steps += int(wave_active.sum()) * (D - 1 - l)
            sweeps += int(wave_active.sum())
            in_active = np.repeat(wave_active, WAVE)
            e2l = np.where(c_l, 0.0, e2[:, l])
            k = np.full(n, l)
            work = ~c_l
            if l + 1 <= D - 3:
                ahead = c_l & in_active & ~conv(l + 1)
                k[ahead] = l + 1
                work = work | ahead
            idx = lanes[work]
            kx = k[idx]
            d0, d1 = dg[idx, kx], dg[idx, kx + 1]
            ee = np.where(kx == l, e2l[idx], e2[idx, kx])
            delta = 0.5 * (d1 - d0)
            root = np.sqrt(delta * delta + ee)
            sigma = d0 - np.copysign(root - np.abs(delta), delta)
            gamma = dg[idx, D - 1] - sigma
            p = gamma * gamma + 1e-150
            s = np.zeros(len(idx))
            for i in range(D - 2, l - 1, -1):
                bb = e2l[idx] if i == l else e2[idx, i]
                r = p + bb
                if i != D - 2:
                    e2[idx, i + 1] = s * r
                t = 1.0 / (p * r)
                ir = t * p
                s = bb * ir
                oldgam = gamma
                al = dg[idx, i]
                f = p * (al - sigma) - bb * oldgam
                gamma = ir * f
                dg[idx, i + 1] = oldgam + (al - gamma)
                p = (f * t) * f + 1e-150
            e2[idx, l] = s * p
            dg[idx, l] = sigma + gamma
        worst_stage = max(worst_stage, int(per_wave.max()))
    a, b2, cc = dg[:, D - 2].copy(), e2[:, D - 2].copy(), dg[:, D - 1].copy()
    sm, df = a + cc, a - cc
    rt = np.sqrt(df * df + 4 * b2)
    r1 = 0.5 * (sm + np.copysign(rt, sm))
    dg[:, D - 2] = r1
    dg[:, D - 1] = (a * cc - b2) / r1
    return dg, steps, sweeps, worst_stage


def oriented(M, name):
    """(dg, e2, rule) of the tridiagonal of M in orientation `name`; index 0 is where the QL deflates"""
    elim, order = name.split("/")
    D = M.shape[-1]
    dg, e2 = base.tridiag(M[:, ::-1, ::-1] if elim == "last" else M)          # entries in the order the reduction produced them
    if order == "last":
        dg = dg[:, ::-1]
        e2 = np.concatenate([e2[:, D - 2::-1], e2[:, D - 1:]], 1)
    return np.ascontiguousarray(dg), np.ascontiguousarray(e2), order == "rule"


def _spd_from(rng, lam):
    n, d = lam.shape
    q = np.linalg.qr(rng.standard_normal((n, d, d)))[0]
    m = np.einsum("nab,nb,ncb->nac", q, lam, q)
    return 0.5 * (m + m.transpose(0, 2, 1))


def _test_set(n, d, seed):
    rng = np.random.default_rng(seed)
    return _spd_from(rng, rng.uniform(0.05, 5.0, size=(n, d)))


def _mandel_perturb(rng, x):
    """an entry-wise 1e-6-relative perturbation of the Mandel vector of x = the same relative perturbation of the symmetric matrix's entries"""
    d = x.shape[-1]
    z = np.empty_like(x)
    for k in range(d):                    # Mandel order: diagonal by diagonal
        for i in range(d - k):
            g = rng.standard_normal(x.shape[0])
            z[:, i, i + k] = z[:, i + k, i] = g
    return x * (1.0 + 1e-6 * z)


def family(d, name):
    """(x1, x2): SPD matrices (n1, d, d), (n2, d, d) of one family (without the test's non-positive-definite column)"""
    if name == "bench":
        x = base.synth(4096, d, 1234)
        return x[list(BENCH_ROWS)], x
    seed = 1000 * d + FAMILIES.index(name)
    rng = np.random.default_rng(seed)
    if name == "near":
        x2 = _test_set(N2, d, seed + 200)
        # (the standard-normal draws are consumed in another order than the test's flat array: the same family, not the same bits)
        return _mandel_perturb(rng, x2)[:N1], x2

    def lam(n):
        v = 10.0 ** rng.uniform(-3.0, 3.0, size=(n, d))
        v[:, 0], v[:, 1] = 1e-3, 1e3
        return v
    return _spd_from(rng, lam(N1)), _spd_from(rng, lam(N2))


def run(d, name):
    x1, x2 = family(d, name)
    pad = (-x2.shape[0]) % WAVE
    if pad:
        x2 = np.concatenate([x2, np.repeat(x2[-1:], pad, 0)], 0)
    Linv = np.linalg.inv(np.linalg.cholesky(x1))
    tot = {o: [0, 0, 0, 0.0] for o in ORIENTATIONS}
    for i in range(x1.shape[0]):
        M = np.einsum("ab,nbc,dc->nad", Linv[i], x2, Linv[i])
        M = 0.5 * (M + M.transpose(0, 2, 1))
        ref = np.sum(np.log(np.linalg.eigvalsh(M)) ** 2, 1)
        for o in ORIENTATIONS:
            dg, e2, rule = oriented(M, o)
            ev, steps, sweeps, worst = ql(dg, e2, rule)
            with np.errstate(invalid="ignore", divide="ignore"):
                err = np.abs(np.sum(np.log(ev) ** 2, 1) - ref)
            t = tot[o]
            t[0] += steps
            t[1] += sweeps
            t[2] = max(t[2], worst)
            t[3] = max(t[3], float(np.max(err / np.maximum(1.0, ref))) if name == "ratio1e6" else float(np.max(err)))
    nw = x1.shape[0] * x2.shape[0] // WAVE
    return {o: (t[0] / nw, t[1] / nw, 16 * t[0] / nw + 25 * t[1] / nw, t[2], t[3]) for o, t in tot.items()}


def main():
    dims = tuple(int(a) for a in sys.argv[1:]) or DIMS
    print("# QL orientation study (tools/sim/ql_orientation_sim.py): eps2 1e-14, look-ahead window 1, floor on p, f^2 t form, wave = 64 columns")
    print("# steps, sweeps: per wave-row;  QL VALU = 16 steps + 25 sweeps;  max stage = largest sweep count of one stage of one wave (cap 60)")
    print("# err = worst |sum log^2 lambda - LAPACK's| (ratio1e6: relative to max(1, sum log^2))")
    best = {}
    for d in dims:
        for name in FAMILIES:
            res = run(d, name)
            print(f"d = {d:2d}  {name}")
            for o in ORIENTATIONS:
                st, sw, valu, worst, err = res[o]
                print(f"    {o:11s} steps {st:7.1f}  sweeps {sw:6.2f}  QL VALU {valu:7.0f}  max stage {worst:2d}  err {err:.1e}", flush=True)
            if name == "bench":
                fixed = [o for o in ORIENTATIONS if not o.endswith("rule")]
                best[d] = (min(fixed, key=lambda o: res[o][2]), res)
    print("# summary, benchmark family: QL VALU per wave-row today (col0/rule) -> best fixed form (the rule's own ~37 VALU not counted)")
    for d, (o, res) in best.items():
        print(f"d = {d:2d}: {res['col0/rule'][2]:6.0f} -> {res[o][2]:6.0f}  {o}   (col0/last {res['col0/last'][2]:6.0f}, last/last {res['last/last'][2]:6.0f})")


if __name__ == "__main__":
    main()
