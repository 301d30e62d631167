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

--sweepctl: the kept orientation of every dimension (spd_pair_gauss_only_orientation) with cheaper forms of the QL's per-sweep control, the
candidates of CHANGELOG "sweep control of the Gaussian-only QL iteration", alone and together:

    c1    look-ahead lanes take only the HIGH words of their shift operands (d[l+1], d[l+2], e2[l+1]) from block l+1, the low words from block l:
          the block-(l+1) values to 2^-20 relative
    c2    one product eps2 d[l+1] shared by the deflation tests of e2[l] and e2[l+1] (another rounding order of the same thresholds)
    c3    a deflated e2[l] keeps its low word: a denormal below 4.3e-314 instead of an exact 0                              (kQlCtlDenormalZero)
    far   look-ahead lanes shift by the root of block l+1 next to d[l+2] instead of the one next to d[l+1] (sa = d[l+2], sb = d[l+1]: one select less)
    sq    the shift's root from the bare v_sqrt_f64: modelled as a relative perturbation of the root, uniform in +-2^-23     (kQlCtlHwSqrt)
    nod1  no idle test: a lane that has deflated e2[l] always sweeps on block l+1, converged or not
    c2b   the idle test of block l+1 against the threshold of stage l, eps2 |d[l] d[l+1]|, instead of its own                (kQlCtlStageThreshold)

per case steps and sweeps per wave-row, the QL's VALU per wave-row at 16 per step + the form's per-sweep count (SWEEP_VALU, from the listing),
the largest sweep count of a stage and the worst error of sum log^2 lambda against LAPACK.

    python tools/sim/ql_orientation_sim.py --sweepctl [D ...] > profiles/sweepctl_sim.txt
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
# --sweepctl: the forms simulated and the VALU instructions of sweep control per sweep that the gfx950 listing of each has (d = 10,
# profiles/sweepctl_isa_count.txt; "far" and "c2b" alone were not built: 25 less the two v_cndmask_b32 of one select of a double, 25 less two multiplies)
SWEEP_FORMS = ((), ("c1",), ("c2",), ("c3",), ("c2", "c3"), ("c1", "c2", "c3"), ("far",), ("sq",), ("sq", "nod1"), ("c2", "c3", "sq"), ("c2", "c3", "sq", "nod1"), ("c2b",), ("c2b", "c3"), ("c2b", "c3", "sq"))
SWEEP_VALU = {(): 25, ("c1",): 25, ("c2",): 24, ("c3",): 24, ("c2", "c3"): 23, ("c1", "c2", "c3"): 57, ("far",): 23, ("sq",): 24, ("sq", "nod1"): 21,
              ("c2", "c3", "sq"): 22, ("c2", "c3", "sq", "nod1"): 20, ("c2b",): 23, ("c2b", "c3"): 22, ("c2b", "c3", "sq"): 21}
_HI = np.int64(-1) << np.int64(32)


def _words(hi, lo):
    """the double with the high word of `hi` and the low word of `lo`"""
    return ((hi.view(np.int64) & _HI) | (lo.view(np.int64) & ~_HI)).view(np.float64)


def ql(dg, e2, rule, ctl=()):
    """Wave-level model of tridiag_eigenvalues (look-ahead window 1, deflated e2[l] zeroed, p floored, f^2 t form).  rule: apply the per-lane
    reversal first; ctl: forms of sweep control (module docstring, --sweepctl).  Returns (eigenvalues, sweep steps, sweeps, largest sweep count of a stage of a wave)."""
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
            if "c2" in ctl and l + 1 <= D - 3:
                x = EPS2 * dg[:, l + 1]
                c_l = e2[:, l] <= np.abs(x * dg[:, l])
                c_l1 = e2[:, l + 1] <= np.abs(x * dg[:, l + 2])
            elif "c2b" in ctl and l + 1 <= D - 3:
                thr = EPS2 * np.abs(dg[:, l] * dg[:, l + 1])
                c_l, c_l1 = e2[:, l] <= thr, e2[:, l + 1] <= thr
            else:
                c_l = conv(l)
                c_l1 = conv(l + 1) if l + 1 <= D - 3 else None
            wave_active = (~c_l).reshape(-1, WAVE).any(1)
            if not wave_active.any():
                break
            per_wave += wave_active
            steps += int(wave_active.sum()) * (D - 1 - l)
            sweeps += int(wave_active.sum())
            in_active = np.repeat(wave_active, WAVE)
            if "c3" in ctl:
                # (in place, as the kernel does it: a lane that sits the sweep out keeps the denormal)
                e2[c_l & in_active, l] = _words(np.zeros(n), e2[:, l])[c_l & in_active]
                e2l = e2[:, l].copy()
            else:
                e2l = np.where(c_l, 0.0, e2[:, l])
            k = np.full(n, l)
            work = ~c_l
            if l + 1 <= D - 3:
                ahead = c_l & in_active if "nod1" in ctl else c_l & in_active & ~c_l1
                k[ahead] = l + 1
                work = work | ahead
            idx = lanes[work]
            kx = k[idx]
            d0, d1 = dg[idx, kx], dg[idx, kx + 1]
            ee = np.where(kx == l, e2l[idx], e2[idx, kx])
            if "c1" in ctl and l + 1 <= D - 3:
                d0, d1, ee = _words(d0, dg[idx, l]), _words(d1, dg[idx, l + 1]), _words(ee, e2l[idx])
            if "far" in ctl and l + 1 <= D - 3:
                la = kx == l + 1
                d0, d1 = np.where(la, dg[idx, l + 2], d0), np.where(la, dg[idx, l + 1], d1)
            delta = 0.5 * (d1 - d0)
            root = np.sqrt(delta * delta + ee)
            if "sq" in ctl:
                root = root * (1.0 + 2.0 ** -23 * np.random.default_rng(1000 * l + it).uniform(-1.0, 1.0, len(idx)))
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


def kept_orientation(d):
    """spd_pair_gauss_only_orientation (csrc/spd_pairwise_body.hpp)"""
    return "col0/last" if d == 14 else "last/last"


def run_sweepctl(d, name):
    """{form: (steps, sweeps, QL VALU, largest stage, err)} per wave-row of the kept orientation of dimension d"""
    x1, x2 = family(d, name)
    pad = (-x2.shape[0]) % WAVE
    if pad:
        x2 = np.concatenate([x2, np.repeat(x2[-1:], pad, 0)], 0)
    Linv = np.linalg.inv(np.linalg.cholesky(x1))
    tot = {f: [0, 0, 0, 0.0] for f in SWEEP_FORMS}
    for i in range(x1.shape[0]):
        M = np.einsum("ab,nbc,dc->nad", Linv[i], x2, Linv[i])
        M = 0.5 * (M + M.transpose(0, 2, 1))
        ref = np.sum(np.log(np.linalg.eigvalsh(M)) ** 2, 1)
        dg, e2, rule = oriented(M, kept_orientation(d))
        for f in SWEEP_FORMS:
            ev, steps, sweeps, worst = ql(dg, e2, rule, f)
            with np.errstate(invalid="ignore", divide="ignore"):
                err = np.abs(np.sum(np.log(ev) ** 2, 1) - ref)
            t = tot[f]
            t[0] += steps
            t[1] += sweeps
            t[2] = max(t[2], worst)
            t[3] = max(t[3], float(np.max(err / np.maximum(1.0, ref))) if name == "ratio1e6" else float(np.max(err)))
    nw = x1.shape[0] * x2.shape[0] // WAVE
    return {f: (t[0] / nw, t[1] / nw, 16 * t[0] / nw + SWEEP_VALU[f] * t[1] / nw, t[2], t[3]) for f, t in tot.items()}


def main_sweepctl(dims):
    print("# sweep control of the Gaussian-only QL (tools/sim/ql_orientation_sim.py --sweepctl): the kept orientation per dimension, eps2 1e-14, wave = 64 columns")
    print("# forms: see the module docstring;  QL VALU = 16 steps + (per-sweep count of the form: " +
          ", ".join(f"{'+'.join(f) or 'today'} {SWEEP_VALU[f]}" for f in SWEEP_FORMS) + ") sweeps")
    print("# err = worst |sum log^2 lambda - LAPACK's| (ratio1e6: relative to max(1, sum log^2))")
    summary = {}
    for d in dims:
        for name in FAMILIES:
            res = run_sweepctl(d, name)
            print(f"d = {d:2d}  {name}  ({kept_orientation(d)})")
            for f in SWEEP_FORMS:
                st, sw, valu, worst, err = res[f]
                print(f"    {'+'.join(f) or 'today':9s} steps {st:7.1f}  sweeps {sw:6.2f}  QL VALU {valu:7.0f}  max stage {worst:2d}  err {err:.1e}", flush=True)
            if name == "bench":
                summary[d] = res
    print("# summary, benchmark family: QL VALU per wave-row, today -> each form (ratio)")
    for d, res in summary.items():
        print(f"d = {d:2d}: {res[()][2]:6.0f}" + "".join(f"  {'+'.join(f)} {res[f][2]:6.0f} ({res[f][2] / res[()][2]:.4f})" for f in SWEEP_FORMS[1:]))


def main():
    if "--sweepctl" in sys.argv[1:]:
        return main_sweepctl(tuple(int(a) for a in sys.argv[1:] if a != "--sweepctl") or DIMS)
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
