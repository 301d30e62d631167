// Per-lane symmetric eigenvalue solver for small fixed D (register resident, no cross-lane traffic):
//   Householder tridiagonalisation of a packed lower triangle, then square-root-free implicit QL
//   (Pal-Walker-Kahan recurrence, the scheme LAPACK's dsterf uses) on (diag, offdiag^2).
// One lane owns one matrix; all indices into the register arrays are compile-time constants.
//
// This is the arithmetic that replaces the reference's per-pair `torch.symeig` call
// (Riemannian_utils/spd_utils_torch.py:109-110).
#pragma once
#include "gabo_device.hpp"

namespace gabo {

// Which end of the tridiagonal sits at index 0, where tridiag_eigenvalues deflates - per lane at run time, or fixed at compile time:
//   kQlOrientPerLane   reduction from column 0 of M, entries in the order produced; the QL reverses them per lane (see there).  The strict path.
//   kQlOrientCol0      reduction from column 0, the entries produced LAST at index 0; no per-lane reversal.
//   kQlOrientLast      reduction from the LAST column of M towards the first (the index map r -> D-1-r on every compile-time index: the
//                      same instructions, no moves), the entries produced last at index 0; no per-lane reversal.
// The tridiagonal of a Householder reduction is the Lanczos tridiagonal of M started at a unit vector: its leading entries carry the bulk of
// the spectrum and the coupling, its trailing ones are small and nearly decoupled - the end a QL iteration wants at its deflation index.  Which
// fixed form a dimension uses, if any: spd_pair_gauss_only_orientation (spd_pairwise_body.hpp).
enum QlOrient : int { kQlOrientPerLane = 0, kQlOrientCol0 = 1, kQlOrientLast = 2 };

// Cheaper forms of the per-sweep control of tridiag_eigenvalues (a bit mask; which a dimension uses: spd_pair_gauss_only_sweepctl,
// spd_pairwise_body.hpp).  Each replaces a value that only feeds the shift or a threshold compare by one that is cheaper to form; none touches
// the arithmetic of a sweep step.  Only for the fixed orientations: the strict path keeps the plain control and its pinned bits.
//   kQlCtlDenormalZero     a deflated e2[l] is cleared in its HIGH word only, in place (one v_cndmask_b32 instead of two): what is left is a
//                          denormal <= 4.3e-314 where the plain form has an exact 0 (fp64 denormals are not flushed: the kernels run in denorm mode 3)
//   kQlCtlHwSqrt           the shift's square root is the bare v_sqrt_f64 (2^-23) instead of x * v_rsq_f64(x): one instruction less, and sqrt(0) = 0
//   kQlCtlStageThreshold   the idle test of block l + 1 compares e2[l+1] with the threshold of stage l, eps2 |d_l d_{l+1}|, already formed for
//                          e2[l], instead of its own eps2 |d_{l+1} d_{l+2}|: two multiplies less.  It decides only whether a look-ahead lane
//                          spends the sweep on block l + 1 or sits it out; stage l + 1 deflates by its own threshold as before.
enum QlSweepCtl : int { kQlCtlPlain = 0, kQlCtlDenormalZero = 1, kQlCtlHwSqrt = 2, kQlCtlStageThreshold = 4 };

// m: packed lower triangle of a symmetric D x D matrix (destroyed).  Out: dg[0..D-1] diagonal and
// e2[0..D-2] squared off-diagonals of the similar tridiagonal matrix (e2[D-1] = 0).
template <int D, int ORIENT = kQlOrientPerLane>
__device__ __forceinline__ void tridiagonalize(double (&m)[tri_size(D)], double (&dg)[D], double (&e2)[D]) {
    constexpr bool kFromLast = ORIENT == kQlOrientLast, kOutRev = ORIENT != kQlOrientPerLane;
    // entry (r, c), r >= c, of the matrix the reduction works on: M itself, or M with rows and columns in reverse order
    auto tri = [](int r, int c) constexpr { return kFromLast ? gabo::tri(D - 1 - c, D - 1 - r) : gabo::tri(r, c); };
    static_for<D - 2>([&](auto kk) {
        constexpr int k = decltype(kk)::value;
        constexpr int n = D - k - 1;  // order of the trailing block; column below the diagonal is x_0..x_{n-1}
        // u = x + sign(x0)|x| e0 ;  H = I - u u^T / hh,  hh = |x|^2 + |x0||x|
        double alpha = m[tri(k + 1, k)];
        double sig = 0.0;
        static_for<n - 1>([&](auto t) { double x = m[tri(k + 2 + decltype(t)::value, k)]; sig = __builtin_fma(x, x, sig); });
        double nn = __builtin_fma(alpha, alpha, sig);
        // A column that is already zero needs no special case when |x| is floored at 1e-145 and hh is taken as |u|^2 / 2 from the u
        // actually used: then u = 1e-145 e0 and H = I - 2 e0 e0^T, a reflection - still an orthogonal similarity, and every
        // intermediate stays finite for |A| < 1e160 (p = A u / hh is 2 A[:, 0] 1e145).  e2[k] below keeps the unfloored value.
        double nrm = sqrt_nz(max_raw(nn, 1e-290));
        double u[n];
        u[0] = alpha + copysign_d(nrm, alpha);
        static_for<n - 1>([&](auto t) { u[decltype(t)::value + 1] = m[tri(k + 2 + decltype(t)::value, k)]; });
        double ihalf = rcp(__builtin_fma(u[0], u[0], sig));       // 1 / |u|^2
        double inv_hh = ihalf + ihalf;
        // p = A22 u / hh   (A22 symmetric, lower stored)
        double p[n];
        static_for<n>([&](auto rr) {
            constexpr int r = decltype(rr)::value;
            double acc = 0.0;
            static_for<n>([&](auto cc) {
                constexpr int c = decltype(cc)::value;
                constexpr int hi = r > c ? r : c, lo = r > c ? c : r;
                acc = __builtin_fma(m[tri(k + 1 + hi, k + 1 + lo)], u[c], acc);
            });
            p[r] = acc * inv_hh;
        });
        double up = 0.0;
        static_for<n>([&](auto rr) { up = __builtin_fma(u[decltype(rr)::value], p[decltype(rr)::value], up); });
        double kap = 0.5 * up * inv_hh;
        // q = p - kap u ;  A22 -= u q^T + q u^T
        static_for<n>([&](auto rr) { p[decltype(rr)::value] = __builtin_fma(-kap, u[decltype(rr)::value], p[decltype(rr)::value]); });
        static_for<n>([&](auto rr) {
            constexpr int r = decltype(rr)::value;
            static_for<r + 1>([&](auto cc) {
                constexpr int c = decltype(cc)::value;
                double v = m[tri(k + 1 + r, k + 1 + c)];
                v = __builtin_fma(-u[r], p[c], v);
                v = __builtin_fma(-p[r], u[c], v);
                m[tri(k + 1 + r, k + 1 + c)] = v;
            });
        });
        dg[kOutRev ? D - 1 - k : k] = m[tri(k, k)];
        e2[kOutRev ? D - 2 - k : k] = nn;
    });
    if constexpr (D >= 2) {
        dg[kOutRev ? 1 : D - 2] = m[tri(D - 2, D - 2)];
        double e = m[tri(D - 1, D - 2)];
        e2[kOutRev ? 0 : D - 2] = e * e;
    }
    dg[kOutRev ? 0 : D - 1] = m[tri(D - 1, D - 1)];
    e2[D - 1] = 0.0;
}

#ifndef GABO_QL_RCP
// Reciprocal used inside the QL sweep: rcp_nr1 (seed + one Newton step, 2^-47) or rcp (seed + cubic correction, ~1 ulp).
// t = 1 / (p r) only scales the plane rotation of a step (c = p^2 t, s = b p t, c + s = 1 up to its error), i.e. a relative
// perturbation of 7e-15 per step on top of the recurrence's own rounding.  Measured on the benchmark distribution (N = 4096, d = 10,
// tools/ab_pairwise.py): worst relative error of d^2 against LAPACK 1.5e-13 instead of 1.0e-13, kernel 2.72 -> 2.66 ms.
#define GABO_QL_RCP rcp_nr1
#endif

// sqrt(x), x > 0, to ~2^-24: the bare hardware seed.  For the Wilkinson SHIFT only - its accuracy sets the convergence RATE of a sweep,
// never the eigenvalues: a shift that misses the Wilkinson value by 1e-7 of the root still contracts e^2 by ~1e-14 per sweep once the
// cubic phase has brought it there.  Wave-level simulation (tools/sim/ql_lookahead_sim.py with the root perturbed): 124.3 -> 125.7 sweep
// steps and 19.3 -> 19.7 sweeps per wave for 4 instructions less per sweep than a seed with one coupled Goldschmidt step (2^-46);
// measured 2.455 -> 2.440 ms.
__device__ __forceinline__ double sqrt_shift(double x) {
    return x * __builtin_amdgcn_rsq(x);
}

// p = gamma^2 / c feeds the next rotation as a divisor and must never be exactly 0 (a shift that hit an eigenvalue exactly gives
// gamma = 0): p = a * b + 1e-150 (p = a b >= 0 here), so that the product p r below stays a normal number - a perturbation far below
// rounding that only registers when p < 1e-134.  Replaces LAPACK's `c == 0` branch with no instruction of its own.
__device__ __forceinline__ double mul_floor_p(double a, double b) {
    double r;
    asm("v_fma_f64 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "s"(1e-150));
    return r;
}

// Eigenvalues of the symmetric tridiagonal (dg, sqrt(e2)) in place in dg (unordered).  Root-free QL, Wilkinson shift.
//
// Lane-uniform structure on purpose: stage l deflates e2[l]; every sweep of stage l runs the full recurrence from
// D-2 down to l with NO per-lane interior-split search, so the unrolled steps carry no predicates or branches and the
// only divergence is the iteration count per stage.  An interior off-diagonal that is (or becomes) negligible is
// simply swept through: the recurrence restarts by itself there (c -> 1, s -> 0).  p > 0 is an invariant (see
// `mul_floor_p`), hence r = p + bb > 0 and c = p / r > 0: no division can see a zero.  The last 2x2 block is closed form.
template <int D, int ORIENT = kQlOrientPerLane, int CTL = kQlCtlPlain>
__device__ __forceinline__ void tridiag_eigenvalues(double (&dg)[D], double (&e2)[D], const double eps2_arg = 0.0) {
    static_assert(CTL == kQlCtlPlain || ORIENT != kQlOrientPerLane, "the strict path keeps the plain sweep control");
    constexpr bool kDenormalZero = (CTL & kQlCtlDenormalZero) != 0, kHwSqrt = (CTL & kQlCtlHwSqrt) != 0, kStageThreshold = (CTL & kQlCtlStageThreshold) != 0;
    // Deflation threshold on e2[l] / |d[l] d[l+1]|.  LAPACK uses eps^2 (4.9e-32); 1e-20 is enough here: dropping an
    // off-diagonal e perturbs a SYMMETRIC function of the eigenvalues (sum log^2) only to second order, ~e^2 f'' <= 1e-20,
    // whatever the gap, and the iteration converges cubically, so the looser test saves the last sweep of many stages
    // (measured: 1e-32 -> 1e-22: -6 % sweep steps; 1e-22 -> 1e-20: another -1 % of the kernel's time; worst-case error of d^2 on the
    // benchmark distribution 1e-13 in all three, tools/sim/ql_lookahead_sim.py).
#ifndef GABO_QL_EPS2
#define GABO_QL_EPS2 1e-20
#endif
    // eps2_arg > 0: the caller's threshold (wave-uniform).  The Gaussian kernel VALUE without a distance output tolerates a looser one: dropping
    // an off-diagonal e^2 <= eps2 |d d'| perturbs sum log^2 lambda by e^2 f'' in ABSOLUTE terms (second order: up to ~50 eps2 for eigenvalues
    // between 0.01 and 100), i.e. K = exp(-beta d^2) by beta times that relative - 4e-12 at the 1e-14 in use, inside what the tests allow such a
    // value; what the strict 1e-20 protects is the RELATIVE accuracy of a tiny distance (nearly identical pairs: d ~ 1e-5, d^2 ~ 1e-10), which
    // only the distance and Laplace outputs expose (spd_pairwise_body.hpp, GABO_QL_EPS2_GAUSS).
    const double eps2 = eps2_arg > 0.0 ? eps2_arg : GABO_QL_EPS2;
    // QL deflates at the top (index 0) and converges fastest when the small end of a graded matrix sits there (LAPACK's
    // dsterf chooses QL vs QR on the same criterion): reverse the arrays per lane when |d[0]| > |d[D-1]|.  Measured on the
    // benchmark distribution: -9 % QL sweep steps per wave against never reversing, for ~40 selects.
    // The strict path (kQlOrientPerLane) keeps this rule: it serves every launch that is not the Gram of a GP fit (distance and Laplace
    // outputs, a distance next to the values, d = 12), so it cannot assume a grading, and a fixed end that is wrong costs more than the rule
    // saves (+13 % sweep steps at d = 10); the bits of its results are pinned by tests/test_gpu_pairwise_gauss_finish.py.  A caller
    // that fixes the orientation has had tridiagonalize<D, ORIENT> put the end of the reduction at index 0 already: on
    // the Gram of a GP fit the rule agrees with that for three lanes in four and the fourth sets the pace of its wave's first stage, so the
    // constant is both cheaper (no compare, no 2 (D - 1) selects of a double) and better (tools/sim/ql_orientation_sim.py, profiles/orient_sim.txt:
    // d = 10, 118.7 -> 111.3 sweep steps per wave).
    if constexpr (D >= 3 && ORIENT == kQlOrientPerLane) {
        const bool flip = __builtin_fabs(dg[0]) > __builtin_fabs(dg[D - 1]);
        static_for<D / 2>([&](auto ii) {
            constexpr int i = decltype(ii)::value;
            double a = dg[i], b = dg[D - 1 - i];
            dg[i] = flip ? b : a;
            dg[D - 1 - i] = flip ? a : b;
        });
        static_for<(D - 1) / 2>([&](auto ii) {
            constexpr int i = decltype(ii)::value;
            double a = e2[i], b = e2[D - 2 - i];
            e2[i] = flip ? b : a;
            e2[D - 2 - i] = flip ? a : b;
        });
    }
    static_for<D - 2>([&](auto ll) {
        constexpr int l = decltype(ll)::value;
        for (int it = 0; it < 60; ++it) {
            // Look-ahead shift.  The 64 lanes of a wave share the instruction stream, so stage l lasts until the SLOWEST lane has
            // deflated e2[l]; a lane that is done would idle through the other lanes' sweeps (measured on the benchmark
            // distribution: 180 sweep steps per wave against 128 per lane).  Instead it keeps sweeping with the wave - same
            // extent D-2 .. l, no per-lane masks in the unrolled steps - but takes its Wilkinson shift from block l+1, i.e. it
            // already works on its NEXT stage.  Its deflated e2[l] is set to exactly 0 first: then the steps below block l+1 pass
            // through as the identity (bb = 0 => c = 1, s = 0) whatever p has become; with a merely negligible e2[l] a tiny p at
            // the end of a converged sweep makes s = bb / (p + bb) large and the pass-through re-couples the deflated row
            // (tools/sim/ql_lookahead_sim.py: 180 -> 189 steps without the zeroing, 180 -> 129 with it).
            constexpr bool kAhead = l + 1 <= D - 3;           // stage l has a block l + 1 to look ahead to
            const double thr0 = eps2 * __builtin_fabs(dg[l] * dg[l + 1]);
            const bool done0 = e2[l] <= thr0;
            // the WAVE leaves stage l when its last lane has deflated e2[l] (a per-lane `break` would keep the wave here until every lane
            // had finished its look-ahead work too, at stage l's longer sweep extent).  Every active lane done: the mask of `done0` against the
            // mask of the active lanes - one vector compare (`ballot(!done0)` costs a second, NaN-aware one).
            if (__builtin_amdgcn_ballot_w64(done0) == __builtin_amdgcn_ballot_w64(true)) break;
            double e2l;
            if constexpr (kDenormalZero && kAhead) {
                // the high word alone, in place: the denormal that is left makes s = bb / (p + bb) <= 4.3e-314 / 1e-150 (p is floored, mul_floor_p),
                // the identity as far as any double of the sweep can tell, and a lane that sits the sweep out passes the test again with it
                e2[l] = __hiloint2double(done0 ? 0 : __double2hiint(e2[l]), __double2loint(e2[l]));
                e2l = e2[l];
            } else {
                e2l = done0 ? 0.0 : e2[l];                   // (e2[l] itself is rewritten at the end of the sweep: s p = 0 for these lanes)
            }
            double sa = dg[l], sb = dg[l + 1], se = e2l;
            bool idle = false;
            if constexpr (kAhead) {
                const bool done1 = e2[l + 1] <= (kStageThreshold ? thr0 : eps2 * __builtin_fabs(dg[l + 1] * dg[l + 2]));
                idle = done0 && done1;                      // nothing to do within the look-ahead window: sit this sweep out
                sa = done0 ? dg[l + 1] : sa;
                sb = done0 ? dg[l + 2] : sb;
                se = done0 ? e2[l + 1] : se;
            } else {
                idle = done0;
            }
            // (`if (!idle)` around the sweep, not `if (idle) continue;`: a per-lane `continue` makes the loop itself divergent for the compiler,
            // which then keeps a per-lane loop state in a VGPR - three v_mov_b32 and two v_cmp_*_i32 per sweep; this way the loop is
            // wave-uniform, its counter and exit live on the scalar unit, and only the sweep is under the lane mask)
            if (!idle) {
                // Wilkinson shift from the leading 2x2: sigma = d_l - e2_l / (delta + sign(delta) sqrt(delta^2 + e2_l)),
                // evaluated division-free as d_l - sign(delta) (sqrt(delta^2 + e2_l) - |delta|).  The cancellation of the
                // rationalised form only costs ~eps |delta| in the SHIFT, which changes the convergence rate, never the result.
                double delta = 0.5 * (sb - sa);
                const double root2 = __builtin_fma(delta, delta, se);
                double root;
                if constexpr (kHwSqrt) root = __builtin_amdgcn_sqrt(root2);
                else root = sqrt_shift(root2);
                double sigma = sa - copysign_d(root - __builtin_fabs(delta), delta);
                double gamma = dg[D - 1] - sigma;
                double p = mul_floor_p(gamma, gamma);
                double s = 0.0;
                static_for_down<D - 2, l>([&](auto ii) {
                    constexpr int i = decltype(ii)::value;
                    double bb = (i == l) ? e2l : e2[i];
                    double r = p + bb;
                    if constexpr (i != D - 2) e2[i + 1] = s * r;
                    // one reciprocal serves the step: t = 1/(p r)  =>  1/r = t p.  With f = p (a_i - sigma) - b gamma_old:
                    //   gamma' = c (a_i - sigma) - s gamma_old = f / r = f (t p),     p' = gamma'^2 / c = gamma'^2 r / p = f^2 t
                    // (c itself is never needed; two instructions less per step than forming c, gamma r and (gamma r)^2 t)
                    double t = GABO_QL_RCP(p * r);
                    double ir = t * p;
                    s = bb * ir;
                    double oldgam = gamma;
                    double al = dg[i];
                    double f = __builtin_fma(p, al - sigma, -(bb * oldgam));
                    gamma = ir * f;
                    dg[i + 1] = oldgam + (al - gamma);
                    p = mul_floor_p(f * t, f);
                });
                e2[l] = s * p;
                // (a look-ahead lane's deflated d_l comes back as sigma + (d_l - sigma): a perturbation of an ulp of |sigma| <= |T|, the
                // size of the backward error of every other step of the sweep)
                dg[l] = sigma + gamma;
            }
        }
    });
    // trailing 2x2 [[a, b], [b, c]]: rt1 = larger-magnitude root, rt2 = det / rt1
    {
        double a = dg[D - 2], b2 = e2[D - 2], cc = dg[D - 1];
        double sm = a + cc, df = a - cc;
        double rt = sqrt_pos(__builtin_fma(df, df, 4.0 * b2));
        double r1 = 0.5 * (sm + copysign_d(rt, sm));
        double det = __builtin_fma(a, cc, -b2);
        dg[D - 2] = r1;
        dg[D - 1] = (r1 == 0.0) ? 0.0 : det * rcp(r1);
    }
}

}  // namespace gabo
