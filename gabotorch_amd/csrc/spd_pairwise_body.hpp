// Kernel templates of the SPD pairwise Gram (see spd_pairwise.hip for the description).
#pragma once
#include "gabo_device.hpp"
#include "spd_eig.hpp"
#include "spd_prep.hpp"
#include "gabo_mirror.hpp"
#include "spd_generic.hpp"
#include "gabo_log_tab.hpp"
#include "gabo_exp_tab256.hpp"
#include "gabo_acosh2_table.hpp"
#include "../../include/gabo_hip.h"

#ifndef GABO_PAIR_WAVES
#define GABO_PAIR_WAVES 2  /* waves per SIMD the pairwise kernel is register-budgeted for */
#else
#define GABO_PAIR_WAVES_FORCED 1  /* A/B builds: one budget for every instantiation (spd_pair_gauss_only_waves) */
#endif

namespace gabo {

// The lane's column of G as a pointer into the GLOBAL address space.  The row loop launders this pointer (so that the G loads are not
// hoisted); laundering a plain `const double*` makes it a generic pointer, the loads become flat_load - which count in vmcnt AND lgkmcnt and
// may return out of order - and every wait in front of their uses becomes `s_waitcnt vmcnt(0) lgkmcnt(0)`, a full drain four times per row.
// With the address space kept the loads are global_load and the waits are the partial vmcnt(N) of in-order returns.
typedef const double __attribute__((address_space(1)))* spd_gcol_ptr;

// sum_k log^2(lambda_k) of M = C C^T with C = W * G (both lower triangular, W wave-uniform, G per lane)
// The same column through a buffer descriptor: address = wave-uniform base (in the descriptor) + the lane's byte offset + a SCALAR offset per
// entry.  The 55 entry offsets k * n2 * 8 are then computed on the scalar unit; with a vector pointer each load needs its own 64-bit vector
// add (v_lshl_add_u64), 54 of them per pair at d = 10.  Usable while T * n2 * 8 < 2^31.
struct SpdGcolBuffer {
    __amdgpu_buffer_rsrc_t rsrc;
    int voff;            // laundered once per row (keeps the loads inside the row loop)
    int stride_bytes;    // n2 * 8
    __device__ __forceinline__ double operator[](int k) const {
        return __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(rsrc, voff, k * stride_bytes, 0));
    }
};
struct SpdGcolPointer {
    spd_gcol_ptr p;
    int64_t stride;
    __device__ __forceinline__ double operator[](int k) const { return p[(int64_t)k * stride]; }
};

// The staged form of the congruence (ai_sumsq with AHEAD > 0): for an instantiation budgeted for more waves per SIMD than the compiler's own
// schedule of the congruence fits (spd_pair_gauss_only_waves).  Left alone, the scheduler takes the row of W once, from its last row to its
// first, and to do so issues most of the 55 loads of G at the top of the pair and holds their destinations beside the growing m[] (194 VGPRs at
// d = 10); squeezed by the register budget alone it gives vector registers back by stretching the scalar live ranges of the W row until they spill
// to lanes (117 scalar spills, 346 lane moves per pair).  Here both operands arrive in stages, and scheduling barriers keep the stages apart:
//   G  column by column, AHEAD columns in front of the column being consumed;
//   W  in groups of consecutive rows of one column's products, at most WLIM doubles a group, one group in front of the group being consumed.  An
//      entry W[r][k] serves the columns 0 .. k and is read again for each (from the scalar cache: 220 doubles per pair at d = 10 instead of 55),
//      so that no more than two groups are ever live in scalar registers.  Scalar loads return out of order - a wait on one is a wait on all -
//      so a group is waited for BEFORE the next one is issued.
// The arithmetic - every operation, its operands and the order along every sum - is that of the plain form.
template <int D, int WLIM>
struct SpdWGroups {
    int n = 0;
    int col[tri_size(D)] = {}, r0[tri_size(D)] = {}, r1[tri_size(D)] = {};      // group g: rows r0 .. r1 - 1 of column col, columns descending
    constexpr SpdWGroups() {
        static_assert(WLIM >= D, "a row of the first column must fit a group");
        for (int c = D - 1; c >= 0; --c) {
            for (int r = c; r < D;) {
                int sum = 0;
                col[n] = c, r0[n] = r;
                while (r < D && sum + (r - c + 1) <= WLIM) sum += r - c + 1, ++r;
                r1[n++] = r;
            }
        }
    }
};
#ifndef GABO_PAIR_WLIM
#define GABO_PAIR_WLIM 16
#endif
template <int D, int AHEAD, class GCOL>
__device__ __forceinline__ void ai_congruence_staged(const double* __restrict__ W, const GCOL& Gj, double (&m)[tri_size(D)]) {
    constexpr SpdWGroups<D, (GABO_PAIR_WLIM < D ? D : GABO_PAIR_WLIM)> kG{};
    double gq[D][D];         // gq[col][k - col] = G[k][col]: at most AHEAD + 1 columns live
    double wq[2][D][D];      // wq[group & 1][r][k] = W[r][k]
    double c[D];             // the current column of C, c[r - col]
    auto issue_g = [&](auto ss) {
        constexpr int col = D - 1 - decltype(ss)::value;
        static_for<D - col>([&](auto kk) { gq[col][decltype(kk)::value] = Gj[tri(col + decltype(kk)::value, col)]; });
    };
    auto issue_w = [&](auto gg) {
        constexpr int g = decltype(gg)::value, col = kG.col[g], r0 = kG.r0[g], r1 = kG.r1[g];
        // a group's loads are its own, not merged with an earlier group's of the same entries: a laundered pointer - in the CONSTANT address
        // space, or the loads behind it become flat loads into vector registers (see spd_gcol_ptr)
        typedef const double __attribute__((address_space(4)))* wrow_ptr;
        wrow_ptr Wg = (wrow_ptr)W;
        asm volatile("" : "+s"(Wg));
        static_for<r1 - r0>([&](auto rr) {
            constexpr int r = r0 + decltype(rr)::value;
            static_for<r - col + 1>([&](auto kk) { wq[g & 1][r][col + decltype(kk)::value] = Wg[tri(r, col + decltype(kk)::value)]; });
        });
    };
    static_for<(AHEAD < D ? AHEAD : D)>(issue_g);
    issue_w(std::integral_constant<int, 0>{});
    static_for<kG.n>([&](auto gg) {
        constexpr int g = decltype(gg)::value, col = kG.col[g], r0 = kG.r0[g], r1 = kG.r1[g];
        if constexpr (r0 == col && D - 1 - col + AHEAD < D) issue_g(std::integral_constant<int, D - 1 - col + AHEAD>{});
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_waitcnt(0xc07f);      // lgkmcnt(0): group g of W has arrived
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (g + 1 < kG.n) issue_w(std::integral_constant<int, g + 1>{});
        static_for<r1 - r0>([&](auto rr) {
            constexpr int r = r0 + decltype(rr)::value;
            double acc = wq[g & 1][r][col] * gq[col][0];
            static_for<r - col>([&](auto kk) {
                constexpr int k = col + 1 + decltype(kk)::value;
                acc = __builtin_fma(wq[g & 1][r][k], gq[col][k - col], acc);
            });
            c[r - col] = acc;
        });
        // the column's rank-1 update once the column of C is whole and the column of G dead (updating row by row would hold G's column beside
        // the entries of M that column 0 creates: 20 registers more at the peak); entry (r, q) of M is first touched by column q
        if constexpr (r1 == D) {
            __builtin_amdgcn_sched_barrier(0);
            static_for<D - col>([&](auto rr) {
                constexpr int r = col + decltype(rr)::value;
                static_for<r - col + 1>([&](auto qq) {
                    constexpr int q = col + decltype(qq)::value;
                    m[tri(r, q)] = col == q ? c[r - col] * c[q - col] : __builtin_fma(c[r - col], c[q - col], m[tri(r, q)]);
                });
            });
        }
    });
    __builtin_amdgcn_sched_barrier(0);
}

// The constants of log_tab by one scalar load per pair, behind the eigenvalue iteration, where the scalar registers are free.  LogTabRegs::load()
// pins them in vector registers, and the compiler forms them once, in front of the row loop: 16 registers held across the whole pair, which
// the staged form's budget does not have.  The same eight doubles.
__constant__ double kLogTabRegs[8] = {1.41421356237309504880, 1.0 / 7.0, -1.0 / 6.0, 0.2, -0.25, 1.0 / 3.0, 6.93147180369123816490e-01,
                                      1.90821492927058770002e-10};
__device__ __forceinline__ LogTabRegs log_tab_regs_scalar() {
    typedef const double __attribute__((address_space(4)))* const_ptr;
    const_ptr p = (const_ptr)kLogTabRegs;
    asm volatile("" : "+s"(p));
    LogTabRegs t;
    t.sqrt2 = p[0], t.c7 = p[1], t.c6 = p[2], t.c5 = p[3], t.c4 = p[4], t.c3 = p[5], t.ln2_hi = p[6], t.ln2_lo = p[7];
    return t;
}

template <int D, int ORIENT = kQlOrientPerLane, int CTL = kQlCtlPlain, int AHEAD = 0, class GCOL>
__device__ __forceinline__ double ai_sumsq(const double* __restrict__ W, const GCOL& Gj, const double* __restrict__ ltab, const double eps2 = 0.0) {
    constexpr int T = tri_size(D);
    // Column `col` of C = W G depends only on column `col` of G:  C[r][col] = sum_{k=col..r} W[r][k] G[k][col].
    // M = C C^T = sum_col C[:,col] C[:,col]^T, so M is accumulated by rank-1 updates and C is never held whole:
    // live state is M (T doubles) + one column of C + one column of G.
    // (kQlOrientLast, whose reduction starts at the last row of M, takes the columns from the last to the first: the order in which the
    // reduction wants M is then the order in which it becomes final.  d = 10 listing: with the columns in ascending order that form has 72 scalar spills
    // and 208 lane moves in the pair body and 233 VGPRs, in descending order none and 194 - against 216 for the other two orientations.)
    constexpr bool kDescending = ORIENT == kQlOrientLast;
    double m[T];
    if constexpr (AHEAD > 0) {
        static_assert(kDescending, "the staged congruence takes the columns from the last to the first");
        ai_congruence_staged<D, AHEAD>(W, Gj, m);
    } else
    static_for<D>([&](auto cc) {
        constexpr int col = kDescending ? D - 1 - decltype(cc)::value : decltype(cc)::value;
        double g[D - col], c[D - col];
        static_for<D - col>([&](auto kk) { g[decltype(kk)::value] = Gj[tri(col + decltype(kk)::value, col)]; });
        static_for<D - col>([&](auto rr) {
            constexpr int r = col + decltype(rr)::value;
            double acc = W[tri(r, col)] * g[0];
            static_for<r - col>([&](auto kk) {
                constexpr int k = col + 1 + decltype(kk)::value;
                acc = __builtin_fma(W[tri(r, k)], g[k - col], acc);
            });
            c[r - col] = acc;
        });
        static_for<D - col>([&](auto rr) {
            constexpr int r = col + decltype(rr)::value;
            static_for<r - col + 1>([&](auto qq) {
                constexpr int q = col + decltype(qq)::value;
                // column 0 touches every entry of M first: it initialises, the later columns accumulate (descending: entry (r, q) is first
                // touched by column q)
                m[tri(r, q)] = (kDescending ? col == q : col == 0) ? c[r - col] * c[q - col] : __builtin_fma(c[r - col], c[q - col], m[tri(r, q)]);
            });
        });
    });
    double dg[D], e2[D];
    tridiagonalize<D, ORIENT>(m, dg, e2);
    tridiag_eigenvalues<D, ORIENT, CTL>(dg, e2, eps2);
    double s = 0.0;
    const LogTabRegs lr = AHEAD > 0 ? log_tab_regs_scalar() : LogTabRegs::load();
    static_for<D>([&](auto kk) { double lg = log_tab(dg[decltype(kk)::value], lr, ltab); s = __builtin_fma(lg, lg, s); });
    return s;
}

// d = 2 (the latent space of the nested kernels, config 5) in closed form with ONE logarithm per pair: M = C C^T, C = W G lower triangular, so
// det M = (c00 c11)^2 exactly and log lambda_- = log det M - log lambda_+; log det M = 2 (log(w00 w11) + log(g00 g11)) is a per-POINT quantity
// (`lw2`: the row's, wave-uniform; `lg2`: the lane's column's, computed once before the row loop).  lambda_+ = (tr + sqrt((m00 - m11)^2 + 4 m10^2)) / 2
// has no cancellation.  ~45 instructions per pair against ~120 for the generic path (two logs, the 2x2 QL finish, three operand loads).
struct Spd2Col {
    double g00, g10, g11, lg;
};
__device__ __forceinline__ double ai_sumsq2(const double* __restrict__ W, const Spd2Col& g, double lw, const LogTabRegs& lr,
                                            const double* __restrict__ ltab, double tiny) {
    const double c00 = W[0] * g.g00, c11 = W[2] * g.g11;
    const double c10 = __builtin_fma(W[1], g.g00, W[2] * g.g10);
    const double m00 = c00 * c00, m10d = (c10 + c10) * c00, m11 = __builtin_fma(c10, c10, c11 * c11);
    const double tr = m00 + m11, df = m00 - m11;
    // (`tiny` = 1e-290 keeps the seed-based square root away from 0 when M is a multiple of the identity)
    const double root = sqrt_nz(__builtin_fma(df, df, __builtin_fma(m10d, m10d, tiny)));
    const double l1 = log_tab(0.5 * (tr + root), lr, ltab);
    const double l2 = __builtin_fma(2.0, lw + g.lg, -l1);
    return __builtin_fma(l1, l1, l2 * l2);
}

__device__ __forceinline__ double finish(double dist, double beta, int mode) {
    if (mode == GABO_OUT_DISTANCE) return dist;
    if (mode == GABO_OUT_LAPLACE) return exp(-(dist * beta));   // kernels_spd.py:185
    return exp(-((dist * dist) * beta));                        // kernels_spd.py:94-98
}

// 1-D grid, block id -> (batch, row chunk of `rows` rows, column group of blockDim.x columns), column group fastest
#ifndef GABO_PAIR_TWO_WAVE_MAX_DIM
// Two waves per SIMD (256 VGPRs) up to d = 14: at d = 13 / 14 the compiler spills 10 / 24 doubles per lane to scratch, which costs far less than
// the halved issue rate of a lone wave (8.5 instead of 4.5 cycles per instruction): N = 4096 Gram 5.92 -> 4.33 ms and 7.77 -> 5.87 ms; d = 15: 9.9 ->
// 9.8, d = 16: 11.9 -> 14.1 (one wave per SIMD from 15 on).
#define GABO_PAIR_TWO_WAVE_MAX_DIM 14
#endif
// Deflation threshold of the QL iteration for Gaussian values alone (tridiag_eigenvalues has the argument): a dropped off-diagonal e^2 <= eps2 |d d'|
// moves d^2 = sum log^2 lambda by e^2 f'' in ABSOLUTE terms, hence K = exp(-beta d^2) by beta times that relative.  With eigenvalues of M between
// 0.01 and 100 (the benchmark's generator) |d d'| and f'' make it up to ~50 eps2 (measured: K moves by up to 2.2e-11 relative at 1e-13, 4e-12 at 1e-14).
// The largest decade that leaves every block of tests/test_gpu_pairwise_gauss_finish.py at or below half of its bound is 1e-14: at 1e-13 the test
// still passes, but its benchmark block stands at 0.7 of the bound and its block of nearly identical pairs (M = I + O(1e-6), d^2 ~1e-10) at 0.8 - 1.1
// (profiles/gaussonly_ab_items.txt); at 1e-12 the dropped entries are a visible part of such a d^2 itself.  N = 4096, d = 10: 1e-15 -> 1e-14 is -0.6 %.
#ifndef GABO_QL_EPS2_GAUSS
#define GABO_QL_EPS2_GAUSS 1e-14
#endif
// Two instantiations per dimension, chosen by launch_spd_ai from what it knows at launch time:
//   <D, false, false>  every output mode, the optional distance output and both forms of the G loads behind run-time branches;
//   <D, true, true>    Gaussian values alone (no distance leaves the kernel) through the buffer form of the G loads - the Gram of a GP fit,
//                      the launch the benchmark times.  One pair body, one exp, and a row loop that keeps nothing in scalar registers but
//                      the row of W, the buffer descriptor and the loop's own state (see the loop).
// The arithmetic of a pair is the same in both.
// d = 12 keeps the general instantiation for every launch: there the W row alone is 156 scalar registers, the compiler spills it in both forms
// (172 against 313 / 2 spills), and the Gaussian-only row loop reads it back with MORE lane moves than one form of the general kernel (569
// v_readlane_b32 against 785 / 2): measured 1.5 % slower at N = 4096 (3.36 -> 3.41 ms) where d = 5, 10, 13 and 14 gain 1 - 4 %.
constexpr bool spd_pair_gauss_only_instantiated(int d) { return d > 2 && d != 12; }
// Orientation of the eigenvalue iteration in the Gaussian-only instantiation (QlOrient, spd_eig.hpp): a compile-time fact per dimension instead
// of the per-lane reversal rule of the strict path.  Wave-level simulation on the benchmark's generator (tools/sim/ql_orientation_sim.py,
// profiles/orient_sim.txt; QL VALU per wave-row at 16 per sweep step + 25 per sweep, the rule's own 4 (D - 1) + 1 instructions not counted):
//     d     per-lane rule   kQlOrientCol0   kQlOrientLast   reduction from the last column, its FIRST entries at index 0
//     5          635             613             604             705
//    10         2360            2240            2215            2670
//    13         3735            3652            3634            4322
//    16         5499            5325            5324            5984
//    20         8193            8020            7977            9112
// kQlOrientLast is the best fixed form, or within 0.1 % of it, at every d from 4 to 20 (d = 3, one QL stage of two steps: 226 / 230 / 215); no stage
// of any wave takes more than 7 sweeps of the 60 allowed in it, on the benchmark's generator, on nearly identical pairs and at eigenvalue ratio
// 1e6 alike.  The last column shows why this is a table and not a guess: the wrong end costs 8 - 16 %.  Measured (N = 4096 Gram, per-lane rule -> kQlOrientCol0 ->
// kQlOrientLast, profiles/orient_ab_bench.txt and profiles/orient_ab_elsewhere.txt): d = 5 0.600 -> 0.580 -> 0.580 ms, d = 10 2.148 -> 2.096 -> 2.094,
// d = 13 3.982 -> 3.900 -> 3.876, d = 14 5.286 -> 5.162 -> 5.344, d = 16 10.83 -> 10.69 -> 9.18, d = 18 16.02 -> 15.97 -> 12.16.  d = 14 keeps the
// reduction from column 0: it is the largest dimension budgeted for two waves per SIMD, the compiler spills vector registers to scratch there in
// every form, and kQlOrientLast measures 1 % slower than the per-lane rule there where kQlOrientCol0 is 2.4 % faster.  (From d = 15 on, one wave per SIMD, most of kQlOrientLast's gain
// is not the iteration's but the register budget's: with the congruence in descending column order - ai_sumsq - the pair body needs fewer
// vector registers, d = 10: 216 -> 194, d = 11: 246 -> 232.)
// A dimension where no fixed form measures faster returns kQlOrientPerLane here and keeps the strict path's code.
#ifndef GABO_PAIR_ORIENT
constexpr int spd_pair_gauss_only_orientation(int d) { return d == 14 ? kQlOrientCol0 : kQlOrientLast; }
#else
constexpr int spd_pair_gauss_only_orientation(int d) { return GABO_PAIR_ORIENT; }      // (A/B builds: one form for every dimension)
#endif
// Sweep control of the eigenvalue iteration in the Gaussian-only instantiation (QlSweepCtl, spd_eig.hpp): all three cheaper forms, 25 -> 21 VALU per
// sweep in the d = 10 listing (profiles/sweepctl_isa_count.txt), same registers, no spill.  Wave-level simulation (tools/sim/ql_orientation_sim.py
// --sweepctl, profiles/sweepctl_sim.txt): d = 10, 111.3 -> 111.7 sweep steps and 17.34 -> 17.42 sweeps per wave-row - the idle test by stage l's
// threshold idles a few lanes a sweep early - for QL VALU 2215 -> 2152; no stage beyond 7 sweeps, worst error of sum log^2 against LAPACK 1.2e-12 -> 1.4e-12.
// Measured, N = 4096 Gram, parent / this form, two alternations per job (profiles/sweepctl_ab_elsewhere.txt): d = 3 0.239 / 0.239 -> 0.242 / 0.237 ms,
// d = 4 0.398 -> 0.391, d = 5 0.586 / 0.592 -> 0.583 / 0.586, d = 6 0.789 -> 0.773, d = 7 1.025 -> 1.015, d = 8 1.356 -> 1.340, d = 9 1.676 -> 1.657,
// d = 10 2.156 / 2.166 -> 2.140 / 2.145, d = 11 2.569 -> 2.547, d = 13 3.967 -> 3.934, d = 14 5.200 -> 5.166, d = 15 7.005 -> 6.931, d = 16 9.183 -> 9.029,
// d = 17 9.930 / 9.945 -> 9.917 / 9.955 (inside the spread), d = 18 12.18 -> 11.95, d = 19 14.91 -> 14.86.  d = 20 keeps the plain control: 20.906 / 20.924 -> 20.955 /
// 20.969 and, in a second job, 20.917 / 20.963 -> 20.950 / 20.986 - 0.15 % slower four times out of four.
// Not in the tree, with their numbers in CHANGELOG: the look-ahead operands selected by their high words alone (the compiler pays for every saved
// select with a move), one multiply shared by the two deflation tests (subsumed by the stage threshold), no idle test at all (fastest, but the
// neighbours of a lane that never converges then sweep 60 times per stage and lose a digit).
#ifndef GABO_PAIR_SWEEPCTL
constexpr int spd_pair_gauss_only_sweepctl(int d) { return d == 20 ? kQlCtlPlain : (kQlCtlDenormalZero | kQlCtlHwSqrt | kQlCtlStageThreshold); }
#else
constexpr int spd_pair_gauss_only_sweepctl(int d) { return GABO_PAIR_SWEEPCTL; }      // (A/B builds: one form for every dimension)
#endif
// Waves per SIMD the Gaussian-only instantiation is register-budgeted for (the general instantiation keeps GABO_PAIR_WAVES), and how many
// columns of G its congruence loads ahead (ai_sumsq's AHEAD; 0: the compiler's own schedule).  Two waves leave the vector pipe 93.7 % busy at
// d = 10 (194 VGPRs), three 97.5 % at d = 9 (168 VGPRs: the last dimension the compiler fits by itself; profiles/waves3_pmc_busy.txt).  The budget
// alone does not buy the third wave at d = 10: -DGABO_PAIR_WAVES=3 on the plain form gives 168 VGPRs with 117 scalar spills, 346 lane moves per
// pair and 44 bytes of scratch, and measures 1.7 % slower (2.160 -> 2.197 ms).  With the staged congruence the body needs 164, nothing spills, and
// the N = 4096 Gram goes 2.188 -> 2.142 and 2.118 -> 2.073 ms in two jobs, the same bits (profiles/waves3_ab_bench.txt).  d = 11 (232) is out of reach of this alone.
#ifndef GABO_PAIR_WAVES_FORCED
constexpr int spd_pair_gauss_only_waves(int d) { return d > GABO_PAIR_TWO_WAVE_MAX_DIM ? 1 : (d == 10 ? 3 : GABO_PAIR_WAVES); }
#else
constexpr int spd_pair_gauss_only_waves(int d) { return d > GABO_PAIR_TWO_WAVE_MAX_DIM ? 1 : GABO_PAIR_WAVES; }      // (A/B builds)
#endif
#ifndef GABO_PAIR_AHEAD
constexpr int spd_pair_gauss_only_ahead(int d) { return d == 10 && spd_pair_gauss_only_waves(d) == 3 ? 2 : 0; }
#else
constexpr int spd_pair_gauss_only_ahead(int d) { return d == 10 ? GABO_PAIR_AHEAD : 0; }      // (A/B builds)
#endif
template <int D, bool GAUSS_ONLY, bool BUFFER_ONLY>
__global__ __launch_bounds__(256, (GAUSS_ONLY ? spd_pair_gauss_only_waves(D) : (D > GABO_PAIR_TWO_WAVE_MAX_DIM ? 1 : GABO_PAIR_WAVES))) void spd_ai_pairwise_kernel(const double* __restrict__ Winv, const double* __restrict__ G,
                                                              double* __restrict__ out, double* __restrict__ dist_out_arg,
                                                              int64_t n1, int64_t n2,
                                                              int64_t w_batch_stride, int64_t g_batch_stride, int rows,
                                                              int col_blocks, int row_chunks, int64_t sym_tiles, double beta, int flags) {
    constexpr int T = tri_size(D);
    static_assert(GAUSS_ONLY == BUFFER_ONLY && (spd_pair_gauss_only_instantiated(D) || !GAUSS_ONLY), "instantiations that launch_spd_ai selects");
    const int mode = GAUSS_ONLY ? GABO_OUT_GAUSSIAN : (flags & GABO_OUT_MASK);
    double* const dist_out = GAUSS_ONLY ? nullptr : dist_out_arg;
    // small matrices (the latent spaces of the nested kernels: d = 2, 3): the finish is a visible part of a pair's ~140 instructions,
    // so the Gaussian mode uses the table-assisted exp of the write-bound kernels (17 instead of ~37 instructions).  From d = 5 on the
    // scalar registers are taken by the W row and OCML's exp measured faster than any variant with pinned coefficients.
    constexpr bool kTabExp = D <= 4;
    __shared__ double tab[kTabExp ? 64 : 1];
    __shared__ __attribute__((aligned(16))) double ltab[512];        // (c, -log c) pairs of log_tab
    for (int k = threadIdx.x; k < 512; k += blockDim.x) ltab[k] = kLogTab[k];
    double ec[6], ec3 = 0.0;
    if constexpr (kTabExp) {
        if (threadIdx.x < 64) tab[threadIdx.x] = kExp2Tab[threadIdx.x];
    }
    __syncthreads();
    if constexpr (kTabExp) {
        static_for<6>([&](auto k) { ec[decltype(k)::value] = kExpTabC[decltype(k)::value]; });
        ec3 = ec[3];
        asm volatile("" : "+v"(ec3));
    }
    int64_t cg, rc, b;
    if (flags & GABO_SYMMETRIC) {
        // Only tiles touching the upper triangle exist in the grid: column group cg owns row chunks
        // [0, min(row_chunks, ceil((cg+1)*cols/rows))).  Enumerating exactly those keeps consecutive block ids
        // (= consecutive XCDs) equally loaded; skipping blocks of a full grid instead leaves XCD 0 with 1/3 of
        // the work of XCD 7.
        const int64_t per_batch = sym_tiles;
        b = blockIdx.x / per_batch;
        int64_t t = blockIdx.x - b * per_batch;
        cg = 0;
        for (;;) {
            int64_t cnt = ((cg + 1) * (int64_t)blockDim.x + rows - 1) / rows;
            if (cnt > row_chunks) cnt = row_chunks;
            if (t < cnt) break;
            t -= cnt;
            ++cg;
        }
        rc = t;
    } else {
        const int64_t bid = blockIdx.x;
        cg = bid % col_blocks;
        rc = (bid / col_blocks) % row_chunks;
        b = bid / ((int64_t)col_blocks * row_chunks);
    }
    const int64_t j0 = cg * blockDim.x;
    const int64_t j = j0 + threadIdx.x;
    const int64_t jc = j < n2 ? j : n2 - 1;  // out-of-range lanes recompute the last column and do not store
    const int64_t i0 = rc * rows;
    const int64_t i1 = (i0 + rows < n1) ? i0 + rows : n1;
    // symmetric mode, tile straddling the diagonal: a wave whose 64 columns all lie left of the tile's first row has nothing
    // to store (i > j for every pair it would evaluate)
    if ((flags & GABO_SYMMETRIC) && j0 + (int64_t)(threadIdx.x | 63) < i0) return;
    const double* Gj = G + b * g_batch_stride + jc;
    double* ob = out + b * n1 * n2;
    // buffer form of the column loads (see SpdGcolBuffer): base = the wave's first column, lane offset = its (clamped) column
    const int64_t jw = j0 + (threadIdx.x & ~63);
    const bool use_buffer = BUFFER_ONLY || (D > 2 && (int64_t)T * n2 * 8 < (1ll << 31));
    SpdGcolBuffer gbuf;
    {
        const double* gw = G + b * g_batch_stride + (jw < n2 ? jw : n2 - 1);
        uint64_t a = (uint64_t)gw;
        a = ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(a >> 32)) << 32) | (uint32_t)__builtin_amdgcn_readfirstlane((int)a);
        gbuf.rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)a, 0, 0x7fffffff, 0x00020000);
        gbuf.voff = (int)((jc - (jw < n2 ? jw : n2 - 1)) * 8);
        gbuf.stride_bytes = (int)(n2 * 8);
    }
    // d = 2: the lane's column (3 numbers) and its log-determinant term stay in registers; lane r of every wave holds the term of row i0 + r
    Spd2Col col2;
    double lw_lane = 0.0, tiny = 1e-290;
    LogTabRegs lr2;
    if constexpr (D == 2) {
        lr2 = LogTabRegs::load();
        asm volatile("" : "+s"(tiny));
        col2.g00 = Gj[0];
        col2.g10 = Gj[n2];
        col2.g11 = Gj[2 * n2];
        col2.lg = log_tab(col2.g00 * col2.g11, lr2, ltab);
        int64_t ir = i0 + (threadIdx.x & 63);
        ir = ir < n1 ? ir : n1 - 1;
        const double* Wr = Winv + b * w_batch_stride + ir * T;
        lw_lane = log_tab(Wr[0] * Wr[2], lr2, ltab);
    }
    // deflation threshold of the QL iteration: 1e-20 where a distance leaves the kernel (distance and Laplace modes, or a distance output next to the
    // Gaussian values); GABO_QL_EPS2_GAUSS for Gaussian values alone (see tridiag_eigenvalues)
    double eps2 = (mode == GABO_OUT_GAUSSIAN && !dist_out) ? GABO_QL_EPS2_GAUSS : 0.0;
    asm volatile("" : "+s"(eps2));
    if constexpr (GAUSS_ONLY && BUFFER_ONLY) {
        // The row of W takes 2 T scalar registers (110 of about 100 at d = 10), so whatever else is live across a pair is spilled to lanes of a
        // vector register and read back with v_readlane_b32 (a VALU issue slot each, plus the s_nop behind it).  Hence nothing per row is
        // recomputed from (i, j, n2, flags, the batch): the W row and the lane's output address advance by constant steps, the row counter is
        // wave-uniform, and which rows a lane stores (all, none for a column beyond n2, those down to the diagonal in symmetric mode) is one
        // per-lane bound set before the loop, as in spd_ai_gauss2_kernel.
        const int nrows = __builtin_amdgcn_readfirstlane((int)(i1 - i0));
        const int64_t jrel = j - i0;
        const int rmax = j >= n2 ? -1 : ((flags & GABO_SYMMETRIC) ? (jrel < 0 ? -1 : (jrel > rows - 1 ? rows - 1 : (int)jrel)) : rows - 1);
        const double* W = Winv + b * w_batch_stride + i0 * T;
        char* orow = reinterpret_cast<char*>(ob + i0 * n2 + j);      // (never dereferenced by a lane with j >= n2)
        for (int r = 0; r < nrows; ++r, W += T) {
            SpdGcolBuffer gb = gbuf;
            asm volatile("" : "+v"(gb.voff));                  // the 55 G loads stay inside the row loop (see the general loop below)
            asm volatile("" : "+s"(gb.stride_bytes));
            const double s = ai_sumsq<D, spd_pair_gauss_only_orientation(D), spd_pair_gauss_only_sweepctl(D), spd_pair_gauss_only_ahead(D)>(W, gb, ltab, eps2);
            double val;
            if constexpr (kTabExp) {
                val = exp_neg_tab(-((s + 1e-15) * beta), ec, ec3, tab);
                val = s != s ? s : val;                    // (a NaN column of x2 stays NaN: see the general loop)
            } else {
                val = exp(-((s + 1e-15) * beta));
            }
            if (r <= rmax) *reinterpret_cast<double*>(orow) = val;
            orow += (unsigned)gb.stride_bytes;                 // n2 * 8 < 2^31 in the buffer form
        }
        return;
    }
    for (int64_t i = i0; i < i1; ++i) {
        const double* W = Winv + b * w_batch_stride + i * T;
        double s;
        if constexpr (D == 2) {
            const int lane = (int)(i - i0);
            const double lw = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(lw_lane), lane),
                                               __builtin_amdgcn_readlane(__double2loint(lw_lane), lane));
            s = ai_sumsq2(W, col2, lw, lr2, ltab, tiny);
        } else {
            // Launder the column pointer so the 55 G loads are NOT hoisted out of the row loop: keeping G resident costs
            // 110 VGPRs (one wave per SIMD less); re-reading it from L2 costs 28 KB per wave-row, which is noise here.
            if (use_buffer) {
                SpdGcolBuffer gb = gbuf;
                asm volatile("" : "+v"(gb.voff));
                asm volatile("" : "+s"(gb.stride_bytes));      // the entry offsets are recomputed per row on the scalar unit, not kept (the W row owns the SGPRs)
                s = ai_sumsq<D>(W, gb, ltab, eps2);
            } else {
                SpdGcolPointer gp{(spd_gcol_ptr)Gj, n2};
                asm volatile("" : "+v"(gp.p));
                s = ai_sumsq<D>(W, gp, ltab, eps2);
            }
        }
        double dist, val;
        if (mode == GABO_OUT_GAUSSIAN && !dist_out) {
            // exp(-beta sqrt(s + 1e-15)^2) (spd_utils_torch.py:120, kernels_spd.py:94-98) without the square root: sqrt(x)^2 = x to an ulp,
            // i.e. 1e-16 beta d^2 relative in K.  (OCML's exp stays: the register-table exp_neg of gabo_device.hpp measured 4 % SLOWER here,
            // 2.75 vs 2.63 ms - its 28 pinned coefficients cost more than the instructions they save once per pair.)
            dist = 0.0;
            if constexpr (kTabExp) {
                val = exp_neg_tab(-((s + 1e-15) * beta), ec, ec3, tab);
                val = s != s ? s : val;        // (the argument clamp of the table exp returns its bound for a NaN: a NaN column of x2 must stay NaN)
            } else {
                val = exp(-((s + 1e-15) * beta));
            }
        } else {
            dist = __builtin_sqrt(s + 1e-15);  // spd_utils_torch.py:120
            val = finish(dist, beta, mode);
        }
        // symmetric mode: only the upper triangle (i <= j) is stored; mirror_upper_kernel fills the rest afterwards,
        // so the result is exactly symmetric and the mirror writes are coalesced.
        if (j < n2 && (!(flags & GABO_SYMMETRIC) || i <= j)) {
            ob[i * n2 + j] = val;
            if (dist_out) dist_out[b * n1 * n2 + i * n2 + j] = dist;
        }
    }
}

// ---- d = 2, Gaussian kernel values only (no distance output): the Gram of the nested kernels' latent space (config 5) ----------------------
// A kernel of its own so that the row loop contains nothing else, and without a square root or a logarithm per pair (round 3):
// M = C C^T, C = W G lower triangular:  log lambda_+- = s +- delta  with  s = log sqrt(det M) = log(c00 c11) = log(w00 w11) + log(g00 g11)
// (a sum of per-POINT terms) and delta = acosh(tau),  tau = tr M / (2 sqrt(det M)) = 1 + ((c00 - c11)^2 + c10^2) / (2 c00 c11)  (sqrt(det M) =
// c00 c11 exactly; the numerator has no cancellation; 1 / (c00 c11) is again a product of per-point terms).  Hence
//     d^2 = log^2 lambda_+ + log^2 lambda_- = 2 s^2 + 2 A(tau),   A(tau) = acosh(tau)^2,
// and A is analytic on all of [1, inf) (the square removes acosh's square-root singularity at 1: A = 2u - u^2/3 + ..., u = tau - 1), so it
// comes from a table: slot = low exponent bits + top 4 mantissa bits of tau (one bit-field extract), local variable t = tau minus tau with its lower bits cleared (exact),
// degree 7, coefficients by four ds_read_b128 (csrc/gabo_acosh2_table.hpp, tools/sim/fit_acosh2_table.py: as accurate as the sqrt + log form,
// 2e-15 of max(1, d^2) on the benchmark distribution).  The block's copy of the table is pre-multiplied by -512 beta / ln2 (and carries the
// 1e-15 of spd_utils_torch.py:120 in its constant terms), the per-point logarithms by sqrt(512 beta / ln2): Y = -s'^2 + Y_A is -beta (d^2 +
// 1e-15) in units of ln2/256, whose exp needs no argument reduction products (Y - rint(Y) is exact).  ~36 instructions per pair where the
// sqrt + log form had ~64.  tau >= 2^12 (eigenvalue ratio of M beyond e^18) or NaN: those lanes take acosh = log(tau + sqrt(tau^2 - 1)) from OCML
// behind a wave-uniform branch.
#ifndef GABO_GAUSS2_MAX_ROWS      /* rows of W a block of the d = 2 Gaussian kernel prepares (<= its 256 threads); GABO_PAIR_ROWS_GAUSS2 <= this */
#define GABO_GAUSS2_MAX_ROWS 64
#endif
constexpr double kGauss2L = 0.0027076061740622863;      // ln2 / 256
// [0..3] l^k / k! (k = 1..4), [4] 1.5 2^52, [5] 2^12
__constant__ double kGauss2C[6] = {kGauss2L, kGauss2L * kGauss2L / 2.0, kGauss2L * kGauss2L * kGauss2L / 6.0,
                                   kGauss2L * kGauss2L * kGauss2L * kGauss2L / 24.0, 6755399441055744.0, 4096.0};

template <bool NT, bool SYM>
__global__ __launch_bounds__(256) void spd_ai_gauss2_kernel(const double* __restrict__ Winv, const double* __restrict__ G,
                                                            double* __restrict__ out, int64_t n1, int64_t n2, int64_t w_batch_stride,
                                                            int64_t g_batch_stride, int rows, int col_blocks, int row_chunks,
                                                            int64_t sym_tiles, double beta, int flags) {
    __shared__ __attribute__((aligned(16))) double ltab[512];
    __shared__ double etab[256];
    __shared__ __attribute__((aligned(16))) double atab[kAcosh2Slots * kAcosh2Stride];
    __shared__ __attribute__((aligned(16))) double wrow[GABO_GAUSS2_MAX_ROWS * 4];
    const int tid = threadIdx.x;
    for (int k = tid; k < 512; k += blockDim.x) ltab[k] = kLogTab[k];
    for (int k = tid; k < 256; k += blockDim.x) etab[k] = kExp2Tab256[k];
    {
        const double sc = beta * (-512.0 / 0.69314718055994530942), eps = beta * (-256.0 / 0.69314718055994530942) * 1e-15;
        // (rows 176..239 of the table are unused - binades 12..15 - and never read by a lane whose value is kept)
        constexpr int kUsedLo = (kAcosh2Binades - 1) * 16 * kAcosh2Stride, kUsedHi = 240 * kAcosh2Stride;
        for (int k = tid; k < kAcosh2Slots * kAcosh2Stride - (kUsedHi - kUsedLo); k += blockDim.x) {
            const int kk = k < kUsedLo ? k : k + (kUsedHi - kUsedLo);
            const double v = kAcosh2Tab[kk] * sc;
            atab[kk] = (kk % kAcosh2Stride == 0) ? v + eps : v;
        }
    }
    int64_t cg, rc, b;
    if constexpr (SYM) {       // see spd_ai_pairwise_kernel
        const int64_t per_batch = sym_tiles;
        b = blockIdx.x / per_batch;
        int64_t t = blockIdx.x - b * per_batch;
        cg = 0;
        for (;;) {
            int64_t cnt = ((cg + 1) * (int64_t)blockDim.x + rows - 1) / rows;
            if (cnt > row_chunks) cnt = row_chunks;
            if (t < cnt) break;
            t -= cnt;
            ++cg;
        }
        rc = t;
    } else {
        const int64_t bid = blockIdx.x;
        cg = bid % col_blocks;
        rc = (bid / col_blocks) % row_chunks;
        b = bid / ((int64_t)col_blocks * row_chunks);
    }
    const int64_t j0 = cg * blockDim.x;
    const int64_t j = j0 + tid;
    const int64_t jc = j < n2 ? j : n2 - 1;
    const int64_t i0 = rc * rows;
    const int64_t i1 = (i0 + rows < n1) ? i0 + rows : n1;
    const double* Gj = G + b * g_batch_stride + jc;
    const double g00 = Gj[0], g10 = Gj[n2], g11 = Gj[2 * n2];
    const LogTabRegs lr = LogTabRegs::load();
    const double sscale = __builtin_sqrt(beta * (512.0 / 0.69314718055994530942));
    // the block's rows of W with their per-point terms: thread r prepares row i0 + r (rows <= 64), everybody reads them back from LDS with a
    // wave-uniform address (a broadcast: no VALU instruction, no scalar-memory round trip per row)
    double w0l = 1.0, w1l = 0.0, w2l = 1.0;
    if (tid < rows) {
        int64_t ir = i0 + tid;
        ir = ir < n1 ? ir : n1 - 1;
        const double* Wr = Winv + b * w_batch_stride + ir * 3;
        w0l = Wr[0], w1l = Wr[1], w2l = Wr[2];
    }
    __syncthreads();                                     // the tables
    // tau = tr M / (2 sqrt(det M)) with M = C C^T, C = W G = [[a, 0], [c, b]]:  tau = 1 + ((a - b)^2 + c^2) / (2 a b)  (no cancellation in the numerator).
    // The quotient is folded into the operands: rows scaled by 1 / sqrt(2 w00 w11), columns by 1 / sqrt(g00 g11) - per-POINT factors - so that
    // with the scaled entries  tau = 1 + (a' - b')^2 + c'^2:  six instructions per pair (round 4: nine, with the product of the two reciprocals
    // formed per pair), tau >= 1 by construction (two FMAs onto 1.0) and NaN operands stay NaN.
    if (tid < rows) {
        const double dw = w0l * w2l;
        const double sw = rsqrt_nz(dw + dw);
        wrow[4 * tid + 0] = w0l * sw;
        wrow[4 * tid + 1] = w1l * sw;
        wrow[4 * tid + 2] = w2l * sw;
        wrow[4 * tid + 3] = sscale * log_tab(dw, lr, ltab);      // sqrt(512 beta / ln2) log(w00 w11)
    }
    __syncthreads();
    if (SYM && j0 + (int64_t)(tid | 63) < i0) return;
    double ec[6];
    static_for<6>([&](auto k) { ec[decltype(k)::value] = kGauss2C[decltype(k)::value]; });
    double c4v = ec[3];
    asm volatile("" : "+v"(c4v));
    const double dg = g00 * g11;
    const double bcol = sscale * log_tab(dg, lr, ltab);       // the lane's column terms
    const double sg = rsqrt_nz(dg);
    const double q00 = g00 * sg, q10 = g10 * sg, q11 = g11 * sg;       // the column's factor scaled by 1 / sqrt(g00 g11)
    double* orow = out + b * n1 * n2 + i0 * n2 + j;
    const int nrows = __builtin_amdgcn_readfirstlane((int)(i1 - i0));      // (wave-uniform: the loop counter and its compare stay on the scalar unit)
    // x1 is x2: row r of the block is stored by the lanes with i0 + r <= j
    const int64_t jrel = j - i0;
    const int rmax = j >= n2 ? -1 : (SYM ? (jrel < 0 ? -1 : (jrel > GABO_GAUSS2_MAX_ROWS - 1 ? GABO_GAUSS2_MAX_ROWS - 1 : (int)jrel)) : GABO_GAUSS2_MAX_ROWS - 1);
    typedef double g2_v2d __attribute__((ext_vector_type(2)));
    if (!SYM && j >= n2) return;       // (no barrier below; the full build then stores without a per-row predicate)
    for (int r = 0; r < nrows; ++r, orow += n2) {
        const g2_v2d wa = *reinterpret_cast<const g2_v2d*>(wrow + 4 * r);
        const g2_v2d wb = *reinterpret_cast<const g2_v2d*>(wrow + 4 * r + 2);
        const double w0 = wa[0], w1 = wa[1], w2 = wb[0], arow = wb[1];
        const double hh = __builtin_fma(w0, q00, -(w2 * q11));          // a' - b'
        const double cc = __builtin_fma(w1, q00, w2 * q10);             // c'
        const double tau = __builtin_fma(cc, cc, __builtin_fma(hh, hh, 1.0));
        const unsigned hi = (unsigned)__double2hiint(tau);
        // row of the table: bits 16..23 of the high word (in range by construction: one v_bfe_u32, no bias subtraction, and the four reads
        // share one address register with immediate offsets)
        static_assert(kAcosh2MBits == 4 && kAcosh2Slots == 256, "row index = 8 bits");
        const unsigned off = __umul24((hi >> 16) & 0xffu, (unsigned)(kAcosh2Stride * sizeof(double)));
        const double t = tau - __hiloint2double((int)(hi & ~((1u << (20 - kAcosh2MBits)) - 1u)), 0);
        const g2_v2d* row = reinterpret_cast<const g2_v2d*>(reinterpret_cast<const char*>(atab) + off);
        static_assert(kAcosh2Deg == 7, "four coefficient pairs");
        const g2_v2d c67 = row[3], c45 = row[2], c23 = row[1], c01 = row[0];
        double ya = __builtin_fma(c67[1], t, c67[0]);
        ya = __builtin_fma(ya, t, c45[1]);
        ya = __builtin_fma(ya, t, c45[0]);
        ya = __builtin_fma(ya, t, c23[1]);
        ya = __builtin_fma(ya, t, c23[0]);
        ya = __builtin_fma(ya, t, c01[1]);
        ya = __builtin_fma(ya, t, c01[0]);
        if (__builtin_expect(__any(!(tau < ec[5])), 0)) {
            if (!(tau < ec[5])) {       // beyond the table (or NaN): acosh from OCML
                const double dl = log(tau + __builtin_sqrt(__builtin_fma(tau, tau, -1.0)));
                ya = -(sscale * sscale) * __builtin_fma(dl, dl, 0.5e-15);
            }
        }
        const double sp = arow + bcol;
        const double y = __builtin_fma(-sp, sp, ya);           // -beta (d^2 + 1e-15) 256 / ln2  (spd_utils_torch.py:120, kernels_spd.py:94-98)
        const double km = y + ec[4];
        const double kk = km - ec[4];
        const double rr = y - kk;
        double p = __builtin_fma(rr, c4v, ec[2]);
        p = __builtin_fma(p, rr, ec[1]);
        p = __builtin_fma(p, rr, ec[0]);
        p = p * rr;
        const int ki = __double2loint(km);
        const double e = etab[ki & 255];
        const double val = __builtin_ldexp(__builtin_fma(e, p, e), ki >> 8);
        if (!SYM || r <= rmax) {
            if constexpr (NT) __builtin_nontemporal_store(val, orow);
            else *orow = val;
        }
    }
}

// prepared: the workspace already holds the factors (W for b1 * n1 matrices, then G: the fused projection of the nested kernels wrote them,
// nested_spd_gram.hip); s1 / s2 then only say whether a set is shared across the batch (0) or not
template <int D>
static int launch_spd_ai(const double* x1, const double* x2, double* out, double* dist_out, int64_t batch, int64_t n1, int64_t n2,
                         int64_t s1, int64_t s2, double beta, int flags, double* ws, int* status, hipStream_t st, bool prepared = false) {
    constexpr int T = tri_size(D);
    const int64_t b1 = (s1 == 0) ? 1 : batch;  // a shared set is factored once
    const int64_t b2 = (s2 == 0) ? 1 : batch;
    double* W = ws;
    double* G = ws + b1 * n1 * T;
    if (!prepared) launch_spd_prep<D>(x1, x2, W, G, b1, b2, n1, n2, s1, s2, status, st, /*lenient2=*/1);
    // tile shape: 64..256 columns per block, `rows` rows per block; keep >= ~8 blocks per CU when the problem allows
    // (d = 10, N = 4096, 8 rows: 256 / 128 / 64 threads per block = 2.57 / 2.56 / 2.55 ms - one-wave blocks: a block's slots are not held until its slowest wave ends; d = 7: 1.25 -> 1.23 ms, d <= 5: no gain)
#ifndef GABO_PAIR_THREADS
#define GABO_PAIR_THREADS (D >= 7 ? 64 : 256)
#endif
    int threads = n2 >= 256 ? GABO_PAIR_THREADS : (n2 > 128 ? 192 : (n2 > 64 ? 128 : 64));
    int64_t col_blocks = (n2 + threads - 1) / threads;
    // rows per block: a wave's prologue (log table into LDS, for d = 2 the per-point log terms) is amortised over them; d = 2 pairs are ~75
    // instructions; measured at N = 4096, d = 2: 64 / 32 / 16 / 8 / 4 rows per block = 66 / 61 / 59 / 63 / 71 us
#ifndef GABO_PAIR_ROWS_D2
#define GABO_PAIR_ROWS_D2 16
#endif
    // d = 10, N = 4096 (blocks vary in duration with their pairs' QL iteration counts: smaller blocks balance the tail, larger ones amortise
    // the prologue): 64 / 32 / 16 / 8 / 4 / 2 rows = 2.72 / 2.64 / 2.60 / 2.58 / 2.58 / 2.62 ms
#ifndef GABO_PAIR_ROWS
#define GABO_PAIR_ROWS (D >= 9 ? 8 : 16)
#endif
    // the d = 2 Gaussian kernel copies a 20 KB table into LDS per block: 64 rows per block amortise it (N = 4096: 16 / 32 / 64 rows = 46.5 / 42.4 /
    // 40.7 us including the prep launch)
#ifndef GABO_PAIR_ROWS_GAUSS2
#define GABO_PAIR_ROWS_GAUSS2 64
#endif
    const bool gauss2 = D == 2 && (flags & GABO_OUT_MASK) == GABO_OUT_GAUSSIAN && !dist_out && beta >= 0.0;
    int rows = D == 2 ? (gauss2 ? GABO_PAIR_ROWS_GAUSS2 : GABO_PAIR_ROWS_D2) : GABO_PAIR_ROWS;
    while (rows > 1 && col_blocks * ((n1 + rows - 1) / rows) * batch < (rows > 16 ? 1024 : 4096)) rows >>= 1;
    int64_t row_chunks = (n1 + rows - 1) / rows;
    int64_t sym_tiles = 0;
    if (flags & GABO_SYMMETRIC) {
        for (int64_t cg = 0; cg < col_blocks; ++cg) {
            int64_t cnt = ((cg + 1) * threads + rows - 1) / rows;
            sym_tiles += cnt < row_chunks ? cnt : row_chunks;
        }
    }
    int64_t nblocks = ((flags & GABO_SYMMETRIC) ? sym_tiles : col_blocks * row_chunks) * batch;
    if (nblocks > 0x7fffffffLL) return GABO_ERR_ARG;
    bool special2 = false;
    if constexpr (D == 2) special2 = gauss2 && rows <= GABO_GAUSS2_MAX_ROWS;
    if (special2) {
        const bool streaming = batch * n1 * n2 * 8 > (32ll << 20) && !(flags & GABO_SYMMETRIC);      // beyond the L2 caches (see sphere_pairwise.hip)
#define GABO_GAUSS2_LAUNCH(...)                                                                                                     \
        hipLaunchKernelGGL((spd_ai_gauss2_kernel<__VA_ARGS__>), dim3((unsigned)nblocks), dim3(threads), 0, st, W, G, out, n1, n2,           \
                           (s1 == 0) ? (int64_t)0 : n1 * T, (s2 == 0) ? (int64_t)0 : n2 * T, rows, (int)col_blocks, (int)row_chunks,       \
                           sym_tiles, beta, flags)
        if (flags & GABO_SYMMETRIC) GABO_GAUSS2_LAUNCH(false, true);        // (never streamed: see `streaming`)
        else if (streaming) GABO_GAUSS2_LAUNCH(true, false);
        else GABO_GAUSS2_LAUNCH(false, false);
#undef GABO_GAUSS2_LAUNCH
    } else {
#define GABO_PAIR_LAUNCH(...)                                                                                                             \
        hipLaunchKernelGGL((spd_ai_pairwise_kernel<D, __VA_ARGS__>), dim3((unsigned)nblocks), dim3(threads), 0, st, W, G, out, dist_out, n1, n2, \
                           (s1 == 0) ? (int64_t)0 : n1 * T, (s2 == 0) ? (int64_t)0 : n2 * T, rows, (int)col_blocks, (int)row_chunks,       \
                           sym_tiles, beta, flags)
        // Gaussian values alone, G within reach of a buffer descriptor's 2^31 bytes: the instantiation with nothing else in it (d = 2 has its
        // own kernel above for that launch)
        bool gauss_only = false;
        if constexpr (spd_pair_gauss_only_instantiated(D)) {
            gauss_only = (flags & GABO_OUT_MASK) == GABO_OUT_GAUSSIAN && !dist_out && (int64_t)T * n2 * 8 < (1ll << 31);
            if (gauss_only) GABO_PAIR_LAUNCH(true, true);
        }
        if (!gauss_only) GABO_PAIR_LAUNCH(false, false);
#undef GABO_PAIR_LAUNCH
    }
    if (flags & GABO_SYMMETRIC) {
        int tiles = (int)((n1 + 31) / 32);
        hipLaunchKernelGGL((mirror_upper_kernel<0>), dim3((unsigned)((int64_t)tiles * (tiles + 1) / 2), (unsigned)batch), dim3(256), 0, st,
                           out, n1, tiles);
        if (dist_out)
            hipLaunchKernelGGL((mirror_upper_kernel<0>), dim3((unsigned)((int64_t)tiles * (tiles + 1) / 2), (unsigned)batch), dim3(256), 0,
                               st, dist_out, n1, tiles);
    }
    return hipGetLastError() == hipSuccess ? GABO_OK : GABO_ERR_LAUNCH;
}

}  // namespace gabo

namespace gabo {
// the pairwise launch alone on factors already in the workspace, d = 2 ... 4 (spd_pairwise.hip; called by nested_spd_gram.hip)
int launch_spd_ai_prepared(int d, double* out, int64_t batch, int64_t n1, int64_t n2, bool shared1, bool shared2, double beta, int flags,
                           double* ws, hipStream_t st);
// dimensions 13..16 are instantiated in their own translation unit (spd_pairwise_wide.hip), 17..20 in two more
int launch_spd_ai_wide2(int d, const double* x1, const double* x2, double* out, double* dist_out, int64_t batch, int64_t n1, int64_t n2,
                        int64_t s1, int64_t s2, double beta, int flags, double* ws, int* status, hipStream_t st);
int launch_spd_ai_wide3(int d, const double* x1, const double* x2, double* out, double* dist_out, int64_t batch, int64_t n1, int64_t n2,
                        int64_t s1, int64_t s2, double beta, int flags, double* ws, int* status, hipStream_t st);
int launch_spd_ai_wide(int d, const double* x1, const double* x2, double* out, double* dist_out, int64_t batch, int64_t n1, int64_t n2,
                       int64_t s1, int64_t s2, double beta, int flags, double* ws, int* status, hipStream_t st);
}  // namespace gabo
