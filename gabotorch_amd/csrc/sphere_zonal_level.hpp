// One level of a zonal series on the sphere (csrc/sphere_zonal.hip states the series and its recurrence): the coefficient of P_k and the factor
// B_k = (k - 1) / (k + d - 2) of  P_k = t + B_k (t - P_{k-2}),  t = c P_{k-1}  (series dimension d; B_0 = B_1 = 0).  Shared by the Gram / element-wise
// kernels of sphere_zonal.hip, which take a series by value, and the kernels that read a table of them from memory: the acquisition kernels of
// sphere_tr.hip and the Gram adjoint of nested_sphere_chain.hip (sph_zonal_strip below).
#pragma once

#include <cstdint>

namespace gabo {

constexpr int kZonalMaxCoeff = 129;

struct ZonalLevel {
    double a, rb;          // coeff_k, B_k
};

// f(c), f'(c)[, f''(c)] of a zonal series at one inner product (any NS series of equal length, one per table row): ONE pass over the levels advances the NS recurrences P^(d), P^(d+2)[, P^(d+4)]
// (order o reads its levels at tab + o * L) in zonal_eval's form - ascending levels, t = c P_{k-1}, P_k = fma(B_k, t - P_{k-2}, t), f = fma(p_k, P_k, f),
// two levels per trip so that P_{k-2} and P_{k-1} swap roles.  The table is the same for every lane: the levels come through the scalar cache
// (constant address space).  A polynomial: no clamp, and nothing to mask at c = +-1.
typedef const ZonalLevel __attribute__((address_space(4)))* ZonalTab;

template <int NS>
static __device__ __forceinline__ void sph_zonal_strip(const double* series, int L, double c, double (&f)[NS]) {
    const ZonalTab tab = (ZonalTab)(uintptr_t)series;
    double p0[NS], p1[NS];
#pragma unroll
    for (int o = 0; o < NS; ++o) {
        const double a0 = tab[o * L].a, a1 = L > 1 ? tab[o * L + 1].a : 0.0;
        p0[o] = 1.0;
        p1[o] = c;
        f[o] = __builtin_fma(a1, c, a0);
    }
    int k = 2;
    for (; k + 1 < L; k += 2) {
#pragma unroll
        for (int o = 0; o < NS; ++o) {
            const double ea = tab[o * L + k].a, eb = tab[o * L + k].rb, da = tab[o * L + k + 1].a, db = tab[o * L + k + 1].rb;
            const double te = c * p1[o];
            p0[o] = __builtin_fma(eb, te - p0[o], te);                    // P_k in the place of P_{k-2}
            f[o] = __builtin_fma(ea, p0[o], f[o]);
            const double to = c * p0[o];
            p1[o] = __builtin_fma(db, to - p1[o], to);                    // P_{k+1} in the place of P_{k-1}
            f[o] = __builtin_fma(da, p1[o], f[o]);
        }
    }
    if (k < L) {
#pragma unroll
        for (int o = 0; o < NS; ++o) {
            const double ea = tab[o * L + k].a, eb = tab[o * L + k].rb;
            const double te = c * p1[o];
            p0[o] = __builtin_fma(eb, te - p0[o], te);
            f[o] = __builtin_fma(ea, p0[o], f[o]);
        }
    }
}

}  // namespace gabo
