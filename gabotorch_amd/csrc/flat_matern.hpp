// The Matern kernels of half-integer smoothness as functions of a distance, for the flat SPD metrics (log-Euclidean, Frobenius): both are
// isometries into R^{d(d+1)/2}, so their Riemannian Matern kernel is the Euclidean one of the library's distance r and is positive definite
// for every lengthscale.  gpytorch's MaternKernel parametrisation, NU2 = 2 nu in {1, 3, 5}, a = sqrt(2 nu) / l, x = a r:
//   k(r)          = m(x) e^-x              m = 1,      1 + x,   1 + x + x^2 / 3
//   dk / dl       = x^2 q(x) e^-x / l      q = 1 / x,  1,       (1 + x) / 3
//   2 dk / d(r^2) = -a^2 q(x) e^-x         (the weight of the x-gradient: no division by r for nu = 3/2, 5/2)
// Every kernel that needs one of the three calls these functions (flat_matern.hip, gp_mll_matern.hip): plain exp, one operation order, the
// fused operations spelled out (the build contracts nothing) - an entry has the same bits whichever launch formed it.
#pragma once
#include "gabo_device.hpp"

namespace gabo {

constexpr double kMaternThird = 1.0 / 3.0;

template <int NU2>
static __device__ __forceinline__ double flat_matern_value(double r, double a) {
    static_assert(NU2 == 1 || NU2 == 3 || NU2 == 5, "flat_matern: 2 nu in {1, 3, 5}");
    const double x = a * r;
    const double e = exp(-x);
    if constexpr (NU2 == 1) return e;
    if constexpr (NU2 == 3) return (1.0 + x) * e;
    return __builtin_fma(x, __builtin_fma(x, kMaternThird, 1.0), 1.0) * e;
}

template <int NU2>
static __device__ __forceinline__ double flat_matern_dlengthscale(double r, double a, double l) {
    static_assert(NU2 == 1 || NU2 == 3 || NU2 == 5, "flat_matern: 2 nu in {1, 3, 5}");
    const double x = a * r;
    const double e = exp(-x);
    if constexpr (NU2 == 1) return (x * e) / l;
    if constexpr (NU2 == 3) return ((x * x) * e) / l;
    return ((x * x) * (((1.0 + x) * kMaternThird) * e)) / l;
}

template <int NU2>
static __device__ __forceinline__ double flat_matern_weight(double r, double a) {
    static_assert(NU2 == 1 || NU2 == 3 || NU2 == 5, "flat_matern: 2 nu in {1, 3, 5}");
    const double x = a * r;
    const double e = exp(-x);
    if constexpr (NU2 == 1) return -(a * e) / r;
    if constexpr (NU2 == 3) return -(a * a) * e;
    return -(a * a) * (((1.0 + x) * kMaternThird) * e);
}

// host: the arguments every entry checks before anything else, and a = sqrt(2 nu) / l as one square root and one division
static inline bool flat_matern_arguments_ok(double lengthscale, int nu2) {
    return (nu2 == 1 || nu2 == 3 || nu2 == 5) && lengthscale > 0.0 && lengthscale <= 1.7976931348623157e308;
}
static inline double flat_matern_scale(double lengthscale, int nu2) { return __builtin_sqrt((double)nu2) / lengthscale; }

}  // namespace gabo
