// Exact-GP marginal log likelihood for a base Gram matrix that is a zonal series of the inner products, one launch per evaluation:
//   K_ij = sum_k a_k P_k(c_ij),   dK_ij / dkappa = sum_k (da_k / dkappa) P_k(c_ij),   Ky = outputscale * K + noise * I,
// the Riemannian Matern / heat kernels on the sphere (csrc/sphere_zonal.hip; coefficients: ops.sphere_matern_coefficients).  During a surrogate
// fit the inner products C = X X^T are fixed and only the coefficients move - as E is fixed and theta moves for exp(-theta E) - so an L-BFGS
// evaluation is the sweeps of csrc/gp_mll.hip (the same two bodies, gp_mll_body.hpp) with the series evaluated in registers where that kernel
// evaluates an exponential: no Gram matrix, no W and no dK in memory.
//
// The series is the recurrence of zonal_eval (sphere_zonal.hip), operation for operation:  t = c P_{k-1};  P_k = fma(B_k, t - P_{k-2}, t);
// f = fma(a_k, P_k, f), ascending k, B_k one IEEE division on the host - an entry K_ij has the bits gabo_sphere_zonal_from_inner returns for
// c_ij.  dK shares the P_k and costs one more fma per level.  a, da and B travel in the kernel arguments as three arrays (3.2 KB; the argument
// block stays below 4 KB), are wave-uniform and only read.  The tiled body evaluates one tile row (four entries) at a time and recomputes K and
// dK in the trace epilogue instead of keeping either across the sweeps: the tile is 32 of the 128 registers of the 1024-thread instantiation.
#include "gabo_device.hpp"
#include "gp_mll_body.hpp"
#include "sphere_zonal_level.hpp"
#include "../../include/gabo_hip.h"

namespace gabo {

struct MllSeriesBase {       // wave-uniform
    double a[kZonalMaxCoeff], da[kZonalMaxCoeff], rb[kZonalMaxCoeff];      // coeff_k, d coeff_k / d kappa, B_k (levels >= n: zeros)
    int n, has_d;
    static constexpr bool kRowLoads = true;

    // f[v] = sum_k a_k P_k(c[v]) and, WITH_D, df[v] = sum_k da_k P_k(c[v]): two levels per iteration as zonal_eval
    template <bool WITH_D, int NV>
    __device__ __forceinline__ void eval(const double (&c)[NV], double (&f)[NV], double (&df)[NV]) const {
        double p0[NV], p1[NV];
        const double a0 = a[0], a1 = a[1], d0 = da[0], d1 = da[1];      // (a1 = 0 for a series of one term)
        static_for<NV>([&](auto vv) {
            constexpr int v = decltype(vv)::value;
            p0[v] = 1.0;
            p1[v] = c[v];
            f[v] = __builtin_fma(a1, c[v], a0);
            if constexpr (WITH_D) df[v] = __builtin_fma(d1, c[v], d0);
        });
        int k = 2;
        for (; k + 1 < n; k += 2) {
            const double ae = a[k], ao = a[k + 1], be = rb[k], bo = rb[k + 1], de = da[k], dn = da[k + 1];
            static_for<NV>([&](auto vv) {
                constexpr int v = decltype(vv)::value;
                const double te = c[v] * p1[v];
                p0[v] = __builtin_fma(be, te - p0[v], te);                  // P_k in the place of P_{k-2}
                f[v] = __builtin_fma(ae, p0[v], f[v]);
                if constexpr (WITH_D) df[v] = __builtin_fma(de, p0[v], df[v]);
                const double to = c[v] * p0[v];
                p1[v] = __builtin_fma(bo, to - p1[v], to);                  // P_{k+1} in the place of P_{k-1}
                f[v] = __builtin_fma(ao, p1[v], f[v]);
                if constexpr (WITH_D) df[v] = __builtin_fma(dn, p1[v], df[v]);
            });
        }
        if (k < n) {
            const double ae = a[k], be = rb[k], de = da[k];
            static_for<NV>([&](auto vv) {
                constexpr int v = decltype(vv)::value;
                const double te = c[v] * p1[v];
                p0[v] = __builtin_fma(be, te - p0[v], te);
                f[v] = __builtin_fma(ae, p0[v], f[v]);
                if constexpr (WITH_D) df[v] = __builtin_fma(de, p0[v], df[v]);
            });
        }
    }

    template <int NV>
    __device__ __forceinline__ void values(const double (&c)[NV], double (&k)[NV]) const {
        eval<false>(c, k, k);
    }
    template <int NV, class Use, class Emit>
    __device__ __forceinline__ void terms(const double (&c)[NV], Use use, Emit emit) const {
        double f[NV], df[NV];
        eval<true>(c, f, df);
        static_for<NV>([&](auto vv) {
            if (use(vv)) emit(vv, f[decltype(vv)::value], df[decltype(vv)::value]);
        });
    }
    __device__ __forceinline__ double d_param(double os, double acc) const { return has_d ? 0.5 * os * acc : 0.0; }
};

// the kernel-argument block: the series, the seven scalars / pointers of the kernels below and the 256 bytes of implicit arguments behind them
static_assert(sizeof(MllSeriesBase) + 7 * 8 + 256 < 4096, "gabo_gp_mll_series: the kernel arguments must stay below 4 KB");

template <int MAXT>
__global__ __launch_bounds__(MAXT) void gp_mll_series_kernel(const double* __restrict__ c, const double* __restrict__ y, int n, double os,
                                                             double noise, double mean, double* __restrict__ out, const MllSeriesBase s) {
    gp_mll_tiled_body<MAXT>(c, y, n, os, noise, mean, out, nullptr, s);
}

template <int THREADS, int MAXE>
__global__ __launch_bounds__(THREADS) void gp_mll_series_small_kernel(const double* __restrict__ c, const double* __restrict__ y, int n,
                                                                      double os, double noise, double mean, double* __restrict__ out,
                                                                      const MllSeriesBase s) {
    gp_mll_small_body<THREADS, MAXE>(c, y, n, os, noise, mean, out, nullptr, s);
}

}  // namespace gabo

extern "C" int gabo_gp_mll_series(const double* c, const double* y, int64_t n, const double* coeff_host, const double* dcoeff_host, int n_coeff,
                                  int series_dim, double outputscale, double noise, double mean, double* out, gabo_stream_t stream) {
    if (n < 1 || n > GABO_GP_MLL_MAX_N || series_dim < 1) return GABO_ERR_DIM;
    if (!c || !y || !out || !coeff_host || n_coeff < 1 || n_coeff > gabo::kZonalMaxCoeff) return GABO_ERR_ARG;
    gabo::MllSeriesBase s = {};
    s.n = n_coeff;
    s.has_d = dcoeff_host ? 1 : 0;
    for (int k = 0; k < n_coeff; ++k) {
        s.a[k] = coeff_host[k];
        if (dcoeff_host) s.da[k] = dcoeff_host[k];
        if (k >= 2) s.rb[k] = ((double)k - 1.0) / ((double)k + (double)series_dim - 2.0);      // (as zonal_series of sphere_zonal.hip)
    }
    if (n <= GABO_MLL_SMALL_N) {                          // (n + 1)(n + 2) / 2 <= 512 packed entries: two per thread
        hipLaunchKernelGGL((gabo::gp_mll_series_small_kernel<256, 2>), dim3(1), dim3(256), gabo::mll_small_lds_bytes(n), (hipStream_t)stream, c,
                           y, (int)n, outputscale, noise, mean, out, s);
        return hipGetLastError() == hipSuccess ? GABO_OK : GABO_ERR_LAUNCH;
    }
    int threads;
    size_t lds;
    gabo::mll_tiled_geometry(n, threads, lds);
    if (threads == 64)
        hipLaunchKernelGGL(gabo::gp_mll_series_kernel<64>, dim3(1), dim3(64), lds, (hipStream_t)stream, c, y, (int)n, outputscale, noise, mean,
                           out, s);
    else
        hipLaunchKernelGGL(gabo::gp_mll_series_kernel<gabo::kMllMaxThreads>, dim3(1), dim3(threads), lds, (hipStream_t)stream, c, y, (int)n,
                           outputscale, noise, mean, out, s);
    return hipGetLastError() == hipSuccess ? GABO_OK : GABO_ERR_LAUNCH;
}
