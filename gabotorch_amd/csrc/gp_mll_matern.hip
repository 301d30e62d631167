// Exact-GP marginal log likelihood for a base Gram matrix that is a Matern function (nu = 1/2, 3/2, 5/2; flat_matern.hpp) of a distance
// matrix fixed during a fit, one launch per evaluation:
//   K_ij = k_nu(r_ij; l),   dK_ij / dl from the same r_ij,   Ky = outputscale * K + noise * I,
// the Matern kernels on the log-Euclidean and Frobenius SPD metrics (csrc/flat_matern.hip).  r is what the GABO_OUT_DISTANCE launch of
// gabo_frobenius_pairwise writes once per fit; an L-BFGS evaluation is the sweeps of csrc/gp_mll.hip (the same two bodies, gp_mll_body.hpp)
// with the Matern function where that kernel evaluates exp(-theta e): no Gram matrix, no W and no dK in memory.  An entry K_ij has the bits
// gabo_flat_matern_from_distance returns for r_ij, so out[0] and out[2..5] are those of gabo_gp_mll_gram on its result.
#include "flat_matern.hpp"
#include "gp_mll_body.hpp"
#include "../../include/gabo_hip.h"

namespace gabo {

template <int NU2>
struct MllMaternBase {       // the parameter is the lengthscale l itself
    static constexpr bool kRowLoads = false;
    double a, l;             // a = sqrt(2 nu) / l
    template <int NV>
    __device__ __forceinline__ void values(const double (&r)[NV], double (&k)[NV]) const {
        static_for<NV>([&](auto vv) {
            constexpr int v = decltype(vv)::value;
            k[v] = flat_matern_value<NU2>(r[v], a);
        });
    }
    template <int NV, class Use, class Emit>
    __device__ __forceinline__ void terms(const double (&r)[NV], Use use, Emit emit) const {
        static_for<NV>([&](auto vv) {
            constexpr int v = decltype(vv)::value;
            if (use(vv)) emit(vv, flat_matern_value<NU2>(r[v], a), flat_matern_dlengthscale<NU2>(r[v], a, l));
        });
    }
    __device__ __forceinline__ double d_param(double os, double acc) const { return 0.5 * os * acc; }
};

template <int MAXT, int NU2>
__global__ __launch_bounds__(MAXT) void gp_mll_matern_kernel(const double* __restrict__ r, const double* __restrict__ y, int n, double a,
                                                             double l, double os, double noise, double mean, double* __restrict__ out) {
    gp_mll_tiled_body<MAXT>(r, y, n, os, noise, mean, out, nullptr, MllMaternBase<NU2>{a, l});
}

template <int THREADS, int MAXE, int NU2>
__global__ __launch_bounds__(THREADS) void gp_mll_matern_small_kernel(const double* __restrict__ r, const double* __restrict__ y, int n,
                                                                      double a, double l, double os, double noise, double mean,
                                                                      double* __restrict__ out) {
    gp_mll_small_body<THREADS, MAXE>(r, y, n, os, noise, mean, out, nullptr, MllMaternBase<NU2>{a, l});
}

template <int NU2>
static int gp_mll_matern_launch(const double* r, const double* y, int64_t n, double a, double l, double outputscale, double noise,
                                double mean, double* out, gabo_stream_t stream) {
    if (n <= GABO_MLL_SMALL_N) {                          // (n + 1)(n + 2) / 2 <= 512 packed entries: two per thread
        hipLaunchKernelGGL((gp_mll_matern_small_kernel<256, 2, NU2>), dim3(1), dim3(256), mll_small_lds_bytes(n), (hipStream_t)stream, r, y,
                           (int)n, a, l, outputscale, noise, mean, out);
        return hipGetLastError() == hipSuccess ? GABO_OK : GABO_ERR_LAUNCH;
    }
    int threads;
    size_t lds;
    mll_tiled_geometry(n, threads, lds);
    if (threads == 64)
        hipLaunchKernelGGL((gp_mll_matern_kernel<64, NU2>), dim3(1), dim3(64), lds, (hipStream_t)stream, r, y, (int)n, a, l, outputscale,
                           noise, mean, out);
    else
        hipLaunchKernelGGL((gp_mll_matern_kernel<kMllMaxThreads, NU2>), dim3(1), dim3(threads), lds, (hipStream_t)stream, r, y, (int)n, a, l,
                           outputscale, noise, mean, out);
    return hipGetLastError() == hipSuccess ? GABO_OK : GABO_ERR_LAUNCH;
}

}  // namespace gabo

extern "C" int gabo_gp_mll_matern(const double* r, const double* y, int64_t n, double lengthscale, int nu2, double outputscale, double noise,
                                  double mean, double* out, gabo_stream_t stream) {
    if (n < 1 || n > GABO_GP_MLL_MAX_N) return GABO_ERR_DIM;
    if (!r || !y || !out || !gabo::flat_matern_arguments_ok(lengthscale, nu2)) return GABO_ERR_ARG;
    const double a = gabo::flat_matern_scale(lengthscale, nu2);
    if (nu2 == 1) return gabo::gp_mll_matern_launch<1>(r, y, n, a, lengthscale, outputscale, noise, mean, out, stream);
    if (nu2 == 3) return gabo::gp_mll_matern_launch<3>(r, y, n, a, lengthscale, outputscale, noise, mean, out, stream);
    return gabo::gp_mll_matern_launch<5>(r, y, n, a, lengthscale, outputscale, noise, mean, out, stream);
}
