// Exact-GP marginal log likelihood and its analytic gradient with respect to the kernel hyper-parameters, one launch per
// evaluation.  This is the inner step of the surrogate fit that runs every BO iteration (examples/.../gabo_spd.py:194
// `fit_gpytorch_model(mll)` -> [3P] gpytorch ExactMarginalLogLikelihood under scipy L-BFGS-B).  For every plain kernel of the path
// the Gram matrix has the form exp(-theta * E) with E = d^2 (Gaussian) or d (Laplace) fixed during the fit, so the pairwise
// distances are evaluated ONCE (gabo_spd_ai_pairwise / gabo_frobenius_pairwise / gabo_sphere_pairwise with GABO_OUT_DISTANCE) and
// each L-BFGS evaluation is the small dense algebra below:
//   Ky = outputscale * exp(-theta E) + noise I,  r = y - mean,  alpha = Ky^-1 r,  W = alpha alpha^T - Ky^-1
//   ll         = -r.alpha/2 - log det(Ky)/2 - n log(2 pi)/2
//   dll/dtheta = tr(W dKy/dtheta)/2,  dKy/dtheta = -outputscale * E o exp(-theta E)
//   dll/dos    = tr(W exp(-theta E))/2,  dll/dnoise = tr(W)/2,  dll/dmean = sum_i alpha_i
// The reference leaves this to autograd through the per-pair Python loop of the kernel on every evaluation.
//
// The problem is one small matrix, so the design target is latency, not throughput: one workgroup, the bordered matrix
// [[Ky, r], [r^T, 0]] distributed over the threads' REGISTERS as 4 x 4 tiles of its lower triangle (one tile per thread, diagonal
// tiles stored in full), and the symmetric sweep operator (Gauss-Jordan on the pivots 0..n-1: a_kk <- -1/p, a_ik <- a_ik/p,
// a_ij <- a_ij - a_ik a_jk/p) applied in place.  After the n sweeps the matrix block holds -Ky^-1, the border holds alpha and the
// corner -r.alpha; the pivots are the Schur complements, so log det(Ky) = sum log p_k and Ky is positive definite iff every p_k > 0.
// One sweep is one barrier: only the pivot column travels through LDS (double-buffered).  A thread reads the 4 + 4 column entries of
// its tile's rows and columns and does 16 FMAs, x_ab <- x_ab - g_a h_b with g = c_row / p, h = c_col.  The pivot row and column need no
// special case in that update: their owners publish them for the next sweep one step ahead and ZERO their register copies, and the
// sweep uses g = -1/p at the pivot row and h = -1 at the pivot column, which turns the same FMA into c_i / p, c_j / p and -1/p there.
#include "gabo_device.hpp"
#include "gp_mll_body.hpp"
#include "../../include/gabo_hip.h"

namespace gabo {

// exp(-theta E), or E itself (gram): the parameter is theta, d/dtheta exp(-theta e) = -e exp(-theta e)
struct MllExpBase {
    static constexpr bool kRowLoads = false;
    double theta;
    int gram;
    template <int NV>
    __device__ __forceinline__ void values(const double (&e)[NV], double (&k)[NV]) const {
        static_for<NV>([&](auto vv) {
            constexpr int v = decltype(vv)::value;
            k[v] = gram ? e[v] : exp(-theta * e[v]);
        });
    }
    template <int NV, class Use, class Emit>
    __device__ __forceinline__ void terms(const double (&e)[NV], Use use, Emit emit) const {
        static_for<NV>([&](auto vv) {
            constexpr int v = decltype(vv)::value;
            if (use(vv)) {
                const double kb = gram ? e[v] : exp(-theta * e[v]);
                emit(vv, kb, e[v] * kb);
            }
        });
    }
    __device__ __forceinline__ double d_param(double os, double acc) const { return gram ? 0.0 : -0.5 * os * acc; }
};

template <int MAXT>
__global__ __launch_bounds__(MAXT) void gp_mll_kernel(const double* __restrict__ e, const double* __restrict__ y, int n,
                                                               double theta, double os, double noise, double mean,
                                                               double* __restrict__ out, int gram, double* __restrict__ w_out) {
    gp_mll_tiled_body<MAXT>(e, y, n, os, noise, mean, out, w_out, MllExpBase{theta, gram});
}

template <int THREADS, int MAXE>
__global__ __launch_bounds__(THREADS) void gp_mll_small_kernel(const double* __restrict__ e, const double* __restrict__ y, int n,
                                                         double theta, double os, double noise, double mean,
                                                         double* __restrict__ out, int gram, double* __restrict__ w_out) {
    gp_mll_small_body<THREADS, MAXE>(e, y, n, os, noise, mean, out, w_out, MllExpBase{theta, gram});
}

}  // namespace gabo

static int gp_mll_dispatch(const double* e, const double* y, int64_t n, double theta, double outputscale, double noise, double mean,
                           double* out, int gram, double* w_out, gabo_stream_t stream) {
    if (n < 1 || n > GABO_GP_MLL_MAX_N) return GABO_ERR_DIM;
    if (!e || !y || !out) return GABO_ERR_ARG;
    if (n <= GABO_MLL_SMALL_N) {                          // (n + 1)(n + 2) / 2 <= 512 packed entries: two per thread
        hipLaunchKernelGGL((gabo::gp_mll_small_kernel<256, 2>), dim3(1), dim3(256), gabo::mll_small_lds_bytes(n), (hipStream_t)stream, e, y,
                           (int)n, theta, outputscale, noise, mean, out, gram, w_out);
        return hipGetLastError() == hipSuccess ? GABO_OK : GABO_ERR_LAUNCH;
    }
    int threads;
    size_t lds;
    gabo::mll_tiled_geometry(n, threads, lds);
    if (threads == 64)
        hipLaunchKernelGGL(gabo::gp_mll_kernel<64>, dim3(1), dim3(64), lds, (hipStream_t)stream, e, y, (int)n, theta, outputscale, noise,
                           mean, out, gram, w_out);
    else
        hipLaunchKernelGGL(gabo::gp_mll_kernel<gabo::kMllMaxThreads>, dim3(1), dim3(threads), lds, (hipStream_t)stream, e, y, (int)n,
                           theta, outputscale, noise, mean, out, gram, w_out);
    return hipGetLastError() == hipSuccess ? GABO_OK : GABO_ERR_LAUNCH;
}

extern "C" int gabo_gp_mll(const double* e, const double* y, int64_t n, double theta, double outputscale, double noise, double mean,
                           double* out, gabo_stream_t stream) {
    return gp_mll_dispatch(e, y, n, theta, outputscale, noise, mean, out, 0, nullptr, stream);
}

extern "C" int gabo_gp_mll_gram(const double* k, const double* y, int64_t n, double outputscale, double noise, double mean, double* out,
                                double* w, gabo_stream_t stream) {
    return gp_mll_dispatch(k, y, n, 0.0, outputscale, noise, mean, out, 1, w, stream);
}
