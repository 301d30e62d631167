// Random phase features of the Riemannian Matern / heat kernels of the affine-invariant metric on S^d_++ (Azangulov et al. 2023, the
// construction for non-compact symmetric spaces): for a point X and a feature l with its Haar matrix H_l the launch needs
//     a(H_l^T X H_l) = 2 log diag chol(H_l^T X H_l)          (lower Cholesky factor),
// one order-d factorisation per (point, feature) pair.  With X = G G^T (G lower, once per point, staged in LDS) H^T X H = M M^T, M = H^T G,
// and the Cholesky factor of M M^T is the L of M = L Q: its diagonal is the norm of row k of M after that row has been made orthogonal to
// the rows before it.  One lane per (point, feature): row k of M needs column k of H only, so H streams through - each entry is read once -
// and the lane keeps the orthogonal rows in registers, (d - 1) d doubles = 180 VGPRs at d = 10 (one wave per SIMD at d = 9 and 10, two at
// d = 7 and 8, three or more below).  The rows are kept unnormalised with the reciprocal of their squared norm: no square root anywhere,
// a_k = log |v_k|^2.
// The factorisation works on the square root G of X (condition sqrt(cond X)), so beyond chol(X) itself nothing squares the condition.
// phases is entry-major, H_l[r][c] at (r d + c) L + l: a wave reads one entry of 64 features as one contiguous run.
// One operation order whatever the launch shape, every multiply-add a spelled-out fma: the bits of a(i, l) depend on X_i and H_l only.
// A NaN or non-SPD X_i (Cholesky pivot not > 0) makes G, and with it every output of row i, NaN; nothing is reported.
#include "gabo_device.hpp"
#include "spd_ai_spectral_lane.hpp"
#include "spd_ai_spectral_value.hpp"
#include "../../include/gabo_hip.h"

#include <cmath>

namespace gabo {

// blockIdx.x = point * chunks + chunk of kSpectralBlock features; out (n, L, d)
template <int D>
__global__ __launch_bounds__(kSpectralBlock) void spd_ai_logdiag_kernel(const double* __restrict__ x, const double* __restrict__ phases,
                                                                        double* __restrict__ out, int64_t L, int chunks) {
    __shared__ __attribute__((aligned(16))) double Gs[tri_size(D) + 1];
    const int64_t i = blockIdx.x / (uint32_t)chunks;
    const int64_t l = (int64_t)(blockIdx.x - (uint32_t)i * (uint32_t)chunks) * kSpectralBlock + threadIdx.x;
    spectral_stage_cholesky<D>(x + i * tri_size(D), Gs);
    const int64_t lc = l < L ? l : L - 1;              // out-of-range lanes recompute the last feature and do not store
    double* o = out + (i * L + lc) * D;
    spectral_logdiag_lane<D>(Gs, phases + lc, L, [&](auto kk, double ak) {
        if (l < L) o[decltype(kk)::value] = ak;
    });
}

// One block per point: F_l = sqrt(w_l) exp(-rho . a_l) (cos, sin)(lam_l . a_l) for every feature, the row's sum of squares in a fixed
// order (per lane over its features in order, then a tree over the lanes), then the lanes scale what they wrote.  out (n, 2 L).
template <int D>
__global__ __launch_bounds__(kSpectralBlock) void spd_ai_spectral_features_kernel(const double* __restrict__ x, const double* __restrict__ phases,
                                                                                  const double* __restrict__ lam, const double* __restrict__ weight,
                                                                                  double* __restrict__ out, int64_t L) {
    __shared__ __attribute__((aligned(16))) double Gs[tri_size(D) + 1];
    __shared__ double red[kSpectralBlock];
    const int64_t i = blockIdx.x;
    spectral_stage_cholesky<D>(x + i * tri_size(D), Gs);
    double* oc = out + i * 2 * L;
    double* os = oc + L;
    double ss = 0.0;
    for (int64_t l0 = 0; l0 < L; l0 += kSpectralBlock) {
        const int64_t l = l0 + threadIdx.x;
        const int64_t lc = l < L ? l : L - 1;
        double theta = 0.0, la = 0.0;
        spectral_logdiag_lane<D>(Gs, phases + lc, L, [&](auto kk, double ak) {
            constexpr int k = decltype(kk)::value;
            theta = __builtin_fma(lam[lc * D + k], ak, theta);
            la = __builtin_fma(-0.25 * (double)(D - 1 - 2 * k), ak, la);          // rho_k = (d + 1 - 2 k) / 4, k = 1 .. d
        });
        const SpectralPair f = spectral_feature_value(theta, la, weight[lc]);
        const double fc = f.c, fs = f.s;
        if (l < L) {
            oc[l] = fc;
            os[l] = fs;
            ss = __builtin_fma(fc, fc, ss);
            ss = __builtin_fma(fs, fs, ss);
        }
    }
    red[threadIdx.x] = ss;
    __syncthreads();
    for (int s = kSpectralBlock / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] = red[threadIdx.x] + red[threadIdx.x + s];
        __syncthreads();
    }
    const double scale = 1.0 / __builtin_sqrt(red[0]);
    for (int64_t l = threadIdx.x; l < L; l += kSpectralBlock) {          // (each lane reads back its own stores)
        oc[l] = oc[l] * scale;
        os[l] = os[l] * scale;
    }
}

}  // namespace gabo

extern "C" {

int gabo_spd_ai_logdiag(const double* x_mandel, const double* phases, double* out, int64_t n, int64_t L, int d, gabo_stream_t stream) {
    if (n < 0 || L < 0) return GABO_ERR_ARG;
    if (d < 2 || d > gabo::kSpectralMaxDim) return GABO_ERR_DIM;
    if (n == 0 || L == 0) return GABO_OK;
    const int64_t chunks = (L + gabo::kSpectralBlock - 1) / gabo::kSpectralBlock;
    if (!x_mandel || !phases || !out || chunks > 0x7fffffffLL || n > 0x7fffffffLL / chunks) return GABO_ERR_ARG;
    const dim3 grid((unsigned)(n * chunks));
#define GABO_CASE(DD)                                                                                                                      \
    case DD:                                                                                                                               \
        hipLaunchKernelGGL(gabo::spd_ai_logdiag_kernel<DD>, grid, dim3(gabo::kSpectralBlock), 0, (hipStream_t)stream, x_mandel, phases, out, \
                           L, (int)chunks);                                                                                                \
        break;
    switch (d) { GABO_CASE(2) GABO_CASE(3) GABO_CASE(4) GABO_CASE(5) GABO_CASE(6) GABO_CASE(7) GABO_CASE(8) GABO_CASE(9) GABO_CASE(10) }
#undef GABO_CASE
    return hipGetLastError() == hipSuccess ? GABO_OK : GABO_ERR_LAUNCH;
}

int gabo_spd_ai_spectral_features(const double* x_mandel, const double* phases, const double* lam, const double* weight, double* out,
                                  int64_t n, int64_t L, int d, gabo_stream_t stream) {
    if (n < 0 || L < 0) return GABO_ERR_ARG;
    if (d < 2 || d > gabo::kSpectralMaxDim) return GABO_ERR_DIM;
    if (n == 0 || L == 0) return GABO_OK;
    if (!x_mandel || !phases || !lam || !weight || !out || n > 0x7fffffffLL) return GABO_ERR_ARG;
    const dim3 grid((unsigned)n);
#define GABO_CASE(DD)                                                                                                                       \
    case DD:                                                                                                                                \
        hipLaunchKernelGGL(gabo::spd_ai_spectral_features_kernel<DD>, grid, dim3(gabo::kSpectralBlock), 0, (hipStream_t)stream, x_mandel,   \
                           phases, lam, weight, out, L);                                                                                    \
        break;
    switch (d) { GABO_CASE(2) GABO_CASE(3) GABO_CASE(4) GABO_CASE(5) GABO_CASE(6) GABO_CASE(7) GABO_CASE(8) GABO_CASE(9) GABO_CASE(10) }
#undef GABO_CASE
    return hipGetLastError() == hipSuccess ? GABO_OK : GABO_ERR_LAUNCH;
}
}
