// The x-gradient of the normalised random phase features of spd_ai_spectral.hip (notation as there): for an upstream gradient Gb of Fh
// (n x 2L), grad_x = d <Gb, Fh> / d x_mandel, in closed form and without a tape.  With s_i = <Gb_i, Fh_i>, per (point i, feature l)
//     P = (Gb_c - s Fh_c) Fh_c + (Gb_s - s Fh_s) Fh_s        (adjoint of -rho . a; the row norm |F_i| cancels)
//     R = Gb_s Fh_c - Gb_c Fh_s                              (adjoint of theta = lam_l . a)
//     gb_k = -rho_k P + lam_lk R                             (adjoint of a_k)
// and d a_k / d X = G^-T (v_k v_k^T / |v_k|^2) G^-1 with v_k the rows the forward's Gram-Schmidt pass leaves (a_k is the difference of the
// log-determinants of two leading minors of H^T X H, whose gradient is t_k t_k^T, t_k row k of the inverse Cholesky factor, and
// H t_k = G^-T v_k / |v_k|).  So
//     Gamma_i = d / d X_i = G^-T S_i G^-1,   S_i = sum_l sum_k (gb_ilk / |v_ilk|^2) v_ilk v_ilk^T   (symmetric),
// and grad_x = mandel(Gamma_i): the diagonal, then the off-diagonals times sqrt 2.
// Two launches.  1: the forward's factorisation once more, one lane per (point, feature), and the lower triangle of the block's part of S_i
// by a halving tree in LDS -> workspace (n, chunks, tri).  2: per point, the chunk partials in ascending order, G and G^-1, the congruence.
// No atomics, no counter, nothing handed between workgroups inside a launch; one operation order whatever n: the bits of row i depend on
// X_i, row i of Fh and Gb, H, lam and L alone.  A NaN or non-SPD X_i makes G NaN and with it every entry of S_i and row i of the result;
// nothing is reported.
#include "gabo_device.hpp"
#include "spd_ai_spectral_lane.hpp"
#include "spd_ai_spectral_value.hpp"
#include "../../include/gabo_hip.h"

namespace gabo {

// blockIdx.x = point * chunks + chunk of kSpectralBlock features (the decode of spd_ai_logdiag_kernel); part (n, chunks, tri)
template <int D>
__global__ __launch_bounds__(kSpectralBlock) void spd_ai_spectral_backward_partial_kernel(
    const double* __restrict__ x, const double* __restrict__ phases, const double* __restrict__ lam, const double* __restrict__ fhat,
    const double* __restrict__ gout, double* __restrict__ part, int64_t L, int chunks) {
    constexpr int T = tri_size(D);
    __shared__ __attribute__((aligned(16))) double Gs[T + 1];
    __shared__ double red[kSpectralBlock];
    __shared__ double acc[T * kSpectralBlock];          // [entry][lane]
    const int64_t i = blockIdx.x / (uint32_t)chunks;
    const int chunk = (int)(blockIdx.x - (uint32_t)i * (uint32_t)chunks);
    const int64_t l = (int64_t)chunk * kSpectralBlock + threadIdx.x;
    spectral_stage_cholesky<D>(x + i * T, Gs);
    const double* fc = fhat + i * 2 * L;
    const double* fs = fc + L;
    const double* gc = gout + i * 2 * L;
    const double* gs = gc + L;
    // s_i over the whole row, the same bits in every chunk of the point: each lane over its features in ascending order, then the tree
    double dot = 0.0;
    for (int64_t ll = threadIdx.x; ll < L; ll += kSpectralBlock) {
        dot = __builtin_fma(gc[ll], fc[ll], dot);
        dot = __builtin_fma(gs[ll], fs[ll], dot);
    }
    red[threadIdx.x] = dot;
    spectral_row_tree(red);
    const double s = red[0];
    const int64_t lc = l < L ? l : L - 1;              // out-of-range lanes recompute the last feature and contribute an exact 0
    const double fcl = fc[lc], fsl = fs[lc], gcl = gc[lc], gsl = gs[lc];
    const double pc = __builtin_fma(-s, fcl, gcl), ps = __builtin_fma(-s, fsl, gsl);
    const double P = __builtin_fma(ps, fsl, pc * fcl);
    const double R = __builtin_fma(-gcl, fsl, gsl * fcl);
    double v[D * D], coef[D];                           // the rows, then c_k = gb_k / |v_k|^2 in place of 1 / |v_k|^2
    spectral_gram_schmidt_lane<D, D>(Gs, phases + lc, L, v, coef, [&](auto, double nn) { return nn; });
    static_for<D>([&](auto kk) {
        constexpr int k = decltype(kk)::value;
        const double gb = __builtin_fma(lam[lc * D + k], R, (-0.25 * (double)(D - 1 - 2 * k)) * P);          // rho_k as the forward spells it
        coef[k] = gb * coef[k];
    });
    // S[r][c] = sum_k (c_k v_k[r]) v_k[c], k ascending, r >= c
    static_for<D>([&](auto rr) {
        constexpr int r = decltype(rr)::value;
        double u[D];
        static_for<D>([&](auto kk) { constexpr int k = decltype(kk)::value; u[k] = coef[k] * v[k * D + r]; });
        static_for<r + 1>([&](auto cc) {
            constexpr int c = decltype(cc)::value;
            double e = u[0] * v[c];
            static_for<D - 1>([&](auto kk) { constexpr int k = 1 + decltype(kk)::value; e = __builtin_fma(u[k], v[k * D + c], e); });
            acc[tri(r, c) * kSpectralBlock + threadIdx.x] = l < L ? e : 0.0;
        });
    });
    __syncthreads();
    for (int h = kSpectralBlock / 2; h > 0; h >>= 1) {          // every entry's halving tree, the lanes shared out over (entry, slot)
        for (int idx = threadIdx.x; idx < T * h; idx += kSpectralBlock) {
            const int e = idx / h, j = idx - e * h;
            acc[e * kSpectralBlock + j] = acc[e * kSpectralBlock + j] + acc[e * kSpectralBlock + j + h];
        }
        __syncthreads();
    }
    if ((int)threadIdx.x < T) part[((int64_t)blockIdx.x) * T + threadIdx.x] = acc[threadIdx.x * kSpectralBlock];
}

// One block of one wave per point: S_i = the chunk partials in ascending order, G = chol(X_i) as the forward forms it, W = G^-1 by forward
// substitution (a lane per column), Y = S W, then the lower triangle of Gamma = W^T Y, a lane per entry, -> grad (n, tri) in Mandel order.
template <int D>
__global__ __launch_bounds__(64) void spd_ai_spectral_backward_finish_kernel(const double* __restrict__ x, const double* __restrict__ part,
                                                                             double* __restrict__ grad, int chunks) {
    constexpr int T = tri_size(D);
    __shared__ __attribute__((aligned(16))) double Gs[T + 1];
    __shared__ double Ss[T], Ws[T], Ys[D * D];
    const int64_t i = blockIdx.x;
    const int t = threadIdx.x;
    spectral_stage_cholesky<D>(x + i * T, Gs);
    if (t < T) {
        const double* p = part + i * chunks * T + t;
        double s = p[0];
        for (int ch = 1; ch < chunks; ++ch) s = s + p[(int64_t)ch * T];
        Ss[t] = s;
    }
    if (t < D) {          // column t of W: W[t][t] = 1 / G[t][t], W[r][t] = -(sum_{t <= k < r} G[r][k] W[k][t]) / G[r][r]
        Ws[tri(t, t)] = 1.0 / Gs[tri(t, t)];
        for (int r = t + 1; r < D; ++r) {
            double s = Gs[tri(r, t)] * Ws[tri(t, t)];
            for (int k = t + 1; k < r; ++k) s = __builtin_fma(Gs[tri(r, k)], Ws[tri(k, t)], s);
            Ws[tri(r, t)] = -s / Gs[tri(r, r)];
        }
    }
    __syncthreads();
    for (int e = t; e < D * D; e += 64) {          // Y[a][b] = sum_{k >= b} S[a][k] W[k][b]
        const int a = e / D, b = e - a * D;
        double s = Ss[a >= b ? tri(a, b) : tri(b, a)] * Ws[tri(b, b)];
        for (int k = b + 1; k < D; ++k) s = __builtin_fma(Ss[a >= k ? tri(a, k) : tri(k, a)], Ws[tri(k, b)], s);
        Ys[e] = s;
    }
    __syncthreads();
    if (t < T) {          // Gamma[r][c] = sum_{a >= r} W[a][r] Y[a][c], r >= c: lane t takes the entry at Mandel position t
        int k = 0, before = 0;
        while (t >= before + (D - k)) {
            before += D - k;
            ++k;
        }
        const int c = t - before, r = c + k;
        double s = Ws[tri(r, r)] * Ys[r * D + c];
        for (int a = r + 1; a < D; ++a) s = __builtin_fma(Ws[tri(a, r)], Ys[a * D + c], s);
        grad[i * T + t] = k == 0 ? s : s * kSqrt2;
    }
}

static bool backward_shape_ok(int64_t n, int64_t L, int d, int64_t* chunks_out) {
    if (n < 0 || L < 0 || d < 2 || d > kSpectralMaxDim) return false;
    const int64_t chunks = (L + kSpectralBlock - 1) / kSpectralBlock;
    if (chunks > 0x7fffffffLL || (chunks > 0 && n > 0x7fffffffLL / chunks)) return false;
    *chunks_out = chunks;
    return true;
}

}  // namespace gabo

extern "C" {

size_t gabo_spd_ai_spectral_features_backward_workspace_bytes(int64_t n, int64_t L, int d) {
    int64_t chunks = 0;
    if (!gabo::backward_shape_ok(n, L, d, &chunks)) return 0;
    return (size_t)(n * chunks) * (size_t)gabo::tri_size(d) * sizeof(double);
}

int gabo_spd_ai_spectral_features_backward(const double* x_mandel, const double* phases, const double* lam, const double* fhat,
                                           const double* grad_out, double* grad_x, void* workspace, size_t workspace_bytes, int64_t n,
                                           int64_t L, int d, gabo_stream_t stream) {
    if (n < 0 || L < 0) return GABO_ERR_ARG;
    if (d < 2 || d > gabo::kSpectralMaxDim) return GABO_ERR_DIM;
    if (n == 0 || L == 0) return GABO_OK;
    int64_t chunks = 0;
    if (!x_mandel || !phases || !lam || !fhat || !grad_out || !grad_x || !workspace || !gabo::backward_shape_ok(n, L, d, &chunks) ||
        workspace_bytes < gabo_spd_ai_spectral_features_backward_workspace_bytes(n, L, d))
        return GABO_ERR_ARG;
    double* part = static_cast<double*>(workspace);
#define GABO_CASE(DD)                                                                                                                       \
    case DD:                                                                                                                                \
        hipLaunchKernelGGL(gabo::spd_ai_spectral_backward_partial_kernel<DD>, dim3((unsigned)(n * chunks)), dim3(gabo::kSpectralBlock), 0, \
                           (hipStream_t)stream, x_mandel, phases, lam, fhat, grad_out, part, L, (int)chunks);                               \
        hipLaunchKernelGGL(gabo::spd_ai_spectral_backward_finish_kernel<DD>, dim3((unsigned)n), dim3(64), 0, (hipStream_t)stream, x_mandel, \
                           part, grad_x, (int)chunks);                                                                                      \
        break;
    switch (d) { GABO_CASE(2) GABO_CASE(3) GABO_CASE(4) GABO_CASE(5) GABO_CASE(6) GABO_CASE(7) GABO_CASE(8) GABO_CASE(9) GABO_CASE(10) }
#undef GABO_CASE
    return hipGetLastError() == hipSuccess ? GABO_OK : GABO_ERR_LAUNCH;
}
}
