// One evaluation of the surrogate-fit objective of [ScaleKernel of] SpdAffineInvariantMaternKernel with its gradient, as ONE host call:
// the marginal log likelihood of Ky = outputscale K(kappa) + noise I with d ll / d (kappa, outputscale, noise, mean).
// During a fit the log-diagonals a_il = 2 log diag chol(H_l^T X_i H_l) (gabo_spd_ai_logdiag, the expensive launch) do not move; only the
// spectral points lam_l = e_l g(kappa) and the weights w_l = prod_{i<j} tanh(pi |lam_li - lam_lj|) do, and d lam_l / d kappa = c lam_l with
// ONE scalar c = g'/g for every feature:  c = -1 / kappa (heat),  c = -nu / (kappa (nu + b kappa^2)), b = d (d^2 - 1) / 96 (Matern).
// With rho_k = (d + 1 - 2k) / 4, u_il = sqrt(w_l) exp(-rho . a_il), theta_il = lam_l . a_il, f_i = [u cos theta | u sin theta],
// s_i = sum_l u_il^2, Fh_i = f_i / sqrt(s_i) and q_l = (d log w_l / d kappa) / 2 = c sum_{i<j} pi |D_ij| / sinh(2 pi |D_ij|):
//     df_cos = q f_cos - c theta f_sin,   df_sin = q f_sin + c theta f_cos,   Gd_i = d Fh_i / d kappa = df_i / sqrt(s_i) - Fh_i (sum_l u_il^2 q_l) / s_i
//     K_ij = Fh_i . Fh_j (K_ii = 1),   dK_ij / d kappa = Gd_i . Fh_j + Fh_i . Gd_j (dK_ii = 0)
//     d ll / d kappa = outputscale sum_ij W_ij dK_ij / 2 = outputscale sum_{i != j} W_ij (Gd_i . Fh_j)        (W = alpha alpha^T - Ky^-1 is symmetric)
//
//   spd_ai_spectral_points_kernel            a lane per feature: lam, w, q and c from (e, gamma, kappa, nu)
//   spd_ai_spectral_features_dkappa_kernel   a block per point: Fh and Gd from the stored a; theta, rho . a and the row sum of squares in the
//                                            operation order of spd_ai_spectral_features_kernel, so Fh has the bits of that launch
//   spd_ai_feature_gram_kernel               K = Fh Fh^T on the fp64 matrix pipe, 16 x 16 tiles i >= j with the mirror image stored from the same
//                                            registers: exactly symmetric, the diagonal v / v (1, or NaN for a NaN row)
//   spd_ai_fit_trace_kernel (+ _finish)      per tile of all n^2: (Gd Fh^T) o W summed in a fixed order -> one partial per tile; one block then
//                                            adds the partials in a fixed order: dK is never stored
//
// Both products use v_mfma_f64_16x16x4_f64 with the lane layout of gp_posterior.hip (A[lane & 15][k = lane >> 4], B[k = lane >> 4][lane & 15],
// C/D col = lane & 15, row = (lane >> 4) + 4 reg) on operands padded with zeros IN the workspace to whole tiles (16 rows) and to 16 columns:
// no guard and no branch in the product loop, no load outside the workspace.  A tile is one workgroup of four waves; wave v runs the
// v-th quarter of the (padded) feature index in ascending order and the quarters are added as (0 + 1) + (2 + 3), so the bits of an entry
// depend on its two rows and on L alone - not on n, the tile or the grid.
#include <hip/hip_runtime.h>

#include <cmath>

#include "fit_chain.hpp"
#include "gabo_device.hpp"
#include "gabo_mirror.hpp"
#include "spd_ai_spectral_value.hpp"
#include "../../include/gabo_hip.h"

namespace gabo {

typedef double v4d __attribute__((ext_vector_type(4)));

constexpr int kFitTile = 16;                 // rows and columns of a product tile
constexpr int kFitKPad = 16;                 // the feature index is padded to a multiple of it: four waves x one k-step of 4
constexpr int64_t kFitMaxFeatures = (int64_t)1 << 24;

__host__ __device__ constexpr int64_t fit_npad(int64_t n) { return (n + kFitTile - 1) / kFitTile * kFitTile; }
__host__ __device__ constexpr int64_t fit_kpad(int64_t k) { return (k + kFitKPad - 1) / kFitKPad * kFitKPad; }

// lam (L, d), w (L), q (L), c (1).  gamma == NULL: the heat kernel.  The operations of ops.spd_ai_spectral_points, in its order.
template <int D>
__global__ __launch_bounds__(kSpectralBlock) void spd_ai_spectral_points_kernel(const double* __restrict__ e, const double* __restrict__ gamma,
                                                                                double* __restrict__ lam, double* __restrict__ weight,
                                                                                double* __restrict__ q, double* __restrict__ c_out, int64_t L,
                                                                                double kappa, double nu) {
    constexpr double kPi = 3.14159265358979311600e+00;
    constexpr double b = D * (D * D - 1) / 96.0;
    const int64_t l = (int64_t)blockIdx.x * kSpectralBlock + threadIdx.x;
    const bool heat = gamma == nullptr;
    const double c = heat ? -1.0 / kappa : -nu / (kappa * (nu + b * (kappa * kappa)));
    if (l == 0) c_out[0] = c;
    if (l >= L) return;
    const double g = heat ? 0.0 : __builtin_sqrt((nu / (kappa * kappa) + b) / gamma[l]);
    double lm[D];
    static_for<D>([&](auto kk) {
        constexpr int k = decltype(kk)::value;
        const double ek = e[l * D + k];
        lm[k] = heat ? ek / kappa : ek * g;
        lam[l * D + k] = lm[k];
    });
    double w = 1.0, s = 0.0;
    static_for<D>([&](auto ii) {
        constexpr int i = decltype(ii)::value;
        static_for<D - 1 - i>([&](auto tt) {
            constexpr int j = i + 1 + decltype(tt)::value;
            const double x = kPi * __builtin_fabs(lm[i] - lm[j]);
            w = w * tanh(x);
            const double x2 = 2.0 * x;
            s = s + (x2 > 0.0 ? x / sinh(x2) : 0.5);          // x / sinh(2 x) -> 1/2 at 0, -> 0 where sinh overflows; a NaN x
                                                              // also takes the 1/2: w is NaN there and the feature with it
        });
    });
    weight[l] = w;
    q[l] = c * s;
}

// One block per row of the outputs (row stride ld >= 2 L).  Rows i < n: Fh_i and Gd_i, columns 2 L ... ld - 1 zero; rows i >= n (the
// padding of the chain's workspace): zeros.
template <int D>
__global__ __launch_bounds__(kSpectralBlock) void spd_ai_spectral_features_dkappa_kernel(const double* __restrict__ a, const double* __restrict__ lam,
                                                                                         const double* __restrict__ weight, const double* __restrict__ q,
                                                                                         const double* __restrict__ c_in, double* __restrict__ fhat,
                                                                                         double* __restrict__ gdot, int64_t n, int64_t L, int64_t ld) {
    __shared__ double red[kSpectralBlock];
    __shared__ double redq[kSpectralBlock];
    const int64_t i = blockIdx.x;
    double* fc = fhat + i * ld;
    double* fs = fc + L;
    double* gc = gdot + i * ld;
    double* gs = gc + L;
    if (i >= n) {
        for (int64_t col = threadIdx.x; col < ld; col += kSpectralBlock) fc[col] = gc[col] = 0.0;
        return;
    }
    const double c = c_in[0];
    double ss = 0.0, sq = 0.0;
    for (int64_t l = threadIdx.x; l < L; l += kSpectralBlock) {
        const double* al = a + (i * L + l) * D;
        double theta = 0.0, la = 0.0;
        static_for<D>([&](auto kk) {
            constexpr int k = decltype(kk)::value;
            const double ak = al[k];
            theta = __builtin_fma(lam[l * D + k], ak, theta);
            la = __builtin_fma(-0.25 * (double)(D - 1 - 2 * k), ak, la);          // rho_k = (d + 1 - 2 k) / 4, k = 1 .. d
        });
        const SpectralPair f = spectral_feature_value(theta, la, weight[l]);
        const double vc = f.c, vs = f.s, ql = q[l], ct = c * theta;
        fc[l] = vc;
        fs[l] = vs;
        gc[l] = __builtin_fma(-ct, vs, ql * vc);
        gs[l] = __builtin_fma(ct, vc, ql * vs);
        ss = __builtin_fma(vc, vc, ss);
        ss = __builtin_fma(vs, vs, ss);
        sq = __builtin_fma(ql * vc, vc, sq);
        sq = __builtin_fma(ql * vs, vs, sq);
    }
    red[threadIdx.x] = ss;
    redq[threadIdx.x] = sq;
    spectral_row_tree(red);
    spectral_row_tree(redq);
    const double scale = 1.0 / __builtin_sqrt(red[0]);
    const double ratio = redq[0] / red[0];
    for (int64_t l = threadIdx.x; l < L; l += kSpectralBlock) {          // (each lane reads back its own stores)
        const double hc = fc[l] * scale, hs = fs[l] * scale;
        fc[l] = hc;
        fs[l] = hs;
        gc[l] = __builtin_fma(-hc, ratio, gc[l] * scale);
        gs[l] = __builtin_fma(-hs, ratio, gs[l] * scale);
    }
    for (int64_t col = 2 * L + threadIdx.x; col < ld; col += kSpectralBlock) fc[col] = gc[col] = 0.0;
}

// Entry (row, col) of the 16 x 16 tile  A_rows B_rows^T  for the calling thread, row = ((tid & 63) >> 4) + 4 (tid >> 6), col = tid & 15:
// pa, pb point at the first of the tile's 16 rows in the two padded operands (row stride kpad, a multiple of kFitKPad).  `part`: 4 x 4 x 64
// doubles of LDS.  All 256 threads call it.
__device__ __forceinline__ double fit_tile_product(const double* __restrict__ pa, const double* __restrict__ pb, int64_t kpad, double* part) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t kq = kpad >> 2;
    const double* ra = pa + (int64_t)(lane & 15) * kpad + wave * kq + (lane >> 4);
    const double* rb = pb + (int64_t)(lane & 15) * kpad + wave * kq + (lane >> 4);
    v4d acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll 8
    for (int64_t k0 = 0; k0 < kq; k0 += 4) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(ra[k0], rb[k0], acc, 0, 0, 0);
#pragma unroll
    for (int r = 0; r < 4; ++r) part[(wave * 4 + r) * 64 + lane] = acc[r];
    __syncthreads();
    const int r = wave;                          // this thread now owns register r of lane `lane` of every wave's accumulator
    return (part[(0 * 4 + r) * 64 + lane] + part[(1 * 4 + r) * 64 + lane]) + (part[(2 * 4 + r) * 64 + lane] + part[(3 * 4 + r) * 64 + lane]);
}

// blockIdx.x: the tile (bi >= bj) of lower_tile_of.  f: npad x kpad.  k: n x n.
__global__ __launch_bounds__(256) void spd_ai_feature_gram_kernel(const double* __restrict__ f, double* __restrict__ k, int64_t n, int64_t kpad) {
    __shared__ double part[4 * 4 * 64];
    int64_t bi, bj;
    lower_tile_of(blockIdx.x, bi, bj);
    const double v = fit_tile_product(f + bi * kFitTile * kpad, f + bj * kFitTile * kpad, kpad, part);
    const int tid = threadIdx.x;
    const int64_t row = bi * kFitTile + ((tid & 63) >> 4) + 4 * (tid >> 6), col = bj * kFitTile + (tid & 15);
    if (row >= n || col > row) return;           // (col <= row < n; a diagonal tile stores its lower half and the mirror of it)
    if (row == col) {
        k[row * n + row] = v / v;                // exactly 1, or NaN for a row of NaN features
    } else {
        k[row * n + col] = v;
        k[col * n + row] = v;
    }
}

// blockIdx.x = bi * tiles + bj over ALL tiles: partial[blockIdx.x] = sum over the tile of W_ij (Gd_i . Fh_j), i != j, i, j < n.
__global__ __launch_bounds__(256) void spd_ai_fit_trace_kernel(const double* __restrict__ gdot, const double* __restrict__ fhat,
                                                               const double* __restrict__ wm, double* __restrict__ partial, int64_t n,
                                                               int64_t kpad, int tiles) {
    __shared__ double part[4 * 4 * 64];
    __shared__ double red[256];
    const int64_t bi = blockIdx.x / (uint32_t)tiles, bj = blockIdx.x - (uint32_t)bi * (uint32_t)tiles;
    const double v = fit_tile_product(gdot + bi * kFitTile * kpad, fhat + bj * kFitTile * kpad, kpad, part);
    const int tid = threadIdx.x;
    const int64_t row = bi * kFitTile + ((tid & 63) >> 4) + 4 * (tid >> 6), col = bj * kFitTile + (tid & 15);
    red[tid] = (row < n && col < n && row != col) ? wm[row * n + col] * v : 0.0;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) red[tid] = red[tid] + red[tid + s];
        __syncthreads();
    }
    if (tid == 0) partial[blockIdx.x] = red[0];
}

// out[6] = outputscale * (the partials added in a fixed order: each thread its own in ascending order, then the halving tree), or 0 when the
// likelihood launch flagged Ky as not positive definite (out[5] != 0).
__global__ __launch_bounds__(256) void spd_ai_fit_trace_finish_kernel(const double* __restrict__ partial, int64_t count, double outputscale,
                                                                      double* __restrict__ out) {
    __shared__ double red[256];
    const int tid = threadIdx.x;
    double s = 0.0;
    for (int64_t b = tid; b < count; b += 256) s = s + partial[b];
    red[tid] = s;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (tid < h) red[tid] = red[tid] + red[tid + h];
        __syncthreads();
    }
    if (tid == 0) out[6] = out[5] != 0.0 ? 0.0 : outputscale * red[0];
}

namespace {

bool spectral_dims_ok(int64_t n, int d) { return n >= 1 && n <= GABO_GP_MLL_LARGE_MAX_N && d >= 2 && d <= kSpectralMaxDim; }

int spectral_points_launch(const double* e, const double* gamma, int64_t L, int d, double kappa, double nu, double* lam, double* weight,
                           double* q, double* c, hipStream_t s) {
    const dim3 grid((unsigned)((L + kSpectralBlock - 1) / kSpectralBlock));
#define GABO_CASE(DD)                                                                                                                         \
    case DD:                                                                                                                                  \
        hipLaunchKernelGGL(spd_ai_spectral_points_kernel<DD>, grid, dim3(kSpectralBlock), 0, s, e, gamma, lam, weight, q, c, L, kappa, nu);   \
        break;
    switch (d) { GABO_CASE(2) GABO_CASE(3) GABO_CASE(4) GABO_CASE(5) GABO_CASE(6) GABO_CASE(7) GABO_CASE(8) GABO_CASE(9) GABO_CASE(10) }
#undef GABO_CASE
    return hipGetLastError() == hipSuccess ? GABO_OK : GABO_ERR_LAUNCH;
}

// rows: blocks to launch (n, or the padded row count of the chain's workspace)
int spectral_features_launch(const double* a, const double* lam, const double* weight, const double* q, const double* c, double* fhat,
                             double* gdot, int64_t n, int64_t rows, int64_t L, int d, int64_t ld, hipStream_t s) {
    const dim3 grid((unsigned)rows);
#define GABO_CASE(DD)                                                                                                                         \
    case DD:                                                                                                                                  \
        hipLaunchKernelGGL(spd_ai_spectral_features_dkappa_kernel<DD>, grid, dim3(kSpectralBlock), 0, s, a, lam, weight, q, c, fhat, gdot, n, \
                           L, ld);                                                                                                            \
        break;
    switch (d) { GABO_CASE(2) GABO_CASE(3) GABO_CASE(4) GABO_CASE(5) GABO_CASE(6) GABO_CASE(7) GABO_CASE(8) GABO_CASE(9) GABO_CASE(10) }
#undef GABO_CASE
    return hipGetLastError() == hipSuccess ? GABO_OK : GABO_ERR_LAUNCH;
}

int feature_gram_launch(const double* fpad, double* k, int64_t n, int64_t kpad, hipStream_t s) {
    const int64_t tiles = fit_npad(n) / kFitTile;
    hipLaunchKernelGGL(spd_ai_feature_gram_kernel, dim3((unsigned)(tiles * (tiles + 1) / 2)), dim3(256), 0, s, fpad, k, n, kpad);
    return hipGetLastError() == hipSuccess ? GABO_OK : GABO_ERR_LAUNCH;
}

struct SpectralFitLayout : FitArena {
    size_t lam, w, q, c, fhat, gdot, kb, wm, out, partial, mll;
    int64_t npad, kpad, tiles;
    SpectralFitLayout(int64_t n, int64_t L, int d) {
        npad = fit_npad(n);
        kpad = fit_kpad(2 * L);
        tiles = npad / kFitTile;
        const size_t nn = (size_t)n * n;
        lam = take((size_t)L * d);
        w = take((size_t)L);
        q = take((size_t)L);
        c = take(1);
        fhat = take((size_t)npad * kpad);
        gdot = take((size_t)npad * kpad);
        kb = take(nn);
        wm = take(nn);
        out = take(8);                                     // [ll, 0, d os, d noise, d mean, flag, d kappa]
        partial = take((size_t)tiles * tiles);
        mll = take_mll(n);
    }
};

}  // namespace
}  // namespace gabo

extern "C" {

int gabo_spd_ai_spectral_points_dkappa(const double* e, const double* gamma, int64_t L, int d, double lengthscale, double nu, double* lam,
                                       double* weight, double* q, double* c, gabo_stream_t stream) {
    if (d < 2 || d > gabo::kSpectralMaxDim) return GABO_ERR_DIM;
    if (L < 1 || L > gabo::kFitMaxFeatures || !e || !lam || !weight || !q || !c) return GABO_ERR_ARG;
    if (!(lengthscale > 0.0) || std::isinf(lengthscale) || !(nu > 0.0) || (!std::isinf(nu) && !gamma)) return GABO_ERR_ARG;
    return gabo::spectral_points_launch(e, std::isinf(nu) ? nullptr : gamma, L, d, lengthscale, nu, lam, weight, q, c, (hipStream_t)stream);
}

int gabo_spd_ai_spectral_features_dkappa(const double* a, const double* lam, const double* weight, const double* q, const double* c,
                                         double* fhat, double* gdot, int64_t n, int64_t L, int d, gabo_stream_t stream) {
    if (d < 2 || d > gabo::kSpectralMaxDim) return GABO_ERR_DIM;
    if (n < 1 || n > 0x7fffffffLL || L < 1 || L > gabo::kFitMaxFeatures || !a || !lam || !weight || !q || !c || !fhat || !gdot) return GABO_ERR_ARG;
    return gabo::spectral_features_launch(a, lam, weight, q, c, fhat, gdot, n, n, L, d, 2 * L, (hipStream_t)stream);
}

size_t gabo_spd_ai_feature_gram_workspace_bytes(int64_t n, int64_t k) {
    if (n < 1 || n > GABO_GP_MLL_LARGE_MAX_N || k < 1 || k > 2 * gabo::kFitMaxFeatures) return 0;
    return (size_t)gabo::fit_npad(n) * (size_t)gabo::fit_kpad(k) * sizeof(double);
}

int gabo_spd_ai_feature_gram(const double* f, double* out, int64_t n, int64_t k, void* workspace, size_t workspace_bytes, gabo_stream_t stream) {
    if (n < 1 || n > GABO_GP_MLL_LARGE_MAX_N) return GABO_ERR_DIM;
    if (k < 1 || k > 2 * gabo::kFitMaxFeatures || !f || !out || !workspace) return GABO_ERR_ARG;
    const size_t need = gabo_spd_ai_feature_gram_workspace_bytes(n, k);
    if (workspace_bytes < need) return GABO_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    const int64_t kpad = gabo::fit_kpad(k);
    // the padded copy: zeros everywhere, then the n rows of k doubles at row stride kpad
    if (hipMemsetAsync(workspace, 0, need, s) != hipSuccess) return GABO_ERR_LAUNCH;
    if (hipMemcpy2DAsync(workspace, (size_t)kpad * sizeof(double), f, (size_t)k * sizeof(double), (size_t)k * sizeof(double), (size_t)n,
                         hipMemcpyDeviceToDevice, s) != hipSuccess)
        return GABO_ERR_LAUNCH;
    return gabo::feature_gram_launch(static_cast<const double*>(workspace), out, n, kpad, s);
}

size_t gabo_gp_mll_spd_ai_spectral_workspace_bytes(int64_t n, int64_t L, int d) {
    if (!gabo::spectral_dims_ok(n, d) || L < 1 || L > gabo::kFitMaxFeatures) return 0;
    return gabo::SpectralFitLayout(n, L, d).total;
}

int gabo_gp_mll_spd_ai_spectral(const double* a, const double* y, const double* e, const double* gamma, int64_t n, int64_t L, int d, double nu,
                                double lengthscale, double outputscale, double noise, double mean, double* out_host, void* workspace,
                                size_t workspace_bytes, double* pinned, size_t pinned_doubles, gabo_stream_t stream) {
    if (!gabo::spectral_dims_ok(n, d)) return GABO_ERR_DIM;
    if (L < 1 || L > gabo::kFitMaxFeatures || !a || !y || !e || !out_host || !workspace || !pinned) return GABO_ERR_ARG;
    if (!(lengthscale > 0.0) || std::isinf(lengthscale) || !(nu > 0.0) || (!std::isinf(nu) && !gamma)) return GABO_ERR_ARG;
    gabo::SpectralFitLayout lay(n, L, d);
    if (workspace_bytes < lay.total || pinned_doubles < 7) return GABO_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    lay.base = static_cast<char*>(workspace);
    auto at = [&lay](size_t off) { return lay.at(off); };
    double* d_out = at(lay.out);
    int rc = gabo::spectral_points_launch(e, std::isinf(nu) ? nullptr : gamma, L, d, lengthscale, nu, at(lay.lam), at(lay.w), at(lay.q), at(lay.c), s);
    if (rc == GABO_OK)
        rc = gabo::spectral_features_launch(a, at(lay.lam), at(lay.w), at(lay.q), at(lay.c), at(lay.fhat), at(lay.gdot), n, lay.npad, L, d, lay.kpad, s);
    if (rc == GABO_OK) rc = gabo::feature_gram_launch(at(lay.fhat), at(lay.kb), n, lay.kpad, s);
    if (rc != GABO_OK) return rc;
    rc = gabo::fit_likelihood(at(lay.kb), y, n, outputscale, noise, mean, d_out, at(lay.wm), lay.base + lay.mll, stream);
    if (rc != GABO_OK) return rc;
    hipLaunchKernelGGL(gabo::spd_ai_fit_trace_kernel, dim3((unsigned)(lay.tiles * lay.tiles)), dim3(256), 0, s, at(lay.gdot), at(lay.fhat),
                       at(lay.wm), at(lay.partial), n, lay.kpad, (int)lay.tiles);
    if (hipGetLastError() != hipSuccess) return GABO_ERR_LAUNCH;
    hipLaunchKernelGGL(gabo::spd_ai_fit_trace_finish_kernel, dim3(1), dim3(256), 0, s, at(lay.partial), lay.tiles * lay.tiles, outputscale, d_out);
    if (hipGetLastError() != hipSuccess) return GABO_ERR_LAUNCH;
    return gabo::fit_finish(d_out, pinned, out_host, 0, 1, s);
}

}  // extern "C"
