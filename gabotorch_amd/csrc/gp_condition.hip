// Conditioning the prediction cache of an exact GP on t more observations without a new factorisation: the bordered updates of L^-1, L^-T,
// alpha = Ky^-1 (y - mean) and A = Ky^-1 ([3P] gpytorch's prediction strategy behind condition_on_observations / get_fantasy_model, SURVEY
// App. B; the "Kriging believer" of Ginsbourger et al. 2010 when the new target is the current posterior mean).  With N points in the cache
// and c = os [k(x_new, x_0 ... x_N-1)], kappa = os k(x_new, x_new) + noise:
//
//   l = L^-1 c,  lambda^2 = kappa - l.l,  u = L^-T l = A c
//   L^-1  <- [[L^-1, 0], [-u^T / lambda, 1 / lambda]]
//   alpha <- [alpha - gamma u ; gamma],  gamma = (y - mean - c.alpha) / lambda^2
//   A     <- [[A + u u^T / lambda^2, -u / lambda^2], [-u^T / lambda^2, 1 / lambda^2]]
//
// O(N^2) per point, all of it matrix-vector work on the fp64 vector pipe (nothing here has a second matrix dimension to feed the matrix
// pipe with, as in gram_eig.hip).  One launch copies the old blocks into the outputs at the new leading dimension (zeros elsewhere, L^-T
// transposed through LDS); then three launches per point append in place:
//
//   gp_condition_l_kernel       l: a wave per row of L^-1, lanes along the row (coalesced), k ascending per lane, one fixed wave sum.
//   gp_condition_u_kernel       u: a workgroup per strip of 64 columns, lanes along the columns (coalesced), wave w takes the rows
//                               i = 16 m + w ascending, the 16 partial sums are added pairwise in a fixed tree.  One more workgroup forms
//                               lambda^2, y and gamma (l.l and c.alpha: two terms per thread at most, wave sums, then the 16 waves in order).
//   gp_condition_store_kernel   row N of L^-1, column N of L^-T, alpha, and A by 32 x 32 tiles on and below the diagonal, each tile writing
//                               its own mirror image through LDS: A is exactly symmetric whatever the input's upper triangle held.
//
// Every sum is over the absolute index of the training point with a tree that depends on that index and N alone: a result's bits depend
// neither on the leading dimension nor on t, so one call with t points equals t calls with one.  Only the lower triangle of the input
// L^-1 and the lower triangle of knew are read.  Divisions and the square root are the IEEE ones.
#include "gabo_device.hpp"
#include "gabo_mirror.hpp"
#include "../../include/gabo_hip.h"

namespace gabo {

constexpr int kCondStrip = 64;           // columns of L^-1 per workgroup of the u kernel (one per lane)
constexpr int kCondWaves = 16;           // its waves: the rows of the strip are dealt to them round robin
constexpr int kCondThreads = kCondStrip * kCondWaves;
static_assert(GABO_GP_MLL_LARGE_MAX_N <= 2 * kCondThreads, "the scalar workgroup takes two terms per thread at most");

// entry k of c for new point j: the cross strip for the old points, the lower triangle of knew for the new points before j
__device__ __forceinline__ double cond_c(const double* __restrict__ kcross, const double* __restrict__ knew, int n, int t, int j, int k,
                                         double outputscale) {
    return outputscale * (k < n ? kcross[(int64_t)j * n + k] : knew[j * t + (k - n)]);
}

// All 32 x 32 tiles of the m x m outputs (m = n + t), blockIdx = (tile column, tile row): the lower triangle of linv, kinv as it is, zeros
// beyond n and above the diagonal of linv; linv_t_out receives the transposed tile.  The tiles of column 0 also copy alpha.
__global__ __launch_bounds__(256) void gp_condition_copy_kernel(const double* __restrict__ linv, const double* __restrict__ alpha,
                                                                const double* __restrict__ kinv, int n, int m, double* __restrict__ linv_out,
                                                                double* __restrict__ linv_t_out, double* __restrict__ alpha_out,
                                                                double* __restrict__ kinv_out) {
    __shared__ double tile[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int i0 = blockIdx.y * 32, k0 = blockIdx.x * 32;
    for (int r = ty; r < 32; r += 8) {
        const int i = i0 + r, k = k0 + tx;
        const double v = (i < n && k <= i) ? linv[(int64_t)i * n + k] : 0.0;
        tile[r][tx] = v;
        if (i < m && k < m) {
            linv_out[(int64_t)i * m + k] = v;
            if (kinv_out) kinv_out[(int64_t)i * m + k] = (i < n && k < n) ? kinv[(int64_t)i * n + k] : 0.0;
        }
    }
    if (blockIdx.x == 0 && ty == 0 && i0 + tx < m) alpha_out[i0 + tx] = i0 + tx < n ? alpha[i0 + tx] : 0.0;
    if (!linv_t_out) return;
    __syncthreads();
    for (int r = ty; r < 32; r += 8) {
        const int k = k0 + r, i = i0 + tx;       // row k of L^-T, columns i
        if (k < m && i < m) linv_t_out[(int64_t)k * m + i] = tile[tx][r];
    }
}

// l[i] = sum_{k <= i} linv[i][k] c[k], i < N = n + j: wave `4 blockIdx + wave` owns row i
__global__ __launch_bounds__(256) void gp_condition_l_kernel(const double* __restrict__ linv, int m, const double* __restrict__ kcross,
                                                             const double* __restrict__ knew, int n, int t, int j, double outputscale,
                                                             double* __restrict__ l) {
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n + j) return;                      // (the whole wave)
    const double* row = linv + (int64_t)i * m;
    double acc = 0.0;
    for (int k = lane; k <= i; k += 64) acc = __builtin_fma(row[k], cond_c(kcross, knew, n, t, j, k, outputscale), acc);
    acc = wave_allsum(acc);
    if (lane == 0) l[i] = acc;
}

// the 16 partial sums of a column, added pairwise: ((p0 + p1) + (p2 + p3)) + ... whatever the grid is
__device__ __forceinline__ double cond_tree16(const double* p, int stride) {
    double s[kCondWaves];
#pragma unroll
    for (int w = 0; w < kCondWaves; ++w) s[w] = p[w * stride];
#pragma unroll
    for (int width = kCondWaves / 2; width >= 1; width >>= 1)
#pragma unroll
        for (int w = 0; w < width; ++w) s[w] = s[2 * w] + s[2 * w + 1];
    return s[0];
}

// Workgroups 0 ... strips - 1: u[k] = sum_{i >= k} linv[i][k] l[i] for the 64 columns of a strip.  Workgroup `strips`: scal = {lambda^2,
// lambda, gamma}, y_out[j] and the status word.
__global__ __launch_bounds__(kCondThreads) void gp_condition_u_kernel(const double* __restrict__ linv, int m, const double* __restrict__ kcross,
                                                                      const double* __restrict__ knew, const double* __restrict__ y_new,
                                                                      const double* __restrict__ alpha, int n, int t, int j,
                                                                      double outputscale, double noise, double mean,
                                                                      const double* __restrict__ l, double* __restrict__ u,
                                                                      double* __restrict__ scal, double* __restrict__ y_out,
                                                                      int* __restrict__ status) {
    __shared__ double sl[GABO_GP_MLL_LARGE_MAX_N];
    __shared__ double part[kCondWaves][kCondStrip];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int N = n + j;
    const int strips = (N + kCondStrip - 1) / kCondStrip;
    if ((int)blockIdx.x < strips) {
        for (int i = tid; i < N; i += kCondThreads) sl[i] = l[i];
        __syncthreads();
        const int k0 = blockIdx.x * kCondStrip, k = k0 + lane;
        double acc = 0.0;
        if (k < N) {
            const double* col = linv + k;
#pragma unroll 4
            for (int i = k0 + wave; i < N; i += kCondWaves)
                if (i >= k) acc = __builtin_fma(col[(int64_t)i * m], sl[i], acc);
        }
        part[wave][lane] = acc;
        __syncthreads();
        if (wave == 0 && k < N) u[k] = cond_tree16(&part[0][lane], kCondStrip);
        return;
    }
    double ll = 0.0, ca = 0.0;
    for (int i = tid; i < N; i += kCondThreads) {
        const double li = l[i];
        ll = __builtin_fma(li, li, ll);
        ca = __builtin_fma(cond_c(kcross, knew, n, t, j, i, outputscale), alpha[i], ca);
    }
    ll = wave_allsum(ll);
    ca = wave_allsum(ca);
    if (lane == 0) {
        part[0][wave] = ll;
        part[1][wave] = ca;
    }
    __syncthreads();
    if (tid != 0) return;
    ll = 0.0;
    ca = 0.0;
    for (int w = 0; w < kCondWaves; ++w) {
        ll += part[0][w];
        ca += part[1][w];
    }
    const double kappa = __builtin_fma(outputscale, knew[j * t + j], noise);
    const double lam2 = kappa - ll;
    const double y = y_new ? y_new[j] : mean + ca;
    scal[0] = lam2;
    scal[1] = sqrt(lam2);
    scal[2] = y_new ? ((y - mean) - ca) / lam2 : 0.0;        // (the believer's residual is zero by definition, not by rounding)
    y_out[j] = y;
    if (!(lam2 > 0.0) || !(lam2 < __builtin_inf())) {
        if (status[0] == 0) {                    // (the first offender: the launches of one call run in order)
            status[0] = GABO_ERR_NOT_SPD;
            status[1] = j;
        }
    }
}

// Workgroups 0 ... vec - 1 (256 entries each): row N of linv, column N of linv_t, alpha.  The others, when kinv is given: tile
// (bi >= bj) of the (N + 1) x (N + 1) leading block of kinv and its mirror image.
__global__ __launch_bounds__(256) void gp_condition_store_kernel(double* __restrict__ linv, double* __restrict__ linv_t, double* __restrict__ alpha,
                                                                 double* __restrict__ kinv, int m, int N, int believer,
                                                                 const double* __restrict__ u, const double* __restrict__ scal) {
    __shared__ double tile[32][33];
    const double lam2 = scal[0];
    const int vec = (N + 256) / 256;             // ceil((N + 1) / 256)
    if ((int)blockIdx.x < vec) {
        const int e = blockIdx.x * 256 + threadIdx.x;
        if (e > N) return;
        const double lam = scal[1], gamma = scal[2];
        const double v = e < N ? -u[e] / lam : 1.0 / lam;
        linv[(int64_t)N * m + e] = v;
        if (linv_t) linv_t[(int64_t)e * m + N] = v;
        if (e == N)
            alpha[N] = gamma;
        else if (!believer)
            alpha[e] = __builtin_fma(-gamma, u[e], alpha[e]);
        return;
    }
    int64_t bi, bj;
    lower_tile_of((int64_t)blockIdx.x - vec, bi, bj);
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int i0 = (int)bi * 32, k0 = (int)bj * 32;
    for (int r = ty; r < 32; r += 8) {
        const int i = i0 + r, k = k0 + tx;
        double v = 0.0;
        if (i <= N && k <= i) {
            if (i < N)
                v = kinv[(int64_t)i * m + k] + (u[i] * u[k]) / lam2;
            else
                v = k < N ? -u[k] / lam2 : 1.0 / lam2;
            kinv[(int64_t)i * m + k] = v;
        }
        tile[r][tx] = v;
    }
    __syncthreads();
    for (int r = ty; r < 32; r += 8) {
        const int k = k0 + r, i = i0 + tx;       // row k, column i > k: the image of (i, k)
        if (i <= N && k < i) kinv[(int64_t)k * m + i] = tile[tx][r];
    }
}

}  // namespace gabo

static bool gp_condition_dims_ok(int64_t n, int64_t t) {
    return n >= 1 && t >= 1 && t <= GABO_GP_CONDITION_MAX_T && n <= GABO_GP_MLL_LARGE_MAX_N && n + t <= GABO_GP_MLL_LARGE_MAX_N;
}

extern "C" size_t gabo_gp_condition_workspace_bytes(int64_t n, int64_t t) {
    if (!gp_condition_dims_ok(n, t)) return 0;
    return (size_t)(2 * (n + t) + 8) * sizeof(double);           // l, u, {lambda^2, lambda, gamma}
}

extern "C" int gabo_gp_condition(const double* linv, const double* alpha, const double* kinv, int64_t n, const double* kcross, const double* knew,
                                 const double* y_new, int64_t t, double outputscale, double noise, double mean, double* linv_out,
                                 double* linv_t_out, double* alpha_out, double* kinv_out, double* y_out, void* workspace, size_t workspace_bytes,
                                 int* status, gabo_stream_t stream) {
    if (t > GABO_GP_CONDITION_MAX_T || n > GABO_GP_MLL_LARGE_MAX_N || (n >= 1 && t >= 1 && n + t > GABO_GP_MLL_LARGE_MAX_N)) return GABO_ERR_DIM;
    if (n < 1 || t < 1 || !linv || !alpha || !kcross || !knew || !linv_out || !alpha_out || !y_out || !workspace || !status) return GABO_ERR_ARG;
    if ((kinv == nullptr) != (kinv_out == nullptr)) return GABO_ERR_ARG;
    if (workspace_bytes < gabo_gp_condition_workspace_bytes(n, t)) return GABO_ERR_ARG;
    const int m = (int)(n + t), n0 = (int)n, tt = (int)t;
    double* l = (double*)workspace;
    double* u = l + m;
    double* scal = u + m;
    const unsigned tiles = (unsigned)((m + 31) / 32);
    hipLaunchKernelGGL(gabo::gp_condition_copy_kernel, dim3(tiles, tiles), dim3(256), 0, (hipStream_t)stream, linv, alpha, kinv, n0, m, linv_out,
                       linv_t_out, alpha_out, kinv_out);
    if (hipGetLastError() != hipSuccess) return GABO_ERR_LAUNCH;
    for (int j = 0; j < tt; ++j) {
        const int N = n0 + j;
        hipLaunchKernelGGL(gabo::gp_condition_l_kernel, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, (hipStream_t)stream, (const double*)linv_out, m,
                           kcross, knew, n0, tt, j, outputscale, l);
        if (hipGetLastError() != hipSuccess) return GABO_ERR_LAUNCH;
        const unsigned strips = (unsigned)((N + gabo::kCondStrip - 1) / gabo::kCondStrip);
        hipLaunchKernelGGL(gabo::gp_condition_u_kernel, dim3(strips + 1), dim3(gabo::kCondThreads), 0, (hipStream_t)stream, (const double*)linv_out,
                           m, kcross, knew, y_new, (const double*)alpha_out, n0, tt, j, outputscale, noise, mean, (const double*)l, u, scal, y_out,
                           status);
        if (hipGetLastError() != hipSuccess) return GABO_ERR_LAUNCH;
        const unsigned vec = (unsigned)((N + 256) / 256);
        const unsigned at = (unsigned)((N + 32) / 32);           // tiles per side of the (N + 1) x (N + 1) block of A
        hipLaunchKernelGGL(gabo::gp_condition_store_kernel, dim3(vec + (kinv_out ? at * (at + 1) / 2 : 0)), dim3(256), 0, (hipStream_t)stream,
                           linv_out, linv_t_out, alpha_out, kinv_out, m, N, y_new ? 0 : 1, (const double*)u, (const double*)scal);
        if (hipGetLastError() != hipSuccess) return GABO_ERR_LAUNCH;
    }
    return GABO_OK;
}
