// Frechet (Karcher) means on the device: SPD matrices under the affine-invariant metric, fused for 2 <= d <= 10, and points of the unit sphere.
//
// The reference iterates  m <- Exp_m( (1/N) sum_j Log_m(x_j) )  on the host, one numpy eig per point and iteration
// (Riemannian_utils/spd_utils.py:235-287, sphere_utils.py:126-149).  In whitened coordinates the SPD step is
//
//     m+ = L expm( S ) L^T,      S = sum_j w_j logm(L^-1 X_j L^-T),      L = chol(m),
//
// and S is exactly what spd_ai_backward_kernel accumulates for one row (spd_backward.hip): M = C C^T with C = L^-1 chol(X_j), the register
// eigen-solver with vectors, log_pos, one LDS column per lane, the rotated reduction.  That kernel gives one row to one wave; a mean has ONE
// row (the base point) and N columns, so here the COLUMNS are spread over the grid and the sum is finished by a second launch:
//
//   prep        once: the Cholesky factors of the data, entry-major (spd_prep.hpp) - they do not change between iterations
//   finish(-1)  once: the start point (given, or the set's first point) -> mean, L, L^-1; the weight normalisation
//   per iteration
//     accumulate  B x P blocks of one wave, lane = data point, a block's share of the columns in chunks of 64 -> one partial sum (T doubles) per block
//     finish      B blocks of one wave: the P partials added in index order, expm, the congruence with L, the new mean and its factors, the residual
//
// The launch boundary is the only synchronisation and every sum has a fixed order: no atomics on floating-point data, no grid barrier, and the
// result has the same bits from run to run (on one device: P depends on the CU count).
//
// The sphere mean has the same shape: partial weighted sums of Log_m(x_j) per block (the statements of GABO_SPH_LOG, spd_manifold.hip), then a
// finish that applies Exp_m (GABO_SPH_EXP).
#include "gabo_device.hpp"
#include "spd_prep.hpp"
#include "spd_eigvec.hpp"
#include "../../include/gabo_hip.h"

#define GABO_MEAN_MAX_DIM 10            /* the fused SPD mean: Z of the eigen-solver is 200 VGPRs at d = 10 */
#define GABO_MEAN_TWO_WAVE_MAX_DIM 8    /* the backward kernel's occupancy budget: two waves per SIMD up to here, one above */
#define GABO_MEAN_TWO_PASS_MIN_DIM 4    /* eigenvalues first, then one vector sweep per stage (spd_eigvec.hpp), as the backward kernel */
#define GABO_SPHERE_MEAN_MAX_DIM 512

namespace gabo {

// How a set's N columns are spread over blocks.  chunks = ceil(N / 64) (lane = data point); the device holds slots = 4 SIMDs x CUs x waves-per-SIMD
// one-wave blocks at a time, of which a set may take slots / B.  P = min(chunks, max(1, slots / B)) blocks per set, each taking
// cpb = ceil(chunks / P) consecutive chunks (P is then lowered to ceil(chunks / cpb): no block without a column).  So N <= 64 is one block, B = 1
// and N = 4096 is 64 blocks of one chunk (every chunk on a SIMD of its own), and a block loops over several chunks only when B x chunks exceeds
// the slots of the device.
struct MeanPlan {
    int64_t chunks, cpb, P;
};

// (asked of the runtime at every call: the current device may change between calls, and the answer is a cached property there)
static int device_cu_count() {
    int dev = 0, v = 0;
    if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && v > 0) return v;
    return 256;
}

// waves_per_simd: how many one-wave blocks per SIMD the plan counts on - the SPD kernels' launch bound; for the sphere kernels a fixed 2 (they could
// hold 4: the plan only decides when a block starts to loop over chunks, and two resident waves per SIMD already hide their loads).
static MeanPlan mean_plan(int64_t batch, int64_t n, int waves_per_simd) {
    MeanPlan pl;
    pl.chunks = (n + 63) / 64;
    const int64_t slots = (int64_t)4 * device_cu_count() * waves_per_simd;
    int64_t want = slots / batch;
    if (want < 1) want = 1;
    pl.P = pl.chunks < want ? pl.chunks : want;
    pl.cpb = (pl.chunks + pl.P - 1) / pl.P;
    pl.P = (pl.chunks + pl.cpb - 1) / pl.cpb;
    return pl;
}

// scale[b]: what a raw weight is multiplied by - 1 / sum_j w_j, or 1 / N without weights.  All 64 lanes of the wave.
__device__ __forceinline__ double weight_scale(const double* __restrict__ weights, int64_t b, int64_t n, int lane) {
    if (!weights) return 1.0 / (double)n;
    double a = 0.0;
    for (int64_t j = lane; j < n; j += 64) a += weights[b * n + j];
    return 1.0 / wave_allsum(a);
}

// ---- SPD ---------------------------------------------------------------------------------------------------------------------------------------
// Block (b, p): S_p = sum over its columns of w_j logm(W G_j G_j^T W^T), W = L^-1 of set b's current mean (wave-uniform: scalar loads), G_j the
// entry-major Cholesky factor of X_j.  The body up to the reduction is spd_ai_backward_kernel's with w_j in place of dLoss/d(d^2); the eigen-solver
// runs with its strict deflation threshold (a mean is iterated to convergence: the residual should reach rounding, not 1e-13).
// A non-positive eigenvalue of M gives NaN, as there.
template <int D>
__global__ __launch_bounds__(64, (D > GABO_MEAN_TWO_WAVE_MAX_DIM ? 1 : 2)) void spd_mean_accumulate_kernel(
    const double* __restrict__ Winv, const double* __restrict__ G, const double* __restrict__ weights, const double* __restrict__ scale,
    double* __restrict__ partial, int64_t n, int P, int64_t cpb, int64_t pstride) {
    constexpr int T = tri_size(D);
    __shared__ double acc[T * 64];
    const int lane = threadIdx.x;
    const int64_t b = blockIdx.x / P;
    const int64_t p = blockIdx.x - b * P;
    const double* W = Winv + b * T;
    const double* Gb = G + b * T * n;
    const double sc = scale[b];
    static_for<T>([&](auto ee) { acc[decltype(ee)::value * 64 + lane] = 0.0; });
    const int64_t jbegin = p * cpb * 64;
    const int64_t jend = (jbegin + cpb * 64 < n) ? jbegin + cpb * 64 : n;
    for (int64_t j0 = jbegin; j0 < jend; j0 += 64) {
        const int64_t j = j0 + lane;
        const bool live = j < n;
        const int64_t jc = live ? j : n - 1;
        const double* Gj = Gb + jc;
        double m[T];
        static_for<T>([&](auto ee) { m[decltype(ee)::value] = 0.0; });
        static_for<D>([&](auto cc) {
            constexpr int col = decltype(cc)::value;
            double g[D - col], c[D - col];
            static_for<D - col>([&](auto kk) { g[decltype(kk)::value] = Gj[(int64_t)tri(col + decltype(kk)::value, col) * n]; });
            static_for<D - col>([&](auto rr) {
                constexpr int r = col + decltype(rr)::value;
                double a = W[tri(r, col)] * g[0];
                static_for<r - col>([&](auto kk) {
                    constexpr int k = col + 1 + decltype(kk)::value;
                    a = __builtin_fma(W[tri(r, k)], g[k - col], a);
                });
                c[r - col] = a;
            });
            static_for<D - col>([&](auto rr) {
                constexpr int r = col + decltype(rr)::value;
                static_for<r - col + 1>([&](auto qq) {
                    constexpr int q = col + decltype(qq)::value;
                    m[tri(r, q)] = __builtin_fma(c[r - col], c[q - col], m[tri(r, q)]);
                });
            });
        });
        double vreg[D * D];
        double lam[D];
        if constexpr (D >= GABO_MEAN_TWO_PASS_MIN_DIM) sym_eig_reg_two_pass<D>(m, lam, vreg);
        else sym_eig_reg<D>(m, lam, vreg);
        double lg[D];
        {
            const LogRegs logc = LogRegs::load();
            static_for<D>([&](auto kk) {
                constexpr int k = decltype(kk)::value;
                const double l = log_pos(lam[k], logc);
                lg[k] = lam[k] > 0.0 ? l : __builtin_nan("");
            });
        }
        const double w = live ? (weights ? weights[b * n + j] : 1.0) * sc : 0.0;
        // acc += w V diag(lg) V^T   (lower triangle).  A point without weight is skipped, not multiplied by zero: the padding lanes of the last chunk
        // and a caller's zero weights must not carry a NaN (a non-positive eigenvalue of a point that is not wanted) into the sum.
        if (w != 0.0) static_for<D>([&](auto rr) {
            constexpr int r = decltype(rr)::value;
            double vl[D];
            static_for<D>([&](auto kk) { vl[decltype(kk)::value] = vreg[r * D + decltype(kk)::value] * (w * lg[decltype(kk)::value]); });
            static_for<r + 1>([&](auto cc) {
                constexpr int c = decltype(cc)::value;
                double f = acc[tri(r, c) * 64 + lane];
                static_for<D>([&](auto kk) { constexpr int k = decltype(kk)::value; f = __builtin_fma(vl[k], vreg[c * D + k], f); });
                acc[tri(r, c) * 64 + lane] = f;
            });
        });
    }
    __syncthreads();
    for (int e = lane; e < T; e += 64) {
        double t = 0.0;
        for (int l = 0; l < 64; ++l) t += acc[e * 64 + ((l + e) & 63)];  // rotated start: threads hit different banks
        partial[(b * pstride + p) * T + e] = t;
    }
}

// One wave per set; every lane carries the whole (tiny) computation in its registers, lane 0 writes.
//   it < 0: the start point -> mean, its factors L and L^-1, the weight scale.
//   it >= 0: S = the P partials in index order; residual[b][it] = ||S||_F (the affine-invariant norm of the mean tangent L S L^T at m);
//            m+ = L expm(S) L^T -> mean (Mandel), L+ = chol(m+), W+ = L+^-1 for the next iteration.
// A start point or an iterate that is not positive definite raises the status word: status[1] = B N + b (past the data's indices).
template <int D>
__global__ __launch_bounds__(64, (D > GABO_MEAN_TWO_WAVE_MAX_DIM ? 1 : 2)) void spd_mean_finish_kernel(
    const double* __restrict__ partial, const double* __restrict__ x, const double* __restrict__ start, const double* __restrict__ weights,
    double* Lfac, double* __restrict__ Winv, double* __restrict__ scale, double* __restrict__ mean, double* __restrict__ resid,
    int* __restrict__ status, int64_t n, int P, int64_t pstride, int iters, int it) {
    constexpr int T = tri_size(D);
    const int lane = threadIdx.x;
    const int64_t b = blockIdx.x;
    double mv[T];                                   // the new mean, Mandel order
    if (it < 0) {
        const double* src = start ? start + b * T : x + b * n * T;
        static_for<T>([&](auto ee) { mv[decltype(ee)::value] = src[decltype(ee)::value]; });
        const double sc = weight_scale(weights, b, n, lane);
        if (lane == 0) scale[b] = sc;
    } else {
        double s[T];
        static_for<T>([&](auto ee) { s[decltype(ee)::value] = 0.0; });
        for (int p = 0; p < P; ++p) {
            const double* pp = partial + (b * pstride + p) * T;
            static_for<T>([&](auto ee) { s[decltype(ee)::value] += pp[decltype(ee)::value]; });
        }
        if (resid) {
            double nn = 0.0;
            static_for<D>([&](auto rr) {
                constexpr int r = decltype(rr)::value;
                static_for<r + 1>([&](auto cc) {
                    constexpr int c = decltype(cc)::value;
                    const double v = s[tri(r, c)];
                    nn = __builtin_fma((r == c) ? v : 2.0 * v, v, nn);
                });
            });
            if (lane == 0) resid[b * iters + it] = __builtin_sqrt(nn);
        }
        // expm(S) = V diag(exp lam) V^T   (S is symmetric and indefinite: the solver's deflation test covers zeros on the diagonal)
        double vreg[D * D];
        double lam[D];
        if constexpr (D >= GABO_MEAN_TWO_PASS_MIN_DIM) sym_eig_reg_two_pass<D>(s, lam, vreg);
        else sym_eig_reg<D>(s, lam, vreg);
        static_for<D>([&](auto kk) { lam[decltype(kk)::value] = exp(lam[decltype(kk)::value]); });
        double ex[T];
        static_for<D>([&](auto rr) {
            constexpr int r = decltype(rr)::value;
            double vl[D];
            static_for<D>([&](auto kk) { vl[decltype(kk)::value] = vreg[r * D + decltype(kk)::value] * lam[decltype(kk)::value]; });
            static_for<r + 1>([&](auto cc) {
                constexpr int c = decltype(cc)::value;
                double f = 0.0;
                static_for<D>([&](auto kk) { constexpr int k = decltype(kk)::value; f = __builtin_fma(vl[k], vreg[c * D + k], f); });
                ex[tri(r, c)] = f;
            });
        });
        // m+ = L E L^T, row by row: a = (L E)[r][:], m+[r][c] = sum_{k <= c} a[k] L[c][k]
        const double* L = Lfac + b * T;
        double lf[T];
        static_for<T>([&](auto ee) { lf[decltype(ee)::value] = L[decltype(ee)::value]; });
        static_for<D>([&](auto rr) {
            constexpr int r = decltype(rr)::value;
            double a[D];
            static_for<D>([&](auto cc) {
                constexpr int c = decltype(cc)::value;
                double t = 0.0;
                static_for<r + 1>([&](auto kk) {
                    constexpr int k = decltype(kk)::value;
                    constexpr int hi = k > c ? k : c, lo = k > c ? c : k;
                    t = __builtin_fma(lf[tri(r, k)], ex[tri(hi, lo)], t);
                });
                a[c] = t;
            });
            static_for<r + 1>([&](auto cc) {
                constexpr int c = decltype(cc)::value;
                double t = 0.0;
                static_for<c + 1>([&](auto kk) { constexpr int k = decltype(kk)::value; t = __builtin_fma(a[k], lf[tri(c, k)], t); });
                mv[mandel_pos(D, r, c)] = (r == c) ? t : t * kSqrt2;
            });
        });
    }
    // the factors of the new mean, from the Mandel vector that is handed out (so that L is the factor of exactly that matrix)
    double a[T], w[T];
    const bool bad = mandel_cholesky<D>(mv, a);
    lower_inverse<D>(a, w);
    if (lane == 0) {
        if (bad) {
            if (atomicCAS(status, 0, GABO_ERR_NOT_SPD) == 0) status[1] = (int)((int64_t)gridDim.x * n + b);
        }
        double* mo = mean + b * T;
        double* lo = Lfac + b * T;
        double* wo = Winv + b * T;
        static_for<T>([&](auto ee) {
            constexpr int e = decltype(ee)::value;
            mo[e] = mv[e];
            lo[e] = a[e];
            wo[e] = w[e];
        });
    }
}

template <int D>
static int launch_spd_frechet_mean(const double* x, const double* weights, const double* start, double* mean, double* resid, int64_t batch,
                                   int64_t n, int iters, double* ws, int* status, hipStream_t st) {
    constexpr int T = tri_size(D);
    const MeanPlan pl = mean_plan(batch, n, D > GABO_MEAN_TWO_WAVE_MAX_DIM ? 1 : 2);
    if (batch * pl.P > 0x7fffffffLL || batch * n > 0x7fffffffLL) return GABO_ERR_ARG;
    double* G = ws;
    double* W = G + batch * n * T;
    double* L = W + batch * T;
    double* scale = L + batch * T;
    double* partial = scale + batch;
    if (iters > 0) launch_spd_prep<D>(nullptr, x, nullptr, G, 0, batch, 0, n, 0, n * T, status, st);
    hipLaunchKernelGGL((spd_mean_finish_kernel<D>), dim3((unsigned)batch), dim3(64), 0, st, partial, x, start, weights, L, W, scale, mean, resid,
                       status, n, (int)pl.P, pl.chunks, iters, -1);
    for (int it = 0; it < iters; ++it) {
        hipLaunchKernelGGL((spd_mean_accumulate_kernel<D>), dim3((unsigned)(batch * pl.P)), dim3(64), 0, st, W, G, weights, scale, partial, n,
                           (int)pl.P, pl.cpb, pl.chunks);
        hipLaunchKernelGGL((spd_mean_finish_kernel<D>), dim3((unsigned)batch), dim3(64), 0, st, partial, x, start, weights, L, W, scale, mean,
                           resid, status, n, (int)pl.P, pl.chunks, iters, it);
    }
    return hipGetLastError() == hipSuccess ? GABO_OK : GABO_ERR_LAUNCH;
}

// ---- sphere ------------------------------------------------------------------------------------------------------------------------------------
// Block (b, p), one wave.  Per chunk of 64 points: lane = point computes theta = acos(clip(<m, x_j>)) and the factors of Log_m(x_j) =
// (x_j - m cos theta) theta / sin theta (0 where theta < 1e-16); then lane = coordinate adds w_j Log_m(x_j)[k] over the chunk's points in index
// order (coalesced along k).  A lane owns the coordinates k = lane + 64 q, q < 8.
__global__ __launch_bounds__(64) void sphere_mean_accumulate_kernel(const double* __restrict__ x, const double* __restrict__ mean,
                                                                    const double* __restrict__ weights, const double* __restrict__ scale,
                                                                    double* __restrict__ partial, int64_t n, int dim, int P, int64_t cpb,
                                                                    int64_t pstride) {
    __shared__ double ms[GABO_SPHERE_MEAN_MAX_DIM];
    __shared__ double cs[64], fs[64], wsh[64];
    const int lane = threadIdx.x;
    const int64_t b = blockIdx.x / P;
    const int64_t p = blockIdx.x - b * P;
    const double* xb = x + b * n * dim;
    const double sc = scale[b];
    for (int k = lane; k < dim; k += 64) ms[k] = mean[b * dim + k];
    double acc[GABO_SPHERE_MEAN_MAX_DIM / 64];
    static_for<GABO_SPHERE_MEAN_MAX_DIM / 64>([&](auto qq) { acc[decltype(qq)::value] = 0.0; });
    __syncthreads();
    const int64_t jbegin = p * cpb * 64;
    const int64_t jend = (jbegin + cpb * 64 < n) ? jbegin + cpb * 64 : n;
    for (int64_t j0 = jbegin; j0 < jend; j0 += 64) {
        const int64_t j = j0 + lane;
        const bool live = j < n;
        const double* X = xb + (live ? j : n - 1) * dim;
        double ip = 0.0;
        for (int k = 0; k < dim; ++k) ip = __builtin_fma(ms[k], X[k], ip);
        ip = ip > 1.0 ? 1.0 : (ip < -1.0 ? -1.0 : ip);
        const double th = acos(ip);
        double cn = 0.0, f = 0.0;
        if (!(th < 1e-16)) {
            cn = cos(th);
            f = th / sin(th);
        }
        cs[lane] = cn;
        fs[lane] = f;
        wsh[lane] = live ? (weights ? weights[b * n + j] : 1.0) * sc : 0.0;
        __syncthreads();
        const int cnt = (int)(jend - j0 < 64 ? jend - j0 : 64);
        static_for<GABO_SPHERE_MEAN_MAX_DIM / 64>([&](auto qq) {
            constexpr int q = decltype(qq)::value;
            const int k = lane + 64 * q;
            if (k < dim) {
                const double mk = ms[k];
                double a = acc[q];
                for (int jj = 0; jj < cnt; ++jj) a += wsh[jj] != 0.0 ? wsh[jj] * ((xb[(j0 + jj) * dim + k] - mk * cs[jj]) * fs[jj]) : 0.0;   // (no weight: skipped, as above)
                acc[q] = a;
            }
        });
        __syncthreads();
    }
    static_for<GABO_SPHERE_MEAN_MAX_DIM / 64>([&](auto qq) {
        constexpr int q = decltype(qq)::value;
        const int k = lane + 64 * q;
        if (k < dim) partial[(b * pstride + p) * dim + k] = acc[q];
    });
}

// One wave per set.  it < 0: the start point -> mean, the weight scale.  it >= 0: u = the P partials in index order, residual[b][it] = |u|,
// mean <- mean cos|u| + u sin|u| / |u|  (unchanged where |u| < 1e-16).
__global__ __launch_bounds__(64) void sphere_mean_finish_kernel(const double* __restrict__ partial, const double* __restrict__ x,
                                                                const double* __restrict__ start, const double* __restrict__ weights,
                                                                double* __restrict__ scale, double* __restrict__ mean, double* __restrict__ resid,
                                                                int64_t n, int dim, int P, int64_t pstride, int iters, int it) {
    __shared__ double us[GABO_SPHERE_MEAN_MAX_DIM];
    const int lane = threadIdx.x;
    const int64_t b = blockIdx.x;
    double* mo = mean + b * dim;
    if (it < 0) {
        const double* src = start ? start + b * dim : x + b * n * dim;
        for (int k = lane; k < dim; k += 64) mo[k] = src[k];
        const double sc = weight_scale(weights, b, n, lane);
        if (lane == 0) scale[b] = sc;
        return;
    }
    double nl = 0.0;
    for (int k = lane; k < dim; k += 64) {
        double u = 0.0;
        for (int p = 0; p < P; ++p) u += partial[(b * pstride + p) * dim + k];
        us[k] = u;
        nl = __builtin_fma(u, u, nl);
    }
    const double nu = __builtin_sqrt(wave_allsum(nl));
    if (resid && lane == 0) resid[b * iters + it] = nu;
    if (!(nu < 1e-16)) {
        const double cn = cos(nu), sn = sin(nu) / nu;
        for (int k = lane; k < dim; k += 64) mo[k] = mo[k] * cn + us[k] * sn;
    }
}

}  // namespace gabo

extern "C" size_t gabo_spd_frechet_mean_workspace_bytes(int64_t batch, int64_t n, int d) {
    if (batch < 1 || n < 1 || d < 2 || d > GABO_MEAN_MAX_DIM) return 0;
    const int64_t T = gabo::tri_size(d);
    // data factors, L^-1 and L of the mean, the weight scale, one partial per chunk of 64 points (P never exceeds the chunks)
    return (size_t)(batch * n * T + 2 * batch * T + batch + batch * ((n + 63) / 64) * T) * sizeof(double);
}

extern "C" int gabo_spd_frechet_mean(const double* x, const double* weights, const double* start, double* mean, double* residual, int64_t batch,
                                     int64_t n, int d, int iters, void* workspace, size_t workspace_bytes, int* status, gabo_stream_t stream) {
    if (batch < 0 || n < 1 || iters < 0) return GABO_ERR_ARG;
    if (d < 2 || d > GABO_MEAN_MAX_DIM) return GABO_ERR_DIM;
    if (batch == 0) return GABO_OK;
    if (!x || !mean || !workspace || !status) return GABO_ERR_ARG;
    if (workspace_bytes < gabo_spd_frechet_mean_workspace_bytes(batch, n, d)) return GABO_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    double* ws = (double*)workspace;
#define GABO_CASE(DD) \
    case DD:          \
        return gabo::launch_spd_frechet_mean<DD>(x, weights, start, mean, residual, batch, n, iters, ws, status, st);
    switch (d) {
        GABO_CASE(2) GABO_CASE(3) GABO_CASE(4) GABO_CASE(5) GABO_CASE(6) GABO_CASE(7) GABO_CASE(8) GABO_CASE(9) GABO_CASE(10)
    }
#undef GABO_CASE
    return GABO_ERR_DIM;
}

extern "C" size_t gabo_sphere_karcher_mean_workspace_bytes(int64_t batch, int64_t n, int dim) {
    if (batch < 1 || n < 1 || dim < 2 || dim > GABO_SPHERE_MEAN_MAX_DIM) return 0;
    return (size_t)(batch + batch * ((n + 63) / 64) * dim) * sizeof(double);
}

extern "C" int gabo_sphere_karcher_mean(const double* x, const double* weights, const double* start, double* mean, double* residual,
                                        int64_t batch, int64_t n, int dim, int iters, void* workspace, size_t workspace_bytes,
                                        gabo_stream_t stream) {
    if (batch < 0 || n < 1 || iters < 0) return GABO_ERR_ARG;
    if (dim < 2 || dim > GABO_SPHERE_MEAN_MAX_DIM) return GABO_ERR_DIM;
    if (batch == 0) return GABO_OK;
    if (!x || !mean || !workspace) return GABO_ERR_ARG;
    if (workspace_bytes < gabo_sphere_karcher_mean_workspace_bytes(batch, n, dim)) return GABO_ERR_ARG;
    const gabo::MeanPlan pl = gabo::mean_plan(batch, n, 2);
    if (batch * pl.P > 0x7fffffffLL) return GABO_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    double* scale = (double*)workspace;
    double* partial = scale + batch;
    hipLaunchKernelGGL(gabo::sphere_mean_finish_kernel, dim3((unsigned)batch), dim3(64), 0, st, partial, x, start, weights, scale, mean, residual, n,
                       dim, (int)pl.P, pl.chunks, iters, -1);
    for (int it = 0; it < iters; ++it) {
        hipLaunchKernelGGL(gabo::sphere_mean_accumulate_kernel, dim3((unsigned)(batch * pl.P)), dim3(64), 0, st, x, mean, weights, scale, partial, n,
                           dim, (int)pl.P, pl.cpb, pl.chunks);
        hipLaunchKernelGGL(gabo::sphere_mean_finish_kernel, dim3((unsigned)batch), dim3(64), 0, st, partial, x, start, weights, scale, mean, residual,
                           n, dim, (int)pl.P, pl.chunks, iters, it);
    }
    return hipGetLastError() == hipSuccess ? GABO_OK : GABO_ERR_LAUNCH;
}
