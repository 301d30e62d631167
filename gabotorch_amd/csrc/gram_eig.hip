// Smallest and largest eigenvalue of K = exp(-theta * E), entry by entry, for every pair (point set b, parameter p) of a study of the
// range of kernel parameters in which a geodesic kernel is positive definite.  The reference does this study on the host
// (examples/kernels/spd/spd_gaussian_kernel_parameters.py:84-125, examples/kernels/sphere/sphere_gaussian_kernel_parameters.py:62-112):
// per point set and per parameter one `kernel.forward`, one copy to numpy and one np.linalg.eig of which only the minimum is kept; the
// beta_min ladders of gabo_spd.py:151-162 and gabo_sphere.py:115-128 are read off the resulting table.  Every plain kernel of the path is
// exp(-theta E) with E = d^2 (Gaussian) or d (Laplace) independent of the parameter (gp_mll.hip uses the same form for the fit), so the
// distances are evaluated once per set and this launch does the rest: no Gram matrix and no spectrum ever leaves the device.
//
// One workgroup per (b, p) matrix; nothing is shared between workgroups.  The workgroup
//   1. forms the packed lower triangle of K (row-major: entry (i, j <= i) at i (i + 1) / 2 + j) from the lower triangle of e[b] with the
//      exp of the Gaussian output of spd_pairwise_body.hpp (OCML's), a wave per row;
//   2. reduces K to tridiagonal form in place by n - 2 Householder reflections (LAPACK dsytd2, lower).  Per step: the column below the
//      diagonal and its norm (block reduction), p = tau K22 v in ONE pass over the trailing triangle - a wave per row, the lanes along
//      the row: the row's own dot product is a wave sum, and every lane keeps what the row adds to ITS columns in registers
//      (T accumulators of 64 columns), summed over the waves through LDS - then w = p - (tau p.v / 2) v (block reduction) and the
//      rank-2 update K22 -= v w^T + w v^T in a second pass.  A column whose part below the sub-diagonal is exactly zero takes no
//      reflector (tau = 0, as dlarfg), which is every column after the first of the rank-one K at theta = 0; entries below 1e-140 count
//      as zero there (kGramEigTiny below);
//   3. finds lambda_min and lambda_max of the tridiagonal by bisection on Sturm counts, one wave each: per round the 64 lanes count
//      at 64 interior points of the interval (multisection, a factor 65 per round), starting from the Gershgorin bounds widened as
//      dstebz does, until the interval no longer splits in fp64; at most kGramEigMaxRounds rounds whatever the data.  A pivot smaller than
//      pivmin = safmin max(1, max e_i^2) is replaced by -pivmin (dstebz).
// Every sum is taken in an order fixed by n alone, so a pair's result does not depend on the rest of the batch.
//
// Storage of the triangle, two instantiations of the one body:
//   n <= GABO_GRAM_EIG_LDS_MAX_N = 192: in LDS.  n (n + 1) / 2 + (5 + 4) npad + 16 doubles (npad = n rounded up to 64; 256 threads = 4
//      waves) is 20 296 doubles at n = 192 and 20 498 at 193, against the 20 480 doubles (160 KiB) of a CU;
//   above: in the caller's workspace, one triangle per workgroup (512 threads = 8 waves; 13 npad + 16 doubles of LDS).
// fp64 on the vector pipe throughout.  The products are matrix-vector ones on a chain of n dependent steps: an MFMA needs a second
// operand dimension that this algorithm does not have, so none is used.
#include "gabo_device.hpp"
#include "../../include/gabo_hip.h"

#include <atomic>
#include <limits>

namespace gabo {

constexpr int kGramEigMaxRounds = 24;             // 65^-24 of the Gershgorin width: fp64 resolution is reached after 9 or 10 rounds at an
                                                  // eigenvalue of the size of the norm and after up to 19 at one next to zero
// A reflector is orthogonal only as far as the norm of its column is accurate, and the squares of entries below 1e-154 lose their bits
// to underflow: at theta = 1e4 (K the identity plus entries down to the denormals, and the rounding residues of the updates below them)
// such columns cost 5e-13 of lambda_min.  Entries of the column below kGramEigTiny count as zero when the reflector is formed - a
// symmetric perturbation of K of that size - and a K with an entry above kGramEigHuge, whose square would overflow, is answered as a
// non-finite one.
constexpr double kGramEigTiny = 1e-140, kGramEigHuge = 1e150;

__host__ __device__ constexpr int gram_eig_npad(int n) { return (n + 63) / 64 * 64; }
// doubles of LDS next to the triangle: v, w, p, d, e (npad each), the column sums per wave (waves x npad), the block sums and a header
__host__ __device__ constexpr int gram_eig_scratch(int n, int waves) { return (5 + waves) * gram_eig_npad(n) + 16; }

template <int THREADS>
static __device__ __forceinline__ double gram_eig_block_sum(double v, double* red) {
    v = wave_allsum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < THREADS / 64; ++k) s += red[k];
    return s;
}

// number of eigenvalues of the tridiagonal (d, e) below x (LAPACK dstebz, the serial count)
static __device__ __forceinline__ int sturm_count(const double* __restrict__ d, const double* __restrict__ e, int n, double x, double pivmin) {
    double q = d[0] - x;
    if (__builtin_fabs(q) < pivmin) q = -pivmin;
    int count = q <= 0.0 ? 1 : 0;
    for (int i = 1; i < n; ++i) {
        const double ei = e[i - 1];
        q = d[i] - x - (ei * ei) * rcp(q);
        if (__builtin_fabs(q) < pivmin) q = -pivmin;
        count += q <= 0.0 ? 1 : 0;
    }
    return count;
}

// LDS_K: the triangle lives in LDS in front of the scratch; otherwise in `ws`, one triangle per workgroup.  T: 64-column groups per row.
template <bool LDS_K, int THREADS, int T>
__global__ __launch_bounds__(THREADS) void gram_eig_kernel(const double* __restrict__ e_all, int n, const double* __restrict__ thetas,
                                                           int n_thetas, double* __restrict__ out, double* __restrict__ ws) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    constexpr int W = THREADS / 64;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.x / n_thetas, pidx = blockIdx.x - b * n_thetas;
    const int tsize = n * (n + 1) / 2;                           // <= 524 800 at n = 1024
    const int npad = gram_eig_npad(n);
    double* A;
    if constexpr (LDS_K)
        A = lds;
    else
        A = ws + (int64_t)blockIdx.x * tsize;
    double* v = LDS_K ? lds + tsize : lds;      // npad: the Householder vector of the step
    double* wv = v + npad;                      // npad: w of the rank-2 update
    double* pr = wv + npad;                     // npad: the rows' own dot products, then p
    double* dg = pr + npad;                     // npad: diagonal of the tridiagonal
    double* od = dg + npad;                     // npad: its off-diagonal
    double* part = od + npad;                   // W x npad: what each wave's rows add to the columns
    double* red = part + W * npad;              // W (<= 8)
    double* hdr = red + 8;                      // [0] the head of the column

    const double* e = e_all + (int64_t)b * n * n;
    const double theta = thetas[pidx];
    double* res = out + 2 * (int64_t)blockIdx.x;

    // ---- 1. K = exp(-theta e), lower triangle ------------------------------------------------------------------------------------------------
    int bad = !(__builtin_fabs(theta) < std::numeric_limits<double>::infinity());
    for (int i = wave; i < n; i += W) {
        const double* src = e + (int64_t)i * n;
        double* row = A + i * (i + 1) / 2;
        for (int c = lane; c <= i; c += 64) {
            const double eij = src[c];
            const double kij = exp(-theta * eij);
            bad |= !(__builtin_fabs(eij) < std::numeric_limits<double>::infinity()) || !(__builtin_fabs(kij) <= kGramEigHuge);
            row[c] = kij;
        }
    }
    if (__syncthreads_or(bad)) {                // (a non-finite entry or parameter, or an entry of K beyond kGramEigHuge: NaN for this pair, uniform exit)
        if (tid == 0) res[0] = res[1] = std::numeric_limits<double>::quiet_NaN();
        return;
    }

    // ---- 2. Householder tridiagonalisation --------------------------------------------------------------------------------------------------
    for (int k = 0; k + 2 < n; ++k) {
        const int k1 = k + 1, m = n - k1;                        // the trailing block: rows and columns k1 .. n - 1, local index c = i - k1
        double ss = 0.0;
        for (int c = tid; c < m; c += THREADS) {
            const int i = k1 + c;
            double x = A[i * (i + 1) / 2 + k];
            x = __builtin_fabs(x) < kGramEigTiny ? 0.0 : x;
            v[c] = x;
            if (c == 0)
                hdr[0] = x;
            else
                ss = __builtin_fma(x, x, ss);
        }
        if (tid == 0) dg[k] = A[k * (k + 1) / 2 + k];
        const double xnorm2 = gram_eig_block_sum<THREADS>(ss, red);
        const double alpha = hdr[0];
        if (xnorm2 == 0.0) {                                     // nothing below the sub-diagonal: H = I (every thread sees the same sum)
            if (tid == 0) od[k] = alpha;
            __syncthreads();
            continue;
        }
        const double beta = -copysign_d(sqrt_nz(__builtin_fma(alpha, alpha, xnorm2)), alpha);
        const double tau = (beta - alpha) * rcp(beta);
        const double scale = rcp(alpha - beta);
        for (int c = tid; c < m; c += THREADS) v[c] = c == 0 ? 1.0 : v[c] * scale;
        if (tid == 0) od[k] = beta;
        __syncthreads();

        // K22 v: row i gives p_i its part left of and on the diagonal (wave sum) and gives the columns j < i theirs (acc)
        double acc[T];
#pragma unroll
        for (int t = 0; t < T; ++t) acc[t] = 0.0;
        for (int i = k1 + wave; i < n; i += W) {
            const double* row = A + i * (i + 1) / 2 + k1;
            const int len = i - k;                               // columns k1 .. i, the diagonal at c = len - 1
            const double vi = v[len - 1];
            double s = 0.0;
#pragma unroll
            for (int t = 0; t < T; ++t) {
                if (64 * t >= len) break;
                const int c = lane + 64 * t;
                if (c < len) {
                    const double a = row[c];
                    s = __builtin_fma(a, v[c], s);
                    if (c < len - 1) acc[t] = __builtin_fma(a, vi, acc[t]);
                }
            }
            s = wave_allsum(s);
            if (lane == 0) pr[len - 1] = s;
        }
#pragma unroll
        for (int t = 0; t < T; ++t) {
            const int c = lane + 64 * t;
            if (c < m) part[wave * npad + c] = acc[t];
        }
        __syncthreads();
        double pv = 0.0;
        for (int c = tid; c < m; c += THREADS) {
            double s = pr[c];
#pragma unroll
            for (int q = 0; q < W; ++q) s += part[q * npad + c];
            s *= tau;
            pr[c] = s;
            pv = __builtin_fma(s, v[c], pv);
        }
        pv = gram_eig_block_sum<THREADS>(pv, red);
        const double half = 0.5 * tau * pv;
        for (int c = tid; c < m; c += THREADS) wv[c] = __builtin_fma(-half, v[c], pr[c]);
        __syncthreads();

        // K22 -= v w^T + w v^T
        for (int i = k1 + wave; i < n; i += W) {
            double* row = A + i * (i + 1) / 2 + k1;
            const int len = i - k;
            const double vi = v[len - 1], wi = wv[len - 1];
            for (int c = lane; c < len; c += 64) {
                double a = row[c];
                a = __builtin_fma(-vi, wv[c], a);
                a = __builtin_fma(-wi, v[c], a);
                row[c] = a;
            }
        }
        __syncthreads();
    }
    if (tid == 0) {                                              // the last 2 x 2 block (1 x 1 at n = 1) is tridiagonal as it stands
        dg[n - 1] = A[tsize - 1];
        if (n >= 2) {
            dg[n - 2] = A[tsize - n - 1];
            od[n - 2] = A[tsize - 2];
        }
    }
    __syncthreads();

    // ---- 3. lambda_min (wave 0) and lambda_max (wave 1) by multisection on Sturm counts ------------------------------------------------------
    if (wave >= 2) return;
    double gl = std::numeric_limits<double>::infinity(), gu = -gl, emax2 = 0.0;
    for (int i = lane; i < n; i += 64) {
        const double lo_e = i > 0 ? __builtin_fabs(od[i - 1]) : 0.0, hi_e = i + 1 < n ? __builtin_fabs(od[i]) : 0.0;
        gl = __builtin_fmin(gl, dg[i] - lo_e - hi_e);
        gu = __builtin_fmax(gu, dg[i] + lo_e + hi_e);
        emax2 = __builtin_fmax(emax2, hi_e * hi_e);
    }
    for (int off = 32; off > 0; off >>= 1) {
        gl = __builtin_fmin(gl, __shfl_xor(gl, off, 64));
        gu = __builtin_fmax(gu, __shfl_xor(gu, off, 64));
        emax2 = __builtin_fmax(emax2, __shfl_xor(emax2, off, 64));
    }
    const double pivmin = std::numeric_limits<double>::min() * __builtin_fmax(1.0, emax2);
    const double bnorm = __builtin_fmax(__builtin_fabs(gl), __builtin_fabs(gu));
    const double widen = 2.1 * bnorm * (0.5 * std::numeric_limits<double>::epsilon()) * (double)n + 2.1 * pivmin;
    // invariant: count(lo) < target <= count(hi); the eigenvalue of that index is the supremum of { x : count(x) < target }
    double lo = gl - widen, hi = gu + widen;
    const int target = wave == 0 ? 1 : n;
    for (int round = 0; round < kGramEigMaxRounds; ++round) {
        const double mid = lo + 0.5 * (hi - lo);
        if (!(lo < mid && mid < hi)) break;                      // the interval no longer splits (wave-uniform)
        double x = __builtin_fma(hi - lo, (double)(lane + 1) * (1.0 / 65.0), lo);
        x = __builtin_fmin(__builtin_fmax(x, lo), hi);
        const bool reached = sturm_count(dg, od, n, x, pivmin) >= target;
        const unsigned long long mask = __ballot(reached);
        const int first = mask ? __builtin_ctzll(mask) : 64;     // the first point at or beyond the eigenvalue
        const double x_hi = __shfl(x, first < 64 ? first : 63, 64), x_lo = __shfl(x, first > 0 ? first - 1 : 0, 64);
        if (first < 64) hi = x_hi;
        if (first > 0) lo = x_lo;
    }
    if (lane == 0) res[wave] = lo + 0.5 * (hi - lo);
}

}  // namespace gabo

static bool gram_eig_args_ok(int64_t batch, int64_t n, int64_t n_thetas) {
    return batch >= 1 && n >= 1 && n_thetas >= 1 && batch <= 0x7fffffff / n_thetas;
}

extern "C" size_t gabo_gram_extreme_eig_workspace_bytes(int64_t batch, int64_t n, int64_t n_thetas) {
    if (!gram_eig_args_ok(batch, n, n_thetas) || n > GABO_GRAM_EIG_MAX_N || n <= GABO_GRAM_EIG_LDS_MAX_N) return 0;
    return (size_t)batch * (size_t)n_thetas * (size_t)(n * (n + 1) / 2) * sizeof(double);
}

template <class K>
static int gram_eig_launch(K kernel, std::atomic<uint64_t>& attr_set, size_t lds_max, size_t lds, int threads, int64_t blocks, const double* e,
                           int n, const double* thetas, int n_thetas, double* out, double* ws, gabo_stream_t stream) {
    int dev = 0;                  // (more than 64 KB of dynamic LDS needs the attribute: set once per device, the maximum of the instantiation)
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev > 63) return GABO_ERR_LAUNCH;
    if (!(attr_set.load(std::memory_order_acquire) >> dev & 1)) {
        if (hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_max) != hipSuccess) return GABO_ERR_LAUNCH;
        attr_set.fetch_or((uint64_t)1 << dev, std::memory_order_release);
    }
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(threads), lds, (hipStream_t)stream, e, n, thetas, n_thetas, out, ws);
    return hipGetLastError() == hipSuccess ? GABO_OK : GABO_ERR_LAUNCH;
}

extern "C" int gabo_gram_extreme_eig(const double* e, int64_t batch, int64_t n, const double* thetas, int64_t n_thetas, double* out,
                                     void* workspace, size_t workspace_bytes, gabo_stream_t stream) {
    if (n > GABO_GRAM_EIG_MAX_N) return GABO_ERR_DIM;
    if (!e || !thetas || !out || !gram_eig_args_ok(batch, n, n_thetas)) return GABO_ERR_ARG;
    const size_t need = gabo_gram_extreme_eig_workspace_bytes(batch, n, n_thetas);
    if (workspace_bytes < need || (need > 0 && !workspace)) return GABO_ERR_ARG;
    const int64_t blocks = batch * n_thetas;
    static std::atomic<uint64_t> attr_lds{0}, attr_ws{0};
    if (n <= GABO_GRAM_EIG_LDS_MAX_N) {
        constexpr int kN = GABO_GRAM_EIG_LDS_MAX_N;
        constexpr size_t lds_max = (size_t)(kN * (kN + 1) / 2 + gabo::gram_eig_scratch(kN, 4)) * sizeof(double);
        static_assert(lds_max + 256 <= 160 * 1024 && kN <= 3 * 64,      // (+ 256: the static LDS of the block-wide OR)
                      "the triangle and its scratch must fit the LDS of a CU, a row three column groups");
        const size_t lds = (size_t)(n * (n + 1) / 2 + gabo::gram_eig_scratch((int)n, 4)) * sizeof(double);
        return gram_eig_launch(gabo::gram_eig_kernel<true, 256, 3>, attr_lds, lds_max, lds, 256, blocks, e, (int)n, thetas, (int)n_thetas, out,
                               nullptr, stream);
    }
    constexpr size_t lds_max = (size_t)gabo::gram_eig_scratch(GABO_GRAM_EIG_MAX_N, 8) * sizeof(double);
    static_assert(lds_max <= 160 * 1024 && GABO_GRAM_EIG_MAX_N <= 16 * 64, "scratch of the workspace form, a row sixteen column groups");
    const size_t lds = (size_t)gabo::gram_eig_scratch((int)n, 8) * sizeof(double);
    return gram_eig_launch(gabo::gram_eig_kernel<false, 512, 16>, attr_ws, lds_max, lds, 512, blocks, e, (int)n, thetas, (int)n_thetas, out,
                           (double*)workspace, stream);
}
