// Joint posterior of an exact GP over a test set, and samples from it: what `preds = model(x_test)` followed by preds.mean / .variance /
// .covariance_matrix / .sample() costs in the reference's two GP-regression demos (examples/kernels/spd/spd_kernels.py:168-174,
// examples/kernels/sphere/sphere_kernels.py:147-150; [3P] gpytorch's exact prediction strategy and MultivariateNormal).
// With L L^T = Ky = os k + noise I, linv = L^-1 and alpha = Ky^-1 (y - mean) from the prediction cache (gabo_gp_factor or torch, any n):
//
//   gp_posterior_project_kernel   V = os k* linv^T (m x n, zero-padded to 64 rows and 16 columns in the workspace), only the non-zero
//                                 triangle of linv is read;  mean_out = mean + os k* alpha.
//   gp_posterior_cov_kernel       for 64 x 64 tiles i >= j:  S_ij = os k**_ij - sum_t V_it V_jt, stored to the tile and, transposed through
//                                 LDS, to its mirror image: ONE read of the lower tiles of k** and one write of the whole matrix, where the
//                                 composition V V^T, subtraction, result takes three passes over m x m.  The diagonal also goes to var_out.
//   mvn_sample_kernel             one workgroup, m <= GABO_MVN_SAMPLE_MAX_M: Cholesky of S + j I on the packed lower triangle in LDS (the storage
//                                 decision of gram_eig.hip's LDS form) with the jitter ladder j = 0, 1e-8, 1e-7, 1e-6, then out[s] = mean + L z_s.
//   mvn_base_samples_kernel       the normals z alone (for the callers that factor larger matrices themselves).
//
// Both products run on the fp64 matrix pipe: v_mfma_f64_16x16x4_f64, A and B one double per lane (A[lane & 15][k = lane >> 4],
// B[k = lane >> 4][lane & 15]), C/D col = lane & 15, row = (lane >> 4) + 4 reg.  The k loop ascends in steps of 4 from 0 whatever m and the
// grid are, and a padded operand is an exact zero made in registers (project) or written to the workspace (V), never an out-of-range load: an
// entry's bits depend on its own row of k*, its own entry of k** and linv only.
//
// The jitter ladder is [3P] gpytorch's psd_safe_cholesky for doubles (try the matrix as it is, then add 1e-8, 1e-7, 1e-6 to the diagonal of the
// ORIGINAL matrix), restated from memory: PARITY UNPINNED, as the rest of SURVEY App. B.
#include "gabo_device.hpp"
#include "gabo_mirror.hpp"
#include "gabo_philox.hpp"
#include "../../include/gabo_hip.h"

#include <atomic>

namespace gabo {

typedef double v4d __attribute__((ext_vector_type(4)));

constexpr int kPostTile = 64;            // rows and columns of a workgroup's tile of the covariance (4 waves x (16 rows, 4 x 16 columns))
constexpr int kPostChunk = 16;           // columns of V staged in LDS per round (V is padded to a multiple of it)
constexpr int kPostStride = kPostChunk + 2;      // row stride of the staged chunk in doubles: (18 row + k) mod 32 is a different bank pair
                                                 // for each of the 16 rows x 2 k of half a wave's operand read
constexpr uint32_t kMvnTag = 0x6d766e7au;        // "mvnz": fourth Philox counter word of the sampler's normals

__host__ __device__ constexpr int64_t post_mpad(int64_t m) { return (m + kPostTile - 1) / kPostTile * kPostTile; }
__host__ __device__ constexpr int64_t post_npad(int64_t n) { return (n + 15) / 16 * 16; }

// One wave per 16 x 16 tile of V (tile row = blockIdx.x * 4 + wave, tile column = blockIdx.y).  Rows m ... mpad - 1 and columns n ... npad - 1
// of V are written as zeros.  The waves of tile column 0 also form the mean, a lane per row, k ascending.
__global__ __launch_bounds__(256) void gp_posterior_project_kernel(const double* __restrict__ kstar, const double* __restrict__ linv,
                                                                   const double* __restrict__ alpha, int64_t m, int n, double mean,
                                                                   double outputscale, double* __restrict__ v, double* __restrict__ mean_out) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t mpad = post_mpad(m);
    const int npad = (int)post_npad(n);
    const int64_t i0 = ((int64_t)blockIdx.x * 4 + wave) * 16;
    if (i0 >= mpad) return;
    const int t0 = blockIdx.y * 16;
    const int r = lane & 15, kk = lane >> 4;
    const int64_t i = i0 + r;                    // A: row of k*
    const int t = t0 + r;                        // B: row of linv (column of V)
    const bool row_ok = i < m, col_ok = t < n;
    const double* arow = kstar + (row_ok ? i : 0) * n;
    const double* brow = linv + (int64_t)(col_ok ? t : 0) * n;
    const int kend = min(n, t0 + 16);            // linv[t][k] = 0 for k > t: nothing beyond the tile's last column
    v4d acc = {0.0, 0.0, 0.0, 0.0};
    for (int k0 = 0; k0 < kend; k0 += 4) {
        const int k = k0 + kk;
        const double a = (row_ok && k < n) ? outputscale * arow[k] : 0.0;
        const double b = (col_ok && k <= t) ? brow[k] : 0.0;
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int64_t row = i0 + kk + 4 * q;     // < mpad
        const int col = t0 + r;                  // < npad
        v[row * npad + col] = (row < m && col < n) ? acc[q] : 0.0;
    }
    if (blockIdx.y == 0 && lane < 16 && row_ok) {
        double s = 0.0;
#pragma unroll 8
        for (int k = 0; k < n; ++k) s = __builtin_fma(outputscale * arow[k], alpha[k], s);
        mean_out[i] = mean + s;
    }
}

// One workgroup per 64 x 64 tile (bi >= bj) of the covariance: wave w owns rows 16 w ... 16 w + 15 of the tile and its four 16-column groups.
// Every lane keeps its 16 results in the accumulator layout from the first load to the store: entry (q, c) is row 16 w + (lane >> 4) + 4 q,
// column 16 c + (lane & 15) of the tile - 16 lanes on one row, 128 contiguous bytes per row of a load or store.  The mirror image goes
// through LDS, 32 rows of the tile at a time (the buffer of the staged chunks is reused), and leaves in rows of 256 contiguous bytes.
// 18 KB of LDS and 95 registers: five workgroups per CU.
// EDGE: a tile on the diagonal or over the last rows of the matrix (every access guarded); otherwise a full tile strictly below the diagonal.
template <bool EDGE>
__device__ __forceinline__ void posterior_cov_tile(const double* __restrict__ v, double* __restrict__ cov, int64_t m, int npad, double outputscale,
                                                   double* __restrict__ var_out, int64_t i0, int64_t j0, double* lds) {
    constexpr int TS = kPostTile + 1;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const bool diag = EDGE && i0 == j0;
    double* sa = lds;
    double* sb = lds + kPostTile * kPostStride;
    const double* va = v + i0 * npad;            // (V has mpad rows: every row of the tile exists)
    const double* vb = v + j0 * npad;
    const int r = lane & 15, kk = lane >> 4;
    const int64_t gi0 = i0 + 16 * wave + kk, gj0 = j0 + r;      // entry (q, c) is (gi0 + 4 q, gj0 + 16 c)
    double* mine = cov + gi0 * m + gj0;
    auto inside = [&](int q, int c) { return !EDGE || (gi0 + 4 * q < m && gj0 + 16 * c < m && (!diag || gj0 + 16 * c <= gi0 + 4 * q)); };
    v4d acc[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[c] = v4d{0.0, 0.0, 0.0, 0.0};

    for (int kc = 0; kc < npad; kc += kPostChunk) {              // (npad is a multiple of the chunk)
        __syncthreads();
#pragma unroll
        for (int e = tid; e < kPostTile * kPostChunk; e += 256) {
            const int row = e / kPostChunk, col = e % kPostChunk;
            sa[row * kPostStride + col] = va[(int64_t)row * npad + kc + col];
            sb[row * kPostStride + col] = vb[(int64_t)row * npad + kc + col];
        }
        __syncthreads();
#pragma unroll
        for (int k0 = 0; k0 < kPostChunk; k0 += 4) {
            const double a = sa[(16 * wave + r) * kPostStride + k0 + kk];
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const double b = sb[(16 * c + r) * kPostStride + k0 + kk];
                acc[c] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[c], 0, 0, 0);
            }
        }
    }
    // this lane's 16 entries of the tile of k** - the only loads of the kernel that come from HBM - requested together (asking for them in
    // front of the products would keep 32 more registers live through the loop above and cost the fifth workgroup per CU), then the tile
    // itself, from the registers
    double kv[4][4];
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int c = 0; c < 4; ++c) kv[q][c] = inside(q, c) ? mine[4 * q * m + 16 * c] : 0.0;
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const double s = outputscale * kv[q][c] - acc[c][q];
            kv[q][c] = s;
            if (inside(q, c)) {
                mine[4 * q * m + 16 * c] = s;
                if (EDGE && gi0 + 4 * q == gj0 + 16 * c) var_out[gi0 + 4 * q] = s;
            }
        }
    // its mirror image: row j0 + c' of the matrix holds column c' of the tile (strictly above the diagonal in a diagonal tile)
    double* tile = lds;
    for (int h = 0; h < 2; ++h) {
        __syncthreads();
        if ((wave >> 1) == h) {
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int c = 0; c < 4; ++c) tile[(16 * (wave & 1) + kk + 4 * q) * TS + 16 * c + r] = kv[q][c];
        }
        __syncthreads();
        const int tr = tid & 31;                                 // row of the half tile = column of the mirror image
        for (int tc = tid >> 5; tc < kPostTile; tc += 8) {
            const int64_t gi = j0 + tc, gj = i0 + 32 * h + tr;
            if (!EDGE || (gi < m && gj < m && (!diag || gj > gi))) cov[gi * m + gj] = tile[tr * TS + tc];
        }
    }
}

__global__ __launch_bounds__(256)
void gp_posterior_cov_kernel(const double* __restrict__ v, double* __restrict__ cov, int64_t m, int npad, double outputscale,
                             double* __restrict__ var_out) {
    __shared__ double lds[2 * kPostTile * kPostStride];         // two staged chunks of V; afterwards half a tile of the result, row stride 65
    static_assert(2 * kPostTile * kPostStride >= (kPostTile / 2) * (kPostTile + 1), "half a result tile reuses the staging buffers");
    int64_t bi, bj;
    lower_tile_of(blockIdx.x, bi, bj);
    const int64_t i0 = bi * kPostTile, j0 = bj * kPostTile;
    if (bi == bj || i0 + kPostTile > m)
        posterior_cov_tile<true>(v, cov, m, npad, outputscale, var_out, i0, j0, lds);
    else
        posterior_cov_tile<false>(v, cov, m, npad, outputscale, var_out, i0, j0, lds);
}

// ---- sampler ---------------------------------------------------------------------------------------------------------------------------------
__host__ __device__ constexpr int mvn_npad(int m) { return (m + 63) / 64 * 64; }
// doubles of LDS next to the packed triangle: the pivots (npad), the normals of four samples (4 x npad), a header
__host__ __device__ constexpr int mvn_scratch(int m) { return 5 * mvn_npad(m) + 16; }
constexpr int kMvnThreads = 1024;                // four lanes per row of the matrix (rows 0 ... 255 >= GABO_MVN_SAMPLE_MAX_M)

// sum over the four lanes of a quad, the same bits in all four ((a0 + a1) + (a2 + a3) up to the order of the operands)
__device__ __forceinline__ double quad_allsum(double v) {
    v += dpp_fetch<0xB1, 0xf>(v);                // quad_perm [1,0,3,2]
    v += dpp_fetch<0x4E, 0xf>(v);                // quad_perm [2,3,0,1]
    return v;
}

// Left-looking Cholesky, a quad of lanes per row: at column k the quad of row i >= k forms A[i][k] - sum_{j<k} L[i][j] L[k][j] (lane q takes
// j = q, q + 4, ... ascending, then the quad sum), row k's is the pivot; after a barrier every row divides by its square root.  Two barriers
// per column and no pass over the trailing matrix.  Square root and division are the IEEE ones: the factor obeys the textbook backward-error
// bound |L L^T - A| <= gamma_(m+1) |L| |L|^T.
__global__ __launch_bounds__(kMvnThreads) void mvn_sample_kernel(const double* __restrict__ mean, const double* __restrict__ cov, int m,
                                                                 int64_t samples, uint64_t seed, const double* __restrict__ base_samples,
                                                                 double* __restrict__ out, double* __restrict__ scale_tril,
                                                                 int* __restrict__ status) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    constexpr int W = kMvnThreads / 64;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int row = tid >> 2, q = tid & 3;
    const int tsize = m * (m + 1) / 2, npad = mvn_npad(m);
    double* A = lds;                             // packed lower triangle, row-major: (i, j <= i) at i (i + 1) / 2 + j
    double* piv = lds + tsize;                   // npad: the pivots before their square root
    double* zb = piv + npad;                     // 4 x npad: the normals of the four samples in work
    const double* ri = A + row * (row + 1) / 2;  // (rows >= m are never dereferenced)
    const double ladder[4] = {0.0, 1e-8, 1e-7, 1e-6};
    int rung = 0;
    bool ok = false;
    for (; rung < 4; ++rung) {
        const double jitter = ladder[rung];
        __syncthreads();
        for (int i = wave; i < m; i += W) {
            const double* src = cov + (int64_t)i * m;
            double* dst = A + i * (i + 1) / 2;
            for (int c = lane; c <= i; c += 64) dst[c] = c == i ? src[c] + jitter : src[c];
        }
        __syncthreads();
        ok = true;
        for (int k = 0; k < m; ++k) {
            const bool mine = row >= k && row < m;
            double v = 0.0;
            if (mine) {
                const double* rk = A + k * (k + 1) / 2;
                double acc = 0.0;
                for (int j = q; j < k; j += 4) acc = __builtin_fma(ri[j], rk[j], acc);
                v = ri[k] - quad_allsum(acc);
                if (row == k && q == 0) piv[k] = v;
            }
            __syncthreads();
            const double d = piv[k];                             // (every thread reads the same word: the verdict is uniform)
            if (!(d > 0.0)) {                                    // non-positive or NaN pivot: next rung, from the input
                ok = false;
                break;
            }
            const double s = sqrt(d);
            if (mine && q == 0) A[row * (row + 1) / 2 + k] = row == k ? s : v / s;
            __syncthreads();
        }
        if (ok) break;
    }
    if (tid == 0) {
        status[1] = ok ? rung : 4;
        if (!ok) status[0] = GABO_ERR_NOT_SPD;
    }
    if (!ok) return;
    if (scale_tril)
        for (int i = wave; i < m; i += W)
            for (int c = lane; c < m; c += 64) scale_tril[(int64_t)i * m + c] = c <= i ? A[i * (i + 1) / 2 + c] : 0.0;
    const int half = (m + 1) / 2;
    for (int64_t s0 = 0; s0 < samples; s0 += 4) {                // four samples per round: a row of L is read once for the four
        const int nb = (int)(samples - s0 < 4 ? samples - s0 : 4);
        __syncthreads();
        if (base_samples) {
            for (int e = tid; e < nb * m; e += kMvnThreads) {
                const int b = e / m, c = e - b * m;
                zb[b * npad + c] = base_samples[(s0 + b) * m + c];
            }
        } else {
            for (int e = tid; e < nb * half; e += kMvnThreads) {
                const int b = e / half, k = e - b * half;
                Philox ph{(uint32_t)seed, (uint32_t)(seed >> 32), (uint64_t)(s0 + b), (uint32_t)k, kMvnTag};
                double z0, z1;
                ph.normal2(z0, z1);
                zb[b * npad + 2 * k] = z0;
                if (2 * k + 1 < m) zb[b * npad + 2 * k + 1] = z1;
            }
        }
        for (int e = tid; e < (4 - nb) * m; e += kMvnThreads) {  // (the unused vectors of the last round: zeros, not what LDS held)
            const int b = nb + e / m, c = e - (e / m) * m;
            zb[b * npad + c] = 0.0;
        }
        __syncthreads();
        if (row < m) {
            double acc[4] = {0.0, 0.0, 0.0, 0.0};
            for (int j = q; j <= row; j += 4) {
                const double l = ri[j];
#pragma unroll
                for (int b = 0; b < 4; ++b) acc[b] = __builtin_fma(l, zb[b * npad + j], acc[b]);
            }
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const double t = quad_allsum(acc[b]);
                if (q == 0 && b < nb) out[(s0 + b) * m + row] = mean[row] + t;
            }
        }
    }
}

__global__ __launch_bounds__(256) void mvn_base_samples_kernel(double* __restrict__ out, int64_t samples, int m, uint64_t seed) {
    const int64_t half = (m + 1) / 2;
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= samples * half) return;
    const int64_t s = e / half;
    const int k = (int)(e - s * half);
    Philox ph{(uint32_t)seed, (uint32_t)(seed >> 32), (uint64_t)s, (uint32_t)k, kMvnTag};
    double z0, z1;
    ph.normal2(z0, z1);
    out[s * m + 2 * k] = z0;
    if (2 * k + 1 < m) out[s * m + 2 * k + 1] = z1;
}

}  // namespace gabo

static bool gp_posterior_dims_ok(int64_t m, int64_t n) { return m >= 1 && m <= GABO_GP_POSTERIOR_MAX_M && n >= 1 && n <= GABO_GP_MLL_LARGE_MAX_N; }

extern "C" size_t gabo_gp_posterior_joint_workspace_bytes(int64_t m, int64_t n) {
    if (!gp_posterior_dims_ok(m, n)) return 0;
    return (size_t)gabo::post_mpad(m) * (size_t)gabo::post_npad(n) * sizeof(double);
}

extern "C" int gabo_gp_posterior_joint(const double* kstar, double* cov, const double* linv, const double* alpha, int64_t m, int64_t n, double mean,
                                       double outputscale, double* mean_out, double* var_out, void* workspace, size_t workspace_bytes,
                                       gabo_stream_t stream) {
    if (n > GABO_GP_MLL_LARGE_MAX_N || m > GABO_GP_POSTERIOR_MAX_M) return GABO_ERR_DIM;
    if (m < 1 || n < 1 || !kstar || !cov || !linv || !alpha || !mean_out || !var_out || !workspace) return GABO_ERR_ARG;
    if (workspace_bytes < gabo_gp_posterior_joint_workspace_bytes(m, n)) return GABO_ERR_ARG;
    double* v = (double*)workspace;
    const int64_t mpad = gabo::post_mpad(m), npad = gabo::post_npad(n);
    const dim3 pgrid((unsigned)(mpad / 64), (unsigned)(npad / 16));
    hipLaunchKernelGGL(gabo::gp_posterior_project_kernel, pgrid, dim3(256), 0, (hipStream_t)stream, kstar, linv, alpha, m, (int)n, mean,
                       outputscale, v, mean_out);
    if (hipGetLastError() != hipSuccess) return GABO_ERR_LAUNCH;
    const int64_t tiles = mpad / gabo::kPostTile;
    hipLaunchKernelGGL(gabo::gp_posterior_cov_kernel, dim3((unsigned)(tiles * (tiles + 1) / 2)), dim3(256), 0, (hipStream_t)stream,
                       (const double*)v, cov, m, (int)npad, outputscale, var_out);
    return hipGetLastError() == hipSuccess ? GABO_OK : GABO_ERR_LAUNCH;
}

extern "C" int gabo_mvn_sample(const double* mean, const double* cov, int64_t m, int64_t samples, uint64_t seed, const double* base_samples,
                               double* out, double* scale_tril, int* status, gabo_stream_t stream) {
    if (m > GABO_MVN_SAMPLE_MAX_M) return GABO_ERR_DIM;
    if (m < 1 || samples < 0 || !mean || !cov || !status || (samples > 0 && !out)) return GABO_ERR_ARG;
    constexpr int kM = GABO_MVN_SAMPLE_MAX_M;
    constexpr size_t lds_max = (size_t)(kM * (kM + 1) / 2 + gabo::mvn_scratch(kM)) * sizeof(double);
    static_assert(lds_max <= 160 * 1024, "the triangle and its scratch must fit the LDS of a CU");
    const size_t lds = (size_t)(m * (m + 1) / 2 + gabo::mvn_scratch((int)m)) * sizeof(double);
    static std::atomic<uint64_t> attr_set{0};
    int dev = 0;                  // (more than 64 KB of dynamic LDS needs the attribute: set once per device, as gram_eig.hip does)
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev > 63) return GABO_ERR_LAUNCH;
    if (!(attr_set.load(std::memory_order_acquire) >> dev & 1)) {
        if (hipFuncSetAttribute((const void*)gabo::mvn_sample_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_max) != hipSuccess)
            return GABO_ERR_LAUNCH;
        attr_set.fetch_or((uint64_t)1 << dev, std::memory_order_release);
    }
    hipLaunchKernelGGL(gabo::mvn_sample_kernel, dim3(1), dim3(gabo::kMvnThreads), lds, (hipStream_t)stream, mean, cov, (int)m, samples, seed, base_samples, out,
                       scale_tril, status);
    return hipGetLastError() == hipSuccess ? GABO_OK : GABO_ERR_LAUNCH;
}

extern "C" int gabo_mvn_base_samples(double* out, int64_t samples, int64_t m, uint64_t seed, gabo_stream_t stream) {
    if (samples < 0 || m < 1 || m > 0x7fffffff || (samples > 0 && !out)) return GABO_ERR_ARG;
    if (samples == 0) return GABO_OK;
    const int64_t work = samples * ((m + 1) / 2);
    if (work > (int64_t)0x7fffffff * 256) return GABO_ERR_ARG;
    hipLaunchKernelGGL(gabo::mvn_base_samples_kernel, dim3((unsigned)((work + 255) / 256)), dim3(256), 0, (hipStream_t)stream, out, samples, (int)m,
                       seed);
    return hipGetLastError() == hipSuccess ? GABO_OK : GABO_ERR_LAUNCH;
}
