// Matern kernels (nu = 1/2, 3/2, 5/2) on the flat SPD metrics: the Gram matrix, its x-gradient and the element-wise forms on features that
// are Mandel vectors - mandel(logm X) for the log-Euclidean metric, mandel(X) for the Frobenius one.  The distance is the library's own,
// r = sqrt(sum_e (x1_e - x2_e + eps_e)^2) with the reference's 1e-15 on every matrix element (frobenius_pairwise_kernel, spd_manifold.hip);
// the formulas are those of flat_matern.hpp.  Layout, grid shape, the d <= 3 register specialisation, the NaN rule and the two-phase backward
// block are the ones of gabo_frobenius_pairwise / gabo_frobenius_backward.
#include "flat_matern.hpp"
#include "../../include/gabo_hip.h"

namespace gabo {

// grid.x = (row chunk, column group), column group fastest; grid.y = batch.  Lane = column j, the x1 row is wave-uniform.
// sym (x1 and x2 are the same set): the pair (i, j) with j > i takes the epsilon with the opposite sign, (x_i - x_j - eps)^2 =
// (x_j - x_i + eps)^2 bit for bit, so that out_ij has the bits of out_ji - the matrix is exactly symmetric at no cost per element.
template <int DSMALL, int NU2>        // DSMALL = d for d <= 3 (x2 vector in registers, compile-time length), 0 = any d
__global__ __launch_bounds__(256) void flat_matern_pairwise_kernel(const double* __restrict__ x1, const double* __restrict__ x2,
                                                                   double* __restrict__ out, int64_t n1, int64_t n2, int d, int64_t s1,
                                                                   int64_t s2, int col_blocks, int rows, double a, int sym) {
    constexpr int DV_REG = DSMALL * (DSMALL + 1) / 2;
    const int dv = DSMALL > 0 ? DV_REG : d * (d + 1) / 2;
    const uint32_t rc = blockIdx.x / (uint32_t)col_blocks, cg = blockIdx.x - rc * (uint32_t)col_blocks;
    const int64_t b = blockIdx.y;
    const int64_t j = (int64_t)cg * blockDim.x + threadIdx.x;
    const int64_t jc = j < n2 ? j : n2 - 1;              // out-of-range lanes recompute the last column and do not store
    const int64_t i0 = (int64_t)rc * rows;
    const int64_t i1 = i0 + rows < n1 ? i0 + rows : n1;
    const double* q = x2 + b * s2 + jc * dv;
    double qv[DV_REG > 0 ? DV_REG : 1];
    if constexpr (DV_REG > 0) {
        static_for<DV_REG>([&](auto ee) { qv[decltype(ee)::value] = q[decltype(ee)::value]; });
    }
    double* ob = out + b * n1 * n2 + j;
    for (int64_t i = i0; i < i1; ++i) {
        const double* p = x1 + b * s1 + i * dv;           // wave-uniform
        const double sgn = (sym && j > i) ? -1.0 : 1.0;
        const double eps_diag = sgn * 1e-15, eps_off = sgn * (kSqrt2 * 1e-15);
        double s = 0.0;
        if constexpr (DV_REG > 0) {
            static_for<DV_REG>([&](auto ee) {
                constexpr int e = decltype(ee)::value;
                double diff = (p[e] - qv[e]) + (e < DSMALL ? eps_diag : eps_off);
                s = __builtin_fma(diff, diff, s);
            });
        } else {
            for (int e = 0; e < dv; ++e) {
                double diff = (p[e] - q[e]) + (e < d ? eps_diag : eps_off);
                s = __builtin_fma(diff, diff, s);
            }
        }
        double val = flat_matern_value<NU2>(__builtin_sqrt(s), a);
        val = s != s ? s : val;                           // a NaN feature gives a NaN value, whatever exp makes of it
        if (j < n2) ob[i * n2] = val;
    }
}

// gx1[b,i,e] = sum_j w_ij (x1_ie - x2_je + sgn*eps_e), w_ij = go_ij * 2 dk/d(r^2) recomputed from the inputs.  One block per (b, i):
// phase 1 the threads own 256 columns j and put w_j in LDS, phase 2 they own the Mandel entries e and walk the 256 columns in order.
// The epsilon is added to the difference, (x1 - x2) + eps as the forward kernel forms it (r has the forward's bits), not to x1 first: at a
// training point x1 - x2 is exactly 0 and x1 + eps would round the epsilon to the spacing of x1, 3 % of it at |x1| = 0.3.
template <int NU2>
__global__ __launch_bounds__(256) void flat_matern_backward_kernel(const double* __restrict__ x1, const double* __restrict__ x2,
                                                                   const double* __restrict__ go, double* __restrict__ gx1, int64_t n1,
                                                                   int64_t n2, int d, int64_t s1, int64_t s2, int64_t go_bs, int64_t go_rs,
                                                                   int64_t go_cs, double a, double eps_sign) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int dv = d * (d + 1) / 2;
    double* P = lds;          // dv : x1 row
    double* Wj = P + dv;      // 256
    const int64_t b = blockIdx.x / n1, i = blockIdx.x - b * n1;
    const double* p = x1 + b * s1 + i * dv;
    for (int e = threadIdx.x; e < dv; e += blockDim.x) P[e] = p[e];
    __syncthreads();
    const double eps_diag = eps_sign * 1e-15, eps_off = eps_sign * (kSqrt2 * 1e-15);
    const int per = (dv + (int)blockDim.x - 1) / (int)blockDim.x;   // <= 3 for d <= 32
    double acc[3] = {0.0, 0.0, 0.0};
    for (int64_t j0 = 0; j0 < n2; j0 += blockDim.x) {
        int64_t j = j0 + threadIdx.x;
        double w = 0.0;
        if (j < n2) {
            const double* q = x2 + b * s2 + j * dv;
            double s = 0.0;
            for (int e = 0; e < d; ++e) { double diff = (P[e] - q[e]) + eps_diag; s = __builtin_fma(diff, diff, s); }
            for (int e = d; e < dv; ++e) { double diff = (P[e] - q[e]) + eps_off; s = __builtin_fma(diff, diff, s); }
            w = go[b * go_bs + i * go_rs + j * go_cs] * flat_matern_weight<NU2>(__builtin_sqrt(s), a);
        }
        Wj[threadIdx.x] = w;
        __syncthreads();
        int64_t cnt = n2 - j0 < (int64_t)blockDim.x ? n2 - j0 : (int64_t)blockDim.x;
        for (int t = 0; t < per; ++t) {
            int e = threadIdx.x + t * blockDim.x;
            if (e < dv) {
                const double* q = x2 + b * s2 + j0 * dv + e;
                const double pe = P[e], ee = e < d ? eps_diag : eps_off;
                double sum = acc[t];
                for (int64_t jj = 0; jj < cnt; ++jj) sum = __builtin_fma(Wj[jj], (pe - q[jj * dv]) + ee, sum);
                acc[t] = sum;
            }
        }
        __syncthreads();
    }
    for (int t = 0; t < per; ++t) {
        int e = threadIdx.x + t * blockDim.x;
        if (e < dv) gx1[(b * n1 + i) * dv + e] = acc[t];
    }
}

template <int NU2, int ORDER>
__global__ __launch_bounds__(256) void flat_matern_from_distance_kernel(const double* __restrict__ r, double* __restrict__ out, int64_t count,
                                                                        double a, double l) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    out[i] = ORDER == 0 ? flat_matern_value<NU2>(r[i], a) : flat_matern_dlengthscale<NU2>(r[i], a, l);
}

}  // namespace gabo

extern "C" {

int gabo_flat_matern_pairwise(const double* x1, const double* x2, double* out, int64_t batch, int64_t n1, int64_t n2, int d,
                              int64_t x1_batch_stride, int64_t x2_batch_stride, double lengthscale, int nu2, gabo_stream_t stream) {
    if (batch < 0 || n1 < 0 || n2 < 0 || x1_batch_stride < 0 || x2_batch_stride < 0) return GABO_ERR_ARG;
    if (!gabo::flat_matern_arguments_ok(lengthscale, nu2)) return GABO_ERR_ARG;
    if (d < 1 || d > 64) return GABO_ERR_DIM;
    if (batch == 0 || n1 == 0 || n2 == 0) return GABO_OK;
    if (!x1 || !x2 || !out) return GABO_ERR_ARG;
    const double a = gabo::flat_matern_scale(lengthscale, nu2);
    const int sym = (x1 == x2 && n1 == n2 && x1_batch_stride == x2_batch_stride) ? 1 : 0;      // one point set: an exactly symmetric matrix
    const int threads = n2 >= 256 ? 256 : (n2 > 128 ? 192 : (n2 > 64 ? 128 : 64));
    const int64_t col_blocks = (n2 + threads - 1) / threads;
    int rows = 64;                                    // rows per block: as many as keep >= ~2048 blocks in flight
    while (rows > 1 && col_blocks * ((n1 + rows - 1) / rows) * batch < 2048) rows >>= 1;
    const int64_t blocks = col_blocks * ((n1 + rows - 1) / rows);
    if (blocks > 0x7fffffffLL) return GABO_ERR_ARG;
    // the batch rides in grid.y (<= 65535): larger batches go out in slices
    for (int64_t b0 = 0; b0 < batch; b0 += 65535) {
        const int64_t nb = batch - b0 < 65535 ? batch - b0 : 65535;
        const dim3 grid((unsigned)blocks, (unsigned)nb);
        const double* x1b = x1 + b0 * x1_batch_stride;
        const double* x2b = x2 + b0 * x2_batch_stride;
        double* outb = out + b0 * n1 * n2;
#define GABO_MATERN_LAUNCH(DS, NU2)                                                                                                       \
    hipLaunchKernelGGL((gabo::flat_matern_pairwise_kernel<DS, NU2>), grid, dim3(threads), 0, (hipStream_t)stream, x1b, x2b, outb, n1, n2, \
                       d, x1_batch_stride, x2_batch_stride, (int)col_blocks, rows, a, sym)
#define GABO_MATERN_NU(DS)                          \
    do {                                            \
        if (nu2 == 1) GABO_MATERN_LAUNCH(DS, 1);    \
        else if (nu2 == 3) GABO_MATERN_LAUNCH(DS, 3); \
        else GABO_MATERN_LAUNCH(DS, 5);             \
    } while (0)
        if (d == 1) GABO_MATERN_NU(1);
        else if (d == 2) GABO_MATERN_NU(2);
        else if (d == 3) GABO_MATERN_NU(3);
        else GABO_MATERN_NU(0);
    }
#undef GABO_MATERN_NU
#undef GABO_MATERN_LAUNCH
    return hipGetLastError() == hipSuccess ? GABO_OK : GABO_ERR_LAUNCH;
}

int gabo_flat_matern_backward(const double* x1, const double* x2, const double* grad_out, double* grad_x1, int64_t batch, int64_t n1,
                              int64_t n2, int d, int64_t x1_batch_stride, int64_t x2_batch_stride, int64_t go_batch_stride,
                              int64_t go_row_stride, int64_t go_col_stride, double lengthscale, int nu2, double eps_sign,
                              gabo_stream_t stream) {
    if (d < 1 || d > GABO_SPD_MAX_DIM) return GABO_ERR_DIM;
    if (batch < 0 || n1 < 0 || n2 < 0 || !gabo::flat_matern_arguments_ok(lengthscale, nu2)) return GABO_ERR_ARG;
    if (batch * n1 == 0) return GABO_OK;
    if (batch * n1 > 0x7fffffffLL) return GABO_ERR_ARG;
    if (!x1 || !grad_x1 || (n2 > 0 && (!x2 || !grad_out))) return GABO_ERR_ARG;
    const double a = gabo::flat_matern_scale(lengthscale, nu2);
    size_t lds = (size_t)(d * (d + 1) / 2 + 256) * sizeof(double);
#define GABO_MATERN_LAUNCH(NU2)                                                                                                          \
    hipLaunchKernelGGL(gabo::flat_matern_backward_kernel<NU2>, dim3((unsigned)(batch * n1)), dim3(256), lds, (hipStream_t)stream, x1, x2, \
                       grad_out, grad_x1, n1, n2, d, x1_batch_stride, x2_batch_stride, go_batch_stride, go_row_stride, go_col_stride, a,  \
                       eps_sign)
    if (nu2 == 1) GABO_MATERN_LAUNCH(1);
    else if (nu2 == 3) GABO_MATERN_LAUNCH(3);
    else GABO_MATERN_LAUNCH(5);
#undef GABO_MATERN_LAUNCH
    return hipGetLastError() == hipSuccess ? GABO_OK : GABO_ERR_LAUNCH;
}

int gabo_flat_matern_from_distance(const double* r, double* out, int64_t count, double lengthscale, int nu2, int order,
                                   gabo_stream_t stream) {
    if (count < 0 || (order != 0 && order != 1) || !gabo::flat_matern_arguments_ok(lengthscale, nu2)) return GABO_ERR_ARG;
    if (count == 0) return GABO_OK;
    const int64_t blocks = (count + 255) / 256;
    if (!r || !out || blocks > 0x7fffffffLL) return GABO_ERR_ARG;
    const double a = gabo::flat_matern_scale(lengthscale, nu2);
#define GABO_MATERN_LAUNCH(NU2, ORDER)                                                                                                   \
    hipLaunchKernelGGL((gabo::flat_matern_from_distance_kernel<NU2, ORDER>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, r, \
                       out, count, a, lengthscale)
    if (order == 0) {
        if (nu2 == 1) GABO_MATERN_LAUNCH(1, 0);
        else if (nu2 == 3) GABO_MATERN_LAUNCH(3, 0);
        else GABO_MATERN_LAUNCH(5, 0);
    } else {
        if (nu2 == 1) GABO_MATERN_LAUNCH(1, 1);
        else if (nu2 == 3) GABO_MATERN_LAUNCH(3, 1);
        else GABO_MATERN_LAUNCH(5, 1);
    }
#undef GABO_MATERN_LAUNCH
    return hipGetLastError() == hipSuccess ? GABO_OK : GABO_ERR_LAUNCH;
}
}
