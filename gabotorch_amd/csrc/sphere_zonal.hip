// Zonal series on the sphere S^d, gfx950, fp64:  f(c) = sum_{k < n_coeff} coeff[k] P_k^{(d)}(c),  c = <x, y>,
// P_k^{(d)} = C_k^{((d-1)/2)}(c) / C_k^{((d-1)/2)}(1) the normalised Gegenbauer polynomial of "series dimension" d (d = 1: Chebyshev):
//     P_0 = 1,  P_1 = c,  (k + d - 2) P_k = (2k + d - 3) c P_{k-1} - (k - 1) P_{k-2}.
// With non-negative coefficients this is a positive-definite kernel for every parameter value: the Riemannian Matern / heat kernels
// (Borovitskiy et al., NeurIPS 2020) are such series (ops.sphere_matern_coefficients), and so are their derivatives in c
// (d/dc P_k^{(d)} = [k (k + d - 1) / d] P_{k-1}^{(d+2)}) and in the lengthscale.  f is a polynomial in c: no clamp, no acos, finite at c = +-1.
//
// With B_k = (k - 1) / (k + d - 2) the recurrence reads P_k = t + B_k (t - P_{k-2}), t = c P_{k-1} (its other factor is 1 + B_k): ONE factor per
// level, and at c = 1 every P_k is 1 to the last bit.  The coefficients and the B_k travel in the kernel arguments (by value: no device
// allocation, no copy), are read through the scalar cache and stay in SGPRs: per level and output
//     t = c P_{k-1};   s = t - P_{k-2};   P_k = fma(B_k, s, t);   f = fma(coeff_k, P_k, f)
// four fp64 VALU instructions with at most one scalar operand each.  The levels are summed in ascending order, two per loop iteration (P_{k-2}
// and P_{k-1} swap roles: no register moves), the next two levels' scalars requested before the current ones are used.
// The Gram kernel forms the inner products as fp64 MFMA tiles like sphere_pairwise.hip (operands loaded per chunk, any dim); a lane finishes its
// 16 results of a chunk in registers, eight at a time, HBM traffic = the output matrix.  The bits of K_ij depend on row i, row j and the series only: the K steps run in
// ascending order from a zero accumulator, padded with 0 * 0, whatever the tile, n1, n2 or batch.
#include "gabo_device.hpp"
#include "gabo_mirror.hpp"
#include "sphere_zonal_level.hpp"
#include "../../include/gabo_hip.h"

namespace gabo {

struct ZonalSeries {       // wave-uniform
    ZonalLevel lv[kZonalMaxCoeff + 3];      // (levels >= n: zeros; the loop requests up to three levels past the last one it uses)
    int n;
};

template <int NV>
__device__ __forceinline__ void zonal_eval(const ZonalSeries& s, const double (&c)[NV], double (&f)[NV]) {
    double p0[NV], p1[NV];
    const double a0 = s.lv[0].a, a1 = s.lv[1].a;      // (a1 = 0 for a series of one term)
    static_for<NV>([&](auto vv) {
        constexpr int v = decltype(vv)::value;
        p0[v] = 1.0;
        p1[v] = c[v];
        f[v] = __builtin_fma(a1, c[v], a0);
    });
    const int n = s.n;
    ZonalLevel e = s.lv[2], o = s.lv[3];
    int k = 2;
    for (; k + 1 < n; k += 2) {
        const ZonalLevel en = s.lv[k + 2], on = s.lv[k + 3];
        static_for<NV>([&](auto vv) {
            constexpr int v = decltype(vv)::value;
            const double te = c[v] * p1[v];
            p0[v] = __builtin_fma(e.rb, te - p0[v], te);                  // P_k in the place of P_{k-2}
            f[v] = __builtin_fma(e.a, p0[v], f[v]);
            const double to = c[v] * p0[v];
            p1[v] = __builtin_fma(o.rb, to - p1[v], to);                  // P_{k+1} in the place of P_{k-1}
            f[v] = __builtin_fma(o.a, p1[v], f[v]);
        });
        e = en;
        o = on;
    }
    if (k < n) {
        static_for<NV>([&](auto vv) {
            constexpr int v = decltype(vv)::value;
            const double te = c[v] * p1[v];
            p0[v] = __builtin_fma(e.rb, te - p0[v], te);
            f[v] = __builtin_fma(e.a, p0[v], f[v]);
        });
    }
}

// element-wise on a precomputed tensor of inner products; four elements per thread and pass
__global__ __launch_bounds__(256) void sphere_zonal_from_inner_kernel(const double* __restrict__ cin, double* __restrict__ out, int64_t n,
                                                                      const ZonalSeries s) {
    const int64_t T = (int64_t)gridDim.x * blockDim.x;
    for (int64_t base = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; base < n; base += 4 * T) {
        double c[4], f[4];
        static_for<4>([&](auto vv) {
            const int64_t g = base + decltype(vv)::value * T;
            c[decltype(vv)::value] = cin[g < n ? g : n - 1];
        });
        zonal_eval<4>(s, c, f);
        static_for<4>([&](auto vv) {
            const int64_t g = base + decltype(vv)::value * T;
            if (g < n) out[g] = f[decltype(vv)::value];
        });
    }
}

typedef double zon_v4d __attribute__((ext_vector_type(4)));

// grid.x: (row chunk group, column group), column group fastest; grid.y: batch.  A block owns 16 * chunks rows x 256 columns, a wave 64
// columns = four 16 x 16 MFMA tiles per 16-row chunk.  Fragment and result layout: sphere_pairwise.hip (A[i = lane & 15][k = lane >> 4],
// B[k = lane >> 4][j = lane & 15]; register r of lane l is row (l >> 4) + 4 r, column l & 15).  No LDS, no barrier.
__global__ __launch_bounds__(256) void sphere_zonal_pairwise_kernel(const double* __restrict__ x1, const double* __restrict__ x2,
                                                                    double* __restrict__ out, int64_t n1, int64_t n2, int dim, int64_t s1,
                                                                    int64_t s2, int col_blocks, int chunks, int flags, const ZonalSeries s) {
    const int tid = threadIdx.x;
    const uint32_t rc = blockIdx.x / (uint32_t)col_blocks, cg = blockIdx.x - rc * (uint32_t)col_blocks;
    const int64_t b = blockIdx.y;
    const int lane = tid & 63, li = lane & 15, lk = lane >> 4;
    const int64_t j0 = (int64_t)cg * blockDim.x + 64 * __builtin_amdgcn_readfirstlane(tid >> 6);      // first column of this wave
    if (j0 >= n2) return;
    const bool sym = (flags & GABO_SYMMETRIC) != 0;
    const double* pb[4];
    static_for<4>([&](auto tt) {
        constexpr int t = decltype(tt)::value;
        int64_t jb = j0 + 16 * t + li;
        jb = jb < n2 ? jb : n2 - 1;                   // out-of-range rows / columns recompute the last one and are not stored
        pb[t] = x2 + b * s2 + jb * dim;
    });
    double* ob = out + b * n1 * n2;
    for (int ch = 0; ch < chunks; ++ch) {
        const int64_t i0 = ((int64_t)rc * chunks + ch) * 16;
        if (i0 >= n1) break;
        // x1 is x2, wave entirely left of the chunk's first row: i > j for every pair it would evaluate (and for every later chunk)
        if (sym && j0 + 63 < i0) break;
        const int64_t ia = (i0 + li < n1) ? i0 + li : n1 - 1;
        const double* pa = x1 + b * s1 + ia * dim;
        zon_v4d acc[4];
        // K is padded to a multiple of 4 with zeros on both sides (0 * 0: an infinite entry must not meet the zero of the other operand); the
        // padded lanes load the last valid entry.  The first step starts from a literal zero accumulator.
        auto kstep = [&](int k0, auto first) {
            const int kk = k0 + lk;
            const bool ok = kk < dim;
            const int kc = ok ? kk : dim - 1;
            double a = pa[kc];
            double bv[4];
            static_for<4>([&](auto tt) { bv[decltype(tt)::value] = pb[decltype(tt)::value][kc]; });
            a = ok ? a : 0.0;
            static_for<4>([&](auto tt) { bv[decltype(tt)::value] = ok ? bv[decltype(tt)::value] : 0.0; });
            static_for<4>([&](auto tt) {
                constexpr int t = decltype(tt)::value;
                if constexpr (decltype(first)::value) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, bv[t], zon_v4d{0.0, 0.0, 0.0, 0.0}, 0, 0, 0);
                else acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, bv[t], acc[t], 0, 0, 0);
            });
        };
        kstep(0, std::true_type{});
        for (int k0 = 4; k0 < dim; k0 += 4) kstep(k0, std::false_type{});
        // two tiles (8 results per lane) at a time: 8 independent recurrences fill the fp64 pipe and leave the kernel at half the registers of 16
        static_for<2>([&](auto hh) {
            constexpr int T0 = 2 * decltype(hh)::value;
            double c[8], f[8];
            static_for<8>([&](auto ee) { c[decltype(ee)::value] = acc[T0 + (decltype(ee)::value >> 2)][decltype(ee)::value & 3]; });
            zonal_eval<8>(s, c, f);
            static_for<2>([&](auto tt) {
                constexpr int t = T0 + decltype(tt)::value;
                const int64_t j = j0 + 16 * t + li;
                static_for<4>([&](auto rr) {
                    constexpr int r = decltype(rr)::value;
                    const int64_t i = i0 + lk + 4 * r;
                    if (i < n1 && j < n2 && (!sym || i <= j)) ob[i * n2 + j] = f[4 * decltype(tt)::value + r];
                });
            });
            __builtin_amdgcn_sched_barrier(0);
        });
    }
}

// diag branch: row k of x1 with row k of x2
__global__ __launch_bounds__(256) void sphere_zonal_diag_kernel(const double* __restrict__ x1, const double* __restrict__ x2,
                                                                double* __restrict__ out, int64_t batch, int64_t n, int dim, int64_t s1,
                                                                int64_t s2, const ZonalSeries s) {
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= batch * n) return;
    const int64_t b = g / n, i = g - b * n;
    const double* p = x1 + b * s1 + i * dim;
    const double* q = x2 + b * s2 + i * dim;
    double c[1] = {0.0}, f[1];
    for (int k = 0; k < dim; ++k) c[0] = __builtin_fma(p[k], q[k], c[0]);
    zonal_eval<1>(s, c, f);
    out[g] = f[0];
}

// host: the series as the kernels take it; GABO_OK or the argument error
static int zonal_series(const double* coeff_host, int n_coeff, int series_dim, ZonalSeries& s) {
    if (n_coeff < 1 || n_coeff > kZonalMaxCoeff || !coeff_host) return GABO_ERR_ARG;
    if (series_dim < 1) return GABO_ERR_DIM;
    s = ZonalSeries{};
    s.n = n_coeff;
    for (int k = 0; k < n_coeff; ++k) {
        s.lv[k].a = coeff_host[k];
        if (k >= 2) s.lv[k].rb = ((double)k - 1.0) / ((double)k + (double)series_dim - 2.0);
    }
    return GABO_OK;
}

}  // namespace gabo

extern "C" int gabo_sphere_zonal_from_inner(const double* inner, double* out, int64_t n, const double* coeff_host, int n_coeff,
                                            int series_dim, gabo_stream_t stream) {
    gabo::ZonalSeries s;
    const int rc = gabo::zonal_series(coeff_host, n_coeff, series_dim, s);
    if (rc != GABO_OK) return rc;
    if (n < 0) return GABO_ERR_ARG;
    if (n == 0) return GABO_OK;
    if (!inner || !out) return GABO_ERR_ARG;
    int64_t blocks = (n + 1023) / 1024;
    if (blocks > 16384) blocks = 16384;
    hipLaunchKernelGGL(gabo::sphere_zonal_from_inner_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, inner, out, n, s);
    return hipGetLastError() == hipSuccess ? GABO_OK : GABO_ERR_LAUNCH;
}

extern "C" int gabo_sphere_zonal_pairwise(const double* x1, const double* x2, double* out, int64_t batch, int64_t n1, int64_t n2, int dim,
                                          int64_t x1_batch_stride, int64_t x2_batch_stride, const double* coeff_host, int n_coeff,
                                          int series_dim, int flags, int diag, gabo_stream_t stream) {
    gabo::ZonalSeries s;
    const int rcs = gabo::zonal_series(coeff_host, n_coeff, series_dim, s);
    if (rcs != GABO_OK) return rcs;
    if (batch < 0 || n1 < 0 || n2 < 0 || x1_batch_stride < 0 || x2_batch_stride < 0) return GABO_ERR_ARG;
    if (dim < 1) return GABO_ERR_DIM;
    if (diag ? n1 != n2 : (batch > 65535 || ((flags & GABO_SYMMETRIC) && n1 != n2))) return GABO_ERR_ARG;
    if (batch == 0 || n1 == 0 || n2 == 0) return GABO_OK;
    if (!x1 || !x2 || !out) return GABO_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    if (diag) {
        const int64_t tot = batch * n1;
        if ((tot + 255) / 256 > 0x7fffffffLL) return GABO_ERR_ARG;
        hipLaunchKernelGGL(gabo::sphere_zonal_diag_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, x1, x2, out, batch, n1, dim,
                           x1_batch_stride, x2_batch_stride, s);
    } else {
        const int threads = n2 >= 256 ? 256 : (n2 > 128 ? 192 : (n2 > 64 ? 128 : 64));
        const int64_t col_blocks = (n2 + threads - 1) / threads;
        // 16-row chunks per block: as many as keep >= 1024 blocks in flight (the chunks of a block share its x2 rows through L1)
        int chunks = 4;
        while (chunks > 1 && col_blocks * ((n1 + 16 * chunks - 1) / (16 * chunks)) * batch < 1024) chunks >>= 1;
        const int64_t row_chunks = (n1 + 16 * chunks - 1) / (16 * chunks);
        const int64_t tiles_x = col_blocks * row_chunks;
        if (tiles_x > 0x7fffffffLL) return GABO_ERR_ARG;
        hipLaunchKernelGGL(gabo::sphere_zonal_pairwise_kernel, dim3((unsigned)tiles_x, (unsigned)batch), dim3(threads), 0, st, x1, x2, out, n1,
                           n2, dim, x1_batch_stride, x2_batch_stride, (int)col_blocks, chunks, flags, s);
        if (flags & GABO_SYMMETRIC) {
            const int tiles = (int)((n1 + 31) / 32);
            hipLaunchKernelGGL((gabo::mirror_upper_kernel<5>), dim3((unsigned)((int64_t)tiles * (tiles + 1) / 2), (unsigned)batch), dim3(256), 0,
                               st, out, n1, tiles);
        }
    }
    return hipGetLastError() == hipSuccess ? GABO_OK : GABO_ERR_LAUNCH;
}
