// The factorisation that the forward and the backward launches of the affine-invariant SPD Matern features share (spd_ai_spectral.hip,
// spd_ai_spectral_backward.hip): chol(X_i) staged in LDS once per block, and the modified Gram-Schmidt pass of one lane over the rows of
// M = H_l^T G.  One operation order for both, every multiply-add a spelled-out fma.
#pragma once
#include "gabo_device.hpp"

namespace gabo {

// chol(X_i) -> Gs (packed lower triangle, tri(r, c)), computed row by row in registers by the first wave (every lane on the same values).
template <int D>
__device__ __forceinline__ void spectral_stage_cholesky(const double* __restrict__ xm, double* __restrict__ Gs) {
    if (threadIdx.x < 64) {
        double g[tri_size(D)], inv[D];
        static_for<D>([&](auto rr) {
            constexpr int r = decltype(rr)::value;
            static_for<r + 1>([&](auto cc) {
                constexpr int c = decltype(cc)::value;
                double s = xm[mandel_pos(D, r, c)];
                if constexpr (r != c) s = s / kSqrt2;
                static_for<c>([&](auto kk) { constexpr int k = decltype(kk)::value; s = __builtin_fma(-g[tri(r, k)], g[tri(c, k)], s); });
                if constexpr (r == c) {
                    double piv = s > 0.0 ? __builtin_sqrt(s) : __builtin_nan("");
                    g[tri(r, r)] = piv;
                    inv[r] = 1.0 / piv;
                } else {
                    g[tri(r, c)] = s * inv[c];
                }
            });
        });
        if (threadIdx.x == 0) static_for<tri_size(D)>([&](auto ee) { Gs[decltype(ee)::value] = g[decltype(ee)::value]; });
    }
    __syncthreads();
}

// Modified Gram-Schmidt over the rows of M = H^T G, row k against rows 0 .. k-1 in that order.  hp points at entry (0, 0) of this lane's H in
// the entry-major array.  For k = 0 .. D-1 in order: prev = step(k, |v_k|^2), the value the loads of the next row are made to wait for; the
// first ROWS rows (D - 1: the last one is only measured; D: every row) are left in v (row k at v[k D]) with vinv[k] = 1 / |v_k|^2.
template <int D, int ROWS, class Step>
__device__ __forceinline__ void spectral_gram_schmidt_lane(const double* __restrict__ Gs, const double* __restrict__ hp, int64_t L,
                                                           double* __restrict__ v, double* __restrict__ vinv, Step&& step) {
    static_assert(ROWS == D - 1 || ROWS == D, "rows 0 .. D-2 are needed by the pass itself");
    double prev = 0.0;
    static_for<D>([&](auto kk) {
        constexpr int k = decltype(kk)::value;
        double h[D], m[D];
        // Offsets (zero) that the compiler must take to depend on the step before: without them hipcc loads all of H and keeps G, read from
        // LDS once, in registers - 150 more live doubles at d = 10 - and spills.  With them H and G stream through, step by step.
        int g0 = 0;
        int64_t h0 = 0;
        if constexpr (k > 0) asm volatile("" : "+v"(g0), "+v"(h0) : "v"(prev));
        static_for<D>([&](auto rr) { constexpr int r = decltype(rr)::value; h[r] = hp[h0 + (int64_t)(r * D + k) * L]; });
        static_for<D>([&](auto jj) {          // m_j = sum_{r >= j} H[r][k] G[r][j]
            constexpr int j = decltype(jj)::value;
            double s = h[j] * Gs[g0 + tri(j, j)];
            static_for<D - 1 - j>([&](auto tt) { constexpr int r = j + 1 + decltype(tt)::value; s = __builtin_fma(h[r], Gs[g0 + tri(r, j)], s); });
            m[j] = s;
        });
        static_for<k>([&](auto pp) {
            constexpr int p = decltype(pp)::value;
            double dot = m[0] * v[p * D];
            static_for<D - 1>([&](auto jj) { constexpr int j = 1 + decltype(jj)::value; dot = __builtin_fma(m[j], v[p * D + j], dot); });
            const double coef = -(dot * vinv[p]);
            static_for<D>([&](auto jj) { constexpr int j = decltype(jj)::value; m[j] = __builtin_fma(coef, v[p * D + j], m[j]); });
        });
        double nn = m[0] * m[0];
        static_for<D - 1>([&](auto jj) { constexpr int j = 1 + decltype(jj)::value; nn = __builtin_fma(m[j], m[j], nn); });
        prev = step(kk, nn);
        if constexpr (k < ROWS) {
            vinv[k] = 1.0 / nn;
            static_for<D>([&](auto jj) { constexpr int j = decltype(jj)::value; v[k * D + j] = m[j]; });
        }
    });
}

// emit(k, a_k) for k = 0 .. D-1 in order, a_k = log of the squared norm of row k of M = H^T G after the pass above.
template <int D, class Emit>
__device__ __forceinline__ void spectral_logdiag_lane(const double* __restrict__ Gs, const double* __restrict__ hp, int64_t L, Emit&& emit) {
    double v[(D - 1) * D], vinv[D - 1];
    spectral_gram_schmidt_lane<D, D - 1>(Gs, hp, L, v, vinv, [&](auto kk, double nn) {
        const double ak = log(nn);
        emit(kk, ak);
        return ak;
    });
}

}  // namespace gabo
