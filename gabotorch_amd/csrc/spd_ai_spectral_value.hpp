// What the translation units of the affine-invariant SPD Matern features share (spd_ai_spectral.hip: the features from the points;
// spd_ai_spectral_fit.hip: the features and their lengthscale derivative from stored log-diagonals; spd_ai_spectral_backward.hip: the
// x-gradient): the block shape, which fixes the order of the row sums, and the one function that turns (theta, -rho . a, w) into a raw
// feature pair.  The first two must produce the same bits.
#pragma once
#include "gabo_device.hpp"

namespace gabo {

constexpr int kSpectralBlock = 128;          // lanes = features per block
constexpr int kSpectralMaxDim = 10;

// sqrt(w) exp(la) (cos theta, sin theta).  Not inlined: inside the feature loop hipcc would hoist the constants of exp and sincos out of
// the loop and hold them in registers through the factorisation (70 VGPRs at d = 10).
struct SpectralPair {
    double c, s;
};
[[maybe_unused]] static __device__ __attribute__((noinline)) SpectralPair spectral_feature_value(double theta, double la, double w) {
    const double amp = __builtin_sqrt(w) * exp(la);
    double sn, cs;
    sincos(theta, &sn, &cs);
    return {amp * cs, amp * sn};
}

// The row sum of the feature kernels: red holds one partial per lane (each over its own features in ascending order); afterwards red[0] is
// their sum by the halving tree.  Ends behind a barrier.
__device__ __forceinline__ void spectral_row_tree(double* red) {
    __syncthreads();
    for (int s = kSpectralBlock / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] = red[threadIdx.x] + red[threadIdx.x + s];
        __syncthreads();
    }
}

}  // namespace gabo
