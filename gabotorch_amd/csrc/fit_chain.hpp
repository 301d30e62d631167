// Host side shared by the one-call fit entries (gabo_nested_spd_fit_evaluate, gabo_nested_sphere_fit_evaluate[_series]): how their device
// workspace is laid out, the likelihood step in the middle of the chain and the read-back that ends it.  Host-only: no kernels here.
#pragma once
#include <hip/hip_runtime.h>

#include <cstring>

#include "../../include/gabo_hip.h"

namespace gabo {

inline size_t fit_align256(size_t b) { return (b + 255) & ~(size_t)255; }

// A workspace as consecutive blocks on 256 bytes: a layout takes its blocks in its constructor (`total` is then the size the entry asks
// for), the entry sets `base` and reads them back through at().
struct FitArena {
    size_t total = 0;
    char* base = nullptr;
    size_t take_bytes(size_t bytes) { const size_t off = total; total += fit_align256(bytes); return off; }
    size_t take(size_t doubles) { return take_bytes(doubles * sizeof(double)); }
    // the block fit_likelihood needs: the tiled likelihood's workspace above GABO_GP_MLL_MAX_N points, nothing below
    size_t take_mll(int64_t n) { return take_bytes(n > GABO_GP_MLL_MAX_N ? gabo_gp_mll_large_workspace_bytes(n) : 0); }
    double* at(size_t off) const { return reinterpret_cast<double*>(base + off); }
};

// Marginal log likelihood of outputscale kb + noise I -> d_out[0..6) and, for wm != NULL, W = alpha alpha^T - Ky^-1: one workgroup up to
// GABO_GP_MLL_MAX_N points, the tiled launches above (their workspace: the arena's take_mll block).
inline int fit_likelihood(const double* kb, const double* y, int64_t n, double outputscale, double noise, double mean, double* d_out, double* wm,
                          void* mll_workspace, gabo_stream_t stream) {
    if (n <= GABO_GP_MLL_MAX_N) return gabo_gp_mll_gram(kb, y, n, outputscale, noise, mean, d_out, wm, stream);
    return gabo_gp_mll_large(kb, y, n, 0.0, outputscale, noise, mean, 1, d_out, wm, mll_workspace, gabo_gp_mll_large_workspace_bytes(n), stream);
}

// The end of a chain: d_out (7 + tail doubles with the gradient, 6 without) through the pinned area h_out to out_host, after the stream has
// drained; without the gradient out_host[6] and the tail are zero.
inline int fit_finish(const double* d_out, double* h_out, double* out_host, size_t tail, int want_grad, hipStream_t s) {
    const size_t out_doubles = want_grad ? 7 + tail : 6;
    if (hipMemcpyAsync(h_out, d_out, sizeof(double) * out_doubles, hipMemcpyDeviceToHost, s) != hipSuccess) return GABO_ERR_LAUNCH;
    if (hipStreamSynchronize(s) != hipSuccess) return GABO_ERR_LAUNCH;
    std::memcpy(out_host, h_out, sizeof(double) * out_doubles);
    if (!want_grad) std::memset(out_host + 6, 0, sizeof(double) * (1 + tail));
    return GABO_OK;
}

}  // namespace gabo
