// The library's own sphere constraints (Riemannian_utils/sphere_constraints_utils_torch.py; kinds GABO_SPHERE_CONSTRAINT_*): the kernel argument that
// states a set of them, the value of one constraint at a point and the host check of a set.  Shared by the trust-region kernels (sphere_tr.hip: one
// wave per point, sph_cons_eval adds the Riemannian gradients) and the constrained sampler of the sweep (spd_sweep.hip: one thread per point), so the
// two evaluate ONE statement of every constraint.
#pragma once
#include "../../include/gabo_hip.h"
#include "spd_tcg_body.hpp"

namespace gabo {

// Equalities first.  A kernel argument: kind / index / bound are read with wave-uniform indices.
struct SphCons {
    int n, neq, strict;
    int kind[kMaxCons];
    int index[kMaxCons];        // the coordinate, or the row of `centres` for the ball
    double bound[kMaxCons];
    double delta_cons;
    const double* centres;      // n_centres x dim
};

// <a, b> by ONE thread (the wave-wide product is dotg of sphere_tr.hip)
struct SphThreadDot {
    __device__ __forceinline__ double operator()(const double* a, const double* b, int n) const {
        double s = 0.0;
        for (int e = 0; e < n; ++e) s = __builtin_fma(a[e], b[e], s);
        return s;
    }
};

// value of constraint k at x (dim doubles, global or LDS), written as the torch function states it.  `dot`: the inner product of the caller's
// geometry (a wave or one thread per point).  *inner: <x, centre> of a ball.
template <typename Dot>
static __device__ __forceinline__ double sph_cons_value(const double* __restrict__ x, int dim, const SphCons& K, int k, double* inner, Dot dot) {
    const int kind = K.kind[k], j = K.index[k];
    const double b = K.bound[k];
    if (kind == GABO_SPHERE_CONSTRAINT_GEODESIC_BALL) {
        const double c = dot(x, K.centres + (int64_t)j * dim, dim);
        *inner = c;
        const double cc = c < -1.0 ? -1.0 : (c > 1.0 ? 1.0 : c);
        return b - acos(cc);
    }
    return kind == GABO_SPHERE_CONSTRAINT_COORD_LOWER ? x[j] - b : b - x[j];
}

// every constraint strictly positive at x, evaluated by the calling thread alone (a NaN is not positive)
static __device__ __forceinline__ bool sph_cons_all_positive(const double* __restrict__ x, int dim, const SphCons& K) {
    bool ok = true;
    for (int k = 0; k < K.n; ++k) {
        double c;
        ok = ok && (sph_cons_value(x, dim, K, k, &c, SphThreadDot{}) > 0.0);
    }
    return ok;
}

// the host arrays of a constraint set checked and packed into the kernel argument
static inline int sph_cons_ok(int n, int neq, const int* kind, const int* index, const double* bound, const double* centres, int n_centres, int dim,
                              int strict, double delta_cons, SphCons* K) {
    if (n < 0 || n > kMaxCons || neq < 0 || neq > n || n_centres < 0) return GABO_ERR_ARG;
    if (n > 0 && (!kind || !index || !bound)) return GABO_ERR_ARG;
    *K = SphCons{};
    K->n = n;
    K->neq = neq;
    K->strict = strict != 0;
    K->delta_cons = delta_cons;
    K->centres = centres;
    for (int k = 0; k < n; ++k) {
        const bool coord = kind[k] == GABO_SPHERE_CONSTRAINT_COORD_LOWER || kind[k] == GABO_SPHERE_CONSTRAINT_COORD_UPPER;
        if (!coord && kind[k] != GABO_SPHERE_CONSTRAINT_GEODESIC_BALL) return GABO_ERR_ARG;
        if (index[k] < 0 || index[k] >= (coord ? dim : n_centres) || (!coord && !centres)) return GABO_ERR_ARG;
        K->kind[k] = kind[k];
        K->index[k] = index[k];
        K->bound[k] = bound[k];
    }
    return GABO_OK;
}

}  // namespace gabo
