"""The range of kernel parameters in which a geodesic kernel is positive definite, found on the device.

The geodesic Gaussian and Laplace kernels are positive definite only for some values of beta (of the lengthscale); the reference finds
the range empirically (examples/kernels/spd/spd_gaussian_kernel_parameters.py:84-125, examples/kernels/sphere/
sphere_gaussian_kernel_parameters.py:62-112): random point sets, per parameter value the Gram matrix and its minimum eigenvalue, and the
share of sets whose Gram matrix is positive definite - the `beta_min` of gabo_spd.py:151-162 and gabo_sphere.py:115-128 is read off that
table.  Every plain kernel is exp(-theta * E) with E = d^2 (Gaussian) or d (Laplace) independent of the parameter, so a study is one
distance launch per call, one eigenvalue launch over all (set, parameter) pairs (ops.gram_extreme_eigenvalues) and one copy to the host.

Nested kernels carry parameters inside the distance and are not covered (TypeError).
"""
import numpy as np
import torch

from .. import _lib, ops
from . import kernels_sphere as _ksph
from . import kernels_spd as _kspd


def _spd_ai_distance(v):
    return ops.spd_ai_pairwise(v, v, 1.0, _lib.GABO_OUT_DISTANCE)


def _frobenius_distance(v):
    return ops.frobenius_pairwise(v, v, 1.0, _lib.GABO_OUT_DISTANCE)


def _log_euclidean_distance(v):
    return ops.frobenius_pairwise(*(2 * (ops.spd_logm_mandel(v),)), 1.0, _lib.GABO_OUT_DISTANCE)


def _sphere_distance(v):
    return ops.sphere_pairwise(v, v, 1.0, _lib.GABO_OUT_DISTANCE)


# kernel class -> (distance of a point set to itself, power of the distance in the exponent, the parameter's name).
# theta = beta for the beta kernels and 1 / lengthscale^2 for the lengthscale kernels.
_FORMS = {
    _kspd.SpdAffineInvariantGaussianKernel: (_spd_ai_distance, 2, "beta"),
    _kspd.SpdAffineInvariantLaplaceKernel: (_spd_ai_distance, 1, "beta"),
    _kspd.SpdFrobeniusGaussianKernel: (_frobenius_distance, 2, "lengthscale"),
    _kspd.SpdLogEuclideanGaussianKernel: (_log_euclidean_distance, 2, "lengthscale"),
    _ksph.SphereGaussianKernel: (_sphere_distance, 2, "beta"),
    _ksph.SphereLaplaceKernel: (_sphere_distance, 1, "lengthscale"),
}


def _theta_of_beta(beta):
    return beta


def _theta_of_lengthscale(lengthscale):
    return 1.0 / lengthscale ** 2


_theta_of_beta.parameter = "beta"
_theta_of_lengthscale.parameter = "lengthscale"


def _form(kernel):
    kind = kernel if isinstance(kernel, type) else type(kernel)
    form = _FORMS.get(kind)          # (the exact class: a nested kernel derived from a plain one has parameters inside the distance)
    if form is None:
        raise TypeError(f"{kind.__name__} is not one of the plain kernels exp(-theta * E): {', '.join(k.__name__ for k in _FORMS)}")
    return form


def parameter_map(kernel):
    """The map parameter -> theta of a plain kernel class or instance (floats, arrays and tensors alike); its `.parameter` is the
    parameter's name, "beta" or "lengthscale".  TypeError for any other kernel."""
    return _theta_of_beta if _form(kernel)[2] == "beta" else _theta_of_lengthscale


def exponent_matrix(kernel, x):
    """(E, theta_of) with K = exp(-theta_of(parameter) * E) the Gram matrix of the point set(s) x under `kernel`: a class or an instance of
    SpdAffineInvariant{Gaussian,Laplace}Kernel, SpdFrobeniusGaussianKernel, SpdLogEuclideanGaussianKernel, Sphere{Gaussian,Laplace}Kernel.
    x: (..., N, d_vec) Mandel vectors or (..., N, dim) unit vectors -> E: (..., N, N) fp64 on the HIP device, E = d^2 or d from one distance
    launch; theta_of: see parameter_map.  TypeError for a nested or foreign kernel."""
    dist, power, _ = _form(kernel)
    with torch.no_grad():
        d = dist(x.to(ops._device_for(x)))
        e = (d * d if power == 2 else d).contiguous()
    return e, parameter_map(kernel)


def _as_tensor(x):
    return x if torch.is_tensor(x) else torch.as_tensor(np.asarray(x, dtype=np.float64))


def min_eigenvalues(kernel, data, params):
    """Minimum eigenvalue of the Gram matrix of every point set under every parameter value.
    data: (T, N, .) -> (T, P) numpy array, or one set (N, .) -> (P,): one distance launch, one eigenvalue launch, one copy to the host.
    A list or tuple of sets is stacked when the sets are of equal size and processed set by set otherwise (the condition-number filter
    of the SPD study leaves sets of unequal size) -> (T, P).  params: (P,) values of beta (of the lengthscale)."""
    if isinstance(data, (list, tuple)):
        sets = [_as_tensor(s) for s in data]
        if len(sets) == 0:
            raise ValueError("min_eigenvalues: no point set")
        if any(s.shape != sets[0].shape for s in sets):
            return np.stack([min_eigenvalues(kernel, s, params) for s in sets])
        data = torch.stack(sets)
    x = _as_tensor(data)
    if x.dim() not in (2, 3):
        raise ValueError(f"min_eigenvalues: data must be (N, .), (T, N, .) or a list of (N, .) sets, got {tuple(x.shape)}")
    p = np.asarray(params.detach().cpu() if torch.is_tensor(params) else params, dtype=np.float64).reshape(-1)
    e, theta_of = exponent_matrix(kernel, x)
    return ops.gram_extreme_eigenvalues(e, theta_of(p))[..., 0].cpu().numpy()


def percentage_pd_kernels(kernel, data, params, min_tolerated_eigenvalue=0.0):
    """(share, eigenvalues): per parameter value the share of point sets whose Gram matrix has lambda_min > min_tolerated_eigenvalue - a
    strict comparison, as spd_gaussian_kernel_parameters.py:123-124 (tolerance -5e-7) and sphere_gaussian_kernel_parameters.py:110-111
    (tolerance 0) have it - as a (P,) array, and the (T, P) minimum eigenvalues it was computed from."""
    eig = np.atleast_2d(min_eigenvalues(kernel, data, params))
    return np.sum(eig > min_tolerated_eigenvalue, axis=0) / eig.shape[0], eig


def smallest_pd_parameter(params, percentage, required=1.0):
    """The smallest parameter value from which on every larger one reaches `required`, or None when the largest does not: how `beta_min`
    is read off the table of percentage_pd_kernels."""
    params = np.asarray(params, dtype=np.float64).reshape(-1)
    percentage = np.asarray(percentage, dtype=np.float64).reshape(-1)
    if params.shape != percentage.shape:
        raise ValueError(f"smallest_pd_parameter: {params.size} parameters but {percentage.size} percentages")
    best = None
    for k in np.argsort(params)[::-1]:
        if not percentage[k] >= required:
            break
        best = float(params[k])
    return best
