"""GPyTorch kernels on the sphere S^n, computed by libgabo_hip.so on the MI355X.
Same class names and signatures as the reference (BoManifolds/kernel_utils/kernels_sphere.py:15-134)."""
from .. import _lib, ops
from .._compat import Kernel
from .kernels_spd import _BetaKernel


class SphereGaussianKernel(_BetaKernel):
    """k(x, y) = exp(-beta acos(<x, y>)^2)   (kernels_sphere.py:15-94)."""

    def forward(self, x1, x2, diag=False, **params):
        return ops.sphere_kernel(x1, x2, self.beta.double(), _lib.GABO_OUT_GAUSSIAN, diag=diag)


class SphereLaplaceKernel(Kernel):
    """k(x, y) = exp(-acos(<x, y>) / lengthscale^2), gpytorch `lengthscale` parameter   (kernels_sphere.py:97-134)."""

    def __init__(self, **kwargs):
        self.has_lengthscale = True
        super().__init__(has_lengthscale=True, ard_num_dims=None, **kwargs)

    def forward(self, x1, x2, diag=False, **params):
        ls = self.lengthscale.double()
        return ops.sphere_kernel(x1, x2, 1.0 / (ls * ls), _lib.GABO_OUT_LAPLACE, diag=diag)


def _matern_arguments(who, nu, num_levels):
    """(nu, num_levels) of a Riemannian Matern kernel class, validated"""
    nu = float(nu)
    if not nu > 0.0:
        raise ValueError(f"{who}: nu = {nu} must be positive (math.inf: the heat kernel)")
    if int(num_levels) != num_levels or not 1 <= int(num_levels) <= ops.SPHERE_ZONAL_MAX_LEVELS:
        raise ValueError(f"{who}: num_levels = {num_levels} outside 1 ... {ops.SPHERE_ZONAL_MAX_LEVELS}")
    return nu, int(num_levels)


class SphereRiemannianMaternKernel(Kernel):
    """Riemannian Matern kernel on the sphere (Borovitskiy et al., NeurIPS 2020; Jaquier et al., CoRL 2021), gpytorch `lengthscale`
    parameter; nu = math.inf is the heat (squared-exponential) kernel.  k(x, y) = sum_{n <= num_levels} p_n P_n(<x, y>) with P_n the
    normalised Gegenbauer polynomials of the sphere and p_n >= 0, sum p_n = 1 (ops.sphere_matern_coefficients): positive definite for EVERY
    lengthscale - no beta_min - and k(x, x) = 1.  The kernel is this truncated sum; a lengthscale well below 1 / num_levels is not resolved.
    nu and num_levels are fixed, not parameters."""

    def __init__(self, nu=2.5, num_levels=32, **kwargs):
        nu, num_levels = _matern_arguments("SphereRiemannianMaternKernel", nu, num_levels)
        self.has_lengthscale = True
        super().__init__(has_lengthscale=True, ard_num_dims=None, **kwargs)
        self.nu, self.num_levels = nu, num_levels

    def forward(self, x1, x2, diag=False, **params):
        # (x1 is x2 - the Gram matrix of one set - takes the symmetric launch inside)
        return ops.sphere_matern_kernel(x1, x2, self.lengthscale.double(), self.nu, self.num_levels, diag=diag)
