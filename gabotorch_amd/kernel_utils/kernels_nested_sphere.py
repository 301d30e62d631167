"""Nested-sphere kernels: the inputs on S^(dim-1) are projected level by level onto the latent sphere (nested_spheres_utils) and a sphere
kernel is evaluated there, all on the MI355X and differentiable in the inputs, the axes and the kernel's own parameter.
NestedSphereGaussianKernel has the reference's constructor, parameters and forward signature (BoManifolds/kernel_utils/
kernels_nested_sphere.py:19-152); NestedSphereRiemannianMaternKernel puts the Riemannian Matern / heat series of kernels_sphere.py in its place."""
import numpy as np
import torch

from .. import _lib, ops
from .._compat import Kernel
from ..manifold_optimization.host_manifolds import Sphere as HostSphere
from ..nested_mappings.nested_spheres_utils import projection_from_sphere_to_subsphere
from .kernels_spd import _BetaKernel
from .kernels_sphere import _matern_arguments


class _NestedSphereAxes:
    """The axes of the nested spheres as parameters raw_axis_S<d>, d = dim ... latent_dim + 1, each with its `<name>_manifold` attribute
    (fit_gpytorch_manifold learns it on that sphere), and the distances to the axes fixed at pi/2."""

    def _register_axes(self, dim, latent_dim):
        self.dim, self.latent_dim = dim, latent_dim
        for d in range(self.dim, self.latent_dim, -1):
            axis = torch.randn(1, d)
            axis = axis / torch.norm(axis)
            self.register_parameter(name="raw_axis_S" + str(d), parameter=torch.nn.Parameter(axis.repeat(*self.batch_shape, 1, 1)))
            setattr(self, "raw_axis_S" + str(d) + "_manifold", HostSphere(d))        # kernels_nested_sphere.py:88-90
        # distance to each axis fixed at pi/2: great subspheres  (kernels_nested_sphere.py:93-94)
        self.distances_to_axis = [np.pi / 2 * torch.ones(1, 1) for _ in range(self.dim, self.latent_dim, -1)]

    @property
    def axes(self):
        return [self._parameters["raw_axis_S" + str(d)] for d in range(self.dim, self.latent_dim, -1)]

    @axes.setter
    def axes(self, values_list):
        self._set_axes(values_list)

    def _set_axes(self, values_list):
        for d in range(self.dim, self.latent_dim, -1):
            value = values_list[self.dim - d]
            name = "raw_axis_S" + str(d)
            if not torch.is_tensor(value):
                value = torch.as_tensor(value)
            self.initialize(**{name: value.to(self._parameters[name])})

    def _project(self, x1, x2):
        axes = [a.double() for a in self.axes]
        px1 = projection_from_sphere_to_subsphere(x1, axes, self.distances_to_axis)[-1]
        px2 = px1 if x2 is x1 else projection_from_sphere_to_subsphere(x2, axes, self.distances_to_axis)[-1]
        return px1, px2


class NestedSphereGaussianKernel(_NestedSphereAxes, _BetaKernel):
    def __init__(self, dim, latent_dim, beta_min, beta_prior=None, **kwargs):
        super().__init__(beta_min, beta_prior, **kwargs)
        self._register_axes(dim, latent_dim)

    def forward(self, x1, x2, diag=False, **params):
        px1, px2 = self._project(x1, x2)
        return ops.sphere_kernel(px1, px2, self.beta.double(), _lib.GABO_OUT_GAUSSIAN, diag=diag)


class NestedSphereRiemannianMaternKernel(_NestedSphereAxes, Kernel):
    """SphereRiemannianMaternKernel on the latent sphere S^(latent_dim-1) of the nested spheres: positive definite for every lengthscale and
    every position of the axes - no beta_min.  gpytorch `lengthscale` parameter; nu (math.inf: the heat kernel) and num_levels are fixed.
    latent_dim >= 2: the series dimension latent_dim - 1 must be at least 1."""

    def __init__(self, dim, latent_dim, nu=2.5, num_levels=32, **kwargs):
        nu, num_levels = _matern_arguments("NestedSphereRiemannianMaternKernel", nu, num_levels)
        if int(latent_dim) != latent_dim or latent_dim < 2:
            raise ValueError(f"NestedSphereRiemannianMaternKernel: latent_dim = {latent_dim} must be an integer >= 2")
        self.has_lengthscale = True
        super().__init__(has_lengthscale=True, ard_num_dims=None, **kwargs)
        self.nu, self.num_levels = nu, num_levels
        self._register_axes(dim, latent_dim)

    def forward(self, x1, x2, diag=False, **params):
        # (x1 is x2: the same projected tensor twice, so the Gram matrix of one set takes the symmetric launch)
        px1, px2 = self._project(x1, x2)
        return ops.sphere_matern_kernel(px1, px2, self.lengthscale.double(), self.nu, self.num_levels, diag=diag)
