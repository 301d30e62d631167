"""GPyTorch kernels on the SPD manifold, computed by libgabo_hip.so on the MI355X.

Same class names, constructor arguments, `beta` parameterisation and `forward` signatures as the reference
(BoManifolds/kernel_utils/kernels_spd.py:17-187).  Inputs are Mandel vectors (..., N, d(d+1)/2); the Mandel->matrix map,
the Cholesky/congruence, the per-pair eigenvalues and exp(-beta d^2) all happen inside one HIP launch.
"""
import torch

from .. import _lib, ops
from .._compat import GreaterThan, Kernel


class _BetaKernel(Kernel):
    """raw_beta parameter + GreaterThan(beta_min) constraint + beta property (kernels_spd.py:33-70)."""

    def __init__(self, beta_min, beta_prior=None, **kwargs):
        super().__init__(has_lengthscale=False, **kwargs)
        self.beta_min = beta_min
        self.register_parameter(name="raw_beta", parameter=torch.nn.Parameter(torch.zeros(*self.batch_shape, 1, 1)))
        if beta_prior is not None:
            self.register_prior("beta_prior", beta_prior, lambda: self.beta, lambda v: self._set_beta(v))
        self.register_constraint("raw_beta", GreaterThan(self.beta_min))

    @property
    def beta(self):
        return self.raw_beta_constraint.transform(self.raw_beta)

    @beta.setter
    def beta(self, value):
        self._set_beta(value)

    def beta_float(self):
        """beta as a Python float (the fp64 value of the parameter, fp32 unless the module was cast), for the launch arguments of the fused paths: the bits of
        `float(self.beta.double())` from ONE tensor operation - softplus of the raw parameter; the constraint's lower bound is added as the
        float32 sum the transform forms (exactly rounded either way) - and remembered per raw value.  The property costs five small tensor
        operations, 25-30 us of a sweep's set-up."""
        raw = self.raw_beta
        con = self.raw_beta_constraint
        if raw.numel() != 1 or type(con) is not GreaterThan or getattr(con, "lower_bound", None) is None:
            return float(self.beta.double())
        key = (raw.detach().item(), id(con))
        held = self.__dict__.get("_beta_float_held")
        if held is None or held[0] != key:
            import numpy as np
            lb = con.__dict__.get("_lower_bound_float")
            if lb is None:
                lb = con.__dict__["_lower_bound_float"] = float(con.lower_bound)
            if raw.dtype not in (torch.float32, torch.float64) or con.lower_bound.dtype != torch.float32 and con.lower_bound.dtype != raw.dtype:
                return float(self.beta.double())
            with torch.no_grad():
                sp = torch.nn.functional.softplus(raw.detach()).item()          # (in the parameter's own precision)
            # the transform's `softplus(raw) + lower_bound.to(raw)`: one exactly rounded sum in the parameter's precision
            val = float(np.float32(sp) + np.float32(lb)) if raw.dtype == torch.float32 else sp + lb
            held = self.__dict__["_beta_float_held"] = (key, val)
        return held[1]

    def _set_beta(self, value):
        if not torch.is_tensor(value):
            value = torch.as_tensor(value).to(self.raw_beta)
        self.initialize(raw_beta=self.raw_beta_constraint.inverse_transform(value))


def _diag_ones(x2):
    # diagonal_distance=True: the reference returns exp(-beta * zeros(..., N2, 1)) (spd_utils_torch.py:72-75)
    return torch.ones(tuple(x2.shape[:-1]) + (1,), dtype=torch.float64, device=x2.device)


class SpdAffineInvariantGaussianKernel(_BetaKernel):
    """k(X, Y) = exp(-beta d_AI(X, Y)^2)   (kernels_spd.py:17-100)."""

    def forward(self, x1, x2, diagonal_distance=False, **params):
        if diagonal_distance is True:
            return _diag_ones(x2)
        return ops.spd_ai_kernel(x1, x2, self.beta.double(), _lib.GABO_OUT_GAUSSIAN)


class SpdAffineInvariantLaplaceKernel(_BetaKernel):
    """k(X, Y) = exp(-beta d_AI(X, Y))   (kernels_spd.py:103-187)."""

    def forward(self, x1, x2, diagonal_distance=False, **params):
        if diagonal_distance is True:
            return _diag_ones(x2)
        return ops.spd_ai_kernel(x1, x2, self.beta.double(), _lib.GABO_OUT_LAPLACE)


class SpdFrobeniusGaussianKernel(Kernel):
    """k(X, Y) = exp(-||X - Y + 1e-15||_F^2 / lengthscale^2) on Mandel inputs   (kernels_spd.py:190-241).
    Differentiable (first order) in x1, x2 and the lengthscale through the HIP backward."""

    def __init__(self, **kwargs):
        self.has_lengthscale = True
        super().__init__(has_lengthscale=True, ard_num_dims=None, **kwargs)

    def forward(self, x1, x2, diagonal_distance=False, **params):
        if diagonal_distance is True:
            return _diag_ones(x2)
        return ops.frobenius_kernel(x1, x2, _beta_from_lengthscale(self.lengthscale), _lib.GABO_OUT_GAUSSIAN)


class SpdLogEuclideanGaussianKernel(Kernel):
    """k(X, Y) = exp(-||logm X - logm Y + 1e-15||_F^2 / lengthscale^2)   (kernels_spd.py:244-313): O(N) matrix logarithms
    (one wave per matrix) + one pairwise Frobenius launch, instead of the reference's two Python loops."""

    def __init__(self, **kwargs):
        self.has_lengthscale = True
        super().__init__(has_lengthscale=True, ard_num_dims=None, **kwargs)

    def forward(self, x1, x2, diagonal_distance=False, **params):
        if diagonal_distance is True:
            return _diag_ones(x2)
        l1 = ops.spd_logm_mandel_diff(x1)
        l2 = l1 if x2 is x1 else ops.spd_logm_mandel_diff(x2)
        return ops.frobenius_kernel(l1, l2, _beta_from_lengthscale(self.lengthscale), _lib.GABO_OUT_GAUSSIAN)


class _FlatMaternKernel(Kernel):
    """The Matern kernel of a flat SPD metric: the metric's feature map is an isometry into R^{d(d+1)/2}, so the Riemannian Matern kernel
    is the Euclidean one of the distance r and is positive definite for every lengthscale (no beta_min, nothing for kernel_parameters to
    find).  gpytorch's MaternKernel parametrisation, x = sqrt(2 nu) r / lengthscale:
        k = exp(-x) | (1 + x) exp(-x) | (1 + x + x^2 / 3) exp(-x)     for nu = 0.5 | 1.5 | 2.5,
    NOT the exp(-r^2 / lengthscale^2) convention of the Gaussian classes (their nu = infinity limit is exp(-r^2 / (2 lengthscale^2))).
    nu is fixed, not a parameter.  Differentiable (first order) in x1, x2 and the lengthscale through the HIP backward."""

    def __init__(self, nu=2.5, **kwargs):
        if isinstance(nu, bool) or not isinstance(nu, (int, float)) or nu not in (0.5, 1.5, 2.5):
            raise ValueError(f"nu must be 0.5, 1.5 or 2.5, got {nu!r}")
        self.has_lengthscale = True
        super().__init__(has_lengthscale=True, ard_num_dims=None, **kwargs)
        self.nu = float(nu)

    def _features(self, x):
        return x

    def forward(self, x1, x2, diagonal_distance=False, **params):
        if diagonal_distance is True:
            return _diag_ones(x2)
        f1 = self._features(x1)
        f2 = f1 if x2 is x1 else self._features(x2)
        return ops.flat_matern_kernel(f1, f2, self.lengthscale.double().reshape(()), self.nu)


class SpdFrobeniusMaternKernel(_FlatMaternKernel):
    """Matern kernel (nu = 0.5, 1.5, 2.5) of the Frobenius distance ||X - Y + 1e-15||_F on Mandel inputs."""


class SpdLogEuclideanMaternKernel(_FlatMaternKernel):
    """Matern kernel (nu = 0.5, 1.5, 2.5) of the log-Euclidean distance ||logm X - logm Y + 1e-15||_F on Mandel inputs: O(N) matrix
    logarithms, reused when x2 is x1, and one pairwise launch."""

    def _features(self, x):
        return ops.spd_logm_mandel_diff(x)


class SpdAffineInvariantMaternKernel(Kernel):
    """Riemannian Matern (nu > 0) or heat (nu = math.inf) kernel of the affine-invariant metric on S^dim_++, which has no closed form, by the
    random phase features of non-compact symmetric spaces (Azangulov et al. 2023): k(X, Y) = <F(X), F(Y)> with 2 num_features features per
    point, each from one order-dim Cholesky factorisation (ops.spd_ai_spectral_features).  A Monte-Carlo approximation of the kernel, error
    O(1 / sqrt(num_features)), that is positive semi-definite with k(X, X) = 1 for EVERY lengthscale and every seed: one `lengthscale`
    (exp(-r^2 / (2 lengthscale^2)) is the flat-space limit of the heat kernel, the convention of the sphere and flat-SPD Matern classes), no
    beta_min.  nu is fixed, not a parameter; the random draw (seed) is fixed at construction and shared by every lengthscale.
    forward takes the cheapest route that supports the gradients asked for: none - one fused launch per point set; the lengthscale only - the
    log-diagonals from one launch, remembered for the last point set (a fit computes them once), then element-wise torch; x with a lengthscale
    that does not require grad (an acquisition maximiser over a fitted, frozen model) - the fused launch, and one backward launch pair per
    point set and backward() (ops.spd_ai_spectral_features_backward; first order); x together with the lengthscale, or x_grad="torch" - a plain
    torch composition (first order, slow).  dim <= 10 on the device."""

    def __init__(self, dim, nu=2.5, num_features=1024, seed=0, x_grad="launch", **kwargs):
        base = ops.spd_ai_spectral_base(dim, num_features, nu, seed)          # (validates dim, num_features and nu)
        if x_grad not in ("launch", "torch"):
            raise ValueError(f"x_grad must be 'launch' or 'torch', got {x_grad!r}")
        self.has_lengthscale = True
        super().__init__(has_lengthscale=True, ard_num_dims=None, **kwargs)
        self.dim, self.nu, self.num_features, self.seed = dim, float(nu), num_features, seed
        self.spectral_base, self.x_grad = base, x_grad
        self._phases = {}               # device -> H (L, d, d)
        self._logdiag_held = None

    def _phases_on(self, device):
        h = self._phases.get(device)
        if h is None:
            h = self._phases[device] = torch.as_tensor(self.spectral_base[2], dtype=torch.float64).to(device)
        return h

    def _logdiag(self, x, phases):
        key = (x.data_ptr(), x._version, tuple(x.shape), x.device, x.dtype)
        held = self._logdiag_held
        if held is None or held[0] != key:
            held = self._logdiag_held = (key, ops.spd_ai_logdiag(x, phases), x)      # (holding x keeps its address its own)
        return held[1]

    def _points(self, x):
        """(..., N, dv) -> the (M, dv) points to compute features of, and how to shape (M, 2L) back; an expanded batch is one point set"""
        bshape = x.shape[:-2]
        if len(bshape) == 0:
            return x, lambda f: f
        if all(st == 0 for st, sz in zip(x.stride()[:len(bshape)], bshape) if sz > 1):
            return x[(0,) * len(bshape)], lambda f: f.expand(bshape + f.shape)
        return x.reshape(-1, x.shape[-1]), lambda f: f.reshape(bshape + (x.shape[-2], f.shape[-1]))

    def forward(self, x1, x2, diagonal_distance=False, **params):
        if diagonal_distance is True:
            return _diag_ones(x2)
        if x1.shape[-1] != self.dim * (self.dim + 1) // 2 or x2.shape[-1] != x1.shape[-1]:
            raise RuntimeError(f"expected Mandel vectors of length {self.dim * (self.dim + 1) // 2}, got {tuple(x1.shape)} and {tuple(x2.shape)}")
        ls = self.lengthscale.double().reshape(())
        dev = ops._device_for(x1, x2)
        lam, w = ops.spd_ai_spectral_points(self.spectral_base, ls.to(dev), self.nu)
        phases = self._phases_on(dev)
        grad = torch.is_grad_enabled()

        def logdiag_of(x):      # the remembered log-diagonals when only the lengthscale is differentiated
            return self._logdiag(x, phases) if grad and ls.requires_grad and not x.requires_grad else None

        same = x2 is x1
        p1, shape1 = self._points(x1)
        p2, shape2 = (p1, shape1) if same else self._points(x2)
        if x1.dim() == 2 and x2.dim() == 2:
            return ops.spd_ai_matern_kernel(p1, p2, phases, lam, w, logdiag1=logdiag_of(p1), logdiag2=None if same else logdiag_of(p2),
                                            x_grad=self.x_grad)
        f1 = shape1(ops.spd_ai_spectral_features(p1, phases, lam, w, logdiag=logdiag_of(p1), x_grad=self.x_grad))
        f2 = f1 if same else shape2(ops.spd_ai_spectral_features(p2, phases, lam, w, logdiag=logdiag_of(p2), x_grad=self.x_grad)).to(f1.device)
        return f1 @ f2.transpose(-1, -2)


def _beta_from_lengthscale(ls):
    # exp(-d^2 / l^2) = exp(-beta d^2) with beta = l^-2, kept in torch so the lengthscale stays differentiable for the GP fit
    ls = ls.double().reshape(())
    return 1.0 / (ls * ls)


class _NestedProjection:
    """The projection matrix W in G(D, d) of the nested SPD kernels: a plain parameter, drawn as qr(randn) after the base kernel's own
    parameters (one torch.randn call, so the nested classes start from the same W under one seed), with its manifold for
    fit_gpytorch_manifold."""

    def _init_projection(self, dim, latent_dim):
        self.dim, self.latent_dim = dim, latent_dim
        q, _ = torch.linalg.qr(torch.randn(dim, latent_dim, dtype=torch.float64))
        self.register_parameter(name="raw_projection_matrix", parameter=torch.nn.Parameter(q.repeat(*self.batch_shape, 1, 1)))
        from ..manifold_optimization.host_manifolds import Grassmann
        self.raw_projection_matrix_manifold = Grassmann(dim, latent_dim)          # kernels_nested_spd.py:75,175

    @property
    def projection_matrix(self):
        return self.raw_projection_matrix

    @projection_matrix.setter
    def projection_matrix(self, value):
        self.initialize(raw_projection_matrix=value)


class NestedSpdAffineInvariantGaussianKernel(_NestedProjection, _BetaKernel):
    """Affine-invariant Gaussian kernel after the nested projection Y = W^T X W, W in G(D, d)
    (kernel_utils/kernels_nested_spd.py:19-136).  The projection matrix is a plain parameter here (pymanopt's Grassmann
    manifold, used by the reference only to draw the initial W, is replaced by qr(randn))."""

    def __init__(self, dim, latent_dim, beta_min, beta_prior=None, **kwargs):
        super().__init__(beta_min, beta_prior, **kwargs)
        self._init_projection(dim, latent_dim)

    def forward(self, x1, x2, diagonal_distance=False, **params):
        if diagonal_distance is True:
            return _diag_ones(x2)
        w = self.projection_matrix.double()
        beta = self.beta.double()
        if ops.nested_spd_gram_applicable(x1, x2, w, beta):      # nobody differentiates this evaluation: projection + factorisation in one launch
            return ops.nested_spd_gram(x1, x2, w, float(beta), _lib.GABO_METRIC_AFFINE_INVARIANT)
        p1 = ops.spd_project_diff(x1, w)
        p2 = p1 if x2 is x1 else ops.spd_project_diff(x2, w)
        return ops.spd_ai_kernel(p1, p2, beta, _lib.GABO_OUT_GAUSSIAN)


class NestedSpdLogEuclideanGaussianKernel(_NestedProjection, SpdLogEuclideanGaussianKernel):
    """Log-Euclidean Gaussian kernel after the nested projection   (kernels_nested_spd.py:139-246; the kernel examples/hd_gabo_spd.py:164 uses)."""

    def __init__(self, dim, latent_dim, **kwargs):
        super().__init__(**kwargs)
        self._init_projection(dim, latent_dim)

    def forward(self, x1, x2, diagonal_distance=False, **params):
        if diagonal_distance is True:
            return _diag_ones(x2)
        w = self.projection_matrix.double()
        if ops.nested_spd_gram_applicable(x1, x2, w, self.lengthscale):      # projection + logm in one launch, then the Frobenius Gram
            return ops.nested_spd_gram(x1, x2, w, float(_beta_from_lengthscale(self.lengthscale)), _lib.GABO_METRIC_LOG_EUCLIDEAN)
        p1 = ops.spd_project_diff(x1, w)
        p2 = p1 if x2 is x1 else ops.spd_project_diff(x2, w)
        return super().forward(p1, p2)


class NestedSpdLogEuclideanMaternKernel(_NestedProjection, SpdLogEuclideanMaternKernel):
    """Log-Euclidean Matern kernel (nu = 0.5, 1.5, 2.5, fixed) after the nested projection Y = W^T X W, W in G(D, d): positive definite for
    every lengthscale and every W, one `lengthscale` in gpytorch's Matern parametrisation.  The projection matrix, its property and its manifold
    are those of NestedSpdLogEuclideanGaussianKernel; under one torch.manual_seed both classes start from the same W."""

    def __init__(self, dim, latent_dim, nu=2.5, **kwargs):
        super().__init__(nu=nu, **kwargs)
        self._init_projection(dim, latent_dim)

    def forward(self, x1, x2, diagonal_distance=False, **params):
        if diagonal_distance is True:
            return _diag_ones(x2)
        w = self.projection_matrix.double()
        if ops.nested_spd_gram_applicable(x1, x2, w, self.lengthscale):      # projection + logm in one launch, then the Matern Gram
            return ops.nested_spd_matern_gram(x1, x2, w, self.lengthscale.double().reshape(()), self.nu)
        p1 = ops.spd_project_diff(x1, w)
        p2 = p1 if x2 is x1 else ops.spd_project_diff(x2, w)
        return super().forward(p1, p2)
