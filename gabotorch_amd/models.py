"""Minimal exact-GP surrogate + analytic acquisition with botorch's call conventions, so the acquisition sweep runs where
gpytorch/botorch are absent (this image, the GPU box).  When those packages exist, their `SingleTaskGP` /
`ExpectedImprovement` can be used with the kernel classes of this package instead; `joint_optimize_manifold` only needs
a callable `acq(X: b x q x d) -> b`.

Semantics restated from botorch/gpytorch ([3P] unpinned): constant mean, ScaleKernel outputscale,
homoskedastic Gaussian noise; eval-mode posterior evaluates k(X*, X_train) with the CANDIDATES as the first argument;
EI(maximize=False): sigma = sqrt(clamp_min(var, 1e-9)), u = -(mu - best_f)/sigma, EI = sigma (phi(u) + u Phi(u)).
The small dense linear algebra here (n_train <= a few hundred) is torch; the kernel evaluations and their gradients are
the HIP kernels.
"""
import functools
import math
import warnings

import torch

from . import _lib as _l, ops as _ops


class BadInitialCandidatesWarning(RuntimeWarning):
    pass


class MultivariateNormal:
    """gpytorch.distributions.MultivariateNormal as the reference's GP-regression demos read it (examples/kernels/spd/spd_kernels.py:168-174)
    [3P]: mean, variance, stddev, covariance_matrix, confidence_region(), sample() / rsample() - what `model(x_test)` returns.  One test
    set (mean (m,), covariance m x m, dense); nothing here is differentiable.  The factor behind the samples is gpytorch's psd_safe_cholesky
    ladder for doubles (ops.mvn_sample): `jitter_used` tells which rung it took."""

    def __init__(self, mean, covariance_matrix, variance=None):
        if mean.dim() != 1 or covariance_matrix.dim() != 2 or tuple(covariance_matrix.shape) != (mean.shape[0], mean.shape[0]):
            raise ValueError(f"MultivariateNormal: mean {tuple(mean.shape)} and covariance {tuple(covariance_matrix.shape)}: one test set, (m,) and m x m")
        self._mean, self._cov, self._var = mean, covariance_matrix, variance
        self._factor = None                       # (scale_tril, rung) of the last factorisation

    @property
    def mean(self):
        return self._mean

    loc = mean

    @property
    def covariance_matrix(self):
        return self._cov

    @property
    def variance(self):
        """the diagonal of the covariance, clamped at 0 (rounding can leave a tiny negative entry where the posterior pins f)"""
        v = torch.diagonal(self._cov) if self._var is None else self._var
        return v.clamp_min(0.0)

    @property
    def stddev(self):
        return self.variance.sqrt()

    @property
    def event_shape(self):
        return self._mean.shape

    def confidence_region(self):
        """(mean - 2 stddev, mean + 2 stddev)"""
        s2 = 2.0 * self.stddev
        return self._mean - s2, self._mean + s2

    def _draw(self, sample_shape, base_samples, seed):
        dev = _ops._device_for(self._cov)
        out, tril, rung = _ops.mvn_sample(self._mean.to(dev), self._cov.to(dev), sample_shape, seed=seed, base_samples=base_samples,
                                          return_scale_tril=True)
        self._factor = (tril, rung)
        return out

    def sample(self, sample_shape=torch.Size(), base_samples=None, seed=None):
        """sample_shape + (m,) draws mean + L z on the distribution's device; z = base_samples (sample_shape + (m,)) when given, else the
        library's counter-based normals for `seed` (None: a seed from numpy's global generator)."""
        return _ops._out(self._draw(tuple(sample_shape), base_samples, seed), self._mean.device)

    rsample = sample

    @property
    def scale_tril(self):
        """L with L L^T = covariance + jitter_used * I, lower triangular"""
        if self._factor is None:
            self._draw((0,), None, 0)
        return _ops._out(self._factor[0], self._mean.device)

    @property
    def jitter_used(self):
        """what the factorisation added to the diagonal: an entry of _lib.GABO_MVN_JITTER_LADDER (reads one word back from the device)"""
        if self._factor is None:
            self._draw((0,), None, 0)
        _ops.check_deferred()
        return _l.GABO_MVN_JITTER_LADDER[int(self._factor[1])]


def _joint_posterior(base_kernel, outputscale, train_x, linv, alpha, mean, X):
    """the distribution of the latent f at the test set X (m x d_vec): k* and k** from the kernel's own launches, then ops.gp_posterior_joint"""
    if not torch.is_tensor(X) or X.dim() != 2:
        raise ValueError(f"forward: X must be one test set, m x d_vec, got {tuple(getattr(X, 'shape', ()))}; batches of candidates go through posterior()")
    with torch.no_grad():
        X = X.double()
        dev = _ops._device_for(linv, X)
        kstar = base_kernel.forward(X, train_x.to(X.device)).double()
        kss = base_kernel.forward(X, X).double()
        if kstar.dim() != 2 or kss.dim() != 2:
            raise ValueError("forward: the kernel returned a batch of matrices; a joint posterior is over one test set")
        mu, var, cov = _ops.gp_posterior_joint(kstar.to(dev), kss.to(dev), linv.to(dev), alpha.to(dev), float(mean), float(outputscale))
        out_dev = X.device
        return MultivariateNormal(_ops._out(mu, out_dev), _ops._out(cov, out_dev), _ops._out(var, out_dev))


def _drop_caches(model):
    model._cache = None
    model._cache_linv_t = None
    model._cache_factors = None
    model._cache_kinv = None


def _held(model, name):
    """what `model` keeps under `name` for exactly its current cache object (None otherwise)"""
    held = getattr(model, name, None)
    return held[1] if held is not None and model._cache is not None and held[0] is model._cache else None


def _condition_cache(model, base_kernel, outputscale, noise, mean, X, Y, holder):
    """The caches of `model` (filled) extended by the points X (t x d_vec) with targets Y (t, or None: the believer's) through
    ops.gp_condition -> (train_x, train_y, linv, linv_t, alpha, kinv or None, factors or None) of the n + t points.  The two kernel strips,
    old x new and new x new, are ONE launch of the kernel's own, forward([train_x; X], X) ((n + t) x t), read with the EARLIER point as
    first argument: the orientation in which the x1-is-x2 build of a training Gram matrix evaluates its entries (i <= j, then mirrored) -
    the library's SPD kernels factor their first argument, so k(a, b) and k(b, a) differ in the last bits, and those bits times cond(Ky)
    would separate this cache from a fresh model's.  The two arguments are different tensors, so the launch never takes the x1-is-x2
    route: the entry of point b against an earlier point a is the same arithmetic whether a arrived in this call or in an earlier one,
    and chained calls give the bits of one call.  holder: the models whose caches a failed update drops (the caller appends the model
    it builds)."""
    if not torch.is_tensor(X) or X.dim() != 2 or X.shape[0] < 1:
        raise ValueError(f"condition_on_observations: X must be one set of new points, t x d_vec, got {tuple(getattr(X, 'shape', ()))}")
    train_x, train_y = model.train_x, model.train_y
    if train_x.dim() != 2 or not train_x.is_cuda:
        raise ValueError("condition_on_observations: the model's training set must be one n x d_vec set on a HIP device")
    if X.device != train_x.device or X.shape[-1] != train_x.shape[-1]:
        raise ValueError(f"condition_on_observations: X {tuple(X.shape)} on {X.device} does not extend the training set {tuple(train_x.shape)} on "
                         f"{train_x.device}")
    t = X.shape[0]
    if Y is not None:
        Y = torch.as_tensor(Y).to(train_x.device, torch.float64).reshape(-1)
        if Y.numel() != t:
            raise ValueError(f"condition_on_observations: {Y.numel()} targets for {t} points")
    linv, alpha = model._cache[0], model._cache[1]
    kinv, factors = _held(model, "_cache_kinv"), _held(model, "_cache_factors")
    with torch.no_grad():
        X = X.double().contiguous()
        n = train_x.shape[0]
        all_x = torch.cat([train_x, X])
        strip = base_kernel.forward(all_x, X).double()
        if tuple(strip.shape) != (n + t, t):
            raise ValueError("condition_on_observations: the kernel returned a batch of matrices; one set of new points at a time")
        kcross, knew = strip[:n].t().contiguous(), strip[n:].t().contiguous()

        def drop():
            for m in holder:
                _drop_caches(m)
        linv_n, linv_t_n, alpha_n, kinv_n, y_used = _ops.gp_condition(linv, alpha, kcross, knew, Y, outputscale=float(outputscale), noise=float(noise),
                                                                      mean=float(mean), kinv=kinv, want_linv_t=True, on_fail=drop)
        if factors is not None:
            factors = torch.cat([factors, _ops.spd_acq_prepare_train(X)], dim=1)
        return (all_x, torch.cat([train_y.to(train_x.device), y_used]), linv_n, linv_t_n, alpha_n, kinv_n, factors)


def _install_caches(model, cache, linv_t, kinv, factors):
    """tied to the cache object by identity, exactly as the models' own routes tie them"""
    model._cache = cache
    model._cache_linv_t = (cache, linv_t)
    model._cache_kinv = (cache, kinv)
    if factors is not None:
        model._cache_factors = (cache, factors)


def _device_cache(model, base_kernel, outputscale, noise, mean, tail=(), matrix_only=False):
    """Fills the caches of `model` from ONE launch instead of Cholesky (+ its info read-back), cholesky_solve and a triangular solve:
    `_cache` = (L^-1, alpha) + tail, with L^-T and the symmetric inverse tied to it.  An affine-invariant kernel on one set of matrices that
    fit the registers takes ops.spd_gp_prepare - what its forward launches (the x1-is-x2 build), the factor and the fused evaluators' training
    factors from one host call - any other kernel its own forward, then ops.gp_factor (csrc/gp_factor.hip).  A factor that does not exist
    drops all four caches again: ops.check_deferred calls `on_fail` before it raises.  matrix_only: a batch of Gram matrices installs nothing."""
    from .kernel_utils import kernels_spd as _ks
    x, factors = model.train_x, None
    drop = functools.partial(_drop_caches, model)
    with torch.no_grad():
        if type(base_kernel) in (_ks.SpdAffineInvariantGaussianKernel, _ks.SpdAffineInvariantLaplaceKernel) and x.dim() == 2 \
                and x.shape[-1] <= _l.GABO_SPD_REG_MAX_DIM * (_l.GABO_SPD_REG_MAX_DIM + 1) // 2:
            mode = _l.GABO_OUT_GAUSSIAN if type(base_kernel) is _ks.SpdAffineInvariantGaussianKernel else _l.GABO_OUT_LAPLACE
            linv, linv_t, alpha, factors, kinv = _ops.spd_gp_prepare(x, model.train_y, base_kernel.beta_float(), mode, outputscale, noise, mean, on_fail=drop)
        else:
            kb = base_kernel.forward(x, x)
            if matrix_only and kb.dim() != 2:
                return
            linv, linv_t, alpha, kinv = _ops.gp_factor(kb.double(), model.train_y, outputscale, noise, mean, defer_check=True, on_fail=drop, want_kinv=True)
    _install_caches(model, (linv, alpha) + tail, linv_t, kinv, factors)


def _torch_cache(ky, y, mean):
    """(L^-1, alpha) of Ky = outputscale K + noise I through torch.linalg: any size, any device.  L^-1 once: the per-call triangular solve
    becomes a GEMM (rocBLAS trsm allocates workspace, which a hipGraph capture of the acquisition evaluation does not allow)."""
    L = torch.linalg.cholesky(ky)
    alpha = torch.cholesky_solve((y.to(L.device) - mean).unsqueeze(-1), L).squeeze(-1)
    return torch.linalg.solve_triangular(L, torch.eye(L.shape[-1], dtype=L.dtype, device=L.device), upper=False), alpha


def _marginal_posterior(kernel, train_x, linv, alpha, X):
    """X: b x 1 x d (or b x d) -> (mean b WITHOUT the constant, variance b); kernel(X1, X2): the scaled kernel matrix.  Differentiable in X."""
    if X.dim() == 2:
        X = X.unsqueeze(-2)
    b = X.shape[0]
    xt = train_x.to(X.device).expand(b, *train_x.shape)                     # stride-0 batch: factored once by the kernel
    ks = kernel(X, xt).squeeze(-2)                                          # b x n   (candidates first)
    kss = kernel(X, X)                                                      # b x 1 x 1
    Li, ad = linv.to(ks.device), alpha.to(ks.device)
    mean = ks @ ad
    v = ks @ Li.transpose(-1, -2)                                           # b x n  = (L^-1 ks^T)^T
    return mean, kss.reshape(b) - (v * v).sum(-1)


class ExactGP(torch.nn.Module):
    def __init__(self, train_x, train_y, base_kernel, outputscale=1.0, noise=1e-2, mean=None):
        super().__init__()
        self.base_kernel = base_kernel
        self.train_x = train_x.double()
        y = train_y.double().reshape(-1)
        self.train_y = y
        self.outputscale = float(outputscale)
        self.noise = float(noise)
        self.mean = float(y.mean()) if mean is None else float(mean)
        self._cache = None
        for p in (self.base_kernel.parameters() if hasattr(self.base_kernel, "parameters") else ()):     # fixed hyper-parameters: no gradient (and no device->host copy of one) in the acquisition path
            p.requires_grad_(False)

    def _train_cache(self):
        if self._cache is None:
            n = self.train_x.shape[-2]
            if self.train_x.is_cuda and 0 < n <= _l.GABO_GP_FACTOR_MAX_N:
                # the cache is the pair (L^-1, alpha); whatever the kernel returns goes to the launch (no guard against a batch of matrices)
                _device_cache(self, self.base_kernel, float(self.outputscale), float(self.noise), float(self.mean))
            else:
                with torch.no_grad():
                    k = self.outputscale * self.base_kernel.forward(self.train_x, self.train_x)
                    k = k + self.noise * torch.eye(k.shape[-1], dtype=k.dtype, device=k.device)
                    self._cache = _torch_cache(k, self.train_y, self.mean)
        return self._cache

    def posterior(self, X):
        """X: b x 1 x d  ->  (mean b, variance b)."""
        Linv, alpha = self._train_cache()
        _ops.check_deferred()
        mean, var = _marginal_posterior(lambda x1, x2: self.outputscale * self.base_kernel.forward(x1, x2), self.train_x, Linv, alpha, X)
        return self.mean + mean, var

    def forward(self, X):
        """`model(x_test)`: the joint posterior of the latent f (no observation noise) over the test set X (m x d_vec) as a
        MultivariateNormal - mean, covariance and samples from the device (ops.gp_posterior_joint, ops.mvn_sample).  No autograd."""
        Linv, alpha = self._train_cache()
        _ops.check_deferred()
        return _joint_posterior(self.base_kernel, self.outputscale, self.train_x, Linv, alpha, self.mean, X)

    def condition_on_observations(self, X, Y=None):
        """gpytorch's ExactGP.condition_on_observations / get_fantasy_model [3P] for prediction: a NEW model over the training set extended
        by X (t x d_vec, on the model's device) with targets Y (t), or - Y=None - the "Kriging believer" targets, the posterior mean at
        each new point given everything before it.  Its caches come from bordered O(n^2) updates of this model's (ops.gp_condition: no
        new factorisation, no host synchronisation); this model and its caches are untouched.  The kernel is shared, outputscale, noise
        and mean are kept (the mean is not re-estimated).  Chained calls give the bits of one call with the points stacked."""
        self._train_cache()
        holder = []
        tx, ty, linv, linv_t, alpha, kinv, factors = _condition_cache(self, self.base_kernel, self.outputscale, self.noise, self.mean, X, Y, holder)
        new = ExactGP(tx, ty, self.base_kernel, outputscale=self.outputscale, noise=self.noise, mean=self.mean)
        _install_caches(new, (linv, alpha), linv_t, kinv, factors)
        holder.append(new)
        return new


class ExpectedImprovement(torch.nn.Module):
    """botorch.acquisition.ExpectedImprovement(model, best_f, maximize) [3P]."""

    is_nonnegative = True

    def __init__(self, model, best_f, maximize=True):
        super().__init__()
        self.model = model
        self.best_f = float(best_f)
        self.maximize = maximize

    def forward(self, X):
        mean, var = self.model.posterior(X)
        sigma = var.clamp_min(1e-9).sqrt()
        u = (mean - self.best_f) / sigma
        if not self.maximize:
            u = -u
        pdf = torch.exp(-0.5 * u * u) / math.sqrt(2.0 * math.pi)
        cdf = 0.5 * (1.0 + torch.erf(u / math.sqrt(2.0)))
        return sigma * (pdf + u * cdf)


class PosteriorMean(torch.nn.Module):
    def __init__(self, model, maximize=True):
        super().__init__()
        self.model, self.maximize = model, maximize

    def forward(self, X):
        mean, _ = self.model.posterior(X)
        return mean if self.maximize else -mean


def is_nonnegative(acq_function):
    return bool(getattr(acq_function, "is_nonnegative", False))


def initialize_q_batch(X, Y, n, eta=1.0, generator=None):
    """botorch.optim.initializers.initialize_q_batch [3P]: Boltzmann sampling on standardised values, argmax forced in.
    `generator` (not in botorch): the random stream of the selection, so that every rank of a sharded sweep selects the same rows."""
    n_samples = X.shape[0]
    if n > n_samples:
        raise RuntimeError(f"n ({n}) cannot be larger than the number of provided samples ({n_samples})")
    if n == n_samples:
        return X
    Ystd = Y.std()
    if Ystd == 0:
        warnings.warn("All acquisition values for raw samples points are the same.", BadInitialCandidatesWarning)
        return X[torch.randperm(n=n_samples, device=X.device, generator=generator)][:n]
    max_val, max_idx = torch.max(Y, dim=0)
    Z = (Y - Y.mean()) / Ystd
    etaZ = eta * Z
    weights = torch.exp(etaZ)
    while torch.isinf(weights).any():
        etaZ *= 0.5
        weights = torch.exp(etaZ)
    idcs = torch.multinomial(weights, n, generator=generator)
    if max_idx not in idcs:
        idcs[-1] = max_idx
    return X[idcs]


def initialize_q_batch_nonneg(X, Y, n, eta=1.0, alpha=1e-4, generator=None):
    """botorch.optim.initializers.initialize_q_batch_nonneg [3P]; `generator` as in initialize_q_batch."""
    n_samples = X.shape[0]
    if n > n_samples:
        raise RuntimeError(f"n ({n}) cannot be larger than the number of provided samples ({n_samples})")
    if n == n_samples:
        return X
    max_val, max_idx = torch.max(Y, dim=0)
    if torch.any(max_val <= 0):
        warnings.warn("All acquisition values for raw sampled points are nonpositive, so initial conditions are being "
                      "selected randomly.", BadInitialCandidatesWarning)
        return X[torch.randperm(n=n_samples, device=X.device, generator=generator)][:n]
    pos = Y > 0
    num_pos = int(pos.sum().item())
    if num_pos < n:
        remaining = n - num_pos
        rand_idx = torch.randperm(n_samples - num_pos, device=Y.device, generator=generator)[:remaining]
        xpos, xneg = X[pos], X[~pos][rand_idx]
        return torch.cat([xpos, xneg], dim=0)[torch.randperm(n, device=X.device, generator=generator)]
    alpha_pos = Y >= alpha * max_val
    while alpha_pos.sum() < n:
        alpha = 0.1 * alpha
        alpha_pos = Y >= alpha * max_val
    alpha_pos_idcs = torch.arange(len(Y), device=Y.device)[alpha_pos]
    weights = torch.exp(eta * (Y[alpha_pos] / max_val - 1))
    idcs = alpha_pos_idcs[torch.multinomial(weights, n, generator=generator)]
    if max_idx not in idcs:
        idcs[-1] = max_idx
    return X[idcs]


def get_best_candidates(batch_candidates, batch_values):
    """botorch.generation.gen.get_best_candidates [3P]: argmax over restarts (ties -> lowest index)."""
    best = torch.argmax(batch_values.view(-1), dim=0)
    return batch_candidates[best]


# ---------------------------------------------------------------------------------------------- trainable surrogate
class GammaPrior:
    """Gamma(concentration, rate) log-density (gpytorch.priors.GammaPrior semantics) [3P]."""

    def __init__(self, concentration, rate):
        self.concentration, self.rate = float(concentration), float(rate)

    def log_prob(self, x):
        a, b = self.concentration, self.rate
        return a * math.log(b) + (a - 1.0) * torch.log(x) - b * x - math.lgamma(a)

    @property
    def mode(self):
        return max((self.concentration - 1.0) / self.rate, 0.0)


class _ExactMll(torch.autograd.Function):
    """log N(y | mean, outputscale * K + noise * I) for a base Gram matrix K on the device: forward and the whole gradient in one
    gabo_gp_mll_gram launch (d ll / d K = outputscale * W / 2 with W = alpha alpha^T - Ky^-1).  A Gram matrix that is not positive
    definite gives -inf (and zero gradients) instead of an exception: the fit's line searches then reject the point."""

    @staticmethod
    def forward(ctx, kbase, y, outputscale, noise, mean):
        from . import ops
        out, w = ops.gp_mll_gram(kbase.detach(), y.detach(), outputscale.item(), noise.item(), mean.item())
        ctx.save_for_backward(out, w)
        ctx.os = outputscale.item()
        ctx.host = [(t.device, t.dtype) for t in (outputscale, noise, mean)]
        return torch.where(out[5] > 0, torch.full_like(out[0], -math.inf), out[0])

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        out, w = ctx.saved_tensors
        ok = (out[5] == 0).to(out.dtype)
        scalars = (g * ok * out[2:5])
        gk = (g * ok * 0.5 * ctx.os) * w
        if any(dev_.type == "cpu" for dev_, _ in ctx.host):
            scalars = scalars.cpu()                       # one read-back for the three host-resident hyper-parameters
        return (gk, None) + tuple(scalars[i].to(dev_, dt_) for i, (dev_, dt_) in enumerate(ctx.host))


def _covar_layout(cm):
    """How a covariance module is read -> (kind, base kernel): "bare", a kernel on its own (the base is `cm`); "scaled", a ScaleKernel - the
    stand-in's or gpytorch's, told by its class name - with ONE outputscale around a base kernel; "other", any other wrapper of a base_kernel
    (batched outputscales, a foreign class), which the likelihood and the prediction evaluate as a whole and the fast fits do not take."""
    base = getattr(cm, "base_kernel", None)
    if base is None:
        return "bare", cm
    return ("scaled" if type(cm).__name__ == "ScaleKernel" and cm.raw_outputscale.numel() == 1 else "other"), base


def _outputscale_fn(cm, kind):
    """() -> the outputscale of a "scaled" or "bare" covariance module as a 0-d fp64 tensor"""
    if kind == "scaled":
        return lambda: cm.outputscale.double().reshape(())
    return lambda: torch.ones((), dtype=torch.float64)


def _plus_priors(ll, pri):
    """ll + log priors, which are a tensor on the parameters' device or - no prior at all - the float 0.0"""
    return ll + (pri.to(ll.device) if torch.is_tensor(pri) else pri)


class SingleTaskGP(torch.nn.Module):
    """Constant-mean exact GP with a Gaussian likelihood and trainable hyper-parameters, laid out like the models of the
    reference examples (examples/gabo_spd.py:165-176: ScaleKernel(base, outputscale_prior=Gamma(2, .15)), noise prior
    Gamma(1.1, .05), noise constraint GreaterThan(1e-8), initial noise = prior mode).  Priors registered on the kernels through
    the gpytorch-compatible `register_prior` are picked up when the stand-in Kernel base class is in use."""

    def __init__(self, train_x, train_y, covar_module, noise_prior=None, noise_lower_bound=1e-8, initial_noise=None):
        super().__init__()
        self.train_x = train_x.double()
        self.train_y = train_y.double().reshape(-1)
        self.covar_module = covar_module
        self.noise_prior = noise_prior
        self.noise_lower_bound = float(noise_lower_bound)
        if initial_noise is not None and initial_noise > noise_lower_bound:
            init_noise = float(initial_noise)
        else:
            init_noise = noise_prior.mode if noise_prior is not None and noise_prior.mode > noise_lower_bound else 1e-2
        self.raw_noise = torch.nn.Parameter(torch.tensor(math.log(math.expm1(init_noise - self.noise_lower_bound)), dtype=torch.float64))
        self.mean_constant = torch.nn.Parameter(torch.zeros((), dtype=torch.float64))
        self._cache = None

    @property
    def noise(self):
        return torch.nn.functional.softplus(self.raw_noise) + self.noise_lower_bound

    def _kxx(self):
        k = self.covar_module.forward(self.train_x, self.train_x)
        n = k.shape[-1]
        return k + self.noise.to(k.device) * torch.eye(n, dtype=k.dtype, device=k.device)

    def _priors(self):
        total = 0.0
        kind, base = _covar_layout(self.covar_module)
        for m in ([self.covar_module] if kind == "bare" else [self.covar_module, base]):
            for _, (prior, closure, _) in getattr(m, "_priors", {}).items():
                total = total + prior.log_prob(closure()).sum()
        if self.noise_prior is not None:
            total = total + self.noise_prior.log_prob(self.noise)
        return total

    def marginal_log_likelihood(self):
        """(log p(y | X) + log priors) / n, the quantity gpytorch's ExactMarginalLogLikelihood returns [3P].
        Up to GABO_GP_MLL_LARGE_MAX_N training points the likelihood and its gradient with respect to the Gram matrix, outputscale, noise
        and mean are ONE launch (gabo_gp_mll_gram) behind a custom autograd node, so autograd only has to differentiate the kernel
        itself (its own HIP backward); above that, torch's Cholesky / solve."""
        from . import _lib
        cm = self.covar_module
        kind, base = _covar_layout(cm)
        kb = (base if kind == "scaled" else cm).forward(self.train_x, self.train_x)
        if kb.is_cuda and kb.dim() == 2 and kb.shape[-1] <= _lib.GABO_GP_MLL_LARGE_MAX_N:
            os_ = _outputscale_fn(cm, kind)()
            ll = _ExactMll.apply(kb.double(), self.train_y.to(kb.device), os_, self.noise.reshape(()), self.mean_constant.reshape(()))
            return _plus_priors(ll, self._priors()) / kb.shape[-1]
        return self._marginal_log_likelihood_torch()

    def _marginal_log_likelihood_torch(self):
        """The same through torch.linalg (any size; the path the launch above is tested against)."""
        k = self._kxx()
        n = k.shape[-1]
        L = torch.linalg.cholesky(k)
        r = (self.train_y.to(k.device) - self.mean_constant.to(k.device)).unsqueeze(-1)
        alpha = torch.cholesky_solve(r, L)
        ll = -0.5 * (r * alpha).sum() - torch.log(torch.diagonal(L)).sum() - 0.5 * n * math.log(2 * math.pi)
        return _plus_priors(ll, self._priors()) / n

    def invalidate(self):
        self._cache = None

    def set_train_data(self, inputs=None, targets=None, strict=True):
        """gpytorch ExactGP.set_train_data [3P]: replace the training set between BO iterations (examples/gabo_spd.py:216; the
        hyper-parameters keep their current values and stay trainable for the next fit)"""
        if inputs is not None:
            if strict and tuple(inputs.shape) != tuple(self.train_x.shape):
                raise RuntimeError("Cannot modify shape of inputs (expected strict=False)")
            self.train_x = inputs.double()
        if targets is not None:
            if strict and targets.numel() != self.train_y.numel():
                raise RuntimeError("Cannot modify shape of targets (expected strict=False)")
            self.train_y = targets.double().reshape(-1)
        self.invalidate()

    # ---- fast surrogate fit: the distances (inner products) are evaluated once, each evaluation is one gabo_gp_mll (_series) launch ----
    def _stationary_form(self):
        """(E, theta_fn, outputscale_fn) when the covariance is [ScaleKernel of] one of the path's plain kernels, all of which
        are exp(-theta * E) with E = d^2 or d fixed during a fit; None for anything else (nested kernels carry extra
        parameters inside the distance, batched hyper-parameters, more than GABO_GP_MLL_LARGE_MAX_N points)."""
        from . import _lib
        from .kernel_utils import kernel_parameters
        kind, base = _covar_layout(self.covar_module)
        if kind == "other":
            return None
        os_fn = _outputscale_fn(self.covar_module, kind)
        x = self.train_x
        if x.dim() != 2 or not 1 <= x.shape[0] <= _lib.GABO_GP_MLL_LARGE_MAX_N:
            return None
        try:                                               # (the table of the plain kernels and their exponents is stated there, once)
            theta_of = kernel_parameters.parameter_map(base)
        except TypeError:
            return None
        if theta_of.parameter == "beta":
            theta_fn = lambda: theta_of(base.beta.double().reshape(()))                        # noqa: E731
        else:
            theta_fn = lambda: theta_of(base.lengthscale.double().reshape(()))                 # noqa: E731
        if theta_fn().numel() != 1:
            return None
        e = kernel_parameters.exponent_matrix(base, x)[0]
        return e, theta_fn, os_fn

    def _series_form(self):
        """(C, kappa -> (p, dp / dkappa, series_dim), outputscale_fn) when the covariance is [ScaleKernel of] SphereRiemannianMaternKernel:
        a zonal series of the inner products C = X X^T, which are fixed during a fit while the coefficients move with the lengthscale kappa
        (ops.gp_mll_series); None for anything else, a batched lengthscale or more than GABO_GP_MLL_LARGE_MAX_N points.  C is the product
        the differentiable route of ops.sphere_matern_kernel forms, so the value agrees with marginal_log_likelihood() to rounding."""
        from . import _lib, ops
        from .kernel_utils.kernels_sphere import SphereRiemannianMaternKernel
        kind, base = _covar_layout(self.covar_module)
        if kind == "other":
            return None
        os_fn = _outputscale_fn(self.covar_module, kind)
        x = self.train_x
        if type(base) is not SphereRiemannianMaternKernel or x.dim() != 2 or not 1 <= x.shape[0] <= _lib.GABO_GP_MLL_LARGE_MAX_N:
            return None
        if base.raw_lengthscale.numel() != 1:
            return None
        with torch.no_grad():
            xd = x.double().to(ops._device_for(x))
            c = (xd @ xd.transpose(-1, -2)).contiguous()
        dim, nu, levels = x.shape[-1], base.nu, base.num_levels
        return c, (lambda kappa: ops.sphere_matern_coefficients_and_derivative(dim, kappa, nu, levels)), os_fn

    def _matern_form(self):
        """(R, lengthscale_fn, nu, outputscale_fn) when the covariance is [ScaleKernel of] SpdLogEuclideanMaternKernel / SpdFrobeniusMaternKernel:
        a Matern function of the distance matrix R of the training features, which is fixed during a fit while the lengthscale moves
        (ops.gp_mll_matern); None for anything else, a batched lengthscale or more than GABO_GP_MLL_LARGE_MAX_N points.  R is what the
        GABO_OUT_DISTANCE launch writes on the features the kernel's forward forms."""
        from . import _lib, ops
        from .kernel_utils import kernels_spd as _ks
        kind, base = _covar_layout(self.covar_module)
        if kind == "other":
            return None
        os_fn = _outputscale_fn(self.covar_module, kind)
        x = self.train_x
        if type(base) not in (_ks.SpdLogEuclideanMaternKernel, _ks.SpdFrobeniusMaternKernel) or x.dim() != 2 \
                or not 1 <= x.shape[0] <= _lib.GABO_GP_MLL_LARGE_MAX_N:
            return None
        if base.raw_lengthscale.numel() != 1:
            return None
        with torch.no_grad():
            xd = x.double().to(ops._device_for(x))
            feat = ops.spd_logm_mandel(xd) if type(base) is _ks.SpdLogEuclideanMaternKernel else xd
            r = ops.frobenius_pairwise(feat, feat, 1.0, _lib.GABO_OUT_DISTANCE).contiguous()
        return r, (lambda: base.lengthscale.double().reshape(())), base.nu, os_fn

    def _spectral_form(self):
        """(A, base draw, lengthscale_fn, nu, outputscale_fn) when the covariance is [ScaleKernel of] SpdAffineInvariantMaternKernel: random
        phase features of the log-diagonals A = ops.spd_ai_logdiag of the training points, which are fixed during a fit while the spectral
        points and weights move with the lengthscale (ops.gp_mll_spd_ai_spectral); None for anything else, a batched lengthscale, dim > 10 or
        more than GABO_GP_MLL_LARGE_MAX_N points.  A comes from the kernel's own _logdiag: the one launch per point set stays one."""
        from . import _lib, ops
        from .kernel_utils.kernels_spd import SpdAffineInvariantMaternKernel
        kind, base = _covar_layout(self.covar_module)
        if kind == "other":
            return None
        os_fn = _outputscale_fn(self.covar_module, kind)
        x = self.train_x
        if type(base) is not SpdAffineInvariantMaternKernel or x.dim() != 2 or not 1 <= x.shape[0] <= _lib.GABO_GP_MLL_LARGE_MAX_N:
            return None
        if base.raw_lengthscale.numel() != 1 or base.dim > 10 or x.shape[-1] != base.dim * (base.dim + 1) // 2:
            return None
        with torch.no_grad():
            dev = ops._device_for(x)
            a = base._logdiag(x, base._phases_on(dev)).to(dev).contiguous()
        return a, base.spectral_base, (lambda: base.lengthscale.double().reshape(())), base.nu, os_fn

    def _fast_evaluator(self):
        """(launch(parameter, outputscale, noise, mean) -> the six numbers of ops.gp_mll, parameter_fn, outputscale_fn, series?) on the matrix
        that is fixed during a fit: the exponent matrix of a plain kernel (parameter theta), else the inner products of the sphere Matern
        kernel, the distances of a flat SPD Matern kernel or the log-diagonals of the affine-invariant SPD Matern kernel (parameter: the
        lengthscale itself, `series`); None when the model has none of the four forms."""
        from . import ops
        form = self._stationary_form()
        if form is not None:
            e, theta_fn, os_fn = form
            y = self.train_y.to(e.device).contiguous()
            return (lambda theta, os_, noise, mean: ops.gp_mll(e, y, theta, os_, noise, mean)), theta_fn, os_fn, False
        form = self._series_form()
        if form is not None:
            c, coeff_fn, os_fn = form
            y = self.train_y.to(c.device).contiguous()
            base = _covar_layout(self.covar_module)[1]
            kappa_fn = lambda: base.lengthscale.double().reshape(())                               # noqa: E731
            return (lambda kappa, os_, noise, mean: ops.gp_mll_series(c, y, *coeff_fn(kappa), os_, noise, mean)), kappa_fn, os_fn, True
        form = self._matern_form()
        if form is not None:
            r, ls_fn, nu, os_fn = form
            y = self.train_y.to(r.device).contiguous()
            return (lambda ls, os_, noise, mean: ops.gp_mll_matern(r, y, ls, nu, os_, noise, mean)), ls_fn, os_fn, True
        form = self._spectral_form()
        if form is not None:
            a, draw, ls_fn, nu, os_fn = form
            y = self.train_y.to(a.device).contiguous()
            return (lambda ls, os_, noise, mean: ops.gp_mll_spd_ai_spectral(a, y, draw, ls, nu, os_, noise, mean)), ls_fn, os_fn, True
        return None

    def _fast_mll_closure(self):
        """() -> (value, backward_fn) evaluating `marginal_log_likelihood` and the gradients of all parameters with one
        gabo_gp_mll launch: the device returns d ll / d (theta, outputscale, noise, mean); the chain rule through the parameter
        transforms and the priors is a handful of scalar torch operations on the parameters' own device."""
        form = self._fast_evaluator()
        if form is None:
            return None
        launch, theta_fn, os_fn, _ = form
        n = self.train_y.numel()

        def evaluate():
            theta, os_, noise, mean = theta_fn(), os_fn(), self.noise, self.mean_constant
            ll, g_theta, g_os, g_noise, g_mean, bad = launch(theta.item(), os_.item(), noise.item(), mean.item())
            if bad:
                raise torch.linalg.LinAlgError("K + noise I is not positive definite")
            pri = self._priors()
            value = (ll + (pri.item() if torch.is_tensor(pri) else pri)) / n
            # a linear stand-in with the same first derivatives as ll at this point, so that autograd does the chain rule
            proxy = _plus_priors(g_theta * theta + g_os * os_.to(theta.device) + g_noise * noise.to(theta.device) + g_mean * mean.to(theta.device), pri) / n
            return value, proxy

        return evaluate

    def _fast_scalar_objective(self, params, evaluator=None, evaluator_takes_value=False):
        """v -> (loss, gradient) in plain Python floats for the layout every reference example uses (stand-in ScaleKernel / kernel
        classes with softplus constraints, Gamma priors): the chain rule through softplus and the priors costs microseconds, so an
        L-BFGS evaluation is the gabo_gp_mll launch and its 48-byte read-back.  None when the model is laid out differently (the
        caller then lets autograd do the chain rule).
        evaluator(theta, outputscale, noise, mean) -> (ll, d theta, d outputscale, d noise, d mean, not_pd): replaces the launch on the
        fixed distance matrix for kernels with further parameters inside the distance (the nested kernels: manifold_gp_fit.py); `params`
        then lists the SCALAR hyper-parameters only.  evaluator_takes_value: that evaluator takes the constrained lengthscale kappa itself in
        the place of theta = l^-2 and returns d / d kappa (a series kernel, as the built-in series evaluator)."""
        import numpy as np

        from . import _compat
        if _compat.HAVE_GPYTORCH:
            return None
        series = bool(evaluator_takes_value) and evaluator is not None
        if evaluator is None:
            form = self._fast_evaluator()
            if form is None:
                return None
            evaluator, series = form[0], form[3]
        cm = self.covar_module
        base = _covar_layout(cm)[1]
        index = {id(p): i for i, p in enumerate(params)}
        plan = {}                      # hyper-parameter -> (position in v, fp32?, lower bound)

        def softplus_param(name, module, raw_name):
            raw = getattr(module, raw_name)
            con = getattr(module, raw_name + "_constraint", None)
            if type(con) not in (_compat.GreaterThan, _compat.Positive) or raw.numel() != 1 or id(raw) not in index:
                return False
            plan[name] = (index[id(raw)], raw.dtype == torch.float32, float(con.lower_bound))
            return True

        uses_beta = hasattr(base, "raw_beta")
        if not softplus_param("theta", base, "raw_beta" if uses_beta else "raw_lengthscale"):
            return None
        if base is not cm and not softplus_param("os", cm, "raw_outputscale"):
            return None
        if id(self.raw_noise) not in index or id(self.mean_constant) not in index:
            return None
        plan["noise"] = (index[id(self.raw_noise)], False, self.noise_lower_bound)
        i_mean = index[id(self.mean_constant)]
        if len(plan) + 1 != len(params):
            return None
        priors = []                    # (hyper-parameter the prior is on, concentration, rate)
        on_base = {"beta_prior": "theta", "lengthscale_prior": "theta"}      # (a lengthscale prior is on l, the constrained value)
        for module, allowed in ([(cm, on_base)] if base is cm else [(cm, {"outputscale_prior": "os"}), (base, on_base)]):
            for name, (prior, _, _) in getattr(module, "_priors", {}).items():
                if name not in allowed or type(prior) is not GammaPrior:
                    return None
                priors.append((allowed[name], prior.concentration, prior.rate))
        if self.noise_prior is not None:
            if type(self.noise_prior) is not GammaPrior:
                return None
            priors.append(("noise", self.noise_prior.concentration, self.noise_prior.rate))
        n = self.train_y.numel()

        def objective(v):
            val, dval = {}, {}
            for name, (i, is32, lb) in plan.items():
                raw = float(np.float32(v[i])) if is32 else float(v[i])
                val[name] = lb + max(raw, 0.0) + math.log1p(math.exp(-abs(raw)))           # softplus
                dval[name] = 1.0 / (1.0 + math.exp(-raw)) if raw >= 0 else math.exp(raw) / (1.0 + math.exp(raw))
            positive = val["theta"]                       # beta, the lengthscale kappa of a series, or the lengthscale l with theta = l^-2
            theta, dtheta = (positive, 1.0) if uses_beta or series else (positive ** -2, -2.0 * positive ** -3)
            ll, g_theta, g_os, g_noise, g_mean, bad = evaluator(theta, val.get("os", 1.0), val["noise"], float(v[i_mean]))
            grad = np.zeros_like(v)
            if bad:
                return 1e10, grad
            d_positive = {"theta": g_theta * dtheta, "os": g_os, "noise": g_noise}       # d total / d (constrained value)
            total = ll
            for name, a, b in priors:
                x = val[name]
                total += a * math.log(b) + (a - 1.0) * math.log(x) - b * x - math.lgamma(a)
                d_positive[name] += (a - 1.0) / x - b
            for name, (i, _, _) in plan.items():
                grad[i] = -d_positive[name] * dval[name] / n
            grad[i_mean] = -g_mean / n
            return -total / n, grad

        return objective

    def _ensure_cache(self):
        """(L^-1, alpha, mean) of the fitted model; freezes the kernel hyper-parameters (prediction mode)."""
        from . import _compat
        cm, n = self.covar_module, self.train_x.shape[-2]
        # the one-launch route only for the stand-in ScaleKernel(base), by its class and without gpytorch: a bare kernel, too, goes to torch
        if self._cache is None and self.train_x.is_cuda and 0 < n <= _l.GABO_GP_FACTOR_MAX_N and type(cm) is _compat.ScaleKernel \
                and not _compat.HAVE_GPYTORCH:
            mu = self.mean_constant.detach().to(self.train_x.device)
            # the cache is the triple (L^-1, alpha, mu); a batch of Gram matrices leaves it empty, for torch to fill
            _device_cache(self, cm.base_kernel, float(cm.outputscale.detach()), float(self.noise.detach()), float(mu), (mu,), matrix_only=True)
        if self._cache is None:
            with torch.no_grad():
                ky = self._kxx()
                mu = self.mean_constant.detach().to(ky.device)
                self._cache = _torch_cache(ky, self.train_y, mu) + (mu,)
        for p in self.covar_module.parameters():                    # on every call, not only when the cache is built
            p.requires_grad_(False)
        return self._cache

    def posterior(self, X):
        Linv, alpha, mu = self._ensure_cache()
        _ops.check_deferred()
        mean, var = _marginal_posterior(self.covar_module.forward, self.train_x, Linv, alpha, X)
        return mu.to(mean.device) + mean, var

    def forward(self, X):
        """`preds = model(x_test)` of the reference's GP-regression demos (examples/kernels/spd/spd_kernels.py:168): the joint posterior of
        the latent f (no observation noise) over the test set X (m x d_vec) as a MultivariateNormal.  The kernel matrices come from the
        covariance module's own launches (any kernel of the library), the rest from ops.gp_posterior_joint.  Freezes the hyper-parameters
        like posterior(); no autograd through the prediction."""
        Linv, alpha, mu = self._ensure_cache()
        _ops.check_deferred()
        base, outputscale = self._base_and_outputscale()
        return _joint_posterior(base, outputscale, self.train_x, Linv, alpha, float(mu), X)

    def _base_and_outputscale(self):
        kind, base = _covar_layout(self.covar_module)
        return (base, float(self.covar_module.outputscale.detach())) if kind == "scaled" else (self.covar_module, 1.0)

    def condition_on_observations(self, X, Y=None):
        """As ExactGP.condition_on_observations: a new SingleTaskGP for prediction over the training set extended by X (t x d_vec) with
        targets Y, or the believer's (Y=None); the covariance module, the noise and the mean constant are the same objects, frozen at their
        current values as posterior() freezes them.  The kernel strips come from the covariance module's own launches: any kernel of the
        library, nested ones included."""
        _, _, mu = self._ensure_cache()
        base, outputscale = self._base_and_outputscale()
        holder = []
        tx, ty, linv, linv_t, alpha, kinv, factors = _condition_cache(self, base, outputscale, float(self.noise.detach()),
                                                                      float(self.mean_constant.detach()), X, Y, holder)
        new = SingleTaskGP(tx, ty, self.covar_module, noise_prior=self.noise_prior, noise_lower_bound=self.noise_lower_bound)
        new.raw_noise, new.mean_constant = self.raw_noise, self.mean_constant
        _install_caches(new, (linv, alpha, mu), linv_t, kinv, factors)
        holder.append(new)
        return new


def fit_gpytorch_model(model, maxiter=200, fast=True):
    """Maximise the marginal log likelihood (+ priors) over every trainable parameter with scipy L-BFGS-B, as
    botorch.fit_gpytorch_model does for the reference examples (examples/gabo_spd.py:194) [3P].
    fast=True: for the plain kernels of the path the pairwise distances are evaluated once and every L-BFGS evaluation is a single
    gabo_gp_mll launch (value + analytic gradient) instead of a kernel launch, a Cholesky and their autograd; fast=False (and any
    other model) differentiates `marginal_log_likelihood` with autograd."""
    import numpy as np
    from scipy.optimize import minimize
    params = [p for p in model.parameters()]
    for p in params:
        p.requires_grad_(True)
    shapes = [p.shape for p in params]
    sizes = [p.numel() for p in params]

    def set_params(v):
        off = 0
        with torch.no_grad():
            for p, sh, sz in zip(params, shapes, sizes):
                p.copy_(torch.as_tensor(v[off:off + sz], dtype=p.dtype).reshape(sh))
                off += sz

    scalar = model._fast_scalar_objective(params) if fast and hasattr(model, "_fast_scalar_objective") else None
    fast = model._fast_mll_closure() if fast and scalar is None and hasattr(model, "_fast_mll_closure") else None

    def fun(v):
        if scalar is not None:
            return scalar(v)
        set_params(v)
        for p in params:
            p.grad = None
        try:
            if fast is not None:
                value, proxy = fast()
                (-proxy).backward()
                loss = torch.tensor(-value)
            else:
                loss = -model.marginal_log_likelihood()
                loss.backward()
        except torch.linalg.LinAlgError:      # a trial point outside the SPD cone of K + noise I (torch.linalg.cholesky); any other
            return 1e10, np.zeros_like(v)      # error - a failed launch, a non-SPD kernel INPUT - is a real failure and propagates
        g = np.concatenate([(p.grad if p.grad is not None else torch.zeros_like(p)).detach().cpu().double().reshape(-1).numpy()
                            for p in params])
        value = float(loss.item())
        if not math.isfinite(value):  # (the one-launch likelihood reports a matrix that is not positive definite as -inf)
            return 1e10, np.zeros_like(v)
        return value, g

    x0 = np.concatenate([p.detach().cpu().double().reshape(-1).numpy() for p in params])
    res = minimize(fun, x0, jac=True, method="L-BFGS-B", options={"maxiter": maxiter})
    set_params(res.x)
    model.invalidate()
    return model
