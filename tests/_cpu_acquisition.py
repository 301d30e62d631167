"""CPU fp64 statement of what the fused acquisition evaluators compute (csrc/spd_acq_body.hpp, csrc/sphere_tr.hip, csrc/gp_acquisition.hip):
kernel strip -> exact-GP posterior -> EI / posterior mean -> gradient back to the candidate.  Test infrastructure only.

Nothing here comes from a device or from gabotorch_amd.ops:
  * the strip k(x, X_j) and the Gram matrix K(X, X) are the oracle's (oracle/spd.py, oracle/sphere.py);
  * the acquisition as a function of the strip is written in CPU torch fp64, the posterior by a dense solve on outputscale K + noise I built
    from scratch, EI as oracle/gp.py states it (sigma = sqrt(clamp_min(var, 1e-9)), Phi = (1 + erf(u / sqrt 2)) / 2); torch.autograd gives d acq / d k_j;
  * the gradient back to the candidate is the oracle's closed-form kernel gradient with grad_k = d acq / d k (these handle repeated eigenvalues by
    divided differences, which autograd through eigh does not).
"""
import math

import numpy as np
import torch

from oracle import spd as ospd
from oracle import sphere as osph

# (family, kernel) -> strip and closed-form gradient of the oracle.  For the lengthscale-parametrised kernels beta = 1 / lengthscale^2.
SPD_KERNELS = ("ai_gaussian", "ai_laplace", "le_gaussian", "frob_gaussian")
SPHERE_KERNELS = ("sphere_gaussian", "sphere_laplace")


def rand_spd_mandel(rng, n, d, lo=0.5, hi=2.0):
    """n SPD matrices with eigenvalues uniform in [lo, hi] and random orthogonal frames, as Mandel vectors."""
    q = np.linalg.qr(rng.standard_normal((n, d, d)))[0]
    m = np.einsum("nab,nb,ncb->nac", q, rng.uniform(lo, hi, (n, d)), q)
    return ospd.symmetric_matrix_to_vector_mandel(0.5 * (m + m.transpose(0, 2, 1)))


def rand_sphere(rng, n, dim):
    x = rng.standard_normal((n, dim))
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def strip(kernel, x, train, beta):
    """k(x_i, X_j): (R, n) numpy fp64."""
    ls = 1.0 / math.sqrt(beta)
    if kernel == "ai_gaussian":
        return ospd.spd_ai_gaussian_kernel(x, train, beta)
    if kernel == "ai_laplace":
        return ospd.spd_ai_laplace_kernel(x, train, beta)
    if kernel == "le_gaussian":
        return ospd.log_euclidean_gaussian_kernel(x, train, ls)
    if kernel == "frob_gaussian":
        return ospd.frobenius_gaussian_kernel(x, train, ls)
    if kernel == "sphere_gaussian":
        return osph.sphere_gaussian_kernel(x, train, beta)
    if kernel == "sphere_laplace":
        return osph.sphere_laplace_kernel(x, train, beta)
    raise ValueError(kernel)


def strip_backward(kernel, x, train, beta, grad_k):
    """d/dx of sum(grad_k * strip): (R, d_vec) Mandel for the SPD kernels, (R, dim) Euclidean for the sphere."""
    ls = 1.0 / math.sqrt(beta)
    fn, scale = {"ai_gaussian": (ospd.spd_ai_gaussian_kernel_grads, beta), "ai_laplace": (ospd.spd_ai_laplace_kernel_grads, beta),
                 "le_gaussian": (ospd.log_euclidean_gaussian_kernel_grads, ls), "frob_gaussian": (ospd.frobenius_gaussian_kernel_grads, ls),
                 "sphere_gaussian": (osph.sphere_gaussian_kernel_grads, beta), "sphere_laplace": (osph.sphere_laplace_kernel_grads, beta)}[kernel]
    return fn(x, train, scale, grad_k)[0]


def kxx(kernel, beta):
    """k(x, x) as the reference's distance functions give it at coincident arguments: d_AI^2 = 1e-15 (spd_utils_torch.py:120), the Frobenius-type
    distances ||0 + 1e-15||_F^2 = d^2 1e-30 (:156: k = 1 to the last bit), <x, x> clamped to 1 - 1e-15 on the sphere (sphere_utils_torch.py:53)."""
    if kernel == "ai_gaussian":
        return math.exp(-beta * 1e-15)
    if kernel == "ai_laplace":
        return math.exp(-beta * math.sqrt(1e-15))
    if kernel in ("le_gaussian", "frob_gaussian"):
        return 1.0
    t0 = math.acos(1.0 - 1e-15)
    return math.exp(-beta * (t0 * t0 if kernel == "sphere_gaussian" else t0))


def acquisition_of_strip(ks, gram, y, mean, outputscale, noise, k_xx, best_f, kind, maximize, solver="solve", of="value"):
    """Acquisition as a function of the strip ks (R, n) of BASE kernel values; gram (n, n) BASE kernel matrix of the training set.
    kind: "ei" or "mean".  -> dict of numpy arrays: value (R,), grad_k (R, n) = d value_i / d ks_ij, mu, var (unclamped), sigma, u.
    solver: "solve" (dense LU, the statement of oracle/gp.py) or "cholesky" (used to measure the reference's own fp64 spread).
    of: the output that grad_k differentiates ("value"; "u", "sigma", "mu" serve the error bounds of the EI-tail tests)."""
    k = torch.tensor(np.asarray(ks, dtype=np.float64), requires_grad=True)
    n = k.shape[1]
    ky = outputscale * torch.tensor(np.asarray(gram, dtype=np.float64)) + noise * torch.eye(n, dtype=torch.float64)
    resid = (torch.tensor(np.asarray(y, dtype=np.float64)) - mean).unsqueeze(-1)
    kso = outputscale * k
    if solver == "solve":
        alpha = torch.linalg.solve(ky, resid)
        sol = torch.linalg.solve(ky, kso.t())
    else:
        chol = torch.linalg.cholesky(ky)
        alpha = torch.cholesky_solve(resid, chol)
        sol = torch.cholesky_solve(kso.t(), chol)
    mu = mean + (kso @ alpha).squeeze(-1)
    var = outputscale * k_xx - (kso * sol.t()).sum(-1)
    sigma = var.clamp_min(1e-9).sqrt()
    u = (mu - best_f) / sigma
    if not maximize:
        u = -u
    if kind == "mean":
        value = mu if maximize else -mu
    else:
        pdf = torch.exp(-0.5 * u * u) / math.sqrt(2.0 * math.pi)
        cdf = 0.5 * (1.0 + torch.erf(u / math.sqrt(2.0)))
        value = sigma * (pdf + u * cdf)
    out = dict(value=value, mu=mu, var=var, sigma=sigma, u=u)
    (out["grad_k"],) = torch.autograd.grad(out[of].sum(), k)
    return {name: v.detach().numpy() for name, v in out.items()}


def acquisition(kernel, x, train, y, beta, mean, outputscale, noise, best_f, kind, maximize, solver="solve", gram=None, of="value"):
    """Value and gradient with respect to the candidates x of the acquisition of an exact GP on `train` with the named kernel.
    -> the dict of acquisition_of_strip plus `grad` (R, d_vec Mandel | dim) and `ks`."""
    ks = strip(kernel, x, train, beta)
    if gram is None:
        gram = strip(kernel, train, train, beta)
    out = acquisition_of_strip(ks, gram, y, mean, outputscale, noise, kxx(kernel, beta), best_f, kind, maximize, solver, of)
    out["ks"] = ks
    out["grad"] = strip_backward(kernel, x, train, beta, out["grad_k"])
    return out
