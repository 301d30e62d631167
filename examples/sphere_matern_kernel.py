#!/usr/bin/env python3
"""Gaussian-process regression on the sphere S^2 with the Riemannian Matern and heat kernels (Borovitskiy et al., NeurIPS 2020) on the
MI355X: the demo of examples/sphere_kernels.py - same test function, same 20 training and 10 test points - with
SphereRiemannianMaternKernel at nu = 2.5 and nu = inf, followed by a table of the smallest eigenvalue of the Gram matrix of 96 points of
S^2 by lengthscale, beside SphereGaussianKernel by beta on the same points: the series kernels are positive definite for every lengthscale
(their eigenvalues stay at rounding level), the geodesic Gaussian kernel only above its beta_min.

    python examples/sphere_matern_kernel.py
"""
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from examples.sphere_kernels import data                                                               # noqa: E402
from gabotorch_amd import models                                                                       # noqa: E402
from gabotorch_amd._compat import ScaleKernel                                                          # noqa: E402
from gabotorch_amd.kernel_utils.kernels_sphere import SphereGaussianKernel, SphereRiemannianMaternKernel       # noqa: E402


def regression(seed=1234, verbose=True, device="cuda:0"):
    _, x_train, y_train, x_test, y_test = data(seed)
    xt, yt, xs = torch.tensor(x_train, device=device), torch.tensor(y_train, device=device), torch.tensor(x_test, device=device)
    results = {}
    for title, nu in (("Riemannian Matern 5/2 kernel", 2.5), ("heat kernel", math.inf)):
        base = SphereRiemannianMaternKernel(nu=nu, num_levels=32)
        covar = ScaleKernel(base, outputscale_prior=models.GammaPrior(2.0, 0.15))
        model = models.SingleTaskGP(xt, yt, covar, noise_prior=models.GammaPrior(1.1, 0.05))
        models.fit_gpytorch_model(model)          # (autograd through the kernel: value and lengthscale derivative are series launches)
        preds = model(xs)
        mean, var, cov = preds.mean.cpu().numpy(), preds.variance.cpu().numpy(), preds.covariance_matrix.cpu().numpy()
        rmse = float(np.sqrt(np.sum((y_test - mean) ** 2) / len(y_test)))
        results[title] = dict(mean=mean, variance=var, covariance=cov, rmse=rmse, lengthscale=float(base.lengthscale.detach()))
        if verbose:
            print(f"Estimation error ({title}) = {rmse:.6f}, lengthscale {results[title]['lengthscale']:.4f}, "
                  f"variance in [{var.min():.3e}, {var.max():.3e}]")
    return results


def smallest_eigenvalues(n=96, seed=1234, verbose=True, device="cuda:0"):
    """lambda_min of the n x n Gram matrix: rows (kernel, parameter, lambda_min)"""
    x = np.random.default_rng(seed).standard_normal((n, 3))
    x = torch.tensor(x / np.linalg.norm(x, axis=1, keepdims=True), device=device)
    rows = []
    with torch.no_grad():
        for nu in (2.5, math.inf):
            k = SphereRiemannianMaternKernel(nu=nu, num_levels=32).double()
            for ls in (0.05, 0.3, 1.0, 3.0):
                k.lengthscale = torch.tensor(ls, dtype=torch.float64)
                rows.append((f"Matern nu = {nu}", f"lengthscale {ls}", float(torch.linalg.eigvalsh(k.forward(x, x)).min())))
        g = SphereGaussianKernel(beta_min=0.05).double()
        for beta in (0.1, 0.5, 2.0, 6.5):
            g.beta = torch.tensor(beta, dtype=torch.float64)
            rows.append(("geodesic Gaussian", f"beta {beta}", float(torch.linalg.eigvalsh(g.forward(x, x).double()).min())))
    if verbose:
        print(f"smallest eigenvalue of the Gram matrix of {n} points on S^2")
        for name, par, lam in rows:
            print(f"  {name:20s} {par:18s} {lam: .3e}")
    return rows


if __name__ == "__main__":
    regression()
    smallest_eigenvalues()
