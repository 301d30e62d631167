#!/usr/bin/env python3
"""Gaussian-process regression on the sphere S^2 with the two geometry-aware kernels on the MI355X - the flow of the reference's
examples/kernels/sphere/sphere_kernels.py:76-189 without the plots: the test function is a Gaussian on the tangent space of a point of the
sphere, 20 training points are drawn "far" from it and 10 test points around it (the reference's draws: numpy's global stream, seed 1234);
per kernel (sphere Gaussian, sphere Laplace) the surrogate is fitted and `preds = model(x_test)` gives mean, variance and covariance of the
joint posterior.  (The reference's third model, a Euclidean RBF kernel of gpytorch, is not a kernel of this library.)

    python examples/sphere_kernels.py
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gabotorch_amd import models                                                                       # noqa: E402
from gabotorch_amd._compat import ScaleKernel                                                          # noqa: E402
from gabotorch_amd.Riemannian_utils.sphere_utils import logmap                                         # noqa: E402
from gabotorch_amd.kernel_utils.kernels_sphere import SphereGaussianKernel, SphereLaplaceKernel        # noqa: E402

DIM = 3
SIGMA = np.array([[0.6, 0.2, 0], [0.2, 0.3, -0.01], [0, -0.01, 0.2]])


def test_function(x, mu):
    """sphere_kernels.py:34-42 for every row of x (N, dim) -> (N,)"""
    proj = np.concatenate([logmap(p, mu) for p in x], axis=1)      # (dim, N)
    q = np.einsum("in,ij,jn->n", proj, np.linalg.inv(SIGMA), proj)
    return np.exp(-0.5 * q) / np.sqrt((2 * np.pi) ** DIM * np.linalg.det(SIGMA))


def data(seed=1234):
    np.random.seed(seed)
    mu = np.array([1 / np.sqrt(2), 1 / np.sqrt(2), 0])
    train = np.random.multivariate_normal(np.array([1.0, 0.0, 0.0]), 0.1 * np.eye(DIM), 20)             # :83-92
    train /= np.linalg.norm(train, axis=1)[:, None]
    test = np.random.multivariate_normal(mu, 0.1 * np.eye(DIM), 10)                                     # :99-109
    test /= np.linalg.norm(test, axis=1)[:, None]
    return mu, train, test_function(train, mu), test, test_function(test, mu)


def run(seed=1234, verbose=True, device="cuda:0"):
    mu, x_train, y_train, x_test, y_test = data(seed)
    xt, yt, xs = torch.tensor(x_train, device=device), torch.tensor(y_train, device=device), torch.tensor(x_test, device=device)
    results = {}
    for title, make in (("Manifold-RBF kernel", lambda: SphereGaussianKernel(beta_min=6.5)), ("Laplace kernel", SphereLaplaceKernel)):
        covar = ScaleKernel(make(), outputscale_prior=models.GammaPrior(2.0, 0.15))                     # :128-129
        model = models.SingleTaskGP(xt, yt, covar, noise_prior=models.GammaPrior(1.1, 0.05))            # :131-137
        models.fit_gpytorch_model(model)                                                               # :141
        preds = model(xs)                                                                              # :147
        mean, var, cov = preds.mean.cpu().numpy(), preds.variance.cpu().numpy(), preds.covariance_matrix.cpu().numpy()
        rmse = float(np.sqrt(np.sum((y_test - mean) ** 2) / len(y_test)))                               # :153
        results[title] = dict(mean=mean, variance=var, covariance=cov, rmse=rmse)
        if verbose:
            print(f"Estimation error ({title}) = {rmse:.6f}, variance in [{var.min():.3e}, {var.max():.3e}]")
    return results


if __name__ == "__main__":
    run()
