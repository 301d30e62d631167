#!/usr/bin/env python3
"""Gaussian-process regression on the SPD manifold with the Riemannian Matern / heat kernel of the AFFINE-INVARIANT metric on the MI355X: the
flow of examples/spd_matern_kernel.py (the C-shaped trajectory of the 2D-letters data as 2 x 2 SPD matrices, time as the target, a part of the
trajectory left out of the training set) with SpdAffineInvariantMaternKernel.  The kernel has no closed form; it is evaluated through random
phase features (one small Cholesky factorisation per point and feature, on the device), a Monte-Carlo approximation with error
O(1 / sqrt(num_features)) that is positive semi-definite for EVERY lengthscale.  `fit_gpytorch_model` takes the one-call route for this kernel
without any change here (SingleTaskGP._spectral_form: the log-diagonals once, then one gabo_gp_mll_spd_ai_spectral call per L-BFGS
evaluation; fast=False keeps autograd), and `model(x_test)` gives the joint posterior over the whole trajectory.

The second part is a table of the smallest eigenvalue of the Gram matrix by lengthscale, beside SpdAffineInvariantGaussianKernel by beta: the
Gaussian kernel of the same metric is positive definite only from some beta upwards (its `beta_min`), the Matern family has no such range.

    python examples/spd_ai_matern_kernel.py [--nu 2.5] [--features 1024] [--samples 10]
"""
import argparse
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gabotorch_amd import models                                                                                  # noqa: E402
from gabotorch_amd._compat import ScaleKernel                                                                     # noqa: E402
from gabotorch_amd.kernel_utils.kernels_spd import SpdAffineInvariantGaussianKernel, SpdAffineInvariantMaternKernel   # noqa: E402

LENGTHSCALES = (0.05, 0.1, 0.3, 1.0, 3.0, 10.0)
BETAS = (0.05, 0.1, 0.3, 1.0, 3.0, 10.0)


def load():
    g = np.load(os.path.join(ROOT, "tests", "golden", "letters_gp.npz"))
    return {k: g[k] for k in g.files}


def min_eigenvalue_table(x, nu, num_features, seed):
    """-> {"matern": [(lengthscale, lambda_min)], "gaussian": [(beta, lambda_min)]} of the Gram matrices of the points x"""
    matern = SpdAffineInvariantMaternKernel(2, nu=nu, num_features=num_features, seed=seed).double()
    gauss = SpdAffineInvariantGaussianKernel(beta_min=0.0).double()
    table = {"matern": [], "gaussian": []}
    with torch.no_grad():
        for ls in LENGTHSCALES:
            matern.lengthscale = torch.tensor(ls, dtype=torch.float64)
            table["matern"].append((ls, float(torch.linalg.eigvalsh(matern.forward(x, x)).min())))
        for beta in BETAS:
            gauss.beta = torch.tensor(beta, dtype=torch.float64)
            k = gauss.forward(x, x).double()
            table["gaussian"].append((beta, float(torch.linalg.eigvalsh(0.5 * (k + k.t())).min())))
    return table


def run(nu=2.5, num_features=1024, nb_samples_post=10, table_points=100, seed=1234, verbose=True, device="cuda:0"):
    g = load()
    x_test = torch.tensor(g["x_test"], device=device)
    y_test = g["y_test"]
    x_train, y_train = x_test[torch.as_tensor(g["train_idx"], device=device)], torch.tensor(g["y_train"], device=device)
    covar = ScaleKernel(SpdAffineInvariantMaternKernel(2, nu=nu, num_features=num_features, seed=seed),
                        outputscale_prior=models.GammaPrior(2.0, 0.15))
    model = models.SingleTaskGP(x_train, y_train, covar, noise_prior=models.GammaPrior(1.1, 0.05))
    models.fit_gpytorch_model(model)
    preds = model(x_test)
    mean, var = preds.mean.cpu().numpy(), preds.variance.cpu().numpy()
    samples = preds.sample(torch.Size([nb_samples_post]), seed=seed).cpu().numpy()
    rmse = float(np.sqrt(np.mean((y_test - mean) ** 2)))
    regression = dict(mean=mean, variance=var, samples=samples, rmse=rmse, jitter=preds.jitter_used,
                      lengthscale=float(covar.base_kernel.lengthscale.detach()))
    name = "heat kernel" if math.isinf(nu) else f"Matern kernel (nu = {nu})"
    if verbose:
        print(f"Affine-invariant {name}, {num_features} features: RMSE {rmse:.4f}, lengthscale {regression['lengthscale']:.3f}, variance in "
              f"[{var.min():.3e}, {var.max():.3e}], {samples.shape[0]} samples, jitter {preds.jitter_used:g}")
    pick = torch.linspace(0, x_test.shape[0] - 1, min(table_points, x_test.shape[0]), device=device).round().long()
    table = min_eigenvalue_table(x_test[pick], nu, num_features, seed)
    if verbose:
        print(f"smallest eigenvalue of the Gram matrix of {len(pick)} points")
        print(f"  {'lengthscale':>12} {name:>28}   |  {'beta':>8} {'Gaussian kernel':>18}")
        for (ls, lm), (beta, lg) in zip(table["matern"], table["gaussian"]):
            print(f"  {ls:12g} {lm:28.3e}   |  {beta:8g} {lg:18.3e}")
    return dict(regression=regression, table=table)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--nu", type=float, default=2.5, help="smoothness (> 0), or inf for the heat kernel")
    ap.add_argument("--features", type=int, default=1024)
    ap.add_argument("--samples", type=int, default=10)
    a = ap.parse_args()
    run(a.nu, a.features, a.samples)
