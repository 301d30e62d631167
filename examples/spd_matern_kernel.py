#!/usr/bin/env python3
"""Gaussian-process regression on the SPD manifold with the Matern kernels of the two flat metrics on the MI355X: the flow of
examples/spd_kernels.py (the C-shaped trajectory of the 2D-letters data as 2 x 2 SPD matrices, time as the target, a part of the trajectory
left out of the training set) with SpdLogEuclideanMaternKernel and SpdFrobeniusMaternKernel in the place of the Gaussian kernels.  Per kernel
the surrogate is fitted - the distance matrix once, then one likelihood launch per L-BFGS evaluation - and `model(x_test)` gives the joint
posterior over the whole trajectory, from which posterior samples are drawn.

The kernels are gpytorch's MaternKernel of the metric's distance (x = sqrt(2 nu) r / lengthscale), positive definite for every lengthscale.

    python examples/spd_matern_kernel.py [--nu 2.5] [--samples 10]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gabotorch_amd import models                                                                        # noqa: E402
from gabotorch_amd._compat import ScaleKernel                                                           # noqa: E402
from gabotorch_amd.kernel_utils.kernels_spd import SpdFrobeniusMaternKernel, SpdLogEuclideanMaternKernel   # noqa: E402


def load():
    g = np.load(os.path.join(ROOT, "tests", "golden", "letters_gp.npz"))
    return {k: g[k] for k in g.files}


def run(nu=2.5, nb_samples_post=10, seed=1234, verbose=True, device="cuda:0"):
    g = load()
    x_test = torch.tensor(g["x_test"], device=device)
    y_test = g["y_test"]
    x_train, y_train = x_test[torch.as_tensor(g["train_idx"], device=device)], torch.tensor(g["y_train"], device=device)
    kernels = [("Log-Euclidean Matern kernel", SpdLogEuclideanMaternKernel), ("Frobenius Matern kernel", SpdFrobeniusMaternKernel)]
    results = {}
    for k, (title, make) in enumerate(kernels):
        covar = ScaleKernel(make(nu=nu), outputscale_prior=models.GammaPrior(2.0, 0.15))
        model = models.SingleTaskGP(x_train, y_train, covar, noise_prior=models.GammaPrior(1.1, 0.05))
        models.fit_gpytorch_model(model)
        preds = model(x_test)
        mean, var = preds.mean.cpu().numpy(), preds.variance.cpu().numpy()
        samples = preds.sample(torch.Size([nb_samples_post]), seed=seed + k).cpu().numpy()
        rmse = float(np.sqrt(np.mean((y_test - mean) ** 2)))
        results[title] = dict(mean=mean, variance=var, samples=samples, rmse=rmse, jitter=preds.jitter_used,
                              lengthscale=float(covar.base_kernel.lengthscale.detach()))
        if verbose:
            print(f"{title} (nu = {nu}): RMSE {rmse:.4f}, lengthscale {results[title]['lengthscale']:.3f}, variance in "
                  f"[{var.min():.3e}, {var.max():.3e}], {samples.shape[0]} samples, jitter {preds.jitter_used:g}")
    return results


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--nu", type=float, default=2.5, choices=[0.5, 1.5, 2.5])
    ap.add_argument("--samples", type=int, default=10)
    a = ap.parse_args()
    run(a.nu, a.samples)
