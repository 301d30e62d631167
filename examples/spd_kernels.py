#!/usr/bin/env python3
"""Gaussian-process regression on the SPD manifold with three kernels on the MI355X - the flow of the reference's
examples/kernels/spd/spd_kernels.py:85-234 without the plots: the C-shaped trajectory of the 2D-letters data turned into 2 x 2 SPD matrices, time
as the target, a part of the trajectory left out of the training set; per kernel (affine-invariant, Frobenius, log-Euclidean Gaussian) the
surrogate is fitted, `preds = model(x_test)` gives the joint posterior over the whole trajectory and ten posterior samples are drawn - kernel
matrices, fit, posterior covariance, its Cholesky factor and the samples all on the device.

The data come from tests/golden/letters_gp.npz (written from the reference's C.mat by tests/golden/make_golden_letters_gp.py).

    python examples/spd_kernels.py [--samples 10] [--fixed]

--fixed: predict with the fixture's hyper-parameters (affine-invariant kernel only) instead of fitting.
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
from gabotorch_amd.kernel_utils.kernels_spd import (SpdAffineInvariantGaussianKernel, SpdFrobeniusGaussianKernel,   # noqa: E402
                                                    SpdLogEuclideanGaussianKernel)


def load():
    g = np.load(os.path.join(ROOT, "tests", "golden", "letters_gp.npz"))
    return {k: g[k] for k in g.files}


def run(nb_samples_post=10, fixed=False, seed=1234, verbose=True, device="cuda:0"):
    g = load()
    x_test = torch.tensor(g["x_test"], device=device)
    y_test = g["y_test"]
    x_train, y_train = x_test[torch.as_tensor(g["train_idx"], device=device)], torch.tensor(g["y_train"], device=device)
    kernels = [("Affine-invariant kernel", lambda: SpdAffineInvariantGaussianKernel(beta_min=0.6))]
    if not fixed:
        kernels += [("Frobenius kernel", SpdFrobeniusGaussianKernel), ("Log-Euclidean kernel", SpdLogEuclideanGaussianKernel)]
    results = {}
    for k, (title, make) in enumerate(kernels):
        covar = ScaleKernel(make(), outputscale_prior=models.GammaPrior(2.0, 0.15))             # spd_kernels.py:150-151
        if fixed:
            covar = covar.double()
            covar.base_kernel.beta = float(g["beta"])
            covar.outputscale = float(g["outputscale"])
            model = models.SingleTaskGP(x_train, y_train, covar, initial_noise=float(g["noise"]))
        else:
            model = models.SingleTaskGP(x_train, y_train, covar, noise_prior=models.GammaPrior(1.1, 0.05))      # :153-158
            models.fit_gpytorch_model(model)                                                                   # :162
        preds = model(x_test)                                                                                  # :168
        mean, var = preds.mean.cpu().numpy(), preds.variance.cpu().numpy()
        cov = preds.covariance_matrix.cpu().numpy()
        samples = preds.sample(torch.Size([nb_samples_post]), seed=seed + k).cpu().numpy()                     # :174
        rmse = float(np.sqrt(np.mean((y_test - mean) ** 2)))
        results[title] = dict(mean=mean, variance=var, covariance=cov, samples=samples, rmse=rmse, jitter=preds.jitter_used)
        if verbose:
            print(f"{title}: RMSE {rmse:.4f}, variance in [{var.min():.3e}, {var.max():.3e}], {samples.shape[0]} samples "
                  f"(spread of the samples around the mean {np.abs(samples - mean).max():.3f}), jitter {preds.jitter_used:g}")
    return results


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=10)
    ap.add_argument("--fixed", action="store_true")
    a = ap.parse_args()
    run(a.samples, a.fixed)
