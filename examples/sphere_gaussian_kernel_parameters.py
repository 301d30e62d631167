#!/usr/bin/env python3
"""Experimental selection of beta_min for the sphere Gaussian kernel on the MI355X - the flow of the reference's
examples/kernels/sphere/sphere_gaussian_kernel_parameters.py:38-115: per trial 10 random means on the sphere, identity-covariance normal samples
around them projected onto the sphere, and for a range of beta the share of point sets whose kernel matrix is positive definite (minimum
eigenvalue above 0).  beta_min is the smallest beta from which on every set is.  The whole study is one distance launch, one eigenvalue
launch and one copy to the host; no plots.

    python examples/sphere_gaussian_kernel_parameters.py [--dim 3] [--samples 500] [--trials 20]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gabotorch_amd.kernel_utils import kernel_parameters                               # noqa: E402
from gabotorch_amd.kernel_utils.kernels_sphere import SphereGaussianKernel             # noqa: E402

NB_PARAMS = 30
NB_SOURCES = 10


def betas_for(dim):
    """sphere_gaussian_kernel_parameters.py:50-58 (dim = ambient dimension; the reference defines no range below 3: the one of 3 is used)"""
    if dim <= 3:
        return np.logspace(0, 5, NB_PARAMS)
    if dim == 4:
        return np.logspace(0, 2, NB_PARAMS)
    if dim <= 10:
        return np.logspace(-0.2, 1.5, NB_PARAMS)
    return np.logspace(-1.5, 0.5, NB_PARAMS)


def sample_sets(dim, samples, trials, fact_cov=1.0):
    """(trials, samples rounded down to a multiple of 10, dim): the reference's 'not extremely rigorous' sampling (:65-82)"""
    per_source = samples // NB_SOURCES
    sets = []
    for _ in range(trials):
        mean = np.random.randn(NB_SOURCES, dim)
        mean /= np.linalg.norm(mean, axis=1)[:, None]
        data = np.concatenate([np.random.multivariate_normal(mean[i], fact_cov * np.eye(dim), per_source) for i in range(NB_SOURCES)])
        sets.append(data / np.linalg.norm(data, axis=1)[:, None])
    return np.stack(sets)


def run(dim=3, samples=500, trials=20, seed=1234, verbose=True):
    np.random.seed(seed)
    betas = betas_for(dim)
    sets = sample_sets(dim, samples, trials)
    share, eig = kernel_parameters.percentage_pd_kernels(SphereGaussianKernel, sets, betas, 0.0)
    beta_min = kernel_parameters.smallest_pd_parameter(betas, share)
    if verbose:
        print(f"S^{dim - 1}, {trials} sets of {sets.shape[1]} points")
        print("        beta   PD share   mean min eigenvalue")
        for b, s, m in zip(betas, share, eig.mean(axis=0)):
            print(f"{b:12.4f} {s:10.2f} {m:21.6e}")
        print(f"beta_min = {beta_min}")
    return betas, share, eig, beta_min


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--dim", type=int, default=3)
    ap.add_argument("--samples", type=int, default=500)
    ap.add_argument("--trials", type=int, default=20)
    a = ap.parse_args()
    run(a.dim, a.samples, a.trials)
