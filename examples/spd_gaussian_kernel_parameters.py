#!/usr/bin/env python3
"""Experimental selection of beta_min for the SPD affine-invariant Gaussian kernel on the MI355X - the flow of the reference's
examples/kernels/spd/spd_gaussian_kernel_parameters.py:42-128: random SPD matrices with eigenvalues in [0.001, 5], those with a condition
number above 100 removed, and for a range of beta the share of point sets whose kernel matrix is positive definite (minimum eigenvalue above
-5e-7).  beta_min is the smallest beta from which on every set is.  The filter leaves sets of unequal size, so the study is one distance launch,
one eigenvalue launch over all beta and one copy to the host per set; no plots.

    python examples/spd_gaussian_kernel_parameters.py [--dim 3] [--samples 500] [--trials 10]
"""
import argparse
import os
import sys
import types

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gabotorch_amd import manifolds                                                                    # noqa: E402
from gabotorch_amd.Riemannian_utils.spd_utils import spd_sample, symmetric_matrix_to_vector_mandel       # noqa: E402
from gabotorch_amd.kernel_utils import kernel_parameters                                               # noqa: E402
from gabotorch_amd.kernel_utils.kernels_spd import SpdAffineInvariantGaussianKernel                    # noqa: E402

MIN_TOLERATED_EIGENVALUE = -5e-7          # spd_gaussian_kernel_parameters.py:53
NB_PARAMS = 30


def betas_for(dim):
    """spd_gaussian_kernel_parameters.py:74-80 (the reference defines no range for dim = 4: the one of dim >= 5 is used)"""
    if dim == 2:
        return np.logspace(-1, 2, NB_PARAMS)
    if dim == 3:
        return np.logspace(-1.1, 1, NB_PARAMS)
    return np.logspace(-1.5, 0.8, NB_PARAMS)


def sample_sets(dim, samples, trials, min_eig=0.001, max_eig=5.0):
    man = manifolds.PositiveDefinite(dim)
    man.rand = types.MethodType(spd_sample, man)
    man.min_eig, man.max_eig = min_eig, max_eig
    sets = []
    for _ in range(trials):
        mats = np.array([man.rand() for _ in range(samples)])
        mats = mats[np.linalg.cond(mats) <= 100]                      # remove too-ill-conditioned matrices (:91-96)
        sets.append(symmetric_matrix_to_vector_mandel(mats))
    return sets


def run(dim=3, samples=500, trials=10, seed=1234, verbose=True):
    np.random.seed(seed)
    betas = betas_for(dim)
    sets = sample_sets(dim, samples, trials)
    share, eig = kernel_parameters.percentage_pd_kernels(SpdAffineInvariantGaussianKernel, sets, betas, MIN_TOLERATED_EIGENVALUE)
    beta_min = kernel_parameters.smallest_pd_parameter(betas, share)
    if verbose:
        print(f"SPD({dim}), {trials} sets of {min(len(s) for s in sets)} ... {max(len(s) for s in sets)} points")
        print("      beta   PD share   mean min eigenvalue")
        for b, s, m in zip(betas, share, eig.mean(axis=0)):
            print(f"{b:10.4f} {s:10.2f} {m:21.6e}")
        print(f"beta_min = {beta_min}")
    return betas, share, eig, beta_min


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--dim", type=int, default=3)
    ap.add_argument("--samples", type=int, default=500)
    ap.add_argument("--trials", type=int, default=10)
    a = ap.parse_args()
    run(a.dim, a.samples, a.trials)
