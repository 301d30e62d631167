"""Plain numpy fp64 statement of the surrogate-fit objective of ScaleKernel(NestedSpdLogEuclideanMaternKernel), written from the formulas and not
from the device code: projection Y_n = W^T X_n W, logm by eigh, the distance with the reference's 1e-15 on every matrix element and the Matern
formulas (tests/_cpu_flat_matern.py), a Cholesky likelihood.  Also the cases, seeded data, directions and central differences that the CPU and
the GPU test share (computed once per process, read-only)."""
import functools
import math

import numpy as np

from tests import _cpu_flat_matern as fm

# (D, d, n, nu): the smallest shapes at which each part of the device chain can go wrong (tests/test_gpu_nested_spd_matern.py lists what each exercises)
CASES = [(5, 2, 12, 2.5), (5, 2, 12, 0.5), (20, 2, 7, 1.5), (12, 3, 65, 2.5), (9, 4, 20, 0.5), (6, 5, 10, 1.5), (32, 2, 9, 2.5), (10, 2, 190, 1.5),
         (6, 2, 260, 2.5)]
SINGLE = [(5, 2, 1, 2.5), (5, 2, 1, 0.5)]
SCALARS = (0.9, 1.3, 0.1, 0.15)          # lengthscale, outputscale, noise, mean
# data seeds, chosen on the CPU so that the objective's own central differences at h and h / 2 agree within the cap along every direction
# (test_nested_spd_matern_cpu.py asserts it).  Seed 1 holds it at every case: the worst allowance / cap is 0.30, at (5, 2, 12, 0.5).
SEEDS = {case: 1 for case in CASES + SINGLE}


def project(x_mats, w):
    y = np.einsum("da,ndk,kb->nab", w, x_mats, w)
    return 0.5 * (y + y.transpose(0, 2, 1))


def features(x_mats, w):
    """Mandel vectors of logm(W^T X_n W)"""
    return fm.logm_mandel(project(np.asarray(x_mats, dtype=np.float64), np.asarray(w, dtype=np.float64)))


def gram(x1_mats, x2_mats, w, lengthscale, nu):
    return fm.gram(features(x1_mats, w), features(x2_mats, w), lengthscale, nu)


def log_likelihood(x_mats, y, w, lengthscale, nu, outputscale, noise, mean):
    n = len(y)
    ky = outputscale * gram(x_mats, x_mats, w, lengthscale, nu) + noise * np.eye(n)
    chol = np.linalg.cholesky(0.5 * (ky + ky.T))
    half = np.linalg.solve(chol, np.asarray(y, dtype=np.float64) - mean)
    return -0.5 * half @ half - np.log(np.diagonal(chol)).sum() - 0.5 * n * math.log(2.0 * math.pi)


@functools.lru_cache(maxsize=None)
def data(case):
    """(SPD matrices n x D x D with spectra uniform in [0.1, 4], targets, W on the Grassmannian, scalars) of a case; read-only"""
    D, d, n, nu = case
    rng = np.random.default_rng(SEEDS[case])
    x, y = fm.random_spd(rng, n, D, 0.1, 4.0), rng.standard_normal(n)
    w = np.linalg.qr(rng.standard_normal((D, d)))[0]
    scalars = np.array(SCALARS)
    for a in (x, y, w, scalars):
        a.setflags(write=False)
    return x, y, w, scalars


def objective(case, w, scalars):
    x, y = data(case)[:2]
    return log_likelihood(x, y, w, scalars[0], case[3], scalars[1], scalars[2], scalars[3])


def tangent(w, u):
    """u projected onto the tangent space of the Grassmannian at w: U - W W^T U"""
    return u - w @ (w.T @ u)


@functools.lru_cache(maxsize=None)
def directions(case):
    """5 seeded directions in (tangent space at W, lengthscale, outputscale, noise, mean), the W part of unit length"""
    D, d, n, nu = case
    w = data(case)[2]
    rng = np.random.default_rng(77 + D + n)
    out = []
    for _ in range(5):
        u = tangent(w, rng.standard_normal((D, d)))
        out.append((u / np.linalg.norm(u), rng.standard_normal(4) * np.array([0.5, 0.5, 0.05, 0.5])))
    return out


@functools.lru_cache(maxsize=None)
def reference_differences(case, h=1e-4):
    """central differences of the numpy objective along each direction at steps h and h / 2"""
    w, scalars = data(case)[2:]
    out = []
    for uw, us in directions(case):
        out.append(tuple((objective(case, w + s * uw, scalars + s * us) - objective(case, w - s * uw, scalars - s * us)) / (2 * s)
                         for s in (h, h / 2)))
    return out


def allowance(d1, d2):
    """(allowance, cap) of a directional derivative against the differences d1 (h) and d2 (h / 2): ten times their own disagreement plus
    1e-9 max(1, |D|); the cap is 1e-5 max(1, |D|)"""
    scale = max(1.0, abs(d2))
    return 10.0 * abs(d1 - d2) + 1e-9 * scale, 1e-5 * scale
