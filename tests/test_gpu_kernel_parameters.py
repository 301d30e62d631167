"""The device path of the kernel-parameter study (csrc/gram_eig.hip, ops.gram_extreme_eigenvalues, kernel_utils.kernel_parameters) against
numpy.linalg.eigvalsh of exp(-theta E) with E from the oracle's distances.

Tolerance of the eigenvalue kernel: 16 n eps max(1, lambda_max) - the backward error of Householder tridiagonalisation plus bisection is
c n eps ||K||_2, and one ulp of exp per entry moves an eigenvalue by at most n eps.
End to end the Gram entries themselves differ from the oracle's by what the Gram tests grant, and an element-wise perturbation delta moves an
eigenvalue by at most N delta (Weyl), with |K| <= 1:
  SPD affine-invariant Gaussian   rtol 1e-9, atol 1e-12   tests/test_gpu_parity.py:58
  SPD affine-invariant Laplace    rtol 1e-10              tests/test_gpu_parity.py:89
  sphere Gaussian and Laplace     rtol 1e-11, atol 1e-13  tests/test_gpu_parity.py:243
  SPD log-Euclidean Gaussian      rtol 1e-9, atol 1e-14   tests/test_gpu_autograd.py:207 (test_gpu_parity.py has no log-Euclidean case)
  SPD Frobenius Gaussian          rtol 1e-9, atol 1e-14   (no Gram test against the oracle: the log-Euclidean kernel is this one on logm X)
"""
import functools

import numpy as np
import pytest
import torch

from gabotorch_amd import _lib, ops
from gabotorch_amd.kernel_utils import kernel_parameters as kp
from gabotorch_amd.kernel_utils import kernels_spd as kspd
from gabotorch_amd.kernel_utils import kernels_sphere as ksph
from oracle import spd as ospd
from oracle import sphere as osph

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
EPS = np.finfo(np.float64).eps
LDS_MAX = _lib.GABO_GRAM_EIG_LDS_MAX_N


def t(x):
    return torch.tensor(np.ascontiguousarray(x), dtype=torch.float64, device=DEV)


def eig_tol(n, lam_max):
    return 16 * n * EPS * max(1.0, lam_max)


def sphere_points(rng, n, dim=3):
    x = rng.standard_normal((n, dim))
    return x / np.linalg.norm(x, axis=-1, keepdims=True)


def spd_points(rng, n, d=3, lo=0.2, hi=5.0):
    out = np.empty((n, d, d))
    for k in range(n):
        q, _ = np.linalg.qr(rng.standard_normal((d, d)))
        m = (q * rng.uniform(lo, hi, d)) @ q.T
        out[k] = 0.5 * (m + m.T)
    return ospd.symmetric_matrix_to_vector_mandel(out)


@functools.lru_cache(maxsize=None)
def sphere_e(n, batch, seed=0):
    """(batch, n, n) squared oracle distances of random points of S^2 (read-only: shared by the tests)"""
    rng = np.random.default_rng(1000 * seed + n)
    e = np.stack([osph.sphere_distance(x, x) ** 2 for x in (sphere_points(rng, n) for _ in range(batch))])
    e.setflags(write=False)
    return e


def extremes(e, thetas):
    """numpy reference: (batch, P, 2)"""
    out = np.empty((e.shape[0], len(thetas), 2))
    for b in range(e.shape[0]):
        for p, th in enumerate(thetas):
            lam = np.linalg.eigvalsh(np.exp(-th * e[b]))
            out[b, p] = lam[0], lam[-1]
    return out


def check(got, want, n):
    assert got.shape == want.shape
    for idx in np.ndindex(want.shape[:-1]):
        tol = eig_tol(n, want[idx][1])
        err = np.abs(got[idx] - want[idx])
        print(f"n = {n} {idx}: |error| = {err[0]:.3e}, {err[1]:.3e}  tolerance {tol:.3e}")
        assert np.all(err <= tol), (n, idx, got[idx], want[idx], tol)


# ---- 1. the kernel alone ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 17, 64, 65, 130, LDS_MAX, LDS_MAX + 1, 257])
def test_extreme_eigenvalues_against_eigvalsh(n):
    thetas = [0.1, 1.0, 5.0, 40.0]
    e = sphere_e(n, 2)
    got = ops.gram_extreme_eigenvalues(t(e), thetas)
    assert got.device == torch.device(DEV) and got.shape == (2, 4, 2)
    check(got.cpu().numpy(), extremes(e, thetas), n)


def test_the_largest_size():
    n, thetas = _lib.GABO_GRAM_EIG_MAX_N, [0.5, 8.0]
    e = sphere_e(n, 1)
    got = ops.gram_extreme_eigenvalues(t(e), torch.tensor(thetas, dtype=torch.float64, device=DEV))
    check(got.cpu().numpy(), extremes(e, thetas), n)


def test_lower_triangle_only_is_read_and_leading_shape_is_kept():
    e = sphere_e(17, 2)
    upper_garbage = np.tril(e) + np.triu(np.full_like(e, 123.0), 1)
    a = ops.gram_extreme_eigenvalues(t(e).reshape(2, 1, 17, 17), [0.7])
    b = ops.gram_extreme_eigenvalues(t(upper_garbage).reshape(2, 1, 17, 17), [0.7])
    assert a.shape == (2, 1, 1, 2) and torch.equal(a, b)


# ---- 2. degenerate spectra -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [65, LDS_MAX + 8])
def test_degenerate_spectra(n):
    e = sphere_e(n, 1)
    # theta = 0: K is all ones (rank one, every reflector after the first sees a zero column); theta = 1e4: the identity to rounding
    thetas = [0.0, 1e4]
    got = ops.gram_extreme_eigenvalues(t(e), thetas).cpu().numpy()
    want = extremes(e, thetas)
    check(got, want, n)
    assert abs(got[0, 0, 0]) <= eig_tol(n, n) and abs(got[0, 0, 1] - n) <= eig_tol(n, n)
    # one point three times: an exactly singular K
    x = sphere_points(np.random.default_rng(n), n)
    x[5] = x[n - 1] = x[2]
    es = (osph.sphere_distance(x, x) ** 2)[None]
    thetas = [0.5, 3.0]
    want = extremes(es, thetas)
    check(ops.gram_extreme_eigenvalues(t(es), thetas).cpu().numpy(), want, n)


# ---- 3. batching -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [40, LDS_MAX + 8])
def test_every_pair_of_a_batch_equals_the_pair_alone_bit_for_bit(n):
    e = t(sphere_e(n, 3, seed=1))
    thetas = torch.tensor([0.05, 0.4, 1.5, 6.0, 30.0], dtype=torch.float64, device=DEV)
    full = ops.gram_extreme_eigenvalues(e, thetas)
    assert full.shape == (3, 5, 2)
    for b in range(3):
        for p in range(5):
            alone = ops.gram_extreme_eigenvalues(e[b], thetas[p:p + 1])
            assert alone.shape == (1, 2) and torch.equal(alone[0], full[b, p]), (b, p, alone, full[b, p])


# ---- 4. end to end ---------------------------------------------------------------------------------------------------------------------------
N_E2E = 65
# kernel class -> (oracle Gram (x, parameter), element-wise (rtol, atol) its Gram is granted against the oracle: the docstring's table)
SPD_CASES = {
    kspd.SpdAffineInvariantGaussianKernel: (lambda x, b: ospd.spd_ai_gaussian_kernel(x, x, b), (1e-9, 1e-12)),
    kspd.SpdAffineInvariantLaplaceKernel: (lambda x, b: ospd.spd_ai_laplace_kernel(x, x, b), (1e-10, 0.0)),
    kspd.SpdFrobeniusGaussianKernel: (lambda x, ls: ospd.frobenius_gaussian_kernel(x, x, ls), (1e-9, 1e-14)),
    kspd.SpdLogEuclideanGaussianKernel: (lambda x, ls: ospd.log_euclidean_gaussian_kernel(x, x, ls), (1e-9, 1e-14)),
}
SPHERE_CASES = {
    ksph.SphereGaussianKernel: (lambda x, b: osph.sphere_gaussian_kernel(x, x, b), (1e-11, 1e-13)),
    ksph.SphereLaplaceKernel: (lambda x, ls: osph.sphere_laplace_kernel(x, x, 1.0 / ls ** 2), (1e-11, 1e-13)),
}


def e2e_tol(n, lam_max, grant):
    return eig_tol(n, lam_max) + n * (grant[0] + grant[1])          # (|K| <= 1)


def oracle_min_eigenvalues(gram, x, params):
    lam = [np.linalg.eigvalsh(gram(x, p)) for p in params]
    return np.array([v[0] for v in lam]), np.array([v[-1] for v in lam])


def check_e2e(kind, gram, grant, x, params):
    got = kp.min_eigenvalues(kind, x, params)
    want, lam_max = oracle_min_eigenvalues(gram, x, params)
    assert isinstance(got, np.ndarray) and got.shape == (len(params),)
    for g, w, top, p in zip(got, want, lam_max, params):
        tol = e2e_tol(len(x), top, grant)
        print(f"{kind.__name__} parameter {p}: lambda_min {g:.6e} oracle {w:.6e} |error| {abs(g - w):.3e} tolerance {tol:.3e}")
        assert abs(g - w) <= tol, (kind.__name__, p, g, w, tol)


@pytest.mark.parametrize("kind", list(SPD_CASES), ids=lambda k: k.__name__)
def test_min_eigenvalues_of_the_spd_kernels(kind):
    x = spd_points(np.random.default_rng(3), N_E2E)
    check_e2e(kind, *SPD_CASES[kind], x, [0.3, 1.0, 2.5])


@pytest.mark.parametrize("dim", [3, 5])
@pytest.mark.parametrize("kind", list(SPHERE_CASES), ids=lambda k: k.__name__)
def test_min_eigenvalues_of_the_sphere_kernels(kind, dim):
    x = sphere_points(np.random.default_rng(dim), N_E2E, dim)
    check_e2e(kind, *SPHERE_CASES[kind], x, [0.4, 1.0, 3.0])
    # an instance is taken like its class
    inst = kind(beta_min=0.0) if kind is ksph.SphereGaussianKernel else kind()
    np.testing.assert_array_equal(kp.min_eigenvalues(inst, x, [1.0]), kp.min_eigenvalues(kind, x, [1.0]))


# ---- 5. verdicts -----------------------------------------------------------------------------------------------------------------------------
SPHERE_BETAS, SPHERE_THRESHOLD = (0.1, 0.5, 6.0, 20.0), 0.0
SPD_BETAS, SPD_THRESHOLD = (0.05, 0.2, 0.8, 3.0), -5e-7
# The seeds of the SPD sets are those, found with the oracle alone, whose lambda_min at beta = 0.2 (+1.0e-4, +1.1e-4, +1.3e-4; -2.7e-2,
# -1.1e-2, -1.1e-2 at beta = 0.05) lies 1000 tolerances (6.5e-5) above the threshold: most sets of this size have it at +1e-5 ... +5e-5.
SPHERE_SEEDS, SPD_SEEDS = (7, 8, 9), (24, 48, 71)


def sphere_set(seed):
    x = np.random.default_rng(seed).standard_normal((96, 3))
    return x / np.linalg.norm(x, axis=-1, keepdims=True)


def spd_set(seed):
    return spd_points(np.random.default_rng(seed), 65)


def oracle_table(gram, grant, sets, params, threshold):
    """(T, P) oracle lambda_min; asserts on the CPU that none of them is within 1000 tolerances of the threshold"""
    rows = []
    for x in sets:
        lam_min, lam_max = oracle_min_eigenvalues(gram, x, params)
        for lo, hi in zip(lam_min, lam_max):
            assert abs(lo - threshold) >= 1000 * e2e_tol(len(x), hi, grant), (lo, threshold, e2e_tol(len(x), hi, grant))
        rows.append(lam_min)
    return np.array(rows)


def test_sphere_verdicts():
    gram, grant = SPHERE_CASES[ksph.SphereGaussianKernel]
    sets = [sphere_set(s) for s in SPHERE_SEEDS]
    table = oracle_table(gram, grant, sets, SPHERE_BETAS, SPHERE_THRESHOLD)
    # S^2, 96 points of default_rng(7): lambda_min = -1.08, -6.7e-3, +1.8e-4, +6.0e-3
    assert list(table[0] > SPHERE_THRESHOLD) == [False, False, True, True]
    got = kp.min_eigenvalues(ksph.SphereGaussianKernel, sets[0], SPHERE_BETAS)
    assert list(got > SPHERE_THRESHOLD) == [False, False, True, True]
    share, eig = kp.percentage_pd_kernels(ksph.SphereGaussianKernel, np.stack(sets), SPHERE_BETAS, SPHERE_THRESHOLD)
    want = np.mean(table > SPHERE_THRESHOLD, axis=0)
    assert eig.shape == (3, 4) and share.shape == (4,)
    np.testing.assert_array_equal(share, want)
    np.testing.assert_array_equal(eig > SPHERE_THRESHOLD, table > SPHERE_THRESHOLD)
    assert kp.smallest_pd_parameter(SPHERE_BETAS, share) == kp.smallest_pd_parameter(SPHERE_BETAS, want) == 6.0


def test_spd_verdicts():
    gram, grant = SPD_CASES[kspd.SpdAffineInvariantGaussianKernel]
    sets = [spd_set(s) for s in SPD_SEEDS]
    table = oracle_table(gram, grant, sets, SPD_BETAS, SPD_THRESHOLD)
    assert list(table[0] > SPD_THRESHOLD) == [False, True, True, True]
    got = kp.min_eigenvalues(kspd.SpdAffineInvariantGaussianKernel, sets[0], SPD_BETAS)
    assert list(got > SPD_THRESHOLD) == [False, True, True, True]
    share, eig = kp.percentage_pd_kernels(kspd.SpdAffineInvariantGaussianKernel, sets, SPD_BETAS, SPD_THRESHOLD)
    want = np.mean(table > SPD_THRESHOLD, axis=0)
    np.testing.assert_array_equal(share, want)
    np.testing.assert_array_equal(eig > SPD_THRESHOLD, table > SPD_THRESHOLD)
    assert kp.smallest_pd_parameter(SPD_BETAS, share) == kp.smallest_pd_parameter(SPD_BETAS, want) == 0.2


# ---- 6. NaN ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [33, LDS_MAX + 8])
def test_nan_stays_in_its_own_pairs(n):
    e = t(sphere_e(n, 2, seed=2))
    thetas = [0.3, 2.0, 9.0]
    clean = ops.gram_extreme_eigenvalues(e, thetas)
    assert bool(torch.isfinite(clean).all())
    dirty = e.clone()
    dirty[1, n - 1, n // 2] = float("nan")                   # (lower triangle)
    got = ops.gram_extreme_eigenvalues(dirty, thetas)
    assert bool(torch.isnan(got[1]).all()) and torch.equal(got[0], clean[0])
    inf = e.clone()
    inf[0, n - 1, 0] = float("inf")                          # exp(-theta inf) = 0 is finite: the entry itself is what counts
    got = ops.gram_extreme_eigenvalues(inf, thetas)
    assert bool(torch.isnan(got[0]).all()) and torch.equal(got[1], clean[1])
    got = ops.gram_extreme_eigenvalues(e, [0.3, float("nan"), 9.0])
    assert bool(torch.isnan(got[:, 1]).all()) and torch.equal(got[:, 0], clean[:, 0]) and torch.equal(got[:, 2], clean[:, 2])


# ---- 7. sets of unequal size -----------------------------------------------------------------------------------------------------------------
def test_a_list_of_sets_of_unequal_size():
    rng = np.random.default_rng(11)
    sets = [spd_points(rng, n) for n in (60, 65, 63)]
    params = [0.1, 0.5, 2.0]
    got = kp.min_eigenvalues(kspd.SpdAffineInvariantGaussianKernel, sets, params)
    assert got.shape == (3, 3)
    for row, x in zip(got, sets):
        np.testing.assert_array_equal(row, kp.min_eigenvalues(kspd.SpdAffineInvariantGaussianKernel, x, params))
    # sets of equal size in a list: one stacked call, the same numbers
    same = [sets[1], spd_points(rng, 65)]
    both = kp.min_eigenvalues(kspd.SpdAffineInvariantGaussianKernel, same, params)
    np.testing.assert_array_equal(both[0], got[1])


def test_refusals_of_the_op():
    with pytest.raises(ValueError):
        ops.gram_extreme_eigenvalues(torch.zeros(3, 3, dtype=torch.float64), [1.0])              # not on the device
    with pytest.raises(ValueError):
        ops.gram_extreme_eigenvalues(torch.zeros(3, 4, dtype=torch.float64, device=DEV), [1.0])
    with pytest.raises(ValueError):
        ops.gram_extreme_eigenvalues(torch.zeros(3, 3, dtype=torch.float64, device=DEV), [])
    with pytest.raises(ValueError):
        ops.gram_extreme_eigenvalues(torch.zeros(1, 1, dtype=torch.float64, device=DEV).expand(1025, 1025), [1.0])
