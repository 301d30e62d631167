"""Host side of the Riemannian Matern / heat kernels on the sphere (no GPU): the series coefficients against 50-digit values
(tests/golden/make_golden_sphere_matern.py), their sums, the constructor's and the C entry points' argument checks."""
import ctypes
import math
import os

import numpy as np
import pytest

from gabotorch_amd import _lib, ops
from gabotorch_amd.kernel_utils.kernels_sphere import SphereRiemannianMaternKernel

U = 2.0 ** -53


@pytest.fixture(scope="module")
def gold(golden):
    g = golden("sphere_matern.npz")
    return {k: g[k] for k in g.files}


def _cases(gold):
    for i, (dim, kappa, nu, L) in enumerate(gold["cases"]):
        yield i, int(dim), float(kappa), float(nu), int(L)


def _log_terms(dim, kappa, nu, L):
    """|log Phi_n| + |log m_n| and Phi'_n / Phi_n, from the definition"""
    d = dim - 1
    n = np.arange(L + 1, dtype=np.float64)
    lam = n * (n + d - 1)
    logm = np.array([0.0] + [math.log(math.comb(k + d, d) - math.comb(k + d - 2, d)) for k in range(1, L + 1)])
    if math.isinf(nu):
        logphi, rate = -kappa * kappa * lam / 2, -kappa * lam
    else:
        base = 2 * nu / kappa ** 2 + lam
        logphi, rate = -(nu + d / 2) * np.log(base), (nu + d / 2) * (4 * nu / kappa ** 3) / base
    return np.abs(logphi) + np.abs(logm), rate


def test_coefficients_match_the_50_digit_values(gold):
    """The weights are formed in log space (so that nothing overflows), which bounds what "a few ulp" can mean: log Phi_n and log m_n each carry
    a relative rounding of about two ulp (one libm logarithm, one product), i.e. an ABSOLUTE error of 2 * 2^-53 * M_n in log w_n with
    M_n = |log Phi_n| + |log m_n|, which is the relative error of w_n; the normaliser carries that of the terms that matter in it
    (M_sig = max M_k over p_k >= 2^-53).  exp, the division and the sum add a few ulp.  Hence
        |p_n - golden| <= 2^-53 (8 + 4 (M_n + M_sig)) golden   [+ 4 ulp per derivative map: three roundings each]
    - a few ulp wherever the logarithms are O(1).  d p_n / d kappa = p_n (r_n - rbar), r = Phi' / Phi, rbar = sum p_k r_k, loses what the
    difference cancels: the same relative bound on the factor p_n (r_n - rbar) plus the rounding of r_n and rbar at their own magnitudes."""
    assert len(gold["cases"]) >= 60
    for i, dim, kappa, nu, L in _cases(gold):
        M, rate = _log_terms(dim, kappa, nu, L)
        p_gold = gold["coef0"][gold["off0"][i]:gold["off0"][i + 1]]
        m_sig = M[p_gold >= U].max()
        rel = U * (8 + 4 * (M + m_sig))
        for order in (0, 1, 2):
            want = gold[f"coef{order}"][gold[f"off{order}"][i]:gold[f"off{order}"][i + 1]]
            got, sd = ops.sphere_matern_coefficients(dim, kappa, nu, L, order)
            assert sd == dim - 1 + 2 * order and got.dtype == np.float64 and got.shape == want.shape
            r = (rel[order:] if len(rel) > order else rel[-1:]) + 4 * order * U
            err = np.abs(got - want)
            assert np.all(err <= r * np.abs(want) + 1e-300), (dim, kappa, nu, L, order, float((err / (np.abs(want) + 1e-300)).max() / U))
        want = gold["coefk"][gold["offk"][i]:gold["offk"][i + 1]]
        got, sd = ops.sphere_matern_coefficients(dim, kappa, nu, L, 0, wrt_lengthscale=True)
        assert sd == dim - 1
        rbar = float((p_gold * rate).sum())
        rsum = float((p_gold * np.abs(rate)).sum())
        tol = p_gold * (rel * np.abs(rate - rbar) + U * (8 + 8 * m_sig) * (np.abs(rate) + rsum)) + 1e-300
        assert np.all(np.abs(got - want) <= tol), (dim, kappa, nu, L, "dkappa", float((np.abs(got - want) / tol).max()))


def test_coefficients_are_a_probability_vector_and_their_lengthscale_derivative_sums_to_zero(gold):
    for i, dim, kappa, nu, L in _cases(gold):
        p, _ = ops.sphere_matern_coefficients(dim, kappa, nu, L)
        assert np.all(p >= 0.0)
        assert abs(math.fsum(p) - 1.0) <= (L + 1) * U
        dp, _ = ops.sphere_matern_coefficients(dim, kappa, nu, L, wrt_lengthscale=True)
        _, rate = _log_terms(dim, kappa, nu, L)
        # the same scale, at the magnitude of the terms: each product p_n (r_n - rbar) and rbar = sum p_n r_n are rounded at their own size
        scale = math.fsum(np.abs(dp)) + 2.0 * math.fsum(p * np.abs(rate))
        assert abs(math.fsum(dp)) <= (L + 1) * U * scale, (dim, kappa, nu, L)


def test_nothing_overflows_at_the_largest_sizes():
    for nu in (0.5, 2.5, 50.0, math.inf):
        for kappa in (1e-3, 0.05, 1.0, 30.0):
            for order in (0, 1, 2):
                p, sd = ops.sphere_matern_coefficients(64, kappa, nu, 128, order)
                assert np.all(np.isfinite(p)) and sd == 63 + 2 * order
            assert abs(math.fsum(ops.sphere_matern_coefficients(64, kappa, nu, 128)[0]) - 1.0) <= 129 * U


def test_orders_and_sizes():
    p, sd = ops.sphere_matern_coefficients(3, 0.3, 2.5, 1)
    assert p.shape == (2,) and sd == 2
    q, sd1 = ops.sphere_matern_coefficients(3, 0.3, 2.5, 1, 1)
    assert q.shape == (1,) and sd1 == 4 and q[0] == p[1] * (1.0 * 2.0) / 2.0          # f = p_0 + p_1 c
    z, sd2 = ops.sphere_matern_coefficients(3, 0.3, 2.5, 1, 2)
    assert z.shape == (1,) and sd2 == 6 and z[0] == 0.0
    assert ops.sphere_matern_coefficients(2, 0.3, math.inf, 128, 2)[0].shape == (127,)


@pytest.mark.parametrize("bad", [dict(dim=1), dict(num_levels=0), dict(num_levels=129), dict(nu=0.0), dict(nu=-1.0), dict(nu=math.nan),
                                 dict(lengthscale=0.0), dict(lengthscale=math.inf), dict(order=3), dict(order=-1)])
def test_coefficient_argument_errors(bad):
    kw = dict(dim=3, lengthscale=0.5, nu=2.5, num_levels=8, order=0)
    kw.update(bad)
    with pytest.raises(ValueError):
        ops.sphere_matern_coefficients(**kw)


def test_kernel_constructor():
    k = SphereRiemannianMaternKernel()
    assert k.nu == 2.5 and k.num_levels == 32 and k.has_lengthscale
    assert [n for n, _ in k.named_parameters()] == ["raw_lengthscale"]          # nu is fixed: model.parameters() does not see it
    assert SphereRiemannianMaternKernel(nu=math.inf, num_levels=128).nu == math.inf
    assert SphereRiemannianMaternKernel(nu=0.5, num_levels=1).num_levels == 1
    for bad in (dict(nu=0.0), dict(nu=-2.5), dict(nu=math.nan), dict(num_levels=0), dict(num_levels=129), dict(num_levels=2.5)):
        with pytest.raises(ValueError):
            SphereRiemannianMaternKernel(**bad)


def test_entry_points_reject_bad_arguments_on_the_host():
    """before anything touches the GPU: null data pointers throughout, sizes that would launch if a check were missing"""
    if not os.path.exists(_lib.LIB_PATH):
        from gabotorch_amd import _build
        _build.build()
    lib = _lib.load()
    coeff = (ctypes.c_double * 130)(*([1.0] * 130))
    cp = ctypes.cast(coeff, ctypes.c_void_p)
    fi, pw = lib.gabo_sphere_zonal_from_inner, lib.gabo_sphere_zonal_pairwise
    for n_coeff in (0, -1, 130):
        assert fi(None, None, 8, cp, n_coeff, 2, None) == _lib.GABO_ERR_ARG
        assert pw(None, None, None, 1, 4, 4, 3, 0, 0, cp, n_coeff, 2, 0, 0, None) == _lib.GABO_ERR_ARG
    for sd in (0, -3):
        assert fi(None, None, 8, cp, 5, sd, None) == _lib.GABO_ERR_DIM
        assert pw(None, None, None, 1, 4, 4, 3, 0, 0, cp, 5, sd, 0, 0, None) == _lib.GABO_ERR_DIM
    assert fi(None, None, 8, None, 5, 2, None) == _lib.GABO_ERR_ARG                      # no coefficients
    assert fi(None, None, -1, cp, 5, 2, None) == _lib.GABO_ERR_ARG
    assert fi(None, None, 8, cp, 5, 2, None) == _lib.GABO_ERR_ARG                        # null data
    assert fi(None, None, 0, cp, 129, 1, None) == _lib.GABO_OK
    for dim in (0, -1):
        assert pw(None, None, None, 1, 4, 4, dim, 0, 0, cp, 5, 2, 0, 0, None) == _lib.GABO_ERR_DIM
    assert pw(None, None, None, 1, 4, 5, 3, 0, 0, cp, 5, 2, _lib.GABO_SYMMETRIC, 0, None) == _lib.GABO_ERR_ARG      # x1 is x2 needs n1 == n2
    assert pw(None, None, None, 1, 4, 5, 3, 0, 0, cp, 5, 2, 0, 1, None) == _lib.GABO_ERR_ARG                        # so does diag
    assert pw(None, None, None, 70000, 4, 4, 3, 0, 0, cp, 5, 2, 0, 0, None) == _lib.GABO_ERR_ARG
    assert pw(None, None, None, 1, 4, 4, 3, -1, 0, cp, 5, 2, 0, 0, None) == _lib.GABO_ERR_ARG
    assert pw(None, None, None, 1, 4, 4, 3, 0, 0, cp, 5, 2, 0, 0, None) == _lib.GABO_ERR_ARG                        # null data
    assert pw(None, None, None, 1, 0, 4, 3, 0, 0, cp, 129, 1, 0, 0, None) == _lib.GABO_OK
