"""Host side of the one-launch marginal likelihood of the sphere Matern kernel (no GPU): the argument checks of gabo_gp_mll_series, the
numpy reference the GPU tests compare against (tests/_cpu_gp_mll_series.py) against differences of itself, and the cached level
multiplicities of ops.sphere_matern_coefficients."""
import math
import os

import numpy as np
import pytest

from gabotorch_amd import _lib, ops
from tests._cpu_gp_mll_series import reference, sphere_points


@pytest.fixture(scope="module", autouse=True)
def _built_library():
    if not os.path.exists(_lib.LIB_PATH):
        from gabotorch_amd import _build
        _build.build()


def test_entry_validates_on_the_host_before_any_hip_call():
    f = _lib.load().gabo_gp_mll_series

    def call(n=5, n_coeff=33, series_dim=2):
        return f(None, None, n, None, None, n_coeff, series_dim, 1.0, 0.1, 0.0, None, None)

    assert call(n=0) == _lib.GABO_ERR_DIM
    assert call(n=_lib.GABO_GP_MLL_MAX_N + 1) == _lib.GABO_ERR_DIM and _lib.GABO_GP_MLL_MAX_N == 160
    assert call(series_dim=0) == _lib.GABO_ERR_DIM
    assert call(n_coeff=0) == _lib.GABO_ERR_ARG
    assert call(n_coeff=130) == _lib.GABO_ERR_ARG
    assert call() == _lib.GABO_ERR_ARG                                   # null c (and y, out, coeff_host)
    # the counts alone: every pointer given, the coefficient count out of range
    import ctypes
    buf = (ctypes.c_double * 256)()
    ptr = ctypes.addressof(buf)
    for bad in (0, 130):
        assert f(ptr, ptr, 5, ptr, None, bad, 2, 1.0, 0.1, 0.0, ptr, None) == _lib.GABO_ERR_ARG
    assert f(None, ptr, 5, ptr, None, 33, 2, 1.0, 0.1, 0.0, ptr, None) == _lib.GABO_ERR_ARG      # null c alone


@pytest.mark.parametrize("dim", [3, 10])
def test_reference_lengthscale_derivative_against_central_differences(dim):
    """out[1] of the numpy reference against central differences of its own likelihood in kappa: h = 1e-5 (truncation h^2 |f'''| / 6 and
    rounding 2^-53 |f| / h are both ~1e-10 relative to the likelihood)"""
    n, nu, levels, kappa, h = 40, 2.5, 32, 0.5, 1e-5
    rng = np.random.default_rng(1000 * dim + n)
    x = sphere_points(rng, n, dim)
    y = rng.standard_normal(n)
    par = (1.7, 0.03, -0.2)
    out, _, _ = reference(x @ x.T, y, dim, kappa, nu, levels, *par)
    up, _, _ = reference(x @ x.T, y, dim, kappa + h, nu, levels, *par)
    dn, _, _ = reference(x @ x.T, y, dim, kappa - h, nu, levels, *par)
    fd = (up[0] - dn[0]) / (2 * h)
    print(f"dim {dim}: d ll / d kappa {out[1]:.12e}, differences {fd:.12e}, relative gap {abs(out[1] - fd) / max(1.0, abs(fd)):.2e}")
    assert abs(out[1] - fd) <= 1e-7 * max(1.0, abs(fd))


def _uncached(dim, kappa, nu, L, wrt_lengthscale):
    """the arithmetic of ops.sphere_matern_coefficients (order 0) with the multiplicities formed afresh"""
    d = dim - 1
    n = np.arange(L + 1, dtype=np.float64)
    lam = n * (n + (d - 1.0))
    logm = np.array([0.0] + [math.log(math.comb(k + d, d) - math.comb(k + d - 2, d)) for k in range(1, L + 1)])
    if math.isinf(nu):
        logphi = -(kappa * kappa) * lam / 2.0
        rate = -kappa * lam
    else:
        base = 2.0 * nu / (kappa * kappa) + lam
        logphi = -(nu + d / 2.0) * np.log(base)
        rate = (nu + d / 2.0) * (4.0 * nu / kappa ** 3) / base
    logw = logphi + logm
    w = np.exp(logw - logw.max())
    p = w / w.sum()
    return p * (rate - (p * rate).sum()) if wrt_lengthscale else p


def test_cached_multiplicities_leave_the_coefficients_bit_identical(golden):
    """every (dim, kappa, nu, levels) of the golden generator, all orders and the lengthscale derivative: a first call (empty cache), a second
    call (cached multiplicities) and the arithmetic with the multiplicities formed afresh agree bit for bit; so does the one-pass helper"""
    cases = golden("sphere_matern.npz")["cases"]
    assert len(cases) > 0
    ops._sphere_level_logm.clear()
    for dim, kappa, nu, L in cases:
        dim, L = int(dim), int(L)
        for order, wrt in ((0, False), (1, False), (2, False), (0, True)):
            first, sd1 = ops.sphere_matern_coefficients(dim, kappa, nu, L, order, wrt_lengthscale=wrt)
            assert (dim, L) in ops._sphere_level_logm
            second, sd2 = ops.sphere_matern_coefficients(dim, kappa, nu, L, order, wrt_lengthscale=wrt)
            assert sd1 == sd2 == dim - 1 + 2 * order and first.tobytes() == second.tobytes()
            if order == 0:
                assert first.tobytes() == _uncached(dim, float(kappa), float(nu), L, wrt).tobytes()
        p, dp, sd = ops.sphere_matern_coefficients_and_derivative(dim, kappa, nu, L)
        assert sd == dim - 1
        assert p.tobytes() == ops.sphere_matern_coefficients(dim, kappa, nu, L)[0].tobytes()
        assert dp.tobytes() == ops.sphere_matern_coefficients(dim, kappa, nu, L, wrt_lengthscale=True)[0].tobytes()
    with pytest.raises(ValueError):                                       # the cached array is shared: nobody may write to it
        ops._sphere_level_logm[(int(cases[0][0]), int(cases[0][3]))][0] = 1.0
