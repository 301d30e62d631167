"""The fixture of the SPD-manifold grid (tests/golden/spd_manifold_grid.npz, 50-digit truth) checked on the CPU: its layout, the two fp64 routes
whose errors its tolerance table is made of, and the conditions that keep test_gpu_spd_manifold_grid.py from going vacuous or loose - every one
asserted on the references alone.  tests/_cpu_spd_manifold.py describes the families and the tolerance rule."""
import numpy as np
import pytest

from oracle import spd as ospd
from tests import _cpu_spd_manifold as cpu


@pytest.fixture(scope="module")
def g(golden):
    return golden(cpu.FIXTURE)


def test_fixture_layout(g):
    assert tuple(int(d) for d in g["orders"]) == cpu.ORDERS
    assert cpu.ORDERS[:12] == tuple(range(1, 13)) and cpu.ORDERS[12:] == (13, 16, 17, 24, 31, 32)
    nf = len(cpu.FAMILIES)
    for d in cpu.ORDERS:
        for name in ("X", "Y", "log", "exp"):
            a = g[f"{name}_{d}"]
            assert a.shape == (nf, d, d) and a.dtype == np.float64
            assert np.array_equal(a, a.transpose(0, 2, 1)), f"{name}_{d} is not exactly symmetric"
        for name in ("dist", "inner", "norm"):
            assert g[f"{name}_{d}"].shape == (nf,) and g[f"{name}_{d}"].dtype == np.float64
    for name in ("err_oracle", "err_whiten"):
        assert g[name].shape == (len(cpu.ORDERS), len(cpu.OPS), nf)
    assert g["eref"].shape == (len(cpu.OPS), nf)
    np.testing.assert_array_equal(g["eref"], np.maximum(g["err_oracle"], g["err_whiten"]).max(axis=0))


def test_truth_is_nonzero_and_finite(g):
    for d in cpu.ORDERS:
        for op in cpu.OPS:
            a = g[f"{op}_{d}"].reshape(len(cpu.FAMILIES), -1)
            assert np.all(np.isfinite(a)) and np.all(np.max(np.abs(a), axis=1) > 0.0), (op, d)


def test_every_tolerance_is_derived_and_capped(g):
    for o, op in enumerate(cpu.OPS):
        for f, fam in enumerate(cpu.FAMILIES):
            tol = cpu.tol(g, op, fam)
            assert tol == max(10.0 * g["eref"][o, f], 1e-12)
            assert tol <= cpu.TOL_CAP == 1e-7, (op, fam, tol)


@pytest.mark.parametrize("d", cpu.ORDERS)
def test_both_fp64_routes_reproduce_their_stored_errors(g, d):
    """Each route's error against the truth, evaluated again here, is the stored one to within eref(op, family) (another LAPACK may round otherwise) -
    so it is at most 2 eref, a fifth of the tolerance the device is held to."""
    k = cpu.ORDERS.index(d)
    now = cpu.route_errors(g, d)
    for name in cpu.ROUTES:
        stored = g[f"err_{name}"][k]
        assert np.all(stored <= g["eref"])
        assert np.all(np.abs(now[name] - stored) <= g["eref"]), (name, d, now[name], stored)


@pytest.mark.parametrize("d", cpu.ORDERS)
def test_the_families_are_in_their_regimes(g, d):
    X, Y = g[f"X_{d}"], g[f"Y_{d}"]
    A, B, C, D = range(4)
    lam = np.linalg.eigvalsh(X)
    assert np.all(lam > 0.0)
    for f in (A, C, D):
        assert lam[f].min() >= 0.5 * (1 - 1e-12) and lam[f].max() <= 2.0 * (1 + 1e-12)
    if d >= 2:
        assert lam[B].max() / lam[B].min() >= 1e7            # cond_2(X); a 1 x 1 matrix has condition 1 ...
    else:
        assert abs(X[B, 0, 0] - 1e-4) <= 1e-19               # ... and is only badly scaled
    # the whitened matrices, formed in fp64 from the stored pair: X is well-conditioned in C and D, so M is recovered to ~1e-15
    assert np.max(np.abs(cpu.whitened(X[C], Y[C]) - np.eye(d))) <= 1e-5
    assert np.max(np.abs(cpu.whitened(X[C], Y[C]) - np.eye(d))) >= 1e-8      # ... and the pair is not identical
    mu = np.linalg.eigvalsh(cpu.whitened(X[D], Y[D]))
    assert mu.min() > 0.0
    if d >= 2:
        assert mu.max() / mu.min() >= cpu.D_MIN_RATIO * (1 - 1e-9) and cpu.D_MIN_RATIO == 1e3
    assert np.abs(np.log(mu)).max() <= 6.0 * (1 + 1e-9)
    ma = np.linalg.eigvalsh(cpu.whitened(X[A], Y[A]))
    assert ma.min() >= 0.5 * (1 - 1e-9) and ma.max() <= 2.0 * (1 + 1e-9)


@pytest.mark.parametrize("d", cpu.ORDERS)
def test_the_builders_give_the_stored_cases(g, d):
    """The seeded builders reproduce the stored inputs (to rounding: the QR and Cholesky of another LAPACK may differ in the last bits)"""
    X, Y, M = cpu.build_order(d)
    for f in range(len(cpu.FAMILIES)):
        np.testing.assert_allclose(X[f], g[f"X_{d}"][f], rtol=0, atol=1e-9 * np.abs(X[f]).max())
        np.testing.assert_allclose(Y[f], g[f"Y_{d}"][f], rtol=0, atol=1e-9 * np.abs(Y[f]).max())


@pytest.mark.parametrize("d", cpu.ORDERS)
def test_longdouble_polynomial_operations_against_the_oracle(g, d):
    X, U = g[f"X_{d}"][0], g[f"log_{d}"][0]                  # family A
    G, H = (a[0] for a in cpu.poly_inputs(d, 1))
    for got, want in ((cpu.egrad2rgrad_ld(X, G), ospd.spd_egrad2rgrad(X, G)), (cpu.ehess2rhess_ld(X, G, H, U), ospd.spd_ehess2rhess(X, G, H, U))):
        assert got.dtype == np.longdouble
        assert float(np.max(np.abs(got - want)) / np.max(np.abs(got))) <= 1e-13
        assert float(np.max(np.abs(got - np.swapaxes(got, -1, -2)))) <= 1e-16 * float(np.max(np.abs(got)))      # a Riemannian gradient is symmetric
