"""The numpy restatements of the Riemannian statistics (tests/_cpu_riemannian_stats.py) against the reference's recorded outputs
(tests/golden/riemannian_stats.npz, written by tests/golden/make_golden_stats.py), their closed forms, and the host-side argument
validation of the new C entries.  No GPU."""
import os

import numpy as np
import pytest

from gabotorch_amd import _lib

from tests import _cpu_riemannian_stats as cpu


@pytest.fixture(scope="module")
def stats(golden):
    return golden("riemannian_stats.npz")


@pytest.fixture(scope="module", autouse=True)
def _built_library():
    if not os.path.exists(_lib.LIB_PATH):
        from gabotorch_amd import _build
        _build.build()


def test_seeded_pools_are_the_fixture_s_inputs(stats):
    """the inputs are derived from a seed, not stored: the fixture keeps each pool's first point (LAPACK's QR may move last bits)"""
    for d in cpu.STATS_SPD_C:
        np.testing.assert_allclose(cpu.stats_spd_pool(d)[0], stats[f"spd{d}_first"], rtol=0, atol=1e-13)
    for dim in cpu.STATS_SPHERE_DIMS:
        np.testing.assert_allclose(cpu.stats_sphere_pool(dim)[0], stats[f"sph{dim}_first"], rtol=0, atol=1e-15)


def test_spd_mean_restatement_matches_the_reference(stats):
    """observed when the fixture was written: <= 2.7e-13 relative Frobenius norm (typically 1e-15; the reference runs a non-symmetric eig)"""
    for d in cpu.STATS_SPD_C:
        X = cpu.from_mandel(cpu.stats_spd_pool(d))
        for n in cpu.STATS_NS:
            want = stats[f"spd{d}_mean_n{n}"]
            got = cpu.spd_mean(X[:n])
            assert np.linalg.norm(got - want) / np.linalg.norm(want) < 1e-10, (d, n)
    got = cpu.to_mandel(cpu.spd_mean(cpu.from_mandel(cpu.stats_spd_pool(3)[:5])))
    np.testing.assert_allclose(got, stats["spd3_mean_mandel_n5"], rtol=0, atol=1e-10 * np.linalg.norm(got))


def test_sphere_mean_restatement_matches_the_reference(stats):
    """observed: <= 2.3e-16 per component"""
    for dim in cpu.STATS_SPHERE_DIMS:
        x = cpu.stats_sphere_pool(dim)
        for n in cpu.STATS_NS:
            want = stats[f"sph{dim}_mean_n{n}"]
            assert want.shape == (dim, 1)
            np.testing.assert_allclose(cpu.sphere_mean(x[:n]), want[:, 0], rtol=0, atol=1e-10, err_msg=f"dim {dim} N {n}")


def test_transport_restatements_match_the_reference(stats):
    """observed: <= 3.2e-14"""
    for d in cpu.STATS_SPD_TRANSPORT_DIMS:
        X = cpu.from_mandel(cpu.stats_spd_pool(d)[:2])
        P = cpu.spd_transport(X[0], X[1])
        np.testing.assert_allclose(P, stats[f"spd{d}_pt"], rtol=0, atol=1e-10)
        np.testing.assert_allclose(P, stats[f"spd{d}_pt_mandel"], rtol=0, atol=1e-10)
        np.testing.assert_allclose(P @ X[0] @ P.T, X[1], rtol=0, atol=1e-10 * np.linalg.norm(X[1]))
    for dim in cpu.STATS_SPHERE_TRANSPORT_DIMS:
        x = cpu.stats_sphere_pool(dim)[:2]
        P = cpu.sphere_transport(x[0], x[1])
        np.testing.assert_allclose(P, stats[f"sph{dim}_pt"], rtol=0, atol=1e-10)
        u = cpu.sphere_log(x[1:2], x[0])[0]                                  # the geodesic's own direction stays tangent and keeps its length
        assert abs((P @ u) @ x[1]) < 1e-14 and abs(np.linalg.norm(P @ u) - np.linalg.norm(u)) < 1e-14
        np.testing.assert_array_equal(cpu.sphere_transport(x[0], x[0]), np.eye(dim))


def test_mean_of_diagonal_matrices_is_the_geometric_mean():
    """commuting matrices: the mean is diag(exp(mean(log lam))), reached in one step; observed 2.2e-16"""
    rng = np.random.default_rng(5)
    lam = 0.1 * np.exp(rng.uniform(0.0, np.log(1e3), (37, 6)))
    X = np.einsum("nk,kl->nkl", lam, np.eye(6))
    want = np.diag(np.exp(np.mean(np.log(lam), axis=0)))
    np.testing.assert_allclose(cpu.spd_mean(X, iters=10), want, rtol=1e-13, atol=0)
    w = rng.uniform(0.1, 1.0, 37)
    want_w = np.diag(np.exp(w @ np.log(lam) / w.sum()))
    np.testing.assert_allclose(cpu.spd_mean(X, weights=w, iters=10), want_w, rtol=1e-13, atol=0)


def test_equal_weights_give_the_unweighted_mean():
    rng = np.random.default_rng(6)
    X = cpu.rand_spd(rng, 9, 4, 10.0)
    np.testing.assert_allclose(cpu.spd_mean(X, weights=np.full(9, 3.0)), cpu.spd_mean(X), rtol=1e-13, atol=0)
    np.testing.assert_allclose(cpu.spd_mean(X, start=X[3], iters=40), cpu.spd_mean(X, iters=40), rtol=1e-11, atol=0)    # converged: the start no longer shows
    x = cpu.rand_sphere(rng, 9, 5)
    np.testing.assert_allclose(cpu.sphere_mean(x, weights=np.full(9, 0.25)), cpu.sphere_mean(x), rtol=0, atol=1e-15)


def test_mean_entry_points_validate_on_the_host():
    """malformed arguments are refused before any HIP call (as tests/test_abi.py checks for the other entries)"""
    lib = _lib.load()
    E_ARG, E_DIM, OK = _lib.GABO_ERR_ARG, _lib.GABO_ERR_DIM, _lib.GABO_OK
    t = 10 * 11 // 2
    # data factors + L^-1, L + weight scale + one partial per chunk of 64 points
    assert lib.gabo_spd_frechet_mean_workspace_bytes(3, 129, 10) == (3 * 129 * t + 2 * 3 * t + 3 + 3 * 3 * t) * 8
    assert lib.gabo_spd_frechet_mean_workspace_bytes(1, 64, 2) == (64 * 3 + 2 * 3 + 1 + 3) * 8
    assert lib.gabo_spd_frechet_mean_workspace_bytes(1, 64, 11) == 0 and lib.gabo_spd_frechet_mean_workspace_bytes(1, 0, 5) == 0
    assert lib.gabo_sphere_karcher_mean_workspace_bytes(2, 65, 130) == (2 + 2 * 2 * 130) * 8
    assert lib.gabo_sphere_karcher_mean_workspace_bytes(2, 65, 513) == 0

    def spd(x=1, mean=1, ws=1, status=1, batch=1, n=4, d=5, iters=10, wsb=1 << 30):
        # (non-null pointers are dummies: every call below is refused before anything dereferences or launches)
        return lib.gabo_spd_frechet_mean(x or None, None, None, mean or None, None, batch, n, d, iters, ws or None, wsb, status or None, None)
    assert spd(n=0) == E_ARG and spd(n=-3) == E_ARG
    assert spd(d=1) == E_DIM and spd(d=11) == E_DIM and spd(d=33) == E_DIM
    assert spd(iters=-1) == E_ARG
    assert spd(batch=-1) == E_ARG
    assert spd(x=0) == E_ARG and spd(mean=0) == E_ARG and spd(ws=0) == E_ARG and spd(status=0) == E_ARG
    assert spd(wsb=lib.gabo_spd_frechet_mean_workspace_bytes(1, 4, 5) - 8) == E_ARG
    assert spd(batch=0) == OK

    def sph(x=1, mean=1, ws=1, batch=1, n=4, dim=5, iters=10, wsb=1 << 30):
        return lib.gabo_sphere_karcher_mean(x or None, None, None, mean or None, None, batch, n, dim, iters, ws or None, wsb, None)
    assert sph(n=0) == E_ARG
    assert sph(dim=1) == E_DIM and sph(dim=513) == E_DIM
    assert sph(iters=-1) == E_ARG and sph(batch=-2) == E_ARG
    assert sph(x=0) == E_ARG and sph(mean=0) == E_ARG and sph(ws=0) == E_ARG
    assert sph(wsb=lib.gabo_sphere_karcher_mean_workspace_bytes(1, 4, 5) - 8) == E_ARG
    assert sph(batch=0) == OK


def test_reference_names_are_exported():
    from gabotorch_amd.Riemannian_utils import spd_utils, sphere_utils
    for name in ("mean", "mean_mandel_vector", "parallel_transport_operator", "parallel_transport_operator_mandel_vector"):
        assert callable(getattr(spd_utils, name))
    for name in ("karcher_mean_sphere", "parallel_transport_operator"):
        assert callable(getattr(sphere_utils, name))
