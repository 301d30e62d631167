"""Error behaviour of the host layer and the C ABI on a GPU box (argument validation, shape contracts, dtype/device handling)."""
import numpy as np
import pytest
import torch

from gabotorch_amd import _lib, ops
from gabotorch_amd.kernel_utils.kernels_spd import SpdAffineInvariantGaussianKernel

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def test_shape_contracts():
    a = torch.rand(4, 6, dtype=torch.float64, device=DEV) + torch.tensor([3., 3, 3, 0, 0, 0], dtype=torch.float64, device=DEV)
    with pytest.raises(RuntimeError, match="not d\\(d\\+1\\)/2"):
        ops.spd_ai_pairwise(torch.ones(3, 7, device=DEV), torch.ones(3, 7, device=DEV))
    with pytest.raises(RuntimeError, match="shapes differ"):
        ops.spd_ai_pairwise(a[None].expand(2, 4, 6), a)                      # batch shapes must match (no broadcasting)
    with pytest.raises(RuntimeError, match="shapes differ"):
        ops.sphere_pairwise(torch.ones(3, 4, device=DEV), torch.ones(3, 5, device=DEV))
    with pytest.raises(RuntimeError, match="same length"):
        ops.sphere_pairwise(torch.ones(3, 4, device=DEV), torch.ones(2, 4, device=DEV), diag=True)
    # fp32 / CPU inputs are accepted, the result is fp64 on the caller's device
    k = ops.spd_ai_pairwise(a.float().cpu(), a.float().cpu(), beta=0.3)
    assert k.dtype == torch.float64 and k.device.type == "cpu" and k.shape == (4, 4)
    # non-contiguous views
    big = torch.zeros(4, 12, dtype=torch.float64, device=DEV)
    big[:, ::2] = a
    np.testing.assert_allclose(ops.spd_ai_pairwise(big[:, ::2], a, beta=0.3).cpu().numpy(), ops.spd_ai_pairwise(a, a, beta=0.3).cpu().numpy())


def test_c_abi_argument_errors_on_device():
    lib = _lib.load()
    x = torch.ones(2, 3, dtype=torch.float64, device=DEV)
    out = torch.empty(2, 2, dtype=torch.float64, device=DEV)
    st = torch.zeros(2, dtype=torch.int32, device=DEV)
    ws = torch.empty(64, dtype=torch.float64, device=DEV)
    # workspace too small / symmetric with n1 != n2 / negative sizes
    assert lib.gabo_spd_ai_pairwise(x.data_ptr(), x.data_ptr(), out.data_ptr(), None, 1, 2, 2, 2, 6, 6, 1.0, 0, ws.data_ptr(), 8, st.data_ptr(), None) == _lib.GABO_ERR_ARG
    assert lib.gabo_spd_ai_pairwise(x.data_ptr(), x.data_ptr(), out.data_ptr(), None, 1, 2, 1, 2, 6, 6, 1.0, _lib.GABO_SYMMETRIC, ws.data_ptr(), 512, st.data_ptr(), None) == _lib.GABO_ERR_ARG
    assert lib.gabo_spd_ai_pairwise(x.data_ptr(), x.data_ptr(), out.data_ptr(), None, -1, 2, 2, 2, 6, 6, 1.0, 0, ws.data_ptr(), 512, st.data_ptr(), None) == _lib.GABO_ERR_ARG
    assert lib.gabo_spd_manifold_op(99, x.data_ptr(), None, None, None, out.data_ptr(), None, 1, 2, None, None) == _lib.GABO_ERR_ARG
    assert lib.gabo_spd_project(x.data_ptr(), x.data_ptr(), out.data_ptr(), 1, 2, 65, None) == _lib.GABO_ERR_DIM
    assert lib.gabo_sphere_from_inner(x.data_ptr(), out.data_ptr(), 4, 1.0, 0, 3, None) == _lib.GABO_ERR_ARG


def test_device_solve_reports_a_non_spd_start():
    """The single-launch solve writes the device status word like every other entry point: a non-SPD starting matrix raises."""
    from gabotorch_amd import manifolds, models
    from gabotorch_amd.manifold_optimization.batched_trust_regions import BatchedTrustRegions
    from gabotorch_amd.manifold_optimization.manifold_optimize import gen_candidates_manifold
    from gabotorch_amd.Riemannian_utils.spd_utils_torch import symmetric_matrix_to_vector_mandel_torch, vector_to_symmetric_matrix_mandel_torch
    rng = np.random.default_rng(0)
    q = np.linalg.qr(rng.standard_normal((8, 3, 3)))[0]
    Xm = np.einsum("nab,nb,ncb->nac", q, rng.uniform(0.5, 2.0, (8, 3)), q)
    X = torch.tensor(Xm, device=DEV)
    xv = symmetric_matrix_to_vector_mandel_torch(X)
    gp = models.ExactGP(xv, torch.tensor(rng.standard_normal(8), device=DEV), SpdAffineInvariantGaussianKernel(beta_min=0.5), outputscale=1.0, noise=1e-2)
    acq = models.ExpectedImprovement(gp, best_f=0.0, maximize=False)
    bad = xv[:3].clone()
    bad[1, :3] = torch.tensor([1.0, -2.0, 1.0], dtype=torch.float64, device=DEV)        # a negative diagonal entry: not SPD
    with pytest.raises(RuntimeError, match="not positive definite"):
        gen_candidates_manifold(bad[:, None], acq, manifolds.PositiveDefinite(3), BatchedTrustRegions(maxiter=3),
                                vector_to_symmetric_matrix_mandel_torch, symmetric_matrix_to_vector_mandel_torch, approx_hessian=True)


def test_a_refused_solve_consumes_its_record_buffer():
    """gabo_tr_solve_record hands ONE pending buffer to the next single-launch solve.  A solve that is refused for its arguments must still
    consume it - otherwise the pointer would be written by a later, unrelated solve (possibly after the tensor is gone)."""
    from gabotorch_amd import manifolds, models
    from gabotorch_amd.manifold_optimization.batched_trust_regions import BatchedTrustRegions
    from gabotorch_amd.manifold_optimization.manifold_optimize import gen_candidates_manifold
    from gabotorch_amd.Riemannian_utils.spd_utils_torch import symmetric_matrix_to_vector_mandel_torch, vector_to_symmetric_matrix_mandel_torch
    lib = _lib.load()
    buf = torch.full((4, 3, 11), float("nan"), dtype=torch.float64, device=DEV)
    assert lib.gabo_tr_solve_record(buf.data_ptr(), 4) == _lib.GABO_OK
    # refused: d = 1
    assert lib.gabo_spd_tr_solve(None, None, None, None, None, None, None, None, 0, None, None, 0, None, 0, 3, 1, 1e-6, 1.0, 0.1, 1, 3, 1.0, 0.1,
                                 1e3, 1e-6, 10, None, None, None, 0, None, None) == _lib.GABO_ERR_DIM
    rng = np.random.default_rng(0)
    q = np.linalg.qr(rng.standard_normal((8, 3, 3)))[0]
    Xm = np.einsum("nab,nb,ncb->nac", q, rng.uniform(0.5, 2.0, (8, 3)), q)
    xv = symmetric_matrix_to_vector_mandel_torch(torch.tensor(Xm, device=DEV))
    gp = models.ExactGP(xv, torch.tensor(rng.standard_normal(8), device=DEV), SpdAffineInvariantGaussianKernel(beta_min=0.5), outputscale=1.0, noise=1e-2)
    acq = models.ExpectedImprovement(gp, best_f=0.0, maximize=False)
    solver = BatchedTrustRegions(maxiter=3)
    gen_candidates_manifold(xv[:3, None], acq, manifolds.PositiveDefinite(3), solver, vector_to_symmetric_matrix_mandel_torch,
                            symmetric_matrix_to_vector_mandel_torch, approx_hessian=True)
    torch.cuda.synchronize()
    assert "one_launch_solve" in solver.log and bool(torch.isnan(buf).all())
    # and withdrawing a pending buffer works
    assert lib.gabo_tr_solve_record(buf.data_ptr(), 4) == _lib.GABO_OK and lib.gabo_tr_solve_record(None, 0) == _lib.GABO_OK
    gen_candidates_manifold(xv[:3, None], acq, manifolds.PositiveDefinite(3), solver, vector_to_symmetric_matrix_mandel_torch,
                            symmetric_matrix_to_vector_mandel_torch, approx_hessian=True)
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf).all())


def _bad_and_good(rng, n=12, d=3, bad_row=5):
    q = np.linalg.qr(rng.standard_normal((n, d, d)))[0]
    m = np.einsum("nab,nb,ncb->nac", q, rng.uniform(0.5, 2.0, (n, d)), q)
    from oracle import spd as ospd
    good = ospd.symmetric_matrix_to_vector_mandel(0.5 * (m + m.transpose(0, 2, 1)))
    bad = good.copy()
    bad[bad_row, 0] = -1.0
    return torch.tensor(bad, device=DEV), torch.tensor(good, device=DEV)


def test_deferred_error_checking_does_not_synchronise_and_names_the_launch():
    """The default: a launch is handed a status word of its own and returns without waiting for the device; the RuntimeError the reference raises
    from torch.cholesky (spd_utils_torch.py:87) comes at the next synchronisation point, naming the launch and the matrix - and only that launch:
    the valid ones queued behind it stay valid."""
    assert ops.set_error_checking("deferred") == "deferred"            # (the default, restored by conftest)
    bad, good = _bad_and_good(np.random.default_rng(0))
    ops.spd_ai_pairwise(good, good)                                     # warm: workspaces, the stream's status ring
    torch.cuda.synchronize()
    try:
        torch.cuda.set_sync_debug_mode("error")                         # any synchronising call below raises
        guarded = True
    except Exception:                                                   # noqa: BLE001  (not available in this build: the assertion is skipped)
        guarded = False
    try:
        k_bad = ops.spd_ai_pairwise(bad, good, beta=0.7)                # no exception here, no wait
        k_good = ops.spd_ai_pairwise(good, good, beta=0.7)
    finally:
        if guarded:
            torch.cuda.set_sync_debug_mode("default")
    with pytest.raises(RuntimeError, match=r"gabo_spd_ai_pairwise: input matrix #5 is not positive definite"):
        ops.check_deferred()
    ops.check_deferred()                                                # the launch behind it was fine, and nothing is pending any more
    assert bool(torch.isfinite(k_good).all()) and k_bad.shape == (12, 12)
    # sync mode: at the call, as the reference
    ops.set_error_checking(True)
    with pytest.raises(RuntimeError, match="input matrix #5"):
        ops.spd_ai_pairwise(bad, good, beta=0.7)
    ops.spd_ai_pairwise(good, good, beta=0.7)
    # off: never
    ops.set_error_checking(False)
    ops.spd_ai_pairwise(bad, good, beta=0.7)
    ops.check_deferred()
    ops.set_error_checking("deferred")                                  # (coming back from False starts from clean words)
    ops.spd_ai_pairwise(good, good, beta=0.7)
    ops.check_deferred()


def test_deferred_errors_on_two_streams_are_attributed_to_their_launches():
    """One status ring per (device, stream): launches on different streams fail independently and each error names its own launch."""
    ops.set_error_checking("deferred")
    rng = np.random.default_rng(1)
    bad_a, good = _bad_and_good(rng, bad_row=3)
    bad_b, _ = _bad_and_good(rng, bad_row=7)
    sa, sb = torch.cuda.Stream(DEV), torch.cuda.Stream(DEV)
    torch.cuda.synchronize()
    with torch.cuda.stream(sa):
        ops.spd_ai_pairwise(good, good)
        ops.spd_ai_pairwise(bad_a, good)                                # stream A: the Gram launch fails at matrix 3
    with torch.cuda.stream(sb):
        ops.spd_acq_prepare_train(bad_b)                                # stream B: factoring a training set fails at matrix 7
        ops.spd_ai_pairwise(good, good)
    seen = []
    for _ in range(2):
        with pytest.raises(RuntimeError) as err:
            ops.check_deferred()
        seen.append(str(err.value))
    ops.check_deferred()                                                # both reported, nothing left
    assert any("gabo_spd_ai_pairwise: input matrix #3" in m for m in seen), seen
    assert any("gabo_spd_acq_prepare_train: input matrix #7" in m for m in seen), seen


def test_switching_error_checking_off_and_on_keeps_a_pending_failure():
    """What the hipGraph plan of BatchedTrustRegions does around its capture: a failed GP factor queued in front of it is still reported."""
    rng = np.random.default_rng(3)
    _, good = _bad_and_good(rng)
    y = torch.tensor(rng.standard_normal(12), device=DEV)
    k = ops.spd_ai_pairwise(good, good, beta=0.7) - 2.0 * torch.eye(12, dtype=torch.float64, device=DEV)        # K - 2 I: indefinite
    ops.check_deferred()
    ops.gp_factor(k, y, 1.0, 0.0, 0.0, defer_check=True)
    assert ops.set_error_checking(False) == "deferred"
    assert ops.set_error_checking("deferred") is False
    with pytest.raises(RuntimeError, match="not positive definite"):
        ops.check_deferred()
    ops.check_deferred()


def test_a_prefetch_token_overtaken_by_a_check_loses_no_later_error():
    """The token names its launches: checked by somebody else in the meantime, it has nothing left to say about the launches behind them."""
    bad, good = _bad_and_good(np.random.default_rng(0))
    ops.spd_ai_pairwise(good, good, beta=0.7)
    token = ops.prefetch_deferred()
    torch.cuda.synchronize()
    ops.check_deferred()
    ops.spd_ai_pairwise(bad, good, beta=0.7)
    torch.cuda.synchronize()
    ops.check_prefetched(token)                                         # silent: its one launch has been checked already
    with pytest.raises(RuntimeError, match=r"gabo_spd_ai_pairwise: input matrix #5 is not positive definite"):
        ops.check_deferred()
    ops.check_deferred()


def test_a_failed_factorisation_drops_the_models_cache():
    """models.ExactGP published its prediction cache before the Cholesky status was known; a caller that caught the RuntimeError and asked
    again got values computed from uninitialised memory.  The cache is now dropped before the error is raised, so the second request fails the same way."""
    from gabotorch_amd import models
    rng = np.random.default_rng(2)
    _, good = _bad_and_good(rng)
    y = torch.tensor(rng.standard_normal(12), device=DEV)
    gp = models.ExactGP(good, y, SpdAffineInvariantGaussianKernel(beta_min=0.5), outputscale=1.0, noise=-2.0)      # K - 2 I: indefinite
    for _ in range(2):
        with pytest.raises(RuntimeError, match="not positive definite"):
            gp.posterior(good[:3, None])
        assert gp._cache is None
    gp.noise = 1e-2
    mean, var = gp.posterior(good[:3, None])
    assert bool(torch.isfinite(mean).all()) and bool((var > -1e-9).all())
