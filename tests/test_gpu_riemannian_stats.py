"""Frechet / Karcher means and parallel transport on the device (csrc/riemannian_mean.hip, ops.spd_frechet_mean, ops.sphere_karcher_mean and the
reference-named functions of Riemannian_utils) against the reference's recorded outputs (tests/golden/riemannian_stats.npz), against the composed
device path, and against closed forms.  Every case is a few milliseconds of device work.

Block layout the shapes are chosen for (riemannian_mean.hip, MeanPlan): lane = data point, chunks of 64; a set of N <= 64 points is one block, N = 65 the
smallest with two, N = 129 leaves the last block one point of its chunk; a block loops over several chunks only when sets x chunks exceeds the wave
slots of the device (2048 on 256 CUs at two waves per SIMD): 700 sets of 129 points."""
import numpy as np
import pytest
import torch

from gabotorch_amd import ops
from gabotorch_amd.Riemannian_utils import spd_utils, sphere_utils
from tests import _cpu_riemannian_stats as cpu

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def stats(golden):
    return golden("riemannian_stats.npz")


def unit(x):
    return x / np.sqrt(np.sum(x * x, axis=-1, keepdims=True))


def dev(a):
    return torch.tensor(np.asarray(a, dtype=np.float64), device=DEV)


def rel(got, want):
    return float(np.linalg.norm(got - want) / np.linalg.norm(want))


# ---------------------------------------------------------------------------------------------------------------- SPD mean against the reference
@pytest.mark.parametrize("d", [2, 3, 5, 8, 9, 10])
def test_fused_spd_mean_matches_the_reference(stats, d):
    """1e-9 relative Frobenius norm, the bar for kernel values against the oracle (test_gpu_parity.py); the numpy restatement stays <= 2.7e-13 of the reference on these inputs"""
    pool = cpu.stats_spd_pool(d)
    for n in cpu.STATS_NS:
        got = ops.spd_frechet_mean(dev(pool[:n]), iters=10, fused=True)
        assert got.shape == (pool.shape[1],) and got.dtype == torch.float64 and got.device.type == "cuda"
        err = rel(cpu.from_mandel(got.cpu().numpy()), stats[f"spd{d}_mean_n{n}"])
        print(f"fused d={d} N={n}: {err:.2e}")
        assert err < 1e-9, (d, n, err)


@pytest.mark.parametrize("d", [2, 3, 5, 8, 9, 10, 12, 16])
def test_composed_spd_mean_matches_the_reference(stats, d):
    pool = cpu.stats_spd_pool(d)
    for n in cpu.STATS_NS:
        got = ops.spd_frechet_mean(dev(pool[:n]), iters=10, fused=False if d <= 10 else None)
        err = rel(cpu.from_mandel(got.cpu().numpy()), stats[f"spd{d}_mean_n{n}"])
        print(f"composed d={d} N={n}: {err:.2e}")
        assert err < 1e-9, (d, n, err)


def test_fused_is_refused_above_its_dimensions():
    x = dev(cpu.to_mandel(cpu.rand_spd(np.random.default_rng(0), 4, 11, 10.0)))
    with pytest.raises(RuntimeError, match="d <= 10"):
        ops.spd_frechet_mean(x, fused=True)
    assert ops.spd_frechet_mean(x).shape == (66,)


# ---------------------------------------------------------------------------------------------------------------- fused against composed
def _three_sets(d, n, seed):
    rng = np.random.default_rng(seed)
    return np.stack([cpu.to_mandel(cpu.rand_spd(rng, n, d, c)) for c in (10.0, 100.0, 1e3)])


@pytest.mark.parametrize("d", [3, 8, 9, 10])
def test_fused_matches_composed_on_batched_weighted_sets(d):
    """Two device implementations of the same iteration on the same inputs: B = 3 sets of different spread in one call (batch strides), random
    weights, weights with zeros, a given start.  Bound 1e-10 relative: both are fp64, their eigen-solvers differ; an order below the bar against
    the reference, two to three above what the reference's own non-symmetric eig leaves on such spreads (2.7e-13)."""
    n = 129
    x = _three_sets(d, n, 100 + d)
    rng = np.random.default_rng(7)
    w = rng.uniform(0.1, 1.0, (3, n))
    wz = w.copy()
    wz[:, ::3] = 0.0
    wz[1, 64:] = 0.0                         # a whole block of set 1 without weight
    start = np.stack([cpu.to_mandel(cpu.rand_spd(rng, 1, d, 10.0)[0]) for _ in range(3)])
    for name, kw in (("plain", {}), ("weights", {"weights": dev(w)}), ("zeros", {"weights": dev(wz)}), ("start", {"start": dev(start)}),
                     ("both", {"weights": dev(w), "start": dev(start)})):
        a, ra = ops.spd_frechet_mean(dev(x), iters=10, return_residual=True, fused=True, **kw)
        b, rb = ops.spd_frechet_mean(dev(x), iters=10, return_residual=True, fused=False, **kw)
        assert a.shape == b.shape == (3, x.shape[-1]) and ra.shape == rb.shape == (3, 10)
        for s in range(3):
            err = rel(cpu.from_mandel(a[s].cpu().numpy()), cpu.from_mandel(b[s].cpu().numpy()))
            print(f"d={d} {name} set {s}: fused vs composed {err:.2e}")
            assert err < 1e-10, (d, name, s, err)
        np.testing.assert_allclose(ra.cpu().numpy(), rb.cpu().numpy(), rtol=1e-8, atol=1e-11)
    # a batched call is the single-set calls side by side
    single = torch.stack([ops.spd_frechet_mean(dev(x[s]), weights=dev(w[s])) for s in range(3)])
    assert torch.equal(single, ops.spd_frechet_mean(dev(x), weights=dev(w)))
    # the CPU restatement with weights and start (one set)
    want = cpu.spd_mean(cpu.from_mandel(x[2]), weights=w[2], start=cpu.from_mandel(start[2]))
    assert rel(cpu.from_mandel(ops.spd_frechet_mean(dev(x[2]), weights=dev(w[2]), start=dev(start[2])).cpu().numpy()), want) < 1e-10


def test_blocks_that_loop_over_several_chunks():
    """700 sets x 3 chunks exceed the device's wave slots: a block takes two chunks (the loop inside a block), the set's second block the partial third"""
    rng = np.random.default_rng(11)
    x = cpu.to_mandel(cpu.rand_spd(rng, 700 * 129, 2, 10.0)).reshape(700, 129, 3)
    a = ops.spd_frechet_mean(dev(x), iters=4, fused=True).cpu().numpy()
    b = ops.spd_frechet_mean(dev(x), iters=4, fused=False).cpu().numpy()
    err = np.max(np.linalg.norm(a - b, axis=1) / np.linalg.norm(b, axis=1))
    print(f"700 x 129, d = 2: fused vs composed {err:.2e}")
    assert err < 1e-10
    s = np.stack([cpu.rand_sphere(rng, 129, 3) for _ in range(700)])
    got = ops.sphere_karcher_mean(dev(s), iters=4).cpu().numpy()
    for k in (0, 350, 699):
        np.testing.assert_allclose(got[k], cpu.sphere_mean(s[k], iters=4), rtol=0, atol=1e-12)


@pytest.mark.parametrize("d", [9, 10])
def test_blocks_that_loop_over_several_chunks_one_wave_per_simd(d):
    """the same loop in the instantiations with one wave per SIMD (half the slots: 1024 on 256 CUs): 400 sets x 3 chunks; a device with more
    slots runs the same case one chunk per block.  Three iterations of 51600 eigen-solves with vectors: a few milliseconds."""
    rng = np.random.default_rng(12 + d)
    x = cpu.to_mandel(cpu.rand_spd(rng, 400 * 129, d, 10.0)).reshape(400, 129, -1)
    w = rng.uniform(0.1, 1.0, (400, 129))
    a = ops.spd_frechet_mean(dev(x), weights=dev(w), iters=3, fused=True).cpu().numpy()
    b = ops.spd_frechet_mean(dev(x), weights=dev(w), iters=3, fused=False).cpu().numpy()
    err = np.max(np.linalg.norm(a - b, axis=1) / np.linalg.norm(b, axis=1))
    print(f"400 x 129, d = {d}: fused vs composed {err:.2e}")
    assert err < 1e-10


def test_sphere_blocks_that_loop_over_several_chunks_above_64_coordinates():
    """700 sets x 3 chunks at dim = 70: two coordinate slots per lane carried across the chunks of a block"""
    rng = np.random.default_rng(13)
    s = np.stack([cpu.rand_sphere(rng, 129, 70, 0.1) for _ in range(700)])
    got = ops.sphere_karcher_mean(dev(s), iters=4).cpu().numpy()
    for k in (0, 123, 699):
        np.testing.assert_allclose(got[k], cpu.sphere_mean(s[k], iters=4), rtol=0, atol=1e-12)


# ---------------------------------------------------------------------------------------------------------------- closed forms
@pytest.mark.parametrize("d", [2, 6, 10])
def test_mean_of_diagonal_matrices(d):
    rng = np.random.default_rng(20 + d)
    lam = 0.1 * np.exp(rng.uniform(0.0, np.log(1e3), (100, d)))
    X = np.einsum("nk,kl->nkl", lam, np.eye(d))
    w = rng.uniform(0.1, 1.0, 100)
    got = cpu.from_mandel(ops.spd_frechet_mean(dev(cpu.to_mandel(X))).cpu().numpy())
    np.testing.assert_allclose(got, np.diag(np.exp(np.mean(np.log(lam), axis=0))), rtol=1e-12, atol=1e-12 * 0.1)
    got = cpu.from_mandel(ops.spd_frechet_mean(dev(cpu.to_mandel(X)), weights=dev(w)).cpu().numpy())
    np.testing.assert_allclose(got, np.diag(np.exp(w @ np.log(lam) / w.sum())), rtol=1e-12, atol=1e-12 * 0.1)


@pytest.mark.parametrize("d", [3, 8, 10])
def test_congruence_invariance_and_residual(d):
    """mean(A X_j A^T) = A mean(X_j) A^T on tightly clustered data (c = 10) after 40 iterations, where the iteration has converged (10 against 40
    iterations agree to 1e-12 there); A = I + 0.3 randn / sqrt(d) is well conditioned, the bound 1e-10 leaves cond(A)^2 x the 1e-12 of convergence.
    The residual - the norm of the mean tangent each iteration starts from - falls from iteration to iteration until it reaches rounding
    (1e-13: d x N x eps of O(1) logarithms) and ends below 1e-10."""
    rng = np.random.default_rng(30 + d)
    X = cpu.rand_spd(rng, 70, d, 10.0)
    A = np.eye(d) + 0.3 * rng.standard_normal((d, d)) / np.sqrt(d)
    m, r = ops.spd_frechet_mean(dev(cpu.to_mandel(X)), iters=40, return_residual=True)
    m = cpu.from_mandel(m.cpu().numpy())
    AX = A @ X @ A.T
    ma = cpu.from_mandel(ops.spd_frechet_mean(dev(cpu.to_mandel(0.5 * (AX + AX.transpose(0, 2, 1)))), iters=40).cpu().numpy())
    err = rel(ma, A @ m @ A.T)
    r = r.cpu().numpy()
    print(f"d={d}: congruence {err:.2e}; residuals {r[:8]} ... {r[-1]:.2e}")
    assert err < 1e-10
    assert r.shape == (40,) and r[-1] < 1e-10
    for k in range(39):
        assert r[k + 1] < r[k] or r[k] <= 1e-13, (k, r[k], r[k + 1])
    assert rel(cpu.from_mandel(ops.spd_frechet_mean(dev(cpu.to_mandel(X)), iters=10).cpu().numpy()), m) < 1e-11


@pytest.mark.parametrize("d", [2, 9])
def test_one_point_is_its_own_mean_and_zero_iterations_return_the_start(d):
    rng = np.random.default_rng(40 + d)
    x = cpu.to_mandel(cpu.rand_spd(rng, 5, d, 1e3))
    # (log of L^-1 X L^-T = I + cond(X) eps, ten times: 1e3 x 1e-16 x 10)
    np.testing.assert_allclose(ops.spd_frechet_mean(dev(x[:1])).cpu().numpy(), x[0], rtol=0, atol=1e-12 * np.linalg.norm(x[0]))
    assert np.array_equal(ops.spd_frechet_mean(dev(x), iters=0).cpu().numpy(), x[0])
    assert np.array_equal(ops.spd_frechet_mean(dev(x), iters=0, start=dev(x[3])).cpu().numpy(), x[3])
    m, r = ops.spd_frechet_mean(dev(x), iters=0, return_residual=True)
    assert r.shape == (0,)
    # CPU tensors in, CPU tensor out
    out = ops.spd_frechet_mean(torch.tensor(x))
    assert out.device.type == "cpu" and out.shape == (x.shape[1],)


# ---------------------------------------------------------------------------------------------------------------- reproducibility and errors
def test_spd_mean_has_the_same_bits_from_run_to_run():
    x = dev(cpu.to_mandel(cpu.rand_spd(np.random.default_rng(50), 1000, 10, 1e3)))
    w = dev(np.random.default_rng(51).uniform(0.1, 1.0, 1000))
    a, ra = ops.spd_frechet_mean(x, weights=w, return_residual=True)
    b, rb = ops.spd_frechet_mean(x, weights=w, return_residual=True)
    assert torch.equal(a, b) and torch.equal(ra, rb)
    assert torch.isfinite(a).all()


def test_non_spd_data_raises(raising):
    x = cpu.to_mandel(cpu.rand_spd(np.random.default_rng(60), 70, 3, 10.0))
    x[66, :3] = [1.0, -2.0, 1.0]                 # a negative diagonal entry
    with raising("not positive definite"):
        ops.spd_frechet_mean(dev(x))
    good = cpu.to_mandel(cpu.rand_spd(np.random.default_rng(61), 4, 3, 10.0))
    with raising("start point / an iterate of set #0 is not positive definite"):
        ops.spd_frechet_mean(dev(good), start=dev(x[66]))


@pytest.mark.parametrize("d", [3, 10])
def test_nan_input_gives_nan_without_a_hang(raising, d):
    """the eigen-solver's sweep cap holds on NaN (60 sweeps per stage, as in the backward kernel): the chain ends and the mean is NaN; under both
    error modes the NaN is reported as a data matrix that is not positive definite, as by the other SPD entries"""
    x = cpu.to_mandel(cpu.rand_spd(np.random.default_rng(70), 65, d, 10.0))
    x[64, 1] = np.nan
    with raising("input matrix #64 is not positive definite"):
        out = ops.spd_frechet_mean(dev(x), iters=3)
        if raising.mode == "deferred":                      # (in this mode the call returns: the launches have run to their end)
            assert torch.isnan(out).all()
    ops.set_error_checking(False)
    assert torch.isnan(ops.spd_frechet_mean(dev(x), iters=3)).all()


@pytest.mark.parametrize("d", [3, 12])
def test_composed_path_reports_non_spd_input_like_the_fused_one(raising, d):
    """fused=False and d >= 11: the same status word, written on the device, with the same messages"""
    rng = np.random.default_rng(71)
    x = cpu.to_mandel(cpu.rand_spd(rng, 70, d, 10.0))
    good = x[:4].copy()
    x[66, :3] = [1.0, -2.0, 1.0]
    with raising("gabo_spd_frechet_mean: input matrix #66 is not positive definite"):
        ops.spd_frechet_mean(dev(x), fused=False)
    with raising("start point / an iterate of set #0 is not positive definite"):
        ops.spd_frechet_mean(dev(good), start=dev(x[66]), fused=False)
    nan = good.copy()
    nan[2, 1] = np.nan
    with raising("gabo_spd_frechet_mean: input matrix #2 is not positive definite"):
        ops.spd_frechet_mean(dev(nan), fused=False)
    batched = np.stack([good, x[64:68]])                 # the offender is matrix 2 of set 1: index 4 + 2
    with raising("input matrix #6 is not positive definite"):
        ops.spd_frechet_mean(dev(batched), fused=False)
    with raising("input matrix #6 is not positive definite"):
        ops.spd_frechet_mean(dev(batched))               # fused at d = 3, composed at d = 12


def test_a_point_of_weight_zero_is_skipped():
    """a zero weight takes the point out of the sum whatever its logarithm is - here NaN (with error checking off: a NaN data matrix raises the
    status word whatever its weight): the mean is that of the other points, where a product with the weight would have made it NaN"""
    rng = np.random.default_rng(72)
    d, n = 4, 70
    X = cpu.rand_spd(rng, n, d, 10.0)
    X[65, 1, 2] = X[65, 2, 1] = np.nan
    w = rng.uniform(0.1, 1.0, n)
    w[65] = 0.0
    keep = np.arange(n) != 65
    ops.set_error_checking(False)
    for fused in (True, False):
        got = ops.spd_frechet_mean(dev(cpu.to_mandel(X)), weights=dev(w), fused=fused).cpu().numpy()
        want = ops.spd_frechet_mean(dev(cpu.to_mandel(X[keep])), weights=dev(w[keep]), fused=fused).cpu().numpy()
        assert np.isfinite(got).all()
        assert rel(got, want) < 1e-12, fused
    x = cpu.rand_sphere(rng, n, 5)
    x[65, 3] = np.nan
    got = ops.sphere_karcher_mean(dev(x), weights=dev(w)).cpu().numpy()
    want = ops.sphere_karcher_mean(dev(x[keep]), weights=dev(w[keep])).cpu().numpy()
    assert np.isfinite(got).all()
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-14)


# ---------------------------------------------------------------------------------------------------------------- sphere
@pytest.mark.parametrize("dim", [2, 3, 10, 64, 65, 130, 512])
def test_sphere_mean_matches_the_reference(stats, dim):
    """1e-10 per component (the bar for distances); unit norm to 1e-14"""
    x = cpu.stats_sphere_pool(dim)
    for n in cpu.STATS_NS:
        got = ops.sphere_karcher_mean(dev(x[:n]), iters=10)
        assert got.shape == (dim,) and got.dtype == torch.float64
        got = got.cpu().numpy()
        err = np.abs(got - stats[f"sph{dim}_mean_n{n}"][:, 0]).max()
        print(f"sphere dim={dim} N={n}: {err:.2e}, | |m| - 1 | = {abs(np.linalg.norm(got) - 1.0):.1e}")
        assert err < 1e-10, (dim, n, err)
        assert abs(np.linalg.norm(got) - 1.0) < 1e-14


def test_sphere_mean_of_a_symmetric_set_is_the_axis():
    rng = np.random.default_rng(80)
    dim = 7
    axis = rng.standard_normal(dim)
    axis /= np.linalg.norm(axis)
    v = rng.standard_normal((40, dim))
    v -= np.outer(v @ axis, axis)
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    ang = rng.uniform(0.1, 1.0, 40)
    x = np.concatenate([np.cos(ang)[:, None] * axis + np.sin(ang)[:, None] * v, np.cos(ang)[:, None] * axis - np.sin(ang)[:, None] * v])
    # started at x[0], 0.1 .. 1 rad off the axis; an iteration contracts the error by 1 - mean(theta cot theta) < 0.2: 30 of them reach rounding,
    # which is 80 points x eps
    got = ops.sphere_karcher_mean(dev(x), iters=30).cpu().numpy()
    np.testing.assert_allclose(got, axis, rtol=0, atol=1e-13)


def test_sphere_mean_weights_start_batch_and_bits():
    rng = np.random.default_rng(81)
    dim, n = 11, 129
    x = np.stack([cpu.rand_sphere(rng, n, dim, s) for s in (0.1, 0.3, 0.5)])
    w = rng.uniform(0.1, 1.0, (3, n))
    w[:, ::4] = 0.0
    start = np.stack([cpu.rand_sphere(rng, 1, dim)[0] for _ in range(3)])
    # the start points lie near other centres: keep them on the data's side of the sphere
    start = unit(start + 2.0 * x.mean(axis=1))
    got, r = ops.sphere_karcher_mean(dev(x), weights=dev(w), start=dev(start), iters=10, return_residual=True)
    again, r2 = ops.sphere_karcher_mean(dev(x), weights=dev(w), start=dev(start), iters=10, return_residual=True)
    assert torch.equal(got, again) and torch.equal(r, r2)
    assert got.shape == (3, dim) and r.shape == (3, 10)
    for s in range(3):
        want, rw = cpu.sphere_mean(x[s], weights=w[s], start=start[s], iters=10, return_residual=True)
        np.testing.assert_allclose(got[s].cpu().numpy(), want, rtol=0, atol=1e-12)
        np.testing.assert_allclose(r[s].cpu().numpy(), rw, rtol=0, atol=1e-12)
        assert torch.equal(got[s], ops.sphere_karcher_mean(dev(x[s]), weights=dev(w[s]), start=dev(start[s])))
    assert np.array_equal(ops.sphere_karcher_mean(dev(x), iters=0).cpu().numpy(), x[:, 0])
    assert np.array_equal(ops.sphere_karcher_mean(dev(x), iters=0, start=dev(start)).cpu().numpy(), start)
    nan = x[0].copy()
    nan[70, 2] = np.nan
    assert torch.isnan(ops.sphere_karcher_mean(dev(nan), iters=3)).all()


# ---------------------------------------------------------------------------------------------------------------- the reference's names
def test_reference_named_spd_functions(stats):
    pool = cpu.stats_spd_pool(3)
    X = cpu.from_mandel(pool)
    m = spd_utils.mean(X[:65], nb_iter=10)
    assert isinstance(m, np.ndarray) and m.shape == (3, 3) and m.dtype == np.float64
    assert rel(m, stats["spd3_mean_n65"]) < 1e-9
    mv = spd_utils.mean_mandel_vector(np.ascontiguousarray(pool[:5].T), nb_iter=10)        # points in COLUMNS
    assert mv.shape == (6,) and mv.dtype == np.float64
    assert rel(mv, stats["spd3_mean_mandel_n5"]) < 1e-9
    for d in cpu.STATS_SPD_TRANSPORT_DIMS:
        v = cpu.stats_spd_pool(d)[:2]
        S = cpu.from_mandel(v)
        P = spd_utils.parallel_transport_operator(S[0], S[1])
        assert P.shape == (d, d) and P.dtype == np.float64           # real by construction
        np.testing.assert_allclose(P, stats[f"spd{d}_pt"], rtol=0, atol=1e-10 * np.abs(stats[f"spd{d}_pt"]).max())
        assert rel(P @ S[0] @ P.T, S[1]) < 1e-10
        Pm = spd_utils.parallel_transport_operator_mandel_vector(v[0], v[1])
        np.testing.assert_allclose(Pm, stats[f"spd{d}_pt_mandel"], rtol=0, atol=1e-10 * np.abs(stats[f"spd{d}_pt"]).max())


def test_reference_named_sphere_functions(stats):
    x = cpu.stats_sphere_pool(10)
    m = sphere_utils.karcher_mean_sphere(np.ascontiguousarray(x[:65].T), nb_iter=10)       # points in COLUMNS
    assert m.shape == (10, 1) and m.dtype == np.float64
    np.testing.assert_allclose(m, stats["sph10_mean_n65"], rtol=0, atol=1e-10)
    for dim in cpu.STATS_SPHERE_TRANSPORT_DIMS:
        p = cpu.stats_sphere_pool(dim)[:2]
        P = sphere_utils.parallel_transport_operator(p[0], p[1])
        assert P.shape == (dim, dim) and P.dtype == np.float64
        np.testing.assert_allclose(P, stats[f"sph{dim}_pt"], rtol=0, atol=1e-10)
        np.testing.assert_allclose(sphere_utils.parallel_transport_operator(p[0][:, None], p[1][:, None]), P, rtol=0, atol=1e-15)
        assert np.array_equal(sphere_utils.parallel_transport_operator(p[0], p[0]), np.eye(dim))      # the reference's shortcut (:107)
