"""The device SPD sampler (gabotorch_amd/csrc/spd_sample.hip: the register form spd_sample_reg_kernel<D> for d <= 8, the LDS form spd_sample_kernel for
d = 9 ... 16) against the oracle of its random stream, oracle.selection.spd_samples - Philox4x32-10 keyed by the 64-bit seed, counter = (64-bit sample
index, draw), Box-Muller, two Gram-Schmidt passes per column, the eigenvalues from the same draw counter.  Cases, bounds and their derivation:
tests/_spd_sampler_cases.py.  Everything goes through ops.spd_sample or the C ABI (gabo_spd_sample_range)."""
import numpy as np
import pytest
import torch

from gabotorch_amd import _lib, ops
from oracle import spd as ospd
from tests import _spd_sampler_cases as cases

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
K_SQRT2 = float("1.41421356237309504880")         # kSqrt2 of csrc/gabo_device.hpp as the compiler reads it
_drawn = {}


def device(seed, first, n, d, lo=cases.LO, hi=cases.HI, mandel=False):
    """ops.spd_sample on the host, launched once per argument set"""
    key = (seed, first, n, d, lo, hi, mandel)
    if key not in _drawn:
        a = ops.spd_sample(n, d, lo, hi, seed=seed, device=DEV, mandel=mandel, first=first).cpu().numpy()
        a.setflags(write=False)
        _drawn[key] = a
    return _drawn[key]


def ratios(seed, first, n, d):
    """error / bound of every sample of one case, and the oracle's (X, lam, kappa)"""
    X, lam, kappa = cases.oracle(seed, first, n, d)
    got = device(seed, first, n, d)
    assert got.shape == X.shape and np.isfinite(got).all()
    return np.abs(got - X).reshape(n, -1).max(1) / cases.bound(d, kappa), (X, lam, kappa)


@pytest.mark.parametrize("d", cases.ORDERS)
def test_every_order_draws_the_oracles_matrices(d):
    """130 samples (three blocks, the last with two lanes) of every order under both seeds: |X_dev - X_oracle|_max <= 16 d eps kappa_i max_eig per sample.

    Largest error / bound over both seeds on an MI355X, per d (first run; the oracle in plain double gives 0.17 at d = 2 falling to 0.002 at d = 16):
      d      1      2      3      4      5      6      7      8      9     10     11     12     13     14     15     16
      ratio  0.0938 0.0469 0.0283 0.0227 0.0105 0.0085 0.0055 0.0065 0.0060 0.0041 0.0040 0.0031 0.0027 0.0024 0.0023 0.0024
    The worst samples are well-conditioned ones (kappa 1 ... 3.4): the error there is the rounding of X itself, a few eps max_eig, which the factor d
    of the bound overstates; the samples with kappa in the hundreds and thousands (198949 at d = 16) sit further below their bound."""
    worst = 0.0
    for seed in cases.SEEDS:
        r, (X, lam, kappa) = ratios(seed, 0, cases.N, d)
        worst = max(worst, float(r.max()))
        i = int(np.argmax(r))
        print(f"spd sampler d={d} seed={seed:#x}: worst error/bound {r.max():.4f} at sample {i} (kappa {kappa[i]:.1f}, largest kappa {kappa.max():.1f})")
        assert (r <= 1.0).all(), (d, hex(seed), i, float(r[i]), float(kappa[i]))
    print(f"spd sampler d={d}: error/bound {worst:.4f}")


@pytest.mark.parametrize("d", cases.ORDERS)
def test_spectrum_symmetry_and_a_single_sample(d):
    """What does not scale with kappa: the eigenvalues of the device's matrices are the oracle's draws to 64 d eps max_eig, the matrix output is
    symmetric to the last bit, and a launch of one sample gives sample 0."""
    for seed in cases.SEEDS:
        got = device(seed, 0, cases.N, d)
        lam = cases.oracle(seed, 0, cases.N, d)[1]
        np.testing.assert_array_equal(got, got.transpose(0, 2, 1))
        np.testing.assert_allclose(np.linalg.eigvalsh(got), np.sort(lam, axis=1), rtol=0, atol=cases.spectrum_bound(d))
        np.testing.assert_array_equal(device(seed, 0, 1, d), got[:1])


@pytest.mark.parametrize("d", cases.ORDERS)
def test_equal_bounds_give_that_multiple_of_the_identity(d):
    """min_eig == max_eig == 2: X = 2 Q Q^T, so |X - 2 I| <= 16 d eps 2 measures the orthogonality of Q alone, whatever the conditioning of the Gaussian
    matrix.  This is the check a Gram-Schmidt with ONE pass fails (orthogonality lost in proportion to kappa; the eigenvalues of Q diag(lam) Q^T move
    only at second order then, and the kappa-scaled bound forgives it): 2050 samples per seed, so that kappa reaches the thousands at every d >= 2 -
    the same statements in double with one pass exceed this bound 9 to 800 times there, with two passes they stay below 0.1 of it."""
    n = 2050
    for seed in cases.SEEDS:
        got = device(seed, 0, n, d, 2.0, 2.0)
        err = np.abs(got - 2.0 * np.eye(d)).reshape(n, -1).max(1)
        assert err.max() <= 16 * d * cases.EPS * 2.0, (d, hex(seed), int(np.argmax(err)), float(err.max()))
        np.testing.assert_array_equal(device(seed, 0, cases.N, d, 2.0, 2.0), got[:cases.N])
        _drawn.pop((seed, 0, n, d, 2.0, 2.0, False))


@pytest.mark.parametrize("d", cases.ORDERS)
def test_mandel_output_is_the_matrix_output_entry_by_entry(d):
    """mandel=1 stores the same sums: the diagonal bit for bit, every off-diagonal entry times kSqrt2 (one IEEE multiplication) bit for bit, at
    mandel_pos - the main diagonal first, then super-diagonal 1, 2, ... (oracle.spd.mandel_index / vector_to_symmetric_matrix_mandel)"""
    r, c = ospd.mandel_index(d)
    for seed in cases.SEEDS:
        mat, vec = device(seed, 0, cases.N, d), device(seed, 0, cases.N, d, mandel=True)
        assert vec.shape == (cases.N, d * (d + 1) // 2)
        np.testing.assert_array_equal(vec[:, :d], mat[:, np.arange(d), np.arange(d)])
        np.testing.assert_array_equal(vec, mat[:, r, c] * np.where(r == c, 1.0, K_SQRT2))
        # (the oracle's inverse map multiplies by the rounded 1 / sqrt(2): two roundings per entry)
        np.testing.assert_allclose(ospd.vector_to_symmetric_matrix_mandel(vec), mat, rtol=0, atol=2 * cases.EPS * cases.HI)


@pytest.mark.parametrize("d", [5, 8, 9, 16])
def test_a_range_is_that_slice_of_the_whole_draw(d):
    """samples 37 ... 86 drawn alone are rows 37 ... 86 of a draw of 200, bit for bit, in both output forms - and they land at the START of the buffer
    handed over, nowhere else (the C ABI on a NaN-filled buffer with room behind the 50 rows)"""
    seed = cases.SEEDS[1]
    lib = _lib.load()
    for mandel in (False, True):
        whole = device(seed, 0, 200, d, mandel=mandel)
        np.testing.assert_array_equal(device(seed, 37, 50, d, mandel=mandel), whole[37:87])
        width = whole[0].size
        buf = torch.full((200, width), float("nan"), dtype=torch.float64, device=DEV)
        assert lib.gabo_spd_sample_range(buf.data_ptr(), 37, 50, d, cases.LO, cases.HI, seed, int(mandel), ops._stream_ptr(torch.device(DEV))) == _lib.GABO_OK
        back = buf.cpu().numpy()
        np.testing.assert_array_equal(back[:50], whole[37:87].reshape(50, width))
        assert np.isnan(back[50:]).all()
        _drawn.pop((seed, 0, 200, d, cases.LO, cases.HI, mandel))


@pytest.mark.parametrize("d", [3, 10])
def test_the_sample_index_is_64_bits_wide(d):
    """first = 2^32 - 3, eight samples: the indices cross the counter's low word; the oracle's samples there, which are not samples 0 ... 4"""
    seed = cases.SEEDS[1]
    r, (X, lam, kappa) = ratios(seed, cases.FIRST_HIGH, 8, d)
    assert (r <= 1.0).all(), (d, r)
    got = device(seed, cases.FIRST_HIGH, 8, d)
    np.testing.assert_allclose(np.linalg.eigvalsh(got), np.sort(lam, axis=1), rtol=0, atol=cases.spectrum_bound(d))
    assert np.abs(got[3:8] - device(seed, 0, cases.N, d)[0:5]).max() > 0.1


@pytest.mark.parametrize("d", [4, 11])
@pytest.mark.parametrize("seed", [0, 2 ** 64 - 1, 1 << 32])
def test_the_seed_is_64_bits_wide(seed, d):
    """seed 0, the all-ones seed (the top bit through the c_uint64 binding) and a seed with only its high word set: the oracle's samples; the high word
    is part of the key (seed 1 << 32 is not seed 0)"""
    r, (X, lam, kappa) = ratios(seed, 0, cases.N, d)
    assert (r <= 1.0).all(), (hex(seed), d, float(r.max()))
    np.testing.assert_allclose(np.linalg.eigvalsh(device(seed, 0, cases.N, d)), np.sort(lam, axis=1), rtol=0, atol=cases.spectrum_bound(d))
    if seed == 1 << 32:
        assert np.abs(device(seed, 0, cases.N, d) - device(0, 0, cases.N, d)).max() > 0.1


def test_range_call_checks_its_arguments_before_it_launches():
    """gabo_spd_sample_range: GABO_ERR_DIM outside d = 1 ... 16; GABO_ERR_ARG for bounds that are not 0 < min <= max, a negative first or n, a null
    output with n > 0; GABO_OK for n = 0 without an output.  No refused call writes a byte of the buffer it was given."""
    lib = _lib.load()
    stream = ops._stream_ptr(torch.device(DEV))
    buf = torch.full((1024,), -7.0, dtype=torch.float64, device=DEV)           # (room for two samples of order 17, were one launched)
    nan = float("nan")

    def call(out, first, n, d, lo, hi, mandel=0):
        return lib.gabo_spd_sample_range(out, first, n, d, lo, hi, 5, mandel, stream)
    for d in (0, 17, -1):
        assert call(buf.data_ptr(), 0, 2, d, 0.3, 4.0) == _lib.GABO_ERR_DIM
    for lo, hi in ((0.0, 4.0), (-0.3, 4.0), (nan, 4.0), (0.3, nan), (nan, nan), (4.0, 0.3)):
        for mandel in (0, 1):
            assert call(buf.data_ptr(), 0, 2, 3, lo, hi, mandel) == _lib.GABO_ERR_ARG, (lo, hi)
    assert call(buf.data_ptr(), -1, 2, 3, 0.3, 4.0) == _lib.GABO_ERR_ARG
    assert call(buf.data_ptr(), 0, -1, 3, 0.3, 4.0) == _lib.GABO_ERR_ARG
    assert call(None, 0, 2, 3, 0.3, 4.0) == _lib.GABO_ERR_ARG
    assert call(None, 0, 0, 3, 0.3, 4.0) == _lib.GABO_OK
    assert call(buf.data_ptr(), 0, 0, 3, 0.3, 4.0) == _lib.GABO_OK
    assert lib.gabo_spd_sample(None, 2, 3, 0.3, 4.0, 5, 0, stream) == _lib.GABO_ERR_ARG
    torch.cuda.synchronize()
    assert bool((buf == -7.0).all())
    with pytest.raises(RuntimeError, match="unsupported dimension"):
        ops.spd_sample(2, 17, 0.3, 4.0, seed=5, device=DEV)
    # an accepted call on the same buffer does write: two samples, the rest untouched
    assert call(buf.data_ptr(), 0, 2, 3, 0.3, 4.0) == _lib.GABO_OK
    back = buf.cpu().numpy()
    np.testing.assert_array_equal(back[:18].reshape(2, 3, 3), device(5, 0, 2, 3))
    assert (back[18:] == -7.0).all()


def test_the_native_sweep_scores_the_samplers_rows():
    """One device_rand native sweep (64 restarts, 256 raw samples, d = 3): rows 1 ... 256 of its raw-row table hold [value, Mandel vector], and the
    vectors are ops.spd_sample's for the seed the sweep drew from numpy - spd_sample_rows with the table's row stride, bit for bit."""
    from gabotorch_amd.manifold_optimization import manifold_optimize as mo
    from tools.sweep_bench import run_sweep
    d, raw = 3, 256
    _, best, val, log = run_sweep("cuda:0", num_restarts=64, raw_samples=raw, d=d, device_rand=True, builtin_constraint=True, native_sweep=True, maxiter=20)
    assert log.get("native_sweep") and log.get("device_selection") and np.isfinite(val)
    np.random.seed(1234)
    seed = int(np.random.randint(0, 2 ** 63 - 1, dtype=np.int64))      # what _native_sweep drew after np.random.seed(1234) in tools.sweep_bench.run_sweep
    states = [v for v in mo._sweep_workspaces.values() if isinstance(v, mo._RowsState) and v.key[0] == d]
    assert len(states) == 1 and states[0].raw.shape == (raw + 1, 1 + d * (d + 1) // 2)
    table = states[0].raw.cpu().numpy()
    want = ops.spd_sample(raw, d, 1e-3, 5.0, seed=seed, device=DEV, mandel=True).cpu().numpy()      # (run_sweep's eigenvalue range)
    np.testing.assert_array_equal(table[1:, 1:], want)
    assert np.isfinite(table[1:, 0]).all()
