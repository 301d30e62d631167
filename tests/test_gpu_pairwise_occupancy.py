"""The Gaussian-only d = 10 instantiation of the SPD pairwise kernel (spd_ai_pairwise_kernel<10, true, true>, the benchmark's launch) at the
smallest shapes where a mistake in its register budget would show: a spilled or clobbered register corrupts a value that is live across the pair
body - the row counter, a lane's store bound, its output address, the row of W - so every case has lanes that must not store, more than one row
per lane, or both.  Needs an MI355X.

The occupancy the kernel is compiled for (spd_pair_gauss_only_waves, spd_pairwise_body.hpp) is a scheduling and register-allocation matter: the
order and association of every fp64 operation of a pair stay what they were.  test_bits_are_pinned holds the kernel to that: its output on a
stored input equals, bit for bit, what the kernel gave at commit c7b2296, two waves per SIMD (tests/golden/spd_ai_gauss_pin_d10.npz, written by
tools/gen_spd_ai_gauss_pin.py; the inputs are stored with the outputs because a QR factorisation is not reproducible to the bit across LAPACK
builds).

Accuracy is judged entry by entry against oracle.spd.spd_ai_gaussian_kernel with the bounds of tests/test_gpu_pairwise_gauss_finish.py for its
`bench` block (imported, not restated): err <= atol or err <= rtol |reference|.
"""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests.test_gpu_pairwise_gauss_finish import BETA, NONPD_COL, bounds, oracle, synthetic_spd_mandel  # noqa: E402

pytestmark = pytest.mark.gpu

D = 10
PIN = "spd_ai_gauss_pin_d10.npz"
PIN_N1, PIN_N2 = 9, 70       # nine rows; one full wave of columns and one whose lanes 6..63 are clamped to the last column and store nothing


def gram(x1, x2, **kw):
    """Gaussian values alone (no distance output: launch_spd_ai picks <10, true, true>); raises if the library reports anything"""
    import torch
    from gabotorch_amd import ops
    a = x1 if isinstance(x1, torch.Tensor) else torch.tensor(x1, device="cuda")
    b = x2 if isinstance(x2, torch.Tensor) else torch.tensor(x2, device="cuda")
    k = ops.spd_ai_pairwise(a, b, beta=BETA, **kw).cpu().numpy()
    ops.check_deferred()
    return k


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def assert_accurate(got, want, what):
    """every entry with a finite reference inside the `bench` bounds against the oracle; the caller has checked where the NaNs are"""
    atol, rtol = bounds("bench", "oracle")
    fin = np.isfinite(want)
    err, mag = np.abs(got[fin] - want[fin]), np.abs(want[fin])
    print(f"{what}: max abs err {err.max():.3e} (bound {atol:.3e}), max rel err {(err / mag).max():.3e} (bound {rtol:.3e})")
    ok = (err <= atol) | (err <= rtol * mag)
    assert ok.all(), f"{what}: {int((~ok).sum())} entries beyond atol {atol:.3e} / rtol {rtol:.3e}; worst abs {err.max():.3e}"


@pytest.fixture(scope="module")
def pin(golden):
    g = golden(PIN)
    return {k: g[k] for k in ("x1", "x2", "k")}


@pytest.fixture(scope="module")
def pin_out(pin):
    return gram(pin["x1"], pin["x2"])


def test_ragged_shape(pin, pin_out):
    """9 x 70: rows beyond the first of a chunk, a wave with clamped lanes, and a column of x2 that is not positive definite - that column is NaN
    in every row and its neighbours are numbers."""
    x1, x2, k = pin["x1"], pin["x2"], pin_out
    assert x1.shape == (PIN_N1, D * (D + 1) // 2) and x2.shape == (PIN_N2, D * (D + 1) // 2) and k.shape == (PIN_N1, PIN_N2)
    want = oracle(x1, x2)
    keep = np.arange(PIN_N2) != NONPD_COL
    assert np.isnan(k[:, NONPD_COL]).all() and np.isnan(want[:, NONPD_COL]).all()
    assert np.isfinite(k[:, keep]).all() and np.isfinite(want[:, keep]).all()
    assert_accurate(k, want, "ragged 9 x 70")


def test_bits_are_pinned(pin, pin_out):
    """the register budget moved registers, not arithmetic: the raw bits of the ragged case are those of the two-wave kernel at commit c7b2296"""
    assert pin_out.shape == pin["k"].shape
    same = bits(pin_out) == bits(pin["k"])
    assert same.all(), f"{int((~same).sum())} of {same.size} entries differ in their bits from the pinned output"


def test_symmetric_build():
    """x1 is x2, 130 points: tiles straddling the diagonal, the per-lane row bound and the mirror.  On and above the diagonal the bits of the full
    build; exactly symmetric."""
    n = 130
    x = synthetic_spd_mandel(n, D, 4101)
    full, sym = gram(x, x), gram(x, x, symmetric=True)
    assert full.shape == sym.shape == (n, n)
    iu = np.triu_indices(n)
    assert np.array_equal(bits(sym)[iu], bits(full)[iu])
    assert np.array_equal(bits(sym), bits(sym.T))
    assert np.isfinite(sym).all()
    assert_accurate(sym, oracle(x, x), "symmetric 130 x 130")


def test_batches():
    """two batches, x1 shared by both (batch stride 0) and x2 per batch, 8 x 64: each batch equals its own unbatched launch bit for bit"""
    import torch
    x1 = synthetic_spd_mandel(8, D, 4102)
    x2 = np.stack([synthetic_spd_mandel(64, D, 4103), synthetic_spd_mandel(64, D, 4104)])
    a = torch.tensor(x1, device="cuda").unsqueeze(0).expand(2, -1, -1)
    assert a.stride(0) == 0
    k = gram(a, torch.tensor(x2, device="cuda"))
    assert k.shape == (2, 8, 64) and np.isfinite(k).all()
    for b in range(2):
        assert np.array_equal(bits(k[b]), bits(gram(x1, x2[b])))
        assert_accurate(k[b], oracle(x1, x2[b]), f"batch {b} of 2, 8 x 64")


def test_eight_row_chunks(pin, pin_out):
    """launch_spd_ai shrinks the rows per block of a small launch down to one, so the cases above run the row loop once per block.  Here it keeps
    its eight (more than 4096 blocks): 521 x 4102, the pinned rows last - 65 full chunks and a one-row chunk - and the pinned columns first, behind
    them 63 further column groups and a ragged 65th.  A pair's bits depend on the launch's shape only through the 64 columns that share its wave
    (a lane that has converged idles or looks ahead while its wave finishes the stage, tridiag_eigenvalues), so wherever a wave holds the same
    columns in both launches - the first 64 pinned columns, and below the last 70 columns against launches of their own - the bits agree:
    whatever the row loop keeps across a pair body (row counter, store bound, output address, W row pointer) survived eight of them."""
    n1, n2 = 521, 4102
    x1 = np.concatenate([synthetic_spd_mandel(n1 - PIN_N1, D, 4105), pin["x1"]])
    x2 = np.concatenate([pin["x2"], synthetic_spd_mandel(n2 - PIN_N2, D, 4106)])
    k = gram(x1, x2)
    assert k.shape == (n1, n2)
    assert np.array_equal(bits(k[n1 - PIN_N1:, :64]), bits(pin["k"][:, :64]))
    assert_accurate(np.delete(k[n1 - PIN_N1:, :PIN_N2], NONPD_COL, axis=1), np.delete(oracle(pin["x1"], pin["x2"]), NONPD_COL, axis=1), "pinned block of 521 x 4102")
    keep = np.arange(n2) != NONPD_COL
    assert np.isnan(k[:, NONPD_COL]).all() and np.isfinite(k[:, keep]).all()
    # rows of a full chunk and the one-row chunk against single launches of their own, over the ragged last column group
    for lo, hi in ((0, 8), (n1 - PIN_N1, n1)):
        assert np.array_equal(bits(k[lo:hi, n2 - 70:]), bits(gram(x1[lo:hi], x2[n2 - 70:])))
