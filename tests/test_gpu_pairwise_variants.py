"""Every launch path of the SPD pairwise kernel against the others.  launch_spd_ai chooses between two instantiations of the kernel - Gaussian
values alone (own row loop, looser deflation threshold) and the general one (distance and Laplace modes, a distance output next to the values) -
and each runs with and without GABO_SYMMETRIC.  Needs an MI355X.

For d in 3, 10, 13 (table-assisted exp, the benchmark's dimension, the first dimension of the wide translation units) on the benchmark's generator:
a 40 x 300 block of x1 against x2 for the plain launches, the 300 x 300 block of x2 against itself for the symmetric ones.  Per block:

  * the distances - distance mode, the distance output written next to Gaussian values, the one written next to Laplace values - are the same
    bits in every launch that produces them: they share one finish;
  * Laplace values are the same bits with and without a distance output, and exp(-beta dist) of it to 2 ulp (the kernel's exp and the host's
    are each within 1 ulp of the true value of the same argument);
  * Gaussian values written next to a distance output are exp(-beta dist^2) of that output to 1 ulp;
  * Gaussian values alone agree with those within the bounds of test_gpu_pairwise_gauss_finish for the benchmark block against the host
    reference (imported, not restated);
  * a symmetric launch returns an exactly symmetric matrix whose upper triangle is, bit for bit, what the plain launch on the same square
    block gives (a pair's arithmetic does not depend on which rows its lane stores).
"""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests.test_gpu_pairwise_gauss_finish import BETA, N1, N2, bounds, synthetic_spd_mandel  # noqa: E402

pytestmark = pytest.mark.gpu

DIMS = (3, 10, 13)


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def _ulps(got, want):
    """largest |got - want| in units of the spacing of `want`"""
    return float(np.max(np.abs(got - want) / np.spacing(np.abs(want))))


def _launch_all(a, b, symmetric):
    """the seven outputs of the five launches as numpy arrays"""
    from gabotorch_amd import _lib, ops
    kw = dict(beta=BETA, symmetric=symmetric)
    k_only = ops.spd_ai_pairwise(a, b, **kw)
    k_with, d_gauss = ops.spd_ai_pairwise(a, b, return_dist=True, **kw)
    d_mode = ops.spd_ai_pairwise(a, b, mode=_lib.GABO_OUT_DISTANCE, symmetric=symmetric)
    lap = ops.spd_ai_pairwise(a, b, mode=_lib.GABO_OUT_LAPLACE, **kw)
    lap_with, d_lap = ops.spd_ai_pairwise(a, b, mode=_lib.GABO_OUT_LAPLACE, return_dist=True, **kw)
    ops.check_deferred()
    return tuple(t.cpu().numpy() for t in (k_only, k_with, d_gauss, d_mode, lap, lap_with, d_lap))


def _check_block(d, tag, outs, shape):
    k_only, k_with, d_gauss, d_mode, lap, lap_with, d_lap = outs
    for o in outs:
        assert o.shape == shape and np.isfinite(o).all()
    # one finish behind every distance
    assert np.array_equal(_bits(d_gauss), _bits(d_mode)), f"d={d} {tag}: distance output next to Gaussian values differs from distance mode"
    assert np.array_equal(_bits(d_lap), _bits(d_mode)), f"d={d} {tag}: distance output next to Laplace values differs from distance mode"
    assert np.array_equal(_bits(lap), _bits(lap_with)), f"d={d} {tag}: Laplace values change with the distance output"
    u_lap = _ulps(lap, np.exp(-(d_mode * BETA)))
    u_gauss = _ulps(k_with, np.exp(-((d_gauss * d_gauss) * BETA)))
    atol, rtol = bounds("bench", "host")
    err = np.abs(k_only - k_with)
    amax = float(err.max())
    rmax = float(np.max(err / np.abs(k_with)))
    print(f"d={d} {tag}: Laplace vs exp(-beta dist) {u_lap:.2f} ulp, Gaussian vs exp(-beta dist^2) {u_gauss:.2f} ulp, Gaussian-only vs with "
          f"distance output: max abs err {amax:.3e} (bound {atol:.3e}), max rel err {rmax:.3e} (bound {rtol:.3e})")
    assert u_lap <= 2.0, f"d={d} {tag}: Laplace values {u_lap:.2f} ulp from exp(-beta dist)"
    assert u_gauss <= 1.0, f"d={d} {tag}: Gaussian values {u_gauss:.2f} ulp from exp(-beta dist^2) of the distance output"
    ok = (err <= atol) | (err <= rtol * np.abs(k_with))
    assert ok.all(), (f"d={d} {tag}: {int((~ok).sum())} Gaussian-only entries beyond atol {atol:.3e} / rtol {rtol:.3e} of the launch with a "
                      f"distance output; worst abs {amax:.3e}, worst rel {rmax:.3e}")


@pytest.mark.parametrize("d", DIMS)
def test_launch_variants_agree(d):
    import torch
    x1, x2 = synthetic_spd_mandel(N1, d, 7000 + d), synthetic_spd_mandel(N2, d, 8000 + d)
    a, b = torch.tensor(x1, device="cuda"), torch.tensor(x2, device="cuda")
    plain = _launch_all(a, b, False)
    _check_block(d, "40 x 300", plain, (N1, N2))
    square = _launch_all(b, b, False)
    _check_block(d, "300 x 300", square, (N2, N2))
    sym = _launch_all(b, b, True)
    _check_block(d, "300 x 300 symmetric", sym, (N2, N2))
    upper = np.triu_indices(N2)
    names = ("Gaussian-only", "Gaussian with distance output", "distance output (Gaussian)", "distance mode", "Laplace",
             "Laplace with distance output", "distance output (Laplace)")
    for name, s, f in zip(names, sym, square):
        assert np.array_equal(_bits(s), _bits(s.T)), f"d={d} symmetric {name}: not symmetric"
        assert np.array_equal(_bits(s[upper]), _bits(f[upper])), f"d={d} symmetric {name}: upper triangle differs from the plain launch"
