"""The Gaussian-only launch of the SPD pairwise kernel where its QL iteration's per-sweep control can go wrong.  The comparison needs an MI355X; the
checks of the inputs do not.

`tridiag_eigenvalues` (csrc/spd_eig.hpp) runs the 64 lanes of a wave in lock step: a lane that has deflated e2[l] works ahead on block l + 1 while the
wave's slowest lane finishes stage l.  The fixed-orientation instantiations (`spd_ai_pairwise_kernel<D, true, true>`: Gaussian values, no distance
output - the Gram of a GP fit) take cheaper forms of that control (QlSweepCtl): a deflated e2[l] is cleared in its high word only and stays a
denormal, the shift's square root is the bare v_sqrt_f64, and whether a look-ahead lane sits a sweep out is decided against stage l's threshold.  All of them
change what a look-ahead lane does next to a slow one, never the arithmetic of a step - so this file holds the launch to the oracle on small
shapes in which such lanes exist: d in 3, 5, 10, 13 (one look-ahead stage, the smallest wide tile, the benchmark's dimension, the first dimension
of the second translation unit), N1 = 9 rows (not a multiple of the 8- or 16-row block) against N2 = 70 columns (a full wave and a partial one).

Blocks (fixed seeds; x1, x2 computed once per case and not modified):

  bench        the benchmark's generator (bench.synthetic_spd_mandel)
  near         x1 = x2 perturbed by 1e-6 relative: M = I + O(1e-6), every lane deflates at once and every select of the control is taken
  ratio1e6     eigenvalue ratio 1e6 in every matrix
  mixed        x1 identity-like (I + O(1e-6)); the columns of x2 alternate identity-like points with ratio-1e6 points: in every wave the fast lanes
               (M = I + O(1e-6)) run look-ahead beside lanes that need every sweep.  beta = BETA_MIXED = 0.01 here, so that the slow lanes' values
               are of order 0.01 - 1 and an absolute bound sees their sum log^2 lambda (at the benchmark's beta they are below 1e-40)
  tri_rising   x1 = I, x2 = SPD tridiagonal matrices graded rising / falling (tests/test_gpu_pairwise_orientation.py: they reach the QL as built,
  tri_falling  the falling ones with a clustered top block against the fixed orientation)

Column NONPD_COL of x2 is, in every block, a symmetric NaN-free matrix that is not positive definite: its factor is NaN in every entry (spd_prep.hpp),
the lane's QL runs on NaN for its full 60 sweeps per stage beside working neighbours, and its column of the result must be NaN, every other entry finite.

How an entry is judged: err <= atol or err <= rtol |reference| against oracle.spd.spd_ai_gaussian_kernel.  bench, near, ratio1e6: atol and rtol
are `bounds(block, "oracle")` of tests/test_gpu_pairwise_gauss_finish.py (imported, not restated; measured there on 40 x 300 pairs over six
dimensions).  mixed, tri_rising, tri_falling: 4 x the worst deviation of the PARENT of this change (commit b228f89: plain sweep control in every
instantiation) on exactly these inputs over the four dimensions, capped at the same atol 1e-12 / rtol 1e-9 - how the orientation test set its
bounds.  Measured on an MI355X (`python tests/test_gpu_ql_sweep_control.py` prints the figures of the library it finds, asserting nothing):

                     parent b228f89                     this change
  block          max abs err    max rel err         max abs err    max rel err
  mixed          2.128e-11      6.734e-11           2.161e-11      7.728e-11
  tri_rising     2.168e-18      3.522e-15           4.554e-18      3.522e-15
  tri_falling    4.662e-17      8.165e-14           3.144e-17      9.956e-14

(mixed: the deviations are the oracle's own - LAPACK finds an eigenvalue of 1e-3 next to 1e3 to 1e-10 relative, which is 1e-9 in sum log^2 and,
at beta = 0.01 and values of order 0.01 - 1, 1e-11 in K.  tri_rising: the absolute figure doubles and stands at 0.53 of 4 x the parent's, but
the entries are judged by either bound and every one of them is within 0.25 of the relative one.)
"""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import test_gpu_pairwise_gauss_finish as finish  # noqa: E402
from tests import test_gpu_pairwise_orientation as orient  # noqa: E402

DIMS = (3, 5, 10, 13)
BLOCKS = ("bench", "near", "ratio1e6", "mixed", "tri_rising", "tri_falling")
N1, N2 = 9, 70
NONPD_COL = 7
BETA = finish.BETA
BETA_MIXED = 0.01

# {block: (max abs err, max rel err)} of the parent commit against the oracle, the table of the docstring
PARENT = {
    "mixed": (2.128e-11, 6.734e-11),
    "tri_rising": (2.168e-18, 3.522e-15),
    "tri_falling": (4.662e-17, 8.165e-14),
}


def bounds(block):
    if block in finish.BLOCKS:
        return finish.bounds(block, "oracle")
    a, r = PARENT[block]
    return min(4.0 * a, finish.ATOL_CAP), min(4.0 * r, finish.RTOL_CAP)


def beta_of(block):
    return BETA_MIXED if block == "mixed" else BETA


def _identity_like(rng, n, d):
    """Mandel vectors of I + 1e-6 E, E symmetric with standard-normal entries"""
    e = rng.standard_normal((n, d, d))
    return finish._mandel(np.eye(d) + 0.5e-6 * (e + e.transpose(0, 2, 1)))


def _ratio1e6(rng, n, d):
    v = 10.0 ** rng.uniform(-3.0, 3.0, size=(n, d))
    v[:, 0], v[:, 1] = 1e-3, 1e3          # every matrix has the full ratio
    return finish._mandel(finish._spd_from(rng, v))


_inputs = {}


def make_inputs(d, block):
    """(x1, x2) Mandel vectors, (N1, d_vec) and (N2, d_vec); column NONPD_COL of x2 is symmetric, NaN-free and not positive definite"""
    if (d, block) in _inputs:
        return _inputs[d, block]
    seed = 5000 * d + BLOCKS.index(block)
    rng = np.random.default_rng(seed)
    if block == "bench":
        import bench
        x1, x2 = bench.synthetic_spd_mandel(N1, d, seed + 100), bench.synthetic_spd_mandel(N2, d, seed + 200)
    elif block == "near":
        x2 = finish.synthetic_spd_mandel(N2, d, seed + 200)
        x1 = (x2 * (1.0 + 1e-6 * rng.standard_normal(x2.shape)))[:N1]
    elif block == "ratio1e6":
        x1, x2 = _ratio1e6(rng, N1, d), _ratio1e6(rng, N2, d)
    elif block == "mixed":
        x1 = _identity_like(rng, N1, d)
        x2 = _identity_like(rng, N2, d)
        x2[1::2] = _ratio1e6(rng, N2 // 2, d)
    else:
        x1 = finish._mandel(np.tile(np.eye(d), (N1, 1, 1)))
        x2 = finish._mandel(orient.tridiagonals(d, block[4:])[:N2])
    bad = rng.uniform(0.05, 5.0, size=(1, d))
    bad[0, d // 2] *= -1.0
    x2 = x2.copy()
    x2[NONPD_COL] = finish._mandel(finish._spd_from(rng, bad))[0]
    x1.setflags(write=False)
    x2.setflags(write=False)
    _inputs[d, block] = (x1, x2)
    return x1, x2


_oracle = {}


def oracle(d, block):
    if (d, block) not in _oracle:
        from oracle import spd as ospd
        x1, x2 = make_inputs(d, block)
        with np.errstate(invalid="ignore", divide="ignore"):
            want = ospd.spd_ai_gaussian_kernel(x1, x2, beta_of(block))
        want.setflags(write=False)
        _oracle[d, block] = want
    return _oracle[d, block]


def launch(d, block):
    """the Gaussian-only launch (Gaussian mode, no distance output); raises if the library's status word is not zero"""
    import torch
    from gabotorch_amd import ops
    x1, x2 = make_inputs(d, block)
    k = ops.spd_ai_pairwise(torch.tensor(x1, device="cuda"), torch.tensor(x2, device="cuda"), beta=beta_of(block)).cpu().numpy()
    ops.check_deferred()
    return k


def deviations(got, want):
    """(max abs err, max rel err over normal references, abs err, |want|) with the non-positive-definite column taken out"""
    keep = np.arange(got.shape[1]) != NONPD_COL
    g, w = got[:, keep], want[:, keep]
    err = np.abs(g - w)
    normal = np.abs(w) >= np.finfo(np.float64).tiny
    rel = float(np.max(err[normal] / np.abs(w[normal]))) if normal.any() else 0.0
    return float(np.max(err)), rel, err, np.abs(w)


def _sym(d, v):
    from oracle import spd as ospd
    return ospd.vector_to_symmetric_matrix_mandel(np.asarray(v))


@pytest.mark.parametrize("block", BLOCKS)
@pytest.mark.parametrize("d", DIMS)
def test_inputs_are_what_the_docstring_says(d, block):
    """CPU side of the case: conditioning of the matrices, the non-positive-definite column, and an oracle that is finite everywhere else.
    Needs no GPU."""
    x1, x2 = make_inputs(d, block)
    assert x1.shape == (N1, d * (d + 1) // 2) and x2.shape == (N2, d * (d + 1) // 2)
    keep = np.arange(N2) != NONPD_COL
    l1, l2 = np.linalg.eigvalsh(_sym(d, x1)), np.linalg.eigvalsh(_sym(d, x2))
    assert l1.min() > 0.0 and l2[keep].min() > 0.0 and l2[NONPD_COL].min() < 0.0 and np.isfinite(x2).all()
    c1, c2 = l1[:, -1] / l1[:, 0], l2[keep][:, -1] / l2[keep][:, 0]
    if block == "ratio1e6":
        assert np.allclose(c1, 1e6, rtol=1e-6) and np.allclose(c2, 1e6, rtol=1e-6)
    elif block == "mixed":
        odd = (np.arange(N2) % 2 == 1)[keep]
        assert c1.max() < 1.0 + 1e-4 and c2[~odd].max() < 1.0 + 1e-4 and np.allclose(c2[odd], 1e6, rtol=1e-6)
    elif block == "near":
        rows = np.arange(N1) != NONPD_COL          # (row NONPD_COL of x1 was drawn from the column that x2 has since lost)
        assert np.abs(x1[rows] / x2[:N1][rows] - 1.0).max() < 1e-5
    else:
        assert c1.max() < 1e3 and c2.max() < 1e3
    want = oracle(d, block)
    assert want.shape == (N1, N2) and np.isnan(want[:, NONPD_COL]).all() and np.isfinite(want[:, keep]).all()
    if block == "mixed":      # the slow lanes' values are within reach of an absolute bound (the reason for BETA_MIXED)
        assert want[:, keep].min() > 1e-4


@pytest.mark.gpu
@pytest.mark.parametrize("block", BLOCKS)
@pytest.mark.parametrize("d", DIMS)
def test_gaussian_only_sweep_control(d, block):
    k, want = launch(d, block), oracle(d, block)
    assert k.shape == (N1, N2)
    keep = np.arange(N2) != NONPD_COL
    # the non-positive-definite column stays NaN in every row; its neighbours in the wave are numbers
    assert np.isnan(k[:, NONPD_COL]).all() and np.isfinite(k[:, keep]).all()
    amax, rmax, err, mag = deviations(k, want)
    atol, rtol = bounds(block)
    print(f"d={d} {block}: max abs err {amax:.3e} (bound {atol:.3e}), max rel err {rmax:.3e} (bound {rtol:.3e})")
    ok = (err <= atol) | (err <= rtol * mag)
    assert ok.all(), (f"d={d} {block}: {int((~ok).sum())} entries beyond atol {atol:.3e} / rtol {rtol:.3e}; worst abs {amax:.3e}, worst rel {rmax:.3e}")


def measure():
    """{block: (max abs, max rel)} over DIMS for the library in use, one line per case on stdout; the worst err / bound per block for the
    blocks whose bounds are fixed"""
    worst = {b: [0.0, 0.0, 0.0] for b in BLOCKS}
    for d in DIMS:
        for block in BLOCKS:
            k, want = launch(d, block), oracle(d, block)
            amax, rmax, err, mag = deviations(k, want)
            nan_ok = bool(np.isnan(k[:, NONPD_COL]).all() and np.isfinite(np.delete(k, NONPD_COL, 1)).all())
            atol, rtol = bounds(block)
            frac = float(np.max(np.minimum(err / atol, err / np.maximum(rtol * mag, 1e-300)))) if atol > 0 else float("nan")
            worst[block] = [max(worst[block][0], amax), max(worst[block][1], rmax), max(worst[block][2], frac)]
            print(f"d={d:2d} {block:11s}: max abs err {amax:.3e}  max rel err {rmax:.3e}  worst err / bound {frac:.2f}  NaN column alone {nan_ok}", flush=True)
    return worst


if __name__ == "__main__":
    import json
    print(json.dumps(measure()))
