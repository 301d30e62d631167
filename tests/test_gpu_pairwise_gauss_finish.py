"""The Gaussian-only launch of the SPD pairwise kernel (Gaussian values, no distance output: the launch that may trade the relative accuracy
of a tiny distance for speed - today a looser deflation threshold) against the CPU oracle and against exp(-beta d^2) formed on the host from the
same library's distance-mode output; and a bit-for-bit pin of the strict path (distance mode), which must never see such a trade.  Needs an MI355X.

Written with a shortcut for that launch's eigenvalue finish (the tenth logarithm from log det M = 2 (log prod W_kk + log prod G_kk), no reciprocal in
the trailing 2x2).  The shortcut measured slower and is not in the tree (CHANGELOG, "Eigenvalue finish and sweep control"); the bounds below are
what it, or any later one, has to meet.

Inputs, for d in 3, 5, 10, 12, 16, 20 (fixed seeds): the benchmark's generator (restated below), a block of nearly identical pairs (X against a
1e-6-relative symmetric perturbation of X) and a block with eigenvalue ratio 1e6; column NONPD_COL of every x2 is replaced by a symmetric
matrix with one negative eigenvalue (no NaN in it): that column of the result is NaN and nothing is raised.

How an entry is judged: its deviation `err` from the reference must satisfy  err <= atol  or  err <= rtol * |reference|  (the entry-wise form
of the bound of test_gpu_parity.py, never looser than its rtol 1e-9 / atol 1e-12).  atol and rtol are 4 x the worst deviations of the kernel
at commit 04997a2 (all ten logarithms; measured on the GPU on exactly these inputs, table below): a shortcut in the finish reorders a ten-term
sum, so a factor below 2 would make the test depend on summation order; 4 leaves one more bit.
`python tests/test_gpu_pairwise_gauss_finish.py` prints the figures of the library it finds without asserting anything.
"""
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

DIMS = (3, 5, 10, 12, 16, 20)
BLOCKS = ("bench", "near", "ratio1e6")
N1, N2 = 40, 300            # 300 columns: a full 256-thread (d < 7) or 64-thread tile next to a partial one
NONPD_COL = 7
BETA = 0.2 + math.log(2.0)  # the benchmark's
PIN = "spd_ai_dist_pin_d10.npz"

# Worst deviations of the ten-logarithm kernel (commit 04997a2) over the six dimensions, per block and reference, measured on an MI355X:
#                        against the oracle                against exp(-beta dist^2), dist from the distance-mode launch
#   block        max abs err      max rel err              max abs err      max rel err
#   bench        2.859e-15        4.725e-12                3.553e-15        4.050e-12
#   near         8.549e-15        3.332e-12                8.549e-15        2.078e-12
#   ratio1e6     1.644e-22        3.604e-03                1.717e-27        1.877e-04
# (rel err over the entries whose reference is a normal number).  The bounds: 4 x these, capped at atol 1e-12 / rtol 1e-9.
PARENT = {
    "bench": {"oracle": (2.859e-15, 4.725e-12), "host": (3.553e-15, 4.050e-12)},
    "near": {"oracle": (8.549e-15, 3.332e-12), "host": (8.549e-15, 2.078e-12)},
    "ratio1e6": {"oracle": (1.644e-22, 3.604e-03), "host": (1.717e-27, 1.877e-04)},
}
ATOL_CAP, RTOL_CAP = 1e-12, 1e-9


def bounds(block, ref):
    a, r = PARENT[block][ref]
    return min(4.0 * a, ATOL_CAP), min(4.0 * r, RTOL_CAP)


def _mandel(m):
    d = m.shape[-1]
    r, c = [], []
    for k in range(d):
        for i in range(d - k):
            r.append(i)
            c.append(i + k)
    r, c = np.array(r), np.array(c)
    return np.ascontiguousarray(m[:, r, c] * np.where(r == c, 1.0, 2.0 ** 0.5))


def _spd_from(rng, lam):
    n, d = lam.shape
    q = np.linalg.qr(rng.standard_normal((n, d, d)))[0]
    m = np.einsum("nab,nb,ncb->nac", q, lam, q)
    return 0.5 * (m + m.transpose(0, 2, 1))


def synthetic_spd_mandel(n, d, seed):
    """bench.py's generator: eigenvalues U[0.05, 5], Q from qr(standard_normal), Mandel layout."""
    rng = np.random.default_rng(seed)
    lam = rng.uniform(0.05, 5.0, size=(n, d))
    return _mandel(_spd_from(rng, lam))


def make_inputs(d, block):
    """(x1, x2) Mandel vectors, (N1, d_vec) and (N2, d_vec); column NONPD_COL of x2 is symmetric, NaN-free and not positive definite."""
    seed = 1000 * d + BLOCKS.index(block)
    rng = np.random.default_rng(seed)
    if block == "bench":
        x1, x2 = synthetic_spd_mandel(N1, d, seed + 100), synthetic_spd_mandel(N2, d, seed + 200)
    elif block == "near":
        x2 = synthetic_spd_mandel(N2, d, seed + 200)
        # a Mandel vector IS a symmetric matrix: an entry-wise relative perturbation of it is a symmetric perturbation of the matrix
        x1 = (x2 * (1.0 + 1e-6 * rng.standard_normal(x2.shape)))[:N1]
    else:
        def lam(n):
            v = 10.0 ** rng.uniform(-3.0, 3.0, size=(n, d))
            v[:, 0], v[:, 1] = 1e-3, 1e3          # every matrix has the full ratio
            return v
        x1, x2 = _mandel(_spd_from(rng, lam(N1))), _mandel(_spd_from(rng, lam(N2)))
    bad = rng.uniform(0.05, 5.0, size=(1, d))
    bad[0, d // 2] *= -1.0
    x2 = x2.copy()
    x2[NONPD_COL] = _mandel(_spd_from(rng, bad))[0]
    return x1, x2


def launches(x1, x2):
    """(Gaussian-only values, exp(-beta dist^2) on the host from the distance-mode launch); raises if the library reports anything"""
    import torch
    from gabotorch_amd import _lib, ops
    a, b = torch.tensor(x1, device="cuda"), torch.tensor(x2, device="cuda")
    k = ops.spd_ai_pairwise(a, b, beta=BETA).cpu().numpy()
    dist = ops.spd_ai_pairwise(a, b, mode=_lib.GABO_OUT_DISTANCE).cpu().numpy()
    ops.check_deferred()
    return k, np.exp(-(dist * dist) * BETA)


def oracle(x1, x2):
    from oracle import spd as ospd
    with np.errstate(invalid="ignore", divide="ignore"):
        return ospd.spd_ai_gaussian_kernel(x1, x2, BETA)


def deviations(got, want):
    """(max abs err, max rel err over normal references, abs err, |want|) with the non-positive-definite column taken out"""
    keep = np.arange(got.shape[1]) != NONPD_COL
    g, w = got[:, keep], want[:, keep]
    err = np.abs(g - w)
    normal = np.abs(w) >= np.finfo(np.float64).tiny
    rel = float(np.max(err[normal] / np.abs(w[normal]))) if normal.any() else 0.0
    return float(np.max(err)), rel, err, np.abs(w)


@pytest.mark.parametrize("block", BLOCKS)
@pytest.mark.parametrize("d", DIMS)
def test_gaussian_only_finish(d, block):
    x1, x2 = make_inputs(d, block)
    k, host = launches(x1, x2)
    want = oracle(x1, x2)
    assert k.shape == (N1, N2)
    # the non-positive-definite column: NaN in every row, from the kernel as from the reference's eigen-solver; every other entry a number
    assert np.isnan(k[:, NONPD_COL]).all() and np.isnan(host[:, NONPD_COL]).all() and np.isnan(want[:, NONPD_COL]).all()
    keep = np.arange(N2) != NONPD_COL
    assert np.isfinite(k[:, keep]).all() and np.isfinite(host[:, keep]).all() and np.isfinite(want[:, keep]).all()
    for ref, w in (("oracle", want), ("host", host)):
        amax, rmax, err, mag = deviations(k, w)
        atol, rtol = bounds(block, ref)
        print(f"d={d} {block} vs {ref}: max abs err {amax:.3e} (bound {atol:.3e}), max rel err {rmax:.3e} (bound {rtol:.3e})")
        ok = (err <= atol) | (err <= rtol * mag)
        assert ok.all(), (f"d={d} {block} vs {ref}: {int((~ok).sum())} entries beyond atol {atol:.3e} / rtol {rtol:.3e}; "
                          f"worst abs {amax:.3e}, worst rel {rmax:.3e}")


def test_distance_mode_bits_are_pinned(golden):
    """Distance mode keeps all ten logarithms and the strict deflation threshold: its output for a fixed input equals, bit for bit, what
    the kernel gave at commit 04997a2 (tests/golden/spd_ai_dist_pin_d10.npz: 16 x 16 pairs, d = 10; the inputs are
    stored with it because a QR factorisation is not reproducible to the bit across LAPACK builds).  Laplace values and the distance
    output written next to Gaussian values come from the same distances."""
    import torch
    from gabotorch_amd import _lib, ops
    g = golden(PIN)
    a, b = torch.tensor(g["x1"], device="cuda"), torch.tensor(g["x2"], device="cuda")
    dist = ops.spd_ai_pairwise(a, b, mode=_lib.GABO_OUT_DISTANCE).cpu().numpy()
    assert dist.shape == (16, 16) and np.array_equal(dist.view(np.int64), g["dist"].view(np.int64))
    _, dist2 = ops.spd_ai_pairwise(a, b, beta=BETA, return_dist=True)
    assert np.array_equal(dist2.cpu().numpy().view(np.int64), g["dist"].view(np.int64))
    lap = ops.spd_ai_pairwise(a, b, beta=BETA, mode=_lib.GABO_OUT_LAPLACE).cpu().numpy()
    np.testing.assert_allclose(lap, np.exp(-BETA * g["dist"]), rtol=1e-15, atol=0)


def measure():
    """the figures of the table above for the library in use: {block: {ref: (max abs, max rel)}}, one line per case on stdout"""
    worst = {b: {"oracle": [0.0, 0.0], "host": [0.0, 0.0]} for b in BLOCKS}
    for d in DIMS:
        for block in BLOCKS:
            x1, x2 = make_inputs(d, block)
            k, host = launches(x1, x2)
            want = oracle(x1, x2)
            nan_ok = bool(np.isnan(k[:, NONPD_COL]).all() and np.isnan(want[:, NONPD_COL]).all())
            for ref, w in (("oracle", want), ("host", host)):
                amax, rmax, _, _ = deviations(k, w)
                worst[block][ref] = [max(worst[block][ref][0], amax), max(worst[block][ref][1], rmax)]
                print(f"d={d:2d} {block:9s} vs {ref:6s}: max abs err {amax:.3e}  max rel err {rmax:.3e}  NaN column {nan_ok}", flush=True)
    return worst


if __name__ == "__main__":
    import json
    print(json.dumps(measure()))
