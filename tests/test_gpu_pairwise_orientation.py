"""The Gaussian-only launch of the SPD pairwise kernel on inputs GRADED AGAINST its fixed QL orientation.  The comparison needs an MI355X; the check of the inputs does not.

That launch no longer decides per lane which end of the Householder tridiagonal sits at the QL iteration's deflation index: the end is a
compile-time fact per dimension (spd_pair_gauss_only_orientation, csrc/spd_pairwise_body.hpp), right for the Gram of a GP fit, whose
tridiagonals are graded one way.  When a matrix is graded the other way a fixed end costs sweeps and some of the RELATIVE accuracy of the small
eigenvalues, never a failure - this file holds the kernel to that on matrices whose grading reaches the QL exactly as built:

  x1 = identity, so W = I and M = x2 up to rounding; x2 = SPD TRIDIAGONAL matrices, which the Householder reduction leaves alone (a column that
  is already zero below the sub-diagonal gets a reflection of one coordinate).  Diagonal d_0 .. d_{d-1}: geometric from 0.2 to 5 ("rising"), from
  5 to 0.2 ("falling") or a per-column permutation of that sequence ("shuffled"); off-diagonals 0.3 sqrt(d_i d_{i+1}), so that x2 =
  D^1/2 (I + 0.3 S) D^1/2 with the eigenvalues of I + 0.3 S in (0.4, 1.6): positive definite, eigenvalues in (0.08, 8), K = exp(-beta sum log^2)
  >= e^-120, a normal number (checked below on the CPU).  For d in 3, 5, 10, 13, 16, 20; N1 = 3 rows against N2 = 150 columns: two full waves
  and a partial one, a partial tile at every block width; the first 16 columns of the "shuffled" block alternate between the rising and the
  falling sequence, so that one wave holds lanes of both gradings next to the permuted ones.

Checked: nothing is reported in the status word, every entry is finite, and the Gaussian-only values agree with the CPU oracle and with
exp(-beta dist^2) formed on the host from the distance-mode launch of the same library (the strict path: per-lane orientation rule, deflation
threshold 1e-20), entry by entry:  err <= atol  or  err <= rtol |reference|.

Bounds, set as tests/test_gpu_pairwise_gauss_finish.py set its own: 4 x the worst absolute and relative deviation of the PARENT of the change
(commit d957b62: per-lane rule in both launches) on exactly these inputs, over the six dimensions, per grading and reference; capped at atol
1e-12 / rtol 1e-9.  Measured on an MI355X (`python tests/test_gpu_pairwise_orientation.py` prints these figures for the library it finds
without asserting anything):

                     against the oracle                against exp(-beta dist^2) from the distance-mode launch
  grading      max abs err      max rel err              max abs err      max rel err
  rising       4.554e-18        1.065e-14                4.554e-18        1.057e-14
  falling      3.469e-18        1.074e-14                6.939e-18        1.074e-14
  shuffled     1.184e-16        2.664e-13                1.106e-16        1.083e-13

(every column of the rising and of the falling block is the same matrix: those rows are the rounding of ONE eigenproblem per dimension, a few
ulps of sum log^2 lambda.)  The kernel with the fixed orientation, same inputs, same machine:

  rising       2.168e-18        1.074e-14                2.168e-18        1.057e-14
  falling      4.662e-17        8.521e-14                4.315e-17        8.521e-14
  shuffled     1.251e-16        3.197e-13                1.212e-16        2.878e-13

"falling" is the adverse grading: the large end sits at the deflation index.  A QL iteration then finds the small eigenvalues to an absolute
accuracy of a few eps |T| instead of a relative one (the reason LAPACK's dsterf chooses between QL and QR by the grading), and log^2 of an
eigenvalue of 0.1 next to |T| = 8 feels that: sum log^2 moves by ~4e-14, tens of its ulps; the deflation threshold has no part in it (the CPU
model of tools/sim/ql_orientation_sim.py shows the same size of deviation at 1e-14 and at 1e-20).  Its worst entries are at 0.83 of the bound (d = 5: abs 4.7e-17 above atol, rel
3.6e-14 against rtol 4.3e-14; the relative deviations of d >= 13, 8.2e-14 - 8.5e-14, pass through atol: those values are below 1e-6).
"""
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

DIMS = (3, 5, 10, 13, 16, 20)
GRADINGS = ("rising", "falling", "shuffled")
N1, N2 = 3, 150
LO, HI, COUPLING = 0.2, 5.0, 0.3
BETA = 0.2 + math.log(2.0)  # the benchmark's

# {grading: {reference: (max abs err, max rel err)}} of the parent commit, the table of the docstring
PARENT = {
    "rising": {"oracle": (4.554e-18, 1.065e-14), "host": (4.554e-18, 1.057e-14)},
    "falling": {"oracle": (3.469e-18, 1.074e-14), "host": (6.939e-18, 1.074e-14)},
    "shuffled": {"oracle": (1.184e-16, 2.664e-13), "host": (1.106e-16, 1.083e-13)},
}
ATOL_CAP, RTOL_CAP = 1e-12, 1e-9


def bounds(grading, ref):
    a, r = PARENT[grading][ref]
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


def tridiagonals(d, grading):
    """(N2, d, d) SPD tridiagonal matrices of one grading"""
    rising = LO * (HI / LO) ** (np.arange(d) / (d - 1.0))
    diag = np.tile(rising if grading == "rising" else rising[::-1], (N2, 1))
    if grading == "shuffled":
        rng = np.random.default_rng(7000 + d)
        diag = np.stack([rng.permutation(rising) for _ in range(N2)])
        diag[0:16:2], diag[1:16:2] = rising, rising[::-1]
    off = COUPLING * np.sqrt(diag[:, :-1] * diag[:, 1:])
    m = np.zeros((N2, d, d))
    i = np.arange(d)
    m[:, i, i] = diag
    m[:, i[1:], i[:-1]] = off
    m[:, i[:-1], i[1:]] = off
    return m


_inputs = {}


def make_inputs(d, grading):
    """(x1, x2) Mandel vectors: N1 identities, N2 tridiagonals; computed once per case and not modified"""
    if (d, grading) not in _inputs:
        x1 = _mandel(np.tile(np.eye(d), (N1, 1, 1)))
        x2 = _mandel(tridiagonals(d, grading))
        x1.setflags(write=False)
        x2.setflags(write=False)
        _inputs[d, grading] = (x1, x2)
    return _inputs[d, grading]


def launches(x1, x2):
    """(Gaussian-only values, exp(-beta dist^2) on the host from the distance-mode launch); raises if the library's status word is not zero"""
    import torch
    from gabotorch_amd import _lib, ops
    a, b = torch.tensor(x1, device="cuda"), torch.tensor(x2, device="cuda")
    k = ops.spd_ai_pairwise(a, b, beta=BETA).cpu().numpy()
    dist = ops.spd_ai_pairwise(a, b, mode=_lib.GABO_OUT_DISTANCE).cpu().numpy()
    ops.check_deferred()
    return k, np.exp(-(dist * dist) * BETA)


def oracle(x1, x2):
    from oracle import spd as ospd
    return ospd.spd_ai_gaussian_kernel(x1, x2, BETA)


def deviations(got, want):
    """(max abs err, max rel err, abs err, |want|)"""
    err = np.abs(got - want)
    return float(np.max(err)), float(np.max(err / np.abs(want))), err, np.abs(want)


@pytest.mark.parametrize("grading", GRADINGS)
@pytest.mark.parametrize("d", DIMS)
def test_inputs_are_what_the_docstring_says(d, grading):
    """CPU side of the case: the matrices are tridiagonal and positive definite with eigenvalues in (0.08, 8), the oracle's values are finite and
    normal numbers.  Needs no GPU."""
    x1, x2 = make_inputs(d, grading)
    m = tridiagonals(d, grading)
    lam = np.linalg.eigvalsh(m)
    assert lam.min() > 0.4 * LO and lam.max() < 1.6 * HI
    assert np.count_nonzero(np.triu(m, 2)) == 0
    want = oracle(x1, x2)
    assert want.shape == (N1, N2) and np.isfinite(want).all()
    assert (want >= np.finfo(np.float64).tiny).all() and (want <= 1.0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("grading", GRADINGS)
@pytest.mark.parametrize("d", DIMS)
def test_gaussian_only_against_adverse_grading(d, grading):
    x1, x2 = make_inputs(d, grading)
    k, host = launches(x1, x2)
    want = oracle(x1, x2)
    assert k.shape == (N1, N2)
    assert np.isfinite(k).all() and np.isfinite(host).all() and np.isfinite(want).all()
    for ref, w in (("oracle", want), ("host", host)):
        amax, rmax, err, mag = deviations(k, w)
        atol, rtol = bounds(grading, ref)
        print(f"d={d} {grading} vs {ref}: max abs err {amax:.3e} (bound {atol:.3e}), max rel err {rmax:.3e} (bound {rtol:.3e})")
        ok = (err <= atol) | (err <= rtol * mag)
        assert ok.all(), (f"d={d} {grading} vs {ref}: {int((~ok).sum())} entries beyond atol {atol:.3e} / rtol {rtol:.3e}; "
                          f"worst abs {amax:.3e}, worst rel {rmax:.3e}")


def measure():
    """the figures of the docstring's table for the library in use: {grading: {ref: (max abs, max rel)}}, one line per case on stdout"""
    worst = {g: {"oracle": [0.0, 0.0], "host": [0.0, 0.0]} for g in GRADINGS}
    for d in DIMS:
        for grading in GRADINGS:
            x1, x2 = make_inputs(d, grading)
            k, host = launches(x1, x2)
            want = oracle(x1, x2)
            for ref, w in (("oracle", want), ("host", host)):
                amax, rmax, _, _ = deviations(k, w)
                worst[grading][ref] = [max(worst[grading][ref][0], amax), max(worst[grading][ref][1], rmax)]
                print(f"d={d:2d} {grading:8s} vs {ref:6s}: max abs err {amax:.3e}  max rel err {rmax:.3e}  finite {bool(np.isfinite(k).all())}", flush=True)
    return worst


if __name__ == "__main__":
    import json
    print(json.dumps(measure()))
