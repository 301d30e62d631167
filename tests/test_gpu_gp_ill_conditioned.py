"""The GP dense-algebra launches of the fit -> predict path on nearly singular training covariances, on the MI355X: gabo_gp_mll and
gabo_gp_mll_gram (the packed, the one-wave tiled and the multi-wave tiled body of csrc/gp_mll_body.hpp), gabo_gp_mll_large (the 32 x 32-tile sweep
of csrc/gp_mll_large.hip) and gabo_gp_factor (csrc/gp_factor.hip) against the np.longdouble reference of tests/_cpu_gp_dense.py, itself checked
against mpmath by tests/test_gp_dense_reference_cpu.py.  A converging optimisation run clusters its training points and shrinks the fitted noise:
the cases are pairs of near-duplicates with cond_2(Ky) from 1e6 to 1e10 (mid) and 1e7 to 1e12 (hard), every one positive definite beyond the
rounding of an fp64 elimination - so none may be flagged - and matrices whose FIRST non-positive pivot sits at a chosen row.

Tolerance of the likelihood outputs and of W:  (64 + c cond_2(Ky)) 2^-53 x (the sum of the absolute values of the output's terms; max |W_ref|
entry-wise for W), the form of tests/test_gpu_gp_mll_series.py.  c is not chosen: it is 4 x the largest |numpy route - reference| / (cond 2^-53
scale) over the whole case table, both forms and the five outputs, where the numpy route is the plain fp64 LAPACK evaluation of the same formulas,
capped at the project's constant 8.  Evaluated at import from the reference alone; measured: 0.745 for the LAPACK route, so c = 2.98.
gabo_gp_factor is held to tests/_cpu_gp_condition.bound: (8 + 4 cond) 2^-53 max |ref|.

Worst error / tolerance on the MI355X, per body and level (the likelihood outputs of both forms | W; factor: the worst of linv, alpha, kinv):
                 benign            mid               hard
    packed       0.019 | 0.084     0.125 | 0.095     0.201 | 0.214
    one-wave     0.027 | 0.128     0.357 | 0.422     0.356 | 0.351
    tiled        0.010 | 0.075     0.073 | 0.132     0.146 | 0.109
    large        0.007 | 0.069     0.038 | 0.096     -
    factor       0.100             0.118             0.182
The large path met these only after a change: it used to apply the explicit inverse of each 32 x 32 pivot block, which costs the condition number
of that block on top of cond(Ky) - W at level mid was off by 2.54, 1.11, 2.17 and 1.12 tolerances at n = 161, 192, 193 and 512 (the likelihood
outputs by up to 0.79), and its two triangles differed in the last bits at every size.  It now takes every product through the pivot block in
Cholesky-factored form (csrc/gp_mll_large.hip).

Where the flag is concerned a negative pivot is the easy case - its logarithm is a NaN that gives it away whatever the flag does - so next to
the matrices with one pivot at -0.1 there are matrices with one pivot that is exactly zero among positive ones.
"""
import numpy as np
import pytest
import torch

from gabotorch_amd import _lib, ops
from tests import _cpu_gp_dense as cpu
from tests._cpu_gp_condition import bound

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = cpu.U
C_NUMPY_ROUTE = cpu.numpy_route_constant(cpu.MLL_CASES)
C = min(8.0, 4.0 * C_NUMPY_ROUTE)
print(f"numpy route: {C_NUMPY_ROUTE:.3f} cond 2^-53 scale at worst -> c = {C:.3f}")


def t(x):
    return torch.tensor(np.ascontiguousarray(x), dtype=torch.float64, device=DEV)


def body(n):
    return "packed" if n <= 30 else "one-wave" if n <= 39 else "tiled" if n <= _lib.GABO_GP_MLL_MAX_N else "large"


def bits(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float64)).tobytes()


def _report(tag, n, level, cond, names, err, tol):
    print(f"[{tag} {level}] n {n}: cond {cond:.3e}; error / tolerance " + ", ".join(f"{name} {e / s:.3f}" for name, e, s in zip(names, err, tol)))


def test_the_limits_are_the_ones_the_sizes_were_chosen_for():
    assert (_lib.GABO_GP_MLL_MAX_N, _lib.GABO_GP_MLL_LARGE_MAX_N, _lib.GABO_GP_FACTOR_MAX_N) == (160, 2048, 96)
    assert 0.0 < C <= 8.0


# ---- a. likelihood and derivatives, b. W -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,level", cpu.MLL_CASES)
def test_likelihood_and_derivatives_against_the_longdouble_reference(n, level):
    e, y, theta, outputscale, noise, mean = cpu.case(n, level)
    for gram in (False, True):
        ref = cpu.case_reference(n, level, gram)
        if gram:
            out = ops.gp_mll_gram(t(cpu.gram_of(n, level)), t(y), outputscale, noise, mean, want_w=False)[0].tolist()
            assert out[1] == 0.0
        else:
            out = ops.gp_mll(t(e), t(y), theta, outputscale, noise, mean)
        assert len(out) == 6 and out[5] == 0.0, out                    # valid, however close to singular: not flagged
        tol = (64.0 + C * ref.cond) * U * ref.scale
        err = np.abs(np.array(out[:5]).astype(cpu.LD) - ref.out).astype(np.float64)
        use = [i for i in range(5) if not (gram and i == 1)]
        _report(body(n) + (" gram" if gram else ""), n, level, ref.cond, [cpu.NAMES[i] for i in use], err[use], tol[use])
        for i in use:
            assert err[i] <= tol[i], (cpu.NAMES[i], gram, err[i], tol[i], float(ref.out[i]))


@pytest.mark.parametrize("n,level", cpu.MLL_CASES)
def test_w_against_the_longdouble_reference(n, level):
    _, y, _, outputscale, noise, mean = cpu.case(n, level)
    ref = cpu.case_reference(n, level, True)
    out, w = ops.gp_mll_gram(t(cpu.gram_of(n, level)), t(y), outputscale, noise, mean)
    w = w.cpu().numpy()
    assert out[5] == 0.0
    tol = (64.0 + C * ref.cond) * U * float(np.max(np.abs(ref.W)))
    err = float(np.max(np.abs(w.astype(cpu.LD) - ref.W)))
    _report(body(n) + " W", n, level, ref.cond, ["W"], [err], [tol])
    assert err <= tol, (err, tol)
    assert np.array_equal(w, w.T)


# ---- c. the flag and the row of the first bad pivot --------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,pos", [(n, pos) for n, positions in cpu.FLAG_POSITIONS.items() for pos in positions])
def test_a_bad_pivot_is_reported_wherever_it_sits_and_leaves_nothing_behind(n, pos):
    """pivot `pos` is the first that is not positive (-0.1; the ones before it are those of the valid matrix): flag 1 and five zeros; the
    next call on the valid matrix, with the same workspace, returns the bits of a run that never saw the bad one"""
    _, y, _, outputscale, noise, mean = cpu.case(n, "benign")
    k = cpu.gram_of(n, "benign")
    bad = t(cpu.indefinite_at(k, y, outputscale, noise, pos))
    k, y = t(k), t(y)
    ops._mll_large_ws.clear()                                          # (the fresh run allocates the workspace the next two calls reuse)
    fresh_out, fresh_w = ops.gp_mll_gram(k, y, outputscale, noise, mean)
    fresh_out, fresh_w = fresh_out.tolist(), fresh_w.cpu().numpy()
    assert fresh_out[5] == 0.0
    out, _ = ops.gp_mll_gram(bad, y, outputscale, noise, mean)
    out = out.tolist()
    assert out[5] == 1.0 and out[:5] == [0.0] * 5, out
    again_out, again_w = ops.gp_mll_gram(k, y, outputscale, noise, mean)
    assert bits(again_out.tolist()) == bits(fresh_out) and bits(again_w.cpu().numpy()) == bits(fresh_w)
    if n <= _lib.GABO_GP_FACTOR_MAX_N:
        fresh = [v.cpu().numpy() for v in ops.gp_factor(k, y, outputscale, noise, mean, want_kinv=True)]
        with pytest.raises(RuntimeError, match="not positive definite"):
            ops.gp_factor(bad, y, outputscale, noise, mean, want_kinv=True)
        again = [v.cpu().numpy() for v in ops.gp_factor(k, y, outputscale, noise, mean, want_kinv=True)]
        assert all(bits(a) == bits(b) for a, b in zip(again, fresh))


@pytest.mark.parametrize("n,pos", [(n, pos) for n, positions in cpu.ZERO_POSITIONS.items() for pos in positions])
def test_an_exactly_zero_pivot_is_reported(n, pos):
    """`not positive definite` is `pivot > 0` failing, on every pivot: a zero pivot among positive ones leaves no negative number, no NaN and
    no logarithm of one behind for a later test to find (the log determinant is -inf, the rest finite)"""
    _, y, _, outputscale, _, mean = cpu.case(n, "benign")
    bad, noise = cpu.zero_pivot_at(cpu.gram_of(n, "benign"), outputscale, pos)
    out, _ = ops.gp_mll_gram(t(bad), t(y), outputscale, noise, mean)
    out = out.tolist()
    assert out[5] == 1.0 and out[:5] == [0.0] * 5, out
    if n <= _lib.GABO_GP_FACTOR_MAX_N:
        with pytest.raises(RuntimeError, match="not positive definite"):
            ops.gp_factor(t(bad), t(y), outputscale, noise, mean)


# ---- d. gabo_gp_factor -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,level", cpu.FACTOR_CASES)
def test_factor_against_the_longdouble_reference(n, level):
    _, y, _, outputscale, noise, mean = cpu.case(n, level)
    ref = cpu.case_reference(n, level, True)
    linv, linv_t, alpha, kinv = (v.cpu().numpy() for v in ops.gp_factor(t(cpu.gram_of(n, level)), t(y), outputscale, noise, mean, want_kinv=True))
    names = ("linv", "alpha", "kinv")
    want = (ref.linv, ref.alpha, ref.kinv)
    err = [float(np.max(np.abs(g.astype(cpu.LD) - w))) for g, w in zip((linv, alpha, kinv), want)]
    tol = [bound(ref.cond, w) for w in want]
    _report("factor", n, level, ref.cond, names, err, tol)
    for name, a, b in zip(names, err, tol):
        assert a <= b, (name, a, b)
    assert np.array_equal(linv_t, linv.T) and np.array_equal(linv, np.tril(linv))
    assert np.array_equal(kinv, kinv.T)


# ---- e. the large path at its size limit -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", cpu.LIMIT_SIZES)
def test_large_path_at_its_size_limit_against_the_oracle(n):
    """63 full pivot blocks and one live row in the 64th, and 64 full blocks (GABO_GP_MLL_LARGE_MAX_N), against oracle/gp.py within the
    tolerances of tests/test_gpu_gp_fit.py::test_gp_mll_beyond_one_workgroup_against_the_oracle (longdouble takes minutes at this size)"""
    from oracle import gp as ogp
    e, y, theta, outputscale, noise, mean = cpu.case(n, "benign")
    want_ll, want_grad = ogp.marginal_log_likelihood(e, y, theta, outputscale, noise, mean)
    out = ops.gp_mll(t(e), t(y), theta, outputscale, noise, mean)
    assert out[5] == 0.0
    print(f"n {n}: ll {out[0]!r} / {want_ll!r}; gradient {out[1:5]} / {want_grad.tolist()}")
    np.testing.assert_allclose(out[0], want_ll, rtol=1e-10)
    np.testing.assert_allclose(out[1:5], want_grad, rtol=1e-8, atol=1e-9 * abs(want_ll))
    kb = np.exp(-theta * e)
    o6, w = ops.gp_mll_gram(t(kb), t(y), outputscale, noise, mean)
    o6 = o6.tolist()
    assert o6[5] == 0.0
    np.testing.assert_allclose(o6[0], out[0], rtol=1e-12)
    np.testing.assert_allclose([o6[2], o6[3], o6[4]], [out[2], out[3], out[4]], rtol=1e-8)
    ky = outputscale * kb + noise * np.eye(n)
    alpha = np.linalg.solve(ky, y - mean)
    np.testing.assert_allclose(w.cpu().numpy(), np.outer(alpha, alpha) - np.linalg.inv(ky), rtol=1e-8, atol=1e-8 * np.abs(alpha).max() ** 2)


def test_two_identical_calls_on_the_large_path_return_identical_bits():
    n, level = cpu.REPEAT_CASE
    e, y, theta, outputscale, noise, mean = cpu.case(n, level)
    e, k, y = t(e), t(cpu.gram_of(n, level)), t(y)
    first = ops.gp_mll(e, y, theta, outputscale, noise, mean)
    assert first[5] == 0.0 and bits(ops.gp_mll(e, y, theta, outputscale, noise, mean)) == bits(first)
    out, w = ops.gp_mll_gram(k, y, outputscale, noise, mean)
    out, w = out.tolist(), w.cpu().numpy()
    out2, w2 = ops.gp_mll_gram(k, y, outputscale, noise, mean)
    assert out[5] == 0.0 and len(out) == 6 and bits(out2.tolist()) == bits(out) and bits(w2.cpu().numpy()) == bits(w)
