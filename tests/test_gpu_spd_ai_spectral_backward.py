"""The backward launch of the affine-invariant Matern features on the MI355X (csrc/spd_ai_spectral_backward.hip,
ops.spd_ai_spectral_features_backward) against the numpy closed form tests/_cpu_spd_ai_spectral_backward.py, from the launch up to autograd
through SpdAffineInvariantMaternKernel.

Tolerance, u = 2^-53, per point i:  scale_i = sqrt 2 |G_i^-1|_F^2 sum_lk |gb_ilk| bounds the sum of the magnitudes of the terms of Gamma_i;
    tol_i = max(8 max|g_fp64 - g_longdouble|_i, (L d + 8 d) u scale_i):
the reference against its more precise evaluation (never the device against itself), and the worst-case rounding of the L d-term sum and the
two triangular solves.  Every comparison prints its worst error / tolerance ratio, and the ratio against 64 u scale_i, before it asserts.
One run on one MI355X (worst error / tol_i, / (64 u scale_i)): the launch over the 60 shapes 0.022, 0.006; at nu = 1/2 and inf 0.003, 0.019;
at condition number 1e6 0.301, 35.5 (the fp64 closed form is itself 6.7e-8 from its long-double evaluation there); launch route against torch
route through the class 0.006, 0.013."""
import functools
import math

import numpy as np
import pytest
import torch

from gabotorch_amd import _lib, ops
from gabotorch_amd.kernel_utils.kernels_spd import SpdAffineInvariantMaternKernel
from tests import _cpu_spd_ai_spectral as ref
from tests import _cpu_spd_ai_spectral_backward as bref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = ref.U
N_SET, L_SET = 6, 130


def t(x):
    return torch.tensor(np.ascontiguousarray(x), dtype=torch.float64, device=DEV)


def bits(x):
    return x.detach().contiguous().view(torch.int64).cpu().numpy()


@functools.lru_cache(maxsize=None)
def points(d, hard=False):
    """-> (v Mandel vectors, h) built as the input sets of tests/test_gpu_spd_ai_spectral.py.  hard: condition number 1e6, n = 5, L = 65"""
    rng = np.random.default_rng([d, int(hard)])
    n, L = (5, 65) if hard else (N_SET, L_SET)
    if hard:
        q = np.linalg.qr(rng.standard_normal((n, d, d)))[0]
        lam = np.stack([rng.permutation(np.logspace(-3.0, 3.0, d)) for _ in range(n)])
        mats = np.einsum("nab,nb,ncb->nac", q, lam, q)
        mats = 0.5 * (mats + mats.transpose(0, 2, 1))
    else:
        mats = ref.random_spd(rng, n, d, 0.3, 3.0)
    return ref.to_mandel(mats), ref.base_draw(d, L, 2.5, 100 + d)[2]


@functools.lru_cache(maxsize=None)
def case(d, L, nu=2.5, hard=False):
    """The inputs of one launch shape on the first 5 points (fewer points are leading rows: row i depends on its own inputs alone) and the
    closed form with its tolerances, computed once: dict(v, h, lam, fhat, gbar, grad, tol, usual, ref_err)"""
    v, h = points(d, hard)
    v, h = v[:5], h[:L]
    lam, w = ref.spectral_points(ref.base_draw(d, L, nu, 3), 0.7, nu)
    fhat = ref.features(ref.logdiag(ref.from_mandel(v), h), lam, w)
    gbar = np.random.default_rng([17, d, L]).standard_normal((5, 2 * L))
    grad, tol, usual, ref_err = bref.backward_with_tolerance(v, h, lam, fhat, gbar, L * d + 8 * d)
    return dict(v=v, h=h, lam=lam, fhat=fhat, gbar=gbar, grad=grad, tol=tol, usual=usual, ref_err=ref_err)


def launch(c, n=5):
    return ops.spd_ai_spectral_features_backward(t(c["v"][:n]), t(c["h"]), t(c["lam"]), t(c["fhat"][:n]), t(c["gbar"][:n]))


def compare(what, got, c, n=5):
    err = np.abs(got - c["grad"][:n]).max(-1)
    r_tol, r_usual = (err / c["tol"][:n]).max(), (err / c["usual"][:n]).max()
    print(f"{what}: worst error / tol {r_tol:.3f}, / (64 u scale) {r_usual:.3f}  (error {err.max():.3e}, tol {c['tol'][:n].max():.3e}, "
          f"reference against long double {c['ref_err'][:n].max():.3e})")
    assert (err <= c["tol"][:n]).all()


# ------------------------------------------------------------------------------------------------------------- 1. the launch
@pytest.mark.parametrize("L", [1, 64, 65, 128, 129, 130])
@pytest.mark.parametrize("n", [1, 5])
@pytest.mark.parametrize("d", [2, 3, 5, 8, 10])
def test_launch_against_the_closed_form(d, n, L):
    c = case(d, L)
    got = launch(c, n)
    assert got.shape == (n, d * (d + 1) // 2)
    compare(f"d={d} n={n} L={L}", got.cpu().numpy(), c, n)


@pytest.mark.parametrize("nu", [0.5, math.inf])
@pytest.mark.parametrize("d", [3, 10])
def test_launch_at_the_other_smoothness_values(d, nu):
    c = case(d, L_SET, nu)
    compare(f"d={d} nu={nu}", launch(c).cpu().numpy(), c)


def test_launch_at_condition_number_1e6():
    c = case(10, 65, 2.5, True)
    compare("d=10 cond 1e6", launch(c).cpu().numpy(), c)


@pytest.mark.parametrize("d", [3, 10])
def test_rows_do_not_depend_on_the_batch_and_two_calls_agree(d):
    c = case(d, L_SET)
    whole = launch(c)
    assert np.array_equal(bits(whole), bits(launch(c)))
    for n in (1, 2):
        assert np.array_equal(bits(launch(c, n)), bits(whole[:n]))


@pytest.mark.parametrize("d", [3, 10])
def test_a_nan_row_and_a_non_spd_row_stay_in_their_own_row(d):
    v, h = points(d)
    v = v.copy()
    lam, w = ref.spectral_points(ref.base_draw(d, L_SET, 2.5, 3), 0.7, 2.5)
    gbar = np.random.default_rng([23, d]).standard_normal((N_SET, 2 * L_SET))
    th, tl, tw = t(h), t(lam), t(w)
    clean_f = ops.spd_ai_spectral_features(t(v), th, tl, tw)
    v[1, 1] = np.nan
    v[4] = -v[4]                              # negative definite
    bad = np.zeros(N_SET, dtype=bool)
    bad[[1, 4]] = True
    good = torch.tensor(~bad, device=DEV)
    prev = ops.set_error_checking(True)
    try:
        f = ops.spd_ai_spectral_features(t(v), th, tl, tw)          # NaN in the two rows
        g = ops.spd_ai_spectral_features_backward(t(v), th, tl, f, t(gbar))
        g_clean_f = ops.spd_ai_spectral_features_backward(t(v), th, tl, clean_f, t(gbar))      # finite features: the points alone make the NaN
        ops.check_deferred()                  # nothing is reported
    finally:
        ops.set_error_checking(prev)
    without = ops.spd_ai_spectral_features_backward(t(v[~bad]), th, tl, f[good], t(gbar[~bad]))
    for got in (g, g_clean_f):
        assert bool(torch.isnan(got[torch.tensor(bad, device=DEV)]).all())
        assert bool(torch.isfinite(got[good]).all()) and np.array_equal(bits(got[good]), bits(without))


def test_library_entry_limits():
    lib = _lib.load()
    assert lib.gabo_spd_ai_spectral_features_backward(None, None, None, None, None, None, None, 0, 3, 4, 11, None) == _lib.GABO_ERR_DIM
    assert lib.gabo_spd_ai_spectral_features_backward(None, None, None, None, None, None, None, 0, 0, 4, 3, None) == _lib.GABO_OK
    with pytest.raises(RuntimeError, match="unsupported dimension"):
        ops.spd_ai_spectral_features_backward(t(np.ones((2, 66))), t(np.ones((4, 11, 11))), t(np.ones((4, 11))), t(np.ones((2, 8))), t(np.ones((2, 8))))


# ------------------------------------------------------------------------------------------------------------- 2. autograd through the class
def make_kernel(d, L, route, frozen=True):
    k = SpdAffineInvariantMaternKernel(d, nu=2.5, num_features=L, seed=2, x_grad=route).double()
    k.lengthscale = torch.tensor(0.9, dtype=torch.float64)
    k = k.to(DEV)
    k.raw_lengthscale.requires_grad_(not frozen)
    return k


@functools.lru_cache(maxsize=None)
def class_case(d):
    n1, n2, L = 4, 6, 64 + 3
    rng = np.random.default_rng([29, d])
    v1, v2 = ref.to_mandel(ref.random_spd(rng, n1, d, 0.5, 2.0)), ref.to_mandel(ref.random_spd(rng, n2, d, 0.5, 2.0))
    c, c_same = rng.standard_normal((n1, n2)), rng.standard_normal((n1, n1))
    base = ref.base_draw(d, L, 2.5, 2)
    lam, w = ref.spectral_points(base, 0.9, 2.5)
    f1, f2 = (ref.features(ref.logdiag(ref.from_mandel(v), base[2]), lam, w) for v in (v1, v2))
    two = bref.backward_with_tolerance(v1, base[2], lam, f1, c @ f2, L * d + 8 * d)
    # one point set: k = (F F^T + its transpose) / 2 off the diagonal and a constant on it, so Gb = (C + C^T - 2 diag C) F
    sym = c_same + c_same.T - 2.0 * np.diag(np.diagonal(c_same))
    one = bref.backward_with_tolerance(v1, base[2], lam, f1, sym @ f1, L * d + 8 * d)
    return dict(v1=v1, v2=v2, c=c, c_same=c_same, two=two, one=one, L=L)


def _class_gradient(d, route, how):
    s = class_case(d)
    kern = make_kernel(d, s["L"], route)
    x1 = t(s["v1"]).requires_grad_(True)
    if how == "two sets":
        loss = (t(s["c"]) * kern.forward(x1, t(s["v2"]))).sum()
    elif how == "one set":
        loss = (t(s["c_same"]) * kern.forward(x1, x1)).sum()
    else:          # a batch of 4 sets of one point each
        xb = x1.reshape(4, 1, -1)
        k = kern.forward(xb, t(s["v2"]))
        assert k.shape == (4, 1, 6)
        loss = (t(s["c"]).reshape(4, 1, 6) * k).sum()
    (g,) = torch.autograd.grad(loss, x1)
    return g.cpu().numpy()


@pytest.mark.parametrize("how", ["two sets", "one set", "batched"])
@pytest.mark.parametrize("d", [2, 4, 10])
def test_class_gradient_by_the_launch_route_against_the_torch_route(d, how):
    s = class_case(d)
    want, tol, usual, ref_err = s["one" if how == "one set" else "two"]
    by_launch, by_torch = _class_gradient(d, "launch", how), _class_gradient(d, "torch", how)
    err = np.abs(by_launch - by_torch).max(-1)
    err_ref = np.abs(by_launch - want).max(-1)
    print(f"d={d} {how}: launch against torch, worst difference / tol {(err / tol).max():.3f}, / (64 u scale) {(err / usual).max():.3f}; "
          f"launch against the closed form / tol {(err_ref / tol).max():.3f}  (tol {tol.max():.3e}, reference against long double {ref_err.max():.3e})")
    assert (err <= tol).all() and (err_ref <= tol).all()


def test_route_selection(monkeypatch):
    d = 3
    s = class_case(d)
    counts = {"cholesky": 0, "backward": 0}
    real_chol, real_bwd = torch.linalg.cholesky, ops.spd_ai_spectral_features_backward
    monkeypatch.setattr(torch.linalg, "cholesky", lambda *a, **kw: (counts.__setitem__("cholesky", counts["cholesky"] + 1), real_chol(*a, **kw))[1])
    monkeypatch.setattr(ops, "spd_ai_spectral_features_backward",
                        lambda *a, **kw: (counts.__setitem__("backward", counts["backward"] + 1), real_bwd(*a, **kw))[1])
    x2 = t(s["v2"])
    # x requires grad, the lengthscale is frozen: the launch pair, once per backward()
    kern = make_kernel(d, s["L"], "launch")
    for rep in (1, 2):
        x1 = t(s["v1"]).requires_grad_(True)
        kern.forward(x1, x2).sum().backward()
        assert counts == {"cholesky": 0, "backward": rep} and x1.grad is not None and bool(torch.isfinite(x1.grad).all())
    # first order only: a second differentiation through the gradient (here in the weights of the sum, which its upstream gradient carries)
    x1, c = t(s["v1"]).requires_grad_(True), t(s["c"]).requires_grad_(True)
    (g,) = torch.autograd.grad((c * kern.forward(x1, x2)).sum(), x1, create_graph=True)
    assert g.requires_grad          # (the node behind g raises when the engine reaches it; no leaf lies behind it to ask torch.autograd.grad for)
    with pytest.raises(RuntimeError, match="once_differentiable"):
        g.sum().backward()
    counts.update(cholesky=0, backward=0)
    # the lengthscale requires grad as well: the torch composition, as before
    kern = make_kernel(d, s["L"], "launch", frozen=False)
    x1 = t(s["v1"]).requires_grad_(True)
    kern.forward(x1, x2).sum().backward()
    assert counts["cholesky"] >= 1 and counts["backward"] == 0 and x1.grad is not None and kern.raw_lengthscale.grad is not None
    # ... and so does x_grad="torch" with a frozen lengthscale
    counts.update(cholesky=0, backward=0)
    kern = make_kernel(d, s["L"], "torch")
    x1 = t(s["v1"]).requires_grad_(True)
    kern.forward(x1, x2).sum().backward()
    assert counts["cholesky"] >= 1 and counts["backward"] == 0
