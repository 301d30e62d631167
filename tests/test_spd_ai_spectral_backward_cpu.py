"""No GPU: the closed form of the x-gradient of the affine-invariant Matern features as the numpy reference states it
(tests/_cpu_spd_ai_spectral_backward.py) against autograd through the torch composition and against central differences of the reference
kernel, and the host-side refusals of ops.spd_ai_spectral_features_backward and of the `x_grad` argument.

Tolerance of the autograd comparison, u = 2^-53, per point:  8 max|closed form fp64 - closed form long double| + 64 u scale_i,
scale_i = sqrt 2 |G_i^-1|_F^2 sum_lk |gb_ilk|  (the sum of the magnitudes of the terms of Gamma_i)."""
import numpy as np
import pytest
import torch

from gabotorch_amd import _lib, ops
from gabotorch_amd.kernel_utils import kernels_spd
from tests import _cpu_spd_ai_spectral as ref
from tests import _cpu_spd_ai_spectral_backward as bref

U = ref.U


def _problem(d, L, n, seed=0):
    rng = np.random.default_rng([seed, d, L, n])
    v = ref.to_mandel(ref.random_spd(rng, n, d, 0.3, 3.0))
    base = ref.base_draw(d, L, 2.5, 7 + d)
    lam, w = ref.spectral_points(base, 0.7, 2.5)
    return rng, v, base, lam, w


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("L", [1, 7])
@pytest.mark.parametrize("d", [2, 3, 5])
def test_closed_form_against_autograd_through_the_torch_composition(d, L, n):
    rng, v, base, lam, w = _problem(d, L, n)
    gbar = rng.standard_normal((n, 2 * L))
    x = torch.tensor(v, requires_grad=True)
    f = ops._spectral_features_torch(ops._spectral_logdiag_torch(x, torch.tensor(base[2])), torch.tensor(lam), torch.tensor(w))
    (want,) = torch.autograd.grad((torch.tensor(gbar) * f).sum(), x)
    got, _, usual, ref_err = bref.backward_with_tolerance(v, base[2], lam, f.detach().numpy(), gbar, 64)
    err = np.abs(got - want.numpy()).max(-1)
    bound = 8.0 * ref_err + usual
    print(f"d={d} L={L} n={n}: worst error / bound {(err / bound).max():.3f} (bound {bound.max():.3e}, fp64 against long double {ref_err.max():.3e})")
    assert (err <= bound).all()


def _richardson(f, at, step):
    """central difference of f at `at`, and the bound on its error: the truncation term estimated from the doubled step (cd(h) - f' =
    (cd(2h) - cd(h)) / 3 + O(h^4); twice that), plus the rounding term 16 u |f| / h"""
    f1p, f1m, f2p, f2m = f(at + step), f(at - step), f(at + 2 * step), f(at - 2 * step)
    cd1, cd2 = (f1p - f1m) / (2 * step), (f2p - f2m) / (4 * step)
    return cd1, 2.0 * abs(cd2 - cd1) / 3.0 + 16.0 * U * max(abs(f1p), abs(f1m), 1.0) / step


@pytest.mark.parametrize("d", [2, 3])
def test_closed_form_against_central_differences_of_the_reference_kernel(d):
    """sum_ij c_ij k(x1_i, x2_j) in every Mandel coordinate of x1: the upstream gradient of the features of x1 is c Fh(x2)"""
    n1, n2, L, kappa, nu = 3, 4, 16, 0.9, 2.5
    rng = np.random.default_rng([11, d])
    v1, v2 = ref.to_mandel(ref.random_spd(rng, n1, d, 0.5, 2.0)), ref.to_mandel(ref.random_spd(rng, n2, d, 0.5, 2.0))
    base = ref.base_draw(d, L, nu, 3)
    lam, w = ref.spectral_points(base, kappa, nu)
    c = rng.standard_normal((n1, n2))
    mats2 = ref.from_mandel(v2)
    f1 = ref.features(ref.logdiag(ref.from_mandel(v1), base[2]), lam, w)
    f2 = ref.features(ref.logdiag(mats2, base[2]), lam, w)
    got = bref.backward(v1, base[2], lam, f1, c @ f2)["grad"]
    worst = 0.0
    for i in range(n1):
        for e in range(v1.shape[1]):
            def f(val):
                vv = v1.copy()
                vv[i, e] = val
                return float((c * ref.kernel(ref.from_mandel(vv), mats2, base, kappa, nu)).sum())
            want, bound = _richardson(f, v1[i, e], 1e-4)
            worst = max(worst, abs(got[i, e] - want) / bound)
    print(f"d={d}: closed form against central differences, worst error / bound {worst:.3f}")
    assert worst <= 1.0


def test_the_backward_op_refuses_wrong_shapes_before_the_library_is_loaded(monkeypatch):
    def no_load():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_lib, "load", no_load)
    n, L, d = 4, 5, 3
    x, h, lam = torch.zeros(n, 6), torch.zeros(L, d, d), torch.zeros(L, d)
    f, g = torch.zeros(n, 2 * L), torch.zeros(n, 2 * L)
    for bad in ((x[None], h, lam, f, g), (x[0], h, lam, f, g),                                   # x is not 2-D
                (torch.zeros(n, 5), h, lam, f, g),                                               # not a Mandel length
                (x, h[:, :2], lam, f, g), (x, h[0], lam, f, g),                                  # phases not (L, d, d)
                (x, h, lam[:, :2], f, g), (x, h, lam[:4], f, g), (x, h, lam.reshape(-1), f, g),  # lam not (L, d)
                (x, h, lam, f[:, :-1], g), (x, h, lam, f[:3], g), (x, h, lam, f.reshape(-1), g),  # fhat not (N, 2L)
                (x, h, lam, f, g[:, :-2]), (x, h, lam, f, g[:2]), (x, h, lam, f, g.t())):         # grad_out not (N, 2L)
        with pytest.raises(RuntimeError):
            ops.spd_ai_spectral_features_backward(*bad)


def test_the_library_entries_check_their_arguments_on_the_host():
    lib = _lib.load()
    name = lib.gabo_spd_ai_spectral_features_backward
    for d in (1, 11, 32):
        assert name(None, None, None, None, None, None, None, 0, 4, 4, d, None) == _lib.GABO_ERR_DIM
        assert lib.gabo_spd_ai_spectral_features_backward_workspace_bytes(4, 4, d) == 0
    assert name(None, None, None, None, None, None, None, 0, -1, 4, 3, None) == _lib.GABO_ERR_ARG
    assert name(None, None, None, None, None, None, None, 0, 4, -1, 3, None) == _lib.GABO_ERR_ARG
    assert name(None, None, None, None, None, None, None, 0, 4, 4, 3, None) == _lib.GABO_ERR_ARG          # null pointers
    assert name(None, None, None, None, None, None, None, 0, 0, 4, 3, None) == _lib.GABO_OK
    assert name(None, None, None, None, None, None, None, 0, 4, 0, 3, None) == _lib.GABO_OK
    assert name(8, 8, 8, 8, 8, 8, 8, 5 * 2 * 6 * 8 - 1, 5, 129, 3, None) == _lib.GABO_ERR_ARG              # a short workspace
    assert name(8, 8, 8, 8, 8, 8, 8, 1 << 40, 1 << 30, 129, 3, None) == _lib.GABO_ERR_ARG                  # n chunks >= 2^31
    # (n, chunks, d(d+1)/2) doubles, chunks of 128 features
    assert lib.gabo_spd_ai_spectral_features_backward_workspace_bytes(5, 128, 10) == 5 * 1 * 55 * 8
    assert lib.gabo_spd_ai_spectral_features_backward_workspace_bytes(5, 129, 3) == 5 * 2 * 6 * 8
    assert lib.gabo_spd_ai_spectral_features_backward_workspace_bytes(1 << 30, 129, 3) == 0
    assert lib.gabo_spd_ai_spectral_features_backward_workspace_bytes(-1, 4, 3) == 0


def test_the_x_grad_argument():
    d, L, n = 3, 4, 2
    _, v, base, lam, w = _problem(d, L, n)
    a = torch.tensor(ref.logdiag(ref.from_mandel(v), base[2]))
    x, h, tl, tw = torch.tensor(v), torch.tensor(base[2]), torch.tensor(lam), torch.tensor(w)
    want = ref.features(a.numpy(), lam, w)
    for route in ("launch", "torch"):          # (with log-diagonals handed in, no route needs a device)
        got = ops.spd_ai_spectral_features(x, h, tl, tw, logdiag=a, x_grad=route)
        assert np.abs(got.numpy() - want).max() <= 64 * U
        k = ops.spd_ai_matern_kernel(x, x, h, tl, tw, logdiag1=a, x_grad=route)
        assert k.shape == (n, n)
    # x_grad="torch" with x requiring grad: the composition, no launch and no device
    xr = x.clone().requires_grad_(True)
    f = ops.spd_ai_spectral_features(xr, h, tl, tw, x_grad="torch")
    assert f.requires_grad and f.shape == (n, 2 * L)
    for bad in ("", "Launch", "autograd", None, True):
        with pytest.raises(ValueError):
            ops.spd_ai_spectral_features(x, h, tl, tw, logdiag=a, x_grad=bad)
        with pytest.raises(ValueError):
            ops.spd_ai_matern_kernel(x, x, h, tl, tw, logdiag1=a, x_grad=bad)
        with pytest.raises(ValueError):
            kernels_spd.SpdAffineInvariantMaternKernel(3, num_features=4, x_grad=bad)
    assert kernels_spd.SpdAffineInvariantMaternKernel(3, num_features=4).x_grad == "launch"
    assert kernels_spd.SpdAffineInvariantMaternKernel(3, num_features=4, x_grad="torch").x_grad == "torch"
