"""The fused acquisition evaluators (acq_eval<D> and its Frobenius-type twin in csrc/spd_acq_body.hpp, sph_acq_eval in csrc/sphere_tr.hip,
gabo_gp_acquisition) against a CPU fp64 reference that shares nothing with the device: tests/_cpu_acquisition.py (oracle strip and Gram,
posterior by torch.linalg.solve, EI as oracle/gp.py states it, autograd for d acq / d k, the oracle's closed-form kernel gradients back to
the candidate).  Values AND gradients, at every instantiated dimension.

Inputs.  Candidate and training eigenvalues uniform in [0.5, 2] with random orthogonal frames (sphere: normalised Gaussian points plus coordinate
axes), y standard normal (1 for a single training point), mean 0.1, outputscale 1, best_f 0, R = 9 candidates; beta and noise per kernel and
dimension in SPD_RECIPE / SPHERE_RECIPE below, chosen on the CPU so that EVERY candidate of every case has reference |u| <= 4 and variance
>= 1e-3 (EI is then neither ~0 nor ~linear) and the reference gradient has max-abs >= 1e-3.  The tests assert these conditions on the reference,
so they cannot go vacuous.  The GP factors come from the ORACLE's Gram matrix: gabo_gp_factor up to the 96 points it holds, the library Cholesky
beyond (n = 129, 300).

Tolerances are the project's numbers for the same quantities against the oracle: value rtol 1e-9, atol 1e-13
(test_gp_acquisition_kernel_against_the_numpy_oracle); gradient rtol 1e-8, atol 1e-10 max|g| per case (test_spd_backward_all_dims_vs_oracle).
They stand as long as they are >= 10 x the reference's own fp64 uncertainty, measured on the CPU as the spread between the dense-solve and
the Cholesky evaluation of the helper on these very inputs (tests/test_acquisition_reference_cpu.py asserts it for a sample of the grid; the
figures below are the maxima over ALL cases, relative on values and as a fraction of max|g| on gradients):
  main grids (180 SPD + 20 sphere cases x 3 acquisitions): values <= 6.8e-12, gradients <= 9.5e-14, cond(K_y) <= 2.8e3;
  gabo_gp_acquisition alone: <= 1.6e-13 and <= 4.8e-15, cond(K_y) <= 2.2e2;  nearly repeated eigenvalues: <= 1.7e-13 and <= 2.2e-14;
  clamped variance: <= 6.6e-12 and <= 1.6e-15, cond(K_y) <= 46;  u >= 8: <= 3e-15 and <= 1.5e-14;
  u <= -8: the two evaluations agree to 1e-14 of the unit sigma 2^-52 max(1, |u|) (see test_expected_improvement_tails for that bound).
The recipes (beta, noise) per dimension: ai_gaussian d = 2: (0.2, 1), 3, 4: (0.3, 0.3), 5, 6, 8: (0.3, 0.1), 7: (0.3, 0.03), 9 ... 12: (0.3, 0.01);
ai_laplace 2, 3: (0.3, 0.1), 4 ... 12: (0.3, 0.01); le_gaussian 2, 3, 5: (0.3, 0.3), 4: (0.2, 0.3), 6, 7: (0.3, 0.1), 8: (0.3, 0.01);
frob_gaussian 2 ... 6: (0.3, 0.3), 7, 8: (0.3, 0.01); sphere: (0.3, 0.01) but for the Gaussian kernel at (dim, n) = (3, 7), (3, 9), (16, 65),
(63, 129), (65, 300): (0.3, 0.1) and (8, 64): (0.3, 0.3).  The edge regimes state their own inputs.
"""
import functools
import math
import types

import numpy as np
import pytest
import torch

from gabotorch_amd import _lib, models, ops
from tests import _cpu_acquisition as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
R = 9
MEAN, OUTPUTSCALE, BEST_F = 0.1, 1.0, 0.0
ACQ = {"ei_min": ("ei", False), "ei_max": ("ei", True), "mean": ("mean", False)}          # (kind, maximize)
ACQS = tuple(ACQ.values())
VALUE_RTOL, VALUE_ATOL, GRAD_RTOL, GRAD_ATOL = 1e-9, 1e-13, 1e-8, 1e-10
N_TRAIN = (1, 63, 64, 65, 129)           # dead lanes in the last chunk of 64, an exact chunk, one and two extra chunks

# (kernel, d) -> (beta, noise).  The starting recipe (0.3, 1e-2) holds the conditions at d >= 8; below, 63+ training points in a small space
# pin the posterior down (|u| up to 22, variance down to 2e-4), so the noise goes up and beta down until they hold.
_A, _B, _C, _D, _E = (0.3, 1e-2), (0.3, 3e-2), (0.3, 0.1), (0.3, 0.3), (0.2, 0.3)
SPD_RECIPE = {("ai_gaussian", d): r for d, r in zip(range(2, 13), [(0.2, 1.0), _D, _D, _C, _C, _B, _C, _A, _A, _A, _A])}
SPD_RECIPE.update({("ai_laplace", d): r for d, r in zip(range(2, 13), [_C, _C] + [_A] * 9)})
SPD_RECIPE.update({("le_gaussian", d): r for d, r in zip(range(2, 9), [_D, _D, _E, _D, _C, _C, _A])})
SPD_RECIPE.update({("frob_gaussian", d): r for d, r in zip(range(2, 9), [_D, _D, _D, _D, _D, _A, _A])})
SPD_GRID = ([("ai_gaussian", d) for d in range(2, 13)] + [("ai_laplace", d) for d in range(2, 13)]
            + [("le_gaussian", d) for d in range(2, 9)] + [("frob_gaussian", d) for d in range(2, 9)])
# (dim, n) of the sphere grid: n = 7, 9, 63, 65, 129, 300 leave a tail after sph_col_dot's unroll by 8, dim = 65, 130, 512 stride over the lanes
SPHERE_GRID = ((2, 1), (3, 7), (3, 9), (8, 64), (16, 65), (63, 129), (64, 8), (65, 300), (130, 63), (512, 300))
# (kernel, dim, n) -> (beta, noise) where the starting recipe does not hold the conditions (the Laplace kernel holds them everywhere)
SPHERE_RECIPE = {("sphere_gaussian", 3, 7): _C, ("sphere_gaussian", 3, 9): _C, ("sphere_gaussian", 8, 64): _D, ("sphere_gaussian", 16, 65): _C,
                 ("sphere_gaussian", 63, 129): _C, ("sphere_gaussian", 65, 300): _C}


def _recipe(kernel, d, n):
    return SPHERE_RECIPE.get((kernel, d, n), _A) if kernel.startswith("sphere") else SPD_RECIPE[kernel, d]


def t(x):
    return torch.tensor(np.ascontiguousarray(x), dtype=torch.float64, device=DEV)


# ------------------------------------------------------------------------------------------------------------- cases (CPU only)
@functools.lru_cache(maxsize=8)
def spd_case(kernel, d, n, recipe=None):
    """(built once for the parametrisations that share it; nothing writes into it)"""
    beta, noise = recipe or _recipe(kernel, d, n)
    rng = np.random.default_rng([ref.SPD_KERNELS.index(kernel), d, n])
    train, x = ref.rand_spd_mandel(rng, n, d), ref.rand_spd_mandel(rng, R, d)
    y = rng.standard_normal(n) if n > 1 else np.ones(1)       # (a single target carries the whole posterior mean: not a draw that may land on `mean`)
    return dict(kernel=kernel, d=d, n=n, beta=beta, noise=noise, train=train, x=x, y=y, gram=ref.strip(kernel, train, train, beta))


@functools.lru_cache(maxsize=8)
def sphere_case(kernel, dim, n, recipe=None):
    """Coordinate-axis vectors among the training points and the same vectors and their negatives among the candidates: <x, X_j> is exactly +-1
    there, OUTSIDE the clamp [-1 + 1e-15, 1 - 1e-15], so that strip entry passes no gradient and its value is the clamped one.  (Normalised
    random coincident points would not do: rounding of the inner product decides which side of 1 - 1e-15 it falls on, and the gradient is
    discontinuous across that boundary - dk = 2 beta k_j just inside, 0 outside.)"""
    beta, noise = recipe or _recipe(kernel, dim, n)
    rng = np.random.default_rng([10 + ref.SPHERE_KERNELS.index(kernel), dim, n])
    eye = np.eye(dim)
    axes = [0] if n == 1 else [0, dim - 1]
    train = np.concatenate([eye[axes], ref.rand_sphere(rng, n - len(axes), dim)])
    x = np.concatenate([eye[axes], -eye[axes], ref.rand_sphere(rng, R - 2 * len(axes), dim)])
    y = rng.standard_normal(n)
    y[:len(axes)] = (0.3, -0.2)[:len(axes)]          # (a candidate ON a training point has mu ~ y_j and sigma^2 ~ noise: keeps its |u| <= 4)
    assert (7 * n + 6 * dim) * 8 <= 150 * 1024       # the evaluator's LDS bound (fused_acquisition.py)
    return dict(kernel=kernel, d=dim, n=n, beta=beta, noise=noise, train=train, x=x, y=y, gram=ref.strip(kernel, train, train, beta),
                exact=2 * len(axes))


def reference(case, kind, maximize, best_f=BEST_F, solver="solve", of="value"):
    return ref.acquisition(case["kernel"], case["x"], case["train"], case["y"], case["beta"], MEAN, OUTPUTSCALE, case["noise"], best_f, kind,
                           maximize, solver=solver, gram=case["gram"], of=of)


def assert_conditions(out, kind):
    """conditions on the inputs, asserted on the reference: not measurements"""
    if kind == "ei":
        assert np.abs(out["u"]).max() <= 4.0, ("|u|", np.abs(out["u"]).max())
        assert out["var"].min() >= 1e-3, ("variance", out["var"].min())
    assert np.abs(out["grad"]).max() >= 1e-3, ("gradient", np.abs(out["grad"]).max())


def assert_matches(value, grad, out, out_sign=1.0, what=""):
    np.testing.assert_allclose(value.cpu().numpy(), out_sign * out["value"], rtol=VALUE_RTOL, atol=VALUE_ATOL, err_msg=f"value {what}")
    if grad is not None:
        np.testing.assert_allclose(grad.cpu().numpy(), out_sign * out["grad"], rtol=GRAD_RTOL, atol=GRAD_ATOL * np.abs(out["grad"]).max(),
                                   err_msg=f"gradient {what}")


# ------------------------------------------------------------------------------------------------------------- device side
def gp_factors(gram, y, noise):
    """(L^-1, L^-T, alpha, A = L^-T L^-1) on the device from the ORACLE's Gram matrix: gabo_gp_factor up to its 96 points, the library Cholesky
    beyond (what models.ExactGP falls back to there)."""
    n = len(y)
    if n <= _lib.GABO_GP_FACTOR_MAX_N:
        return ops.gp_factor(t(gram), t(y), OUTPUTSCALE, noise, MEAN, want_kinv=True)
    ky = OUTPUTSCALE * t(gram) + noise * torch.eye(n, dtype=torch.float64, device=DEV)
    chol = torch.linalg.cholesky(ky)
    alpha = torch.cholesky_solve((t(y) - MEAN).unsqueeze(-1), chol).squeeze(-1).contiguous()
    linv = torch.linalg.solve_triangular(chol, torch.eye(n, dtype=torch.float64, device=DEV), upper=False).tril().contiguous()
    linv_t = linv.t().contiguous()
    return linv, linv_t, alpha, (linv_t @ linv).contiguous()


def spd_flags(kernel):
    metric = {"ai": _lib.GABO_METRIC_AFFINE_INVARIANT, "le": _lib.GABO_METRIC_LOG_EUCLIDEAN, "frob": _lib.GABO_METRIC_FROBENIUS}[kernel.split("_")[0]]
    return (_lib.GABO_OUT_LAPLACE if kernel.endswith("laplace") else _lib.GABO_OUT_GAUSSIAN) | metric


def spd_train_operand(kernel, train):
    """the training-side operand as fused_acquisition.py prepares it"""
    if kernel.startswith("ai"):
        return ops.spd_acq_prepare_train(train)
    feat = ops.spd_logm_mandel(train) if kernel.startswith("le") else train
    return feat.t().contiguous()


class SpdDevice:
    def __init__(self, case):
        assert case["n"] <= int(_lib.load().gabo_spd_acq_max_train(case["d"]))
        self.case = case
        self.x = t(case["x"])
        self.operand = spd_train_operand(case["kernel"], t(case["train"]))
        self.linv, self.linv_t, self.alpha, self.kinv = gp_factors(case["gram"], case["y"], case["noise"])

    def eval(self, kind, maximize, out_sign=1.0, form="sym", need_grad=True, best_f=BEST_F, x=None, **kw):
        c = self.case
        la, lb = (self.kinv, self.kinv) if form == "sym" else (self.linv, self.linv_t)
        code = _lib.GABO_ACQ_EXPECTED_IMPROVEMENT if kind == "ei" else _lib.GABO_ACQ_POSTERIOR_MEAN
        return ops.spd_acq_eval(self.x if x is None else x, self.operand, self.alpha, la, lb, c["beta"], spd_flags(c["kernel"]), MEAN, OUTPUTSCALE,
                                ref.kxx(c["kernel"], c["beta"]), best_f, code, maximize, out_sign=out_sign, need_grad=need_grad, **kw)


class SphereDevice:
    """sphere_acq_params() of FusedAcquisition on a surrogate view whose factors come from the oracle's Gram matrix"""

    def __init__(self, case):
        self.case = case
        self.x = t(case["x"])
        self.train = t(case["train"])
        self.linv, self.linv_t, self.alpha, self.kinv = gp_factors(case["gram"], case["y"], case["noise"])

    def eval(self, kind, maximize, form="sym", need_grad=True, best_f=BEST_F, x=None):
        """-> value, gradient of out_sign * acquisition with the out_sign = -1 that sphere_acq_params() sets (cost = -acquisition)"""
        from gabotorch_amd.fused_acquisition import FusedAcquisition
        c = self.case
        cache = (self.linv, self.alpha)
        model = types.SimpleNamespace(_cache=cache, _cache_linv_t=(cache, self.linv_t), _cache_kinv=(cache, self.kinv if form == "sym" else None))
        acq = models.ExpectedImprovement(model, best_f, maximize) if kind == "ei" else models.PosteriorMean(model, maximize)
        mode = _lib.GABO_OUT_GAUSSIAN if c["kernel"] == "sphere_gaussian" else _lib.GABO_OUT_LAPLACE
        fused = FusedAcquisition(acq, "sphere", mode, c["beta"], False, DEV, view=(None, OUTPUTSCALE, MEAN, cache, self.train))
        assert fused.single_launch and (fused.kinv is not None) == (form == "sym")
        return ops.sphere_acq_eval(self.x if x is None else x, fused.sphere_acq_params(), need_grad=need_grad)


# ------------------------------------------------------------------------------------------------------------- main grids
@pytest.mark.parametrize("acq", list(ACQ))
@pytest.mark.parametrize("n", N_TRAIN)
@pytest.mark.parametrize("kernel,d", SPD_GRID)
def test_spd_evaluators_against_the_cpu_reference(kernel, d, n, acq):
    """value and Mandel gradient of every instantiation: d >= 9 takes the LDS-column Jacobi eigen-solver and D * D > 64 in the `U` phase, d >= 11
    a second trip of the `e = lane; e < T; e += 64` loops"""
    kind, maximize = ACQ[acq]
    case = spd_case(kernel, d, n)
    dev = SpdDevice(case)
    out = reference(case, kind, maximize)
    assert_conditions(out, kind)
    for out_sign in (1.0, -1.0):
        for form in ("sym", "tri"):
            value, grad = dev.eval(kind, maximize, out_sign, form)
            assert_matches(value, grad, out, out_sign, f"out_sign={out_sign} {form}")
            if d <= 8:          # "the same eigenvalues, bit for bit, without the eigenvectors" (spd_acq_body.hpp)
                only, none = dev.eval(kind, maximize, out_sign, form, need_grad=False)
                assert none is None and torch.equal(only, value)


@pytest.mark.parametrize("kernel,d,n", [("ai_gaussian", 5, 65), ("ai_laplace", 11, 63), ("le_gaussian", 4, 65), ("frob_gaussian", 8, 129)])
def test_spd_active_mask_leaves_masked_rows_untouched(kernel, d, n):
    case = spd_case(kernel, d, n)
    dev = SpdDevice(case)
    value, grad = dev.eval("ei", False, -1.0)
    mask = torch.tensor([1, 0, 1, 1, 0, 0, 1, 0, 1], dtype=torch.int32, device=DEV)
    keep = mask == 0
    buf_v = torch.linspace(-7.25, 3.5, R, dtype=torch.float64, device=DEV)
    buf_g = torch.linspace(11.0, -5.0, grad.numel(), dtype=torch.float64, device=DEV).reshape(grad.shape).contiguous()
    before_v, before_g = buf_v.clone(), buf_g.clone()
    got_v, got_g = dev.eval("ei", False, -1.0, active_ptr=mask.data_ptr(), out=(buf_v, buf_g))
    assert got_v is buf_v and got_g is buf_g
    assert torch.equal(buf_v[keep].view(torch.int64), before_v[keep].view(torch.int64))
    assert torch.equal(buf_g[keep].view(torch.int64), before_g[keep].view(torch.int64))
    assert torch.equal(buf_v[~keep], value[~keep]) and torch.equal(buf_g[~keep], grad[~keep])
    assert_matches(buf_v[~keep], None, {"value": reference(case, "ei", False)["value"][(~keep).cpu().numpy()]}, -1.0)


@pytest.mark.parametrize("acq", list(ACQ))
@pytest.mark.parametrize("dim,n", SPHERE_GRID)
@pytest.mark.parametrize("kernel", ref.SPHERE_KERNELS)
def test_sphere_evaluator_against_the_cpu_reference(kernel, dim, n, acq):
    kind, maximize = ACQ[acq]
    case = sphere_case(kernel, dim, n)
    ip = case["x"] @ case["train"].T
    assert (np.abs(ip[:case["exact"]]) == 1.0).sum() == case["exact"]        # the clamp-edge pairs: exactly +-1, outside the clamp
    dev = SphereDevice(case)
    out = reference(case, kind, maximize)
    assert_conditions(out, kind)
    # the entry at <x, X_j> = +1 carries weight in the acquisition (so a gradient that leaked through the clamp would show: just inside,
    # dk/dc = 2 beta k_j for the Gaussian kernel, and beyond all bounds for the Laplace one)
    leak = np.abs(out["grad_k"][0, 0]) * 2.0 * case["beta"] * out["ks"][0, 0]
    assert leak >= 1e3 * GRAD_ATOL * np.abs(out["grad"]).max(), leak
    for form in ("sym", "tri"):
        value, grad = dev.eval(kind, maximize, form)
        assert_matches(value, grad, out, -1.0, form)
        only, none = dev.eval(kind, maximize, form, need_grad=False)
        assert none is None and torch.equal(only, value)


@pytest.mark.parametrize("acq", list(ACQ))
@pytest.mark.parametrize("n", [1, 64, 65, 257])
def test_gp_acquisition_kernel_against_the_cpu_reference(n, acq):
    """gabo_gp_acquisition alone on a synthetic strip (the inputs of test_gp_acquisition_kernel_against_the_numpy_oracle, more sizes), with the
    analytic d/dk of the helper in place of 1e-6 finite differences"""
    rng = np.random.default_rng(12 + n)
    a, b = rng.standard_normal((n, 3)), rng.standard_normal((R, 3))
    ktr = np.exp(-0.5 * ((a[:, None] - a[None]) ** 2).sum(-1))
    ks = np.exp(-0.5 * ((b[:, None] - a[None]) ** 2).sum(-1))
    y = rng.standard_normal(n)
    noise = 0.3          # (257 points in R^3 pin the posterior down: the conditions on u and the variance need this much)
    chol = np.linalg.cholesky(OUTPUTSCALE * ktr + noise * np.eye(n))
    linv = np.linalg.inv(chol)
    alpha = np.linalg.solve(chol.T, np.linalg.solve(chol, y - MEAN))
    kind, maximize = ACQ[acq]
    out = ref.acquisition_of_strip(ks, ktr, y, MEAN, OUTPUTSCALE, noise, 1.0, BEST_F, kind, maximize)
    out["grad"] = out["grad_k"]
    assert_conditions(out, kind)
    code = _lib.GABO_ACQ_EXPECTED_IMPROVEMENT if kind == "ei" else _lib.GABO_ACQ_POSTERIOR_MEAN
    for out_sign in (1.0, -1.0):
        value, grad = ops.gp_acquisition(t(ks), t(alpha), t(linv), t(linv.T), MEAN, OUTPUTSCALE, 1.0, BEST_F, code, maximize, out_sign=out_sign)
        assert_matches(value, grad, out, out_sign, f"out_sign={out_sign}")


# ------------------------------------------------------------------------------------------------------------- edge regimes
EDGE_SPD_DIMS, EDGE_SPHERE_DIMS = (3, 8, 9, 12), (3, 65)
EDGE = [("ai_gaussian", d) for d in EDGE_SPD_DIMS] + [("sphere_gaussian", dim) for dim in EDGE_SPHERE_DIMS]
N_CLAMPED = 12


def device_for(case):
    return SphereDevice(case) if case["kernel"].startswith("sphere") else SpdDevice(case)


def device_eval(dev, kind, maximize, **kw):
    """-> value, gradient of -acquisition on both families"""
    if isinstance(dev, SphereDevice):
        return dev.eval(kind, maximize, **kw)
    return dev.eval(kind, maximize, -1.0, **kw)


def clamped_variance_case(kernel, d):
    """Candidates ON training points of a small, well separated training set with noise 1e-12.  The posterior variance at a training point is
    noise (1 - noise [Ky^-1]_jj), between 0 and the noise, so it is the noise that has to lie below the clamp at 1e-9 (with noise 1e-6 the
    variance there is 1e-6 and nothing is clamped); beta = 3 / d keeps the Gram matrix itself well conditioned (cond(Ky) < 1e2), so the tiny
    noise costs the reference no digits.  Affine-invariant: M = L^-1 X_j L^-T = I at the candidate's own training point, D equal eigenvalues.
    Sphere: the training points that serve as candidates are the coordinate axes and their negatives, <x, X_j> = 1 exactly (see sphere_case).
    At sigma = sqrt(1e-9) an error of 1e-16 in mu is 3e-12 in u: the targets are mean + 1e-3 N(0, 1) and best_f = mean, which keeps the terms of
    mu - best_f small and with them the reference's own uncertainty 10 x below the tolerances; y at the first candidate is best_f + 1e-5, so that
    one u is of order 1, the others lie far out on both sides."""
    rng = np.random.default_rng([77, ref.SPD_KERNELS.index(kernel) if kernel in ref.SPD_KERNELS else 9, d])
    n, beta, noise = N_CLAMPED, 6.0 / d, 1e-12
    if kernel.startswith("sphere"):
        m = min(d, 4)
        train = np.concatenate([np.eye(d)[:m], -np.eye(d)[:m], ref.rand_sphere(rng, n - 2 * m, d)])
        x = train[:2 * m].copy()
        beta = 2.0
    else:
        train = ref.rand_spd_mandel(rng, n, d)
        x = train[:R].copy()
    y = MEAN + 1e-3 * rng.standard_normal(n)
    y[0] = MEAN + 1e-5
    return dict(kernel=kernel, d=d, n=n, beta=beta, noise=noise, train=train, x=x, y=y, gram=ref.strip(kernel, train, train, beta), best_f=MEAN)


@pytest.mark.parametrize("kernel,d", EDGE)
def test_clamped_variance_regime(kernel, d):
    """sigma = sqrt(1e-9) and no variance term in the gradient: d EI = sgn Phi(u) d mu.  (The Laplace kernels have their kink at distance 0: no
    gradient to compare at a training point, as in test_fused_spd_acquisition_matches_autograd.)"""
    case = clamped_variance_case(kernel, d)
    assert np.linalg.cond(OUTPUTSCALE * case["gram"] + case["noise"] * np.eye(case["n"])) < 1e2
    dev = device_for(case)
    for maximize in (False, True):
        out = reference(case, "ei", maximize, best_f=case["best_f"])
        assert out["var"].max() < 1e-10 and (out["sigma"] == math.sqrt(1e-9)).all()
        assert 0.1 < abs(out["u"][0]) < 1.0 and (out["u"] > 8).any() and (out["u"] < -8).any()
        mean_only = reference(case, "mean", maximize)
        cdf = 0.5 * (1.0 + np.array([math.erf(v / math.sqrt(2.0)) for v in out["u"]]))
        np.testing.assert_allclose(out["grad"], cdf[:, None] * mean_only["grad"], rtol=1e-12, atol=1e-16 * np.abs(out["grad"]).max())       # the reference: mean term only
        assert np.abs(out["grad"]).max() >= 1e-5 and np.abs(out["grad"][0]).max() >= 1e-7       # (targets of size 1e-3: gradients of that order)
        for form in ("sym", "tri"):
            value, grad = device_eval(dev, "ei", maximize, form=form, best_f=case["best_f"])
            assert_matches(value, grad, out, -1.0, f"maximize={maximize} {form}")


NEARLY_REPEATED_GAPS = np.array([0.0, 1e-8, 1e-4, 3e-3, 0.0, 1e-8, 1e-4, 3e-3, 0.5])


def nearly_repeated_case(d):
    """the main-grid case (d, 65 training points) of the log-Euclidean kernel with candidates whose eigenvalues pair up (noise 0.1 at d = 8 too: these
    candidates reach |u| = 4.4 at the 0.01 of the main grid)"""
    case = dict(spd_case("le_gaussian", d, 65, recipe=(0.3, 0.3) if d == 3 else (0.3, 0.1)))
    rng = np.random.default_rng([5, d])
    lam = np.sort(rng.uniform(0.5, 2.0, (R, d)), axis=1)
    pair = rng.integers(0, d - 1, R)
    lam[np.arange(R), pair + 1] = lam[np.arange(R), pair] * (1.0 + NEARLY_REPEATED_GAPS)
    q = np.linalg.qr(rng.standard_normal((R, d, d)))[0]
    mats = np.einsum("nab,nb,ncb->nac", q, lam, q)
    case["x"] = ref.ospd.symmetric_matrix_to_vector_mandel(0.5 * (mats + mats.transpose(0, 2, 1)))
    return case


@pytest.mark.parametrize("d", [3, 8])
def test_log_euclidean_candidates_with_nearly_repeated_eigenvalues(d):
    """Two eigenvalues of the candidate equal, and a relative 1e-8, 1e-4 and 3e-3 apart: z = (l_a - l_b) / (l_a + l_b) lies on both sides of the 1e-3
    below which the adjoint of dlogm switches to its series (spd_acq_body.hpp), the last one just outside it, where the quotient of differences has
    lost the most digits.  The oracle's divided differences are cancellation-free at every gap (oracle/spd.py dlogm_adjoint)."""
    case = nearly_repeated_case(d)
    gaps = NEARLY_REPEATED_GAPS
    got = np.linalg.eigvalsh(ref.ospd.vector_to_symmetric_matrix_mandel(case["x"]))
    rel = np.min(np.diff(got, axis=1) / got[:, :-1], axis=1)           # the smallest relative gap of each candidate
    assert (rel[gaps == 0] < 1e-14).all() and (np.abs(rel[:8] - gaps[:8])[gaps[:8] > 0] < 1e-14 + 1e-6 * gaps[:8][gaps[:8] > 0]).all(), rel
    dev = SpdDevice(case)
    for kind, maximize in ACQS:
        out = reference(case, kind, maximize)
        assert_conditions(out, kind)
        assert np.abs(out["grad"]).max(axis=1).min() >= 1e-4          # every candidate has a gradient to compare
        for form in ("sym", "tri"):
            value, grad = dev.eval(kind, maximize, -1.0, form)
            assert_matches(value, grad, out, -1.0, f"{kind} maximize={maximize} {form}")


# |Delta| <= TAIL_C sigma 2^-52 max(1, |u|) [times the row's gradient scale]: see test_expected_improvement_tails
TAIL_C = 1.0


def tail_case(kernel, d):
    return sphere_case(kernel, d, {3: 9, 65: 300}[d]) if kernel.startswith("sphere") else spd_case(kernel, d, 65)


@pytest.mark.parametrize("tail", ["low", "high"])
@pytest.mark.parametrize("kernel,d", EDGE)
def test_expected_improvement_tails(kernel, d, tail):
    """u <= -8 on every candidate ("low") and u >= 8 ("high"), by the choice of best_f.

    high: EI = sigma (phi + u Phi) -> sigma u, nothing cancels, the main-grid tolerances apply.
    low:  Phi = (1 + erf(u / sqrt 2)) / 2 is a difference of two numbers next to 1, known to 2^-53 absolutely whoever evaluates it (the reference
    included), while phi + u Phi ~ phi / u^2 is itself ~1e-16: no relative comparison is possible.  The absolute errors are
        |d value| <= sigma |u| |d Phi|                                        ~ sigma 2^-52 max(1, |u|),
        |d grad|  <= |d h| |grad sigma| + sigma |d Phi| |grad u|,  h = phi + u Phi   ~ sigma 2^-52 max(1, |u|) max(|grad u|, |grad sigma| / sigma)
    with the row's gradient scale G = max(|grad u|_inf, |grad sigma|_inf / sigma) from the helper.  The constant: next to -1 the values of erf are
    2^-53 apart, so two correctly rounded evaluations of Phi differ by at most one such step halved, 0.25 of the unit above, and two that are
    good to one ulp by 0.5.  The helper's dense-solve and Cholesky evaluations of these inputs land on the same step (they differ by less than
    1e-14 of the unit on values and gradients, measured on the CPU over the six cases), so the measured spread does not raise that figure:
    TAIL_C = 1.  For u < -8.3 Phi rounds to 0 or one step on any evaluation and the bound exceeds the value itself: what this regime checks is
    that nothing larger than the rounding of Phi comes out of the evaluators there."""
    case = tail_case(kernel, d)
    base = reference(case, "ei", False)
    # minimisation: u = (best_f - mu) / sigma
    best_f = float((base["mu"] - 8.5 * base["sigma"]).min() if tail == "low" else (base["mu"] + 8.5 * base["sigma"]).max())
    out = reference(case, "ei", False, best_f=best_f)
    dev = device_for(case)
    if tail == "high":
        assert out["u"].min() >= 8.0 and out["var"].min() >= 1e-3 and np.abs(out["grad"]).max() >= 1e-3
        for form in ("sym", "tri"):
            value, grad = device_eval(dev, "ei", False, form=form, best_f=best_f)
            assert_matches(value, grad, out, -1.0, form)
        return
    assert out["u"].max() <= -8.0 and out["var"].min() >= 1e-3
    unit = TAIL_C * out["sigma"] * 2.0 ** -52 * np.maximum(1.0, np.abs(out["u"]))
    g_u = np.abs(reference(case, "ei", False, best_f=best_f, of="u")["grad"]).max(axis=1)
    g_s = np.abs(reference(case, "ei", False, best_f=best_f, of="sigma")["grad"]).max(axis=1) / out["sigma"]
    scale = np.maximum(g_u, g_s)
    assert (scale > 0).all()
    for form in ("sym", "tri"):
        value, grad = device_eval(dev, "ei", False, form=form, best_f=best_f)
        dv = np.abs(value.cpu().numpy() + out["value"])
        dg = np.abs(grad.cpu().numpy() + out["grad"]).max(axis=1)
        assert (dv <= unit).all(), (form, dv / unit)
        assert (dg <= unit * scale).all(), (form, dg / (unit * scale))
