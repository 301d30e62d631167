"""NestedSpdLogEuclideanMaternKernel without a GPU: the class surface, the host-side argument checks of gabo_nested_spd_matern_gram and
gabo_nested_spd_fit_evaluate_matern through _lib alone (all before the first HIP call), and the condition under which the GPU difference test
(tests/test_gpu_nested_spd_matern.py) compares: the numpy objective's own central differences at h and h / 2 agree within the cap."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

from gabotorch_amd import _lib, models
from gabotorch_amd._compat import ScaleKernel
from gabotorch_amd.kernel_utils import kernels_nested_spd, kernels_spd
from tests import _cpu_nested_spd_matern as ref

DIM, ARG = _lib.GABO_ERR_DIM, _lib.GABO_ERR_ARG


@pytest.fixture(scope="module", autouse=True)
def _built_library():
    if not os.path.exists(_lib.LIB_PATH):
        from gabotorch_amd import _build
        _build.build()


_buf = (ctypes.c_double * 4096)()
PTR = ctypes.addressof(_buf)


def test_class_surface():
    cls = kernels_spd.NestedSpdLogEuclideanMaternKernel
    assert kernels_nested_spd.NestedSpdLogEuclideanMaternKernel is cls and "NestedSpdLogEuclideanMaternKernel" in kernels_nested_spd.__all__
    assert issubclass(cls, kernels_spd.SpdLogEuclideanMaternKernel)
    for nu in (1.0, 2, 3.5, math.inf, True, "2.5", None):
        with pytest.raises(ValueError, match="nu must be 0.5, 1.5 or 2.5"):
            cls(5, 2, nu=nu)
    assert cls(5, 2).nu == 2.5 and cls(5, 2, nu=0.5).nu == 0.5
    torch.manual_seed(7)
    matern = cls(6, 3, nu=1.5)
    torch.manual_seed(7)
    gauss = kernels_spd.NestedSpdLogEuclideanGaussianKernel(6, 3)
    assert torch.equal(matern.projection_matrix, gauss.projection_matrix)          # the same torch.randn draw
    w = matern.projection_matrix.detach()
    assert w.shape == (6, 3) and w.dtype == torch.float64
    np.testing.assert_allclose((w.T @ w).numpy(), np.eye(3), atol=1e-14)
    assert sorted(n for n, _ in matern.named_parameters()) == ["raw_lengthscale", "raw_projection_matrix"]
    assert sorted(n for n, _ in matern.named_parameters()) == sorted(n for n, _ in gauss.named_parameters())
    assert matern.raw_projection_matrix_manifold._shape == gauss.raw_projection_matrix_manifold._shape == (6, 3)
    assert (matern.dim, matern.latent_dim) == (6, 3)
    matern.projection_matrix = torch.eye(6, 3, dtype=torch.float64)
    assert torch.equal(matern.raw_projection_matrix.detach(), torch.eye(6, 3, dtype=torch.float64))
    x = torch.zeros(4, 21, dtype=torch.float64)
    assert torch.equal(matern.forward(x, x, diagonal_distance=True), torch.ones(4, 1, dtype=torch.float64))


def test_the_model_keeps_no_fixed_distance_form_and_kernel_parameters_refuses_the_class():
    from gabotorch_amd.kernel_utils import kernel_parameters
    base = kernels_spd.NestedSpdLogEuclideanMaternKernel(3, 2)
    gp = models.SingleTaskGP(torch.zeros(2, 6, dtype=torch.float64), torch.zeros(2, dtype=torch.float64), ScaleKernel(base).double())
    assert gp._matern_form() is None            # the projection moves the distances during a fit
    with pytest.raises(TypeError):
        kernel_parameters.parameter_map(base)


def _fit_call(n=12, D=5, d=2, lengthscale=0.9, nu2=5, ws=None, pinned=None, skip=None, null=False):
    lib = _lib.load()
    ws = lib.gabo_nested_spd_fit_workspace_bytes(n, D, d) if ws is None else ws
    pinned = 2 * D * d + 7 if pinned is None else pinned
    args = [PTR, PTR, PTR, PTR, n, D, d, lengthscale, nu2, 1.0, 0.1, 0.0, 1, PTR, PTR, ws, PTR, pinned, None]
    if null:
        args = [None if a == PTR else a for a in args]
    if skip is not None:
        args[skip] = None
    return lib.gabo_nested_spd_fit_evaluate_matern(*args)


def _gram_call(n1=6, n2=4, D=5, dl=2, lengthscale=0.9, nu2=5, batch=1, ws=None, skip=None):
    lib = _lib.load()
    ws = lib.gabo_nested_spd_gram_workspace_bytes(batch, n1, n2, dl) if ws is None else ws
    args = [PTR, PTR + 8, PTR, PTR, batch, n1, n2, D, dl, lengthscale, nu2, PTR, ws, PTR, None]
    if skip is not None:
        args[skip] = None
    return lib.gabo_nested_spd_matern_gram(*args)


BAD_LENGTHSCALES = (0.0, -1.0, math.nan, math.inf, -math.inf)
BAD_NU2 = (0, 2, 4, 7, -1)


def test_fit_entry_refuses_its_arguments_before_any_hip_call():
    for null in (False, True):               # (with null pointers too: the dimension error wins over the argument error)
        assert _fit_call(D=40, null=null) == DIM and _fit_call(D=_lib.GABO_SPD_MAX_DIM + 1, null=null) == DIM
        assert _fit_call(D=1, d=1, null=null) == DIM and _fit_call(d=0, null=null) == DIM and _fit_call(d=5, null=null) == DIM
        assert _fit_call(n=0, null=null) == DIM and _fit_call(n=_lib.GABO_GP_MLL_LARGE_MAX_N + 1, null=null) == DIM
    assert _fit_call(null=True) == ARG
    for skip in (0, 1, 2, 3, 13, 14, 16):     # each pointer null in turn, every other argument valid
        assert _fit_call(skip=skip) == ARG, skip
    for bad in BAD_LENGTHSCALES:
        assert _fit_call(lengthscale=bad) == ARG, bad
    for bad in BAD_NU2:
        assert _fit_call(nu2=bad) == ARG, bad
    need_ws, need_pinned = _lib.load().gabo_nested_spd_fit_workspace_bytes(12, 5, 2), 2 * 5 * 2 + 7
    assert need_ws > 0
    assert _fit_call(ws=need_ws - 1) == ARG and _fit_call(pinned=need_pinned - 1) == ARG
    assert _fit_call(ws=0) == ARG and _fit_call(pinned=0) == ARG


def test_gram_entry_refuses_its_arguments_before_any_hip_call():
    for bad in BAD_LENGTHSCALES:
        assert _gram_call(lengthscale=bad) == ARG, bad
        assert _gram_call(lengthscale=bad, D=40) == ARG, bad          # the Matern check comes first
    for bad in BAD_NU2:
        assert _gram_call(nu2=bad) == ARG, bad
    assert _gram_call(batch=-1) == ARG and _gram_call(n1=-1) == ARG and _gram_call(n2=-1) == ARG
    assert _gram_call(D=40) == DIM and _gram_call(D=1) == DIM
    assert _gram_call(dl=1) == DIM and _gram_call(dl=5, D=8) == DIM and _gram_call(dl=4, D=3) == DIM
    assert _gram_call(batch=0) == _lib.GABO_OK and _gram_call(n1=0) == _lib.GABO_OK and _gram_call(n2=0) == _lib.GABO_OK
    for skip in (0, 1, 2, 3, 11, 13):
        assert _gram_call(skip=skip) == ARG, skip
    need = _lib.load().gabo_nested_spd_gram_workspace_bytes(1, 6, 4, 2)
    assert _gram_call(ws=need - 1) == ARG and _gram_call(ws=0) == ARG


@pytest.mark.parametrize("case", ref.CASES, ids=lambda c: "D{}-d{}-n{}-nu{}".format(*c))
def test_the_reference_differences_hold_the_cap_of_the_gpu_test(case):
    """for every case and direction of the GPU difference test: 10 |D_h - D_{h/2}| + 1e-9 max(1, |D|) <= 1e-5 max(1, |D|), h = 1e-4"""
    for k, (d1, d2) in enumerate(ref.reference_differences(case)):
        allowance, cap = ref.allowance(d1, d2)
        print(f"direction {k}: differences {d1:.12e} (h) {d2:.12e} (h/2), allowance {allowance:.3e}, cap {cap:.3e}")
        assert np.isfinite(d1) and np.isfinite(d2) and allowance <= cap
