"""What the kernel-parameter study decides on the host: gabo_gram_extreme_eig (csrc/gram_eig.hip) refuses malformed calls before any HIP call
and sizes its workspace from the storage switch, and kernel_utils.kernel_parameters turns eigenvalue tables into verdicts - none of it needs
a GPU (the eigenvalue launch is stubbed)."""
import ctypes

import numpy as np
import pytest
import torch

from gabotorch_amd import _lib, ops
from gabotorch_amd.kernel_utils import kernel_parameters as kp
from gabotorch_amd.kernel_utils import kernels_nested_spd, kernels_nested_sphere, kernels_spd, kernels_sphere


@pytest.fixture(scope="module", autouse=True)
def _built_library():
    import os
    if not os.path.exists(_lib.LIB_PATH):
        from gabotorch_amd import _build
        _build.build()


def _call(lib, e=8, batch=2, n=5, thetas=16, n_thetas=3, out=24, ws=None, ws_bytes=0):
    """made-up addresses that are never touched: the verdict on the arguments comes first"""
    p = lambda a: None if a is None else ctypes.c_void_p(a)          # noqa: E731
    return lib.gabo_gram_extreme_eig(p(e), batch, n, p(thetas), n_thetas, p(out), p(ws), ws_bytes, None)


def test_malformed_calls_are_refused_before_any_hip_call():
    lib = _lib.load()
    assert _lib.GABO_GRAM_EIG_MAX_N == 1024 and 1 <= _lib.GABO_GRAM_EIG_LDS_MAX_N < _lib.GABO_GRAM_EIG_MAX_N
    assert _call(lib, n=_lib.GABO_GRAM_EIG_MAX_N + 1) == _lib.GABO_ERR_DIM
    assert _call(lib, n=_lib.GABO_GRAM_EIG_MAX_N + 1, e=None) == _lib.GABO_ERR_DIM
    for bad in (dict(e=None), dict(thetas=None), dict(out=None), dict(n=0), dict(n=-3), dict(batch=0), dict(batch=-1), dict(n_thetas=0),
                dict(n_thetas=-2), dict(batch=1 << 20, n_thetas=1 << 12)):
        assert _call(lib, **bad) == _lib.GABO_ERR_ARG, bad
    # beyond the LDS form the triangles live in the caller's workspace: too small or missing is refused
    n = _lib.GABO_GRAM_EIG_LDS_MAX_N + 1
    need = lib.gabo_gram_extreme_eig_workspace_bytes(2, n, 3)
    assert need > 0
    assert _call(lib, n=n, ws=256, ws_bytes=need - 1) == _lib.GABO_ERR_ARG
    assert _call(lib, n=n, ws=256, ws_bytes=0) == _lib.GABO_ERR_ARG
    assert _call(lib, n=n, ws=None, ws_bytes=need) == _lib.GABO_ERR_ARG


@pytest.mark.parametrize("batch,n,n_thetas", [(1, 1, 1), (10, 192, 30), (1, 193, 1), (10, 500, 30), (20, 500, 30), (1, 1024, 2)])
def test_workspace_is_one_packed_triangle_per_pair_beyond_the_lds_form(batch, n, n_thetas):
    lib = _lib.load()
    got = lib.gabo_gram_extreme_eig_workspace_bytes(batch, n, n_thetas)
    assert got == (0 if n <= _lib.GABO_GRAM_EIG_LDS_MAX_N else batch * n_thetas * (n * (n + 1) // 2) * 8)


def test_workspace_of_a_refused_call_is_zero():
    lib = _lib.load()
    for args in ((0, 500, 3), (2, 0, 3), (2, 500, 0), (-1, 500, 3), (2, 1025, 3)):
        assert lib.gabo_gram_extreme_eig_workspace_bytes(*args) == 0, args
    # the reference's largest study (20 sets of 500 points, 30 parameters): 600 MB
    assert lib.gabo_gram_extreme_eig_workspace_bytes(20, 500, 30) == 601_200_000


def test_the_lds_form_fits_a_compute_unit_and_the_next_size_does_not():
    """the switch point follows from the LDS arithmetic stated in csrc/gram_eig.hip: triangle + (5 + 4 waves) padded vectors + 16 doubles"""
    def doubles(n):
        return n * (n + 1) // 2 + 9 * ((n + 63) // 64 * 64) + 16
    assert doubles(_lib.GABO_GRAM_EIG_LDS_MAX_N) * 8 <= 160 * 1024 < doubles(_lib.GABO_GRAM_EIG_LDS_MAX_N + 1) * 8


# ---- the parameter -> theta map ---------------------------------------------------------------------------------------------------------------
BETA_KERNELS = (kernels_spd.SpdAffineInvariantGaussianKernel, kernels_spd.SpdAffineInvariantLaplaceKernel, kernels_sphere.SphereGaussianKernel)
LENGTHSCALE_KERNELS = (kernels_spd.SpdFrobeniusGaussianKernel, kernels_spd.SpdLogEuclideanGaussianKernel, kernels_sphere.SphereLaplaceKernel)


def test_theta_is_beta_or_the_inverse_squared_lengthscale():
    values = np.array([0.25, 1.0, 4.0])
    for kind in BETA_KERNELS:
        m = kp.parameter_map(kind)
        assert m.parameter == "beta" and m(0.3) == 0.3
        np.testing.assert_array_equal(m(values), values)
        assert kp.parameter_map(kind(beta_min=0.0)) is m
    for kind in LENGTHSCALE_KERNELS:
        m = kp.parameter_map(kind)
        assert m.parameter == "lengthscale" and m(2.0) == 0.25
        np.testing.assert_array_equal(m(values), [16.0, 1.0, 0.0625])
        assert torch.equal(m(torch.tensor(2.0, dtype=torch.float64)), torch.tensor(0.25, dtype=torch.float64))
        assert kp.parameter_map(kind()) is m


def test_nested_and_foreign_kernels_are_a_type_error():
    nested = [kernels_nested_spd.NestedSpdAffineInvariantGaussianKernel, kernels_nested_spd.NestedSpdLogEuclideanGaussianKernel]
    nested += [getattr(kernels_nested_sphere, n) for n in dir(kernels_nested_sphere)
               if n.startswith("Nested") and isinstance(getattr(kernels_nested_sphere, n), type)]
    assert len(nested) >= 3
    for kind in nested + [object, torch.nn.Linear]:
        with pytest.raises(TypeError):
            kp.parameter_map(kind)
        with pytest.raises(TypeError):
            kp.exponent_matrix(kind, torch.zeros(4, 3, dtype=torch.float64))
    with pytest.raises(TypeError):          # an instance of a nested kernel derived from a plain one
        kp.min_eigenvalues(kernels_nested_spd.NestedSpdLogEuclideanGaussianKernel(3, 2), torch.zeros(4, 6, dtype=torch.float64), [1.0])


# ---- verdicts on hand-made tables --------------------------------------------------------------------------------------------------------------
@pytest.fixture
def stubbed(monkeypatch):
    """the two launches replaced: the 'distance' of a set is its first column broadcast, and the 'eigenvalues' of a pair are read from the table
    TABLE[first entry of the set][index of theta] - so that the host code around them is all that runs"""
    calls = {"distance": 0, "eig": 0}
    table = {}

    def distance(x1, x2, beta=1.0, mode=None, **kw):
        calls["distance"] += 1
        assert mode == _lib.GABO_OUT_DISTANCE and x1 is x2
        return x1[..., :, :1].expand(*x1.shape[:-1], x1.shape[-2]).clone()

    def eig(e, thetas):
        calls["eig"] += 1
        ids = np.sqrt(e.reshape(-1, e.shape[-2], e.shape[-1])[:, 0, 0].numpy())        # (E = d^2 for the stubbed Gaussian kernel)
        out = torch.zeros(len(ids), len(thetas), 2, dtype=torch.float64)
        for b, k in enumerate(ids):
            out[b, :, 0] = torch.tensor(table[int(round(k))], dtype=torch.float64)
        calls["thetas"] = np.asarray(thetas)
        return out.reshape(tuple(e.shape[:-2]) + (len(thetas), 2))

    monkeypatch.setattr(ops, "sphere_pairwise", distance)
    monkeypatch.setattr(ops, "_device_for", lambda *ts: torch.device("cpu"))
    monkeypatch.setattr(ops, "gram_extreme_eigenvalues", eig)
    return calls, table


def _sets(ids, n=4):
    return torch.stack([torch.full((n, 3), float(k), dtype=torch.float64) for k in ids])


def test_percentage_uses_a_strict_comparison_and_one_launch_each(stubbed):
    calls, table = stubbed
    table.update({1: [-1.0, 0.0, 1e-9, 2.0], 2: [-1.0, 1e-3, -5e-7, 2.0], 3: [0.5, 0.0, -5.0000001e-7, 2.0], 4: [-0.1, -0.2, -4.9999999e-7, 3.0]})
    params = [0.1, 0.2, 0.3, 0.4]
    share, eig = kp.percentage_pd_kernels(kernels_sphere.SphereGaussianKernel, _sets([1, 2, 3, 4]), params)
    assert calls["distance"] == 1 and calls["eig"] == 1
    np.testing.assert_array_equal(calls["thetas"], params)
    np.testing.assert_array_equal(eig, [table[k] for k in (1, 2, 3, 4)])
    np.testing.assert_array_equal(share, [0.25, 0.25, 0.25, 1.0])            # (0 > 0 is false)
    share, _ = kp.percentage_pd_kernels(kernels_sphere.SphereGaussianKernel, _sets([1, 2, 3, 4]), params, min_tolerated_eigenvalue=-5e-7)
    np.testing.assert_array_equal(share, [0.25, 0.75, 0.5, 1.0])             # (-5e-7 > -5e-7 is false, -4.9999999e-7 is above, -5.0000001e-7 below)
    # one set: (P,) eigenvalues from min_eigenvalues, a share of 0 or 1
    one = kp.min_eigenvalues(kernels_sphere.SphereGaussianKernel, _sets([2])[0], params)
    assert one.shape == (4,)
    share, eig = kp.percentage_pd_kernels(kernels_sphere.SphereGaussianKernel, _sets([2])[0], params)
    assert eig.shape == (1, 4)
    np.testing.assert_array_equal(share, [0.0, 1.0, 0.0, 1.0])


def test_lengthscales_reach_the_launch_as_inverse_squares(stubbed):
    calls, table = stubbed
    table[1] = [1.0, 1.0]
    kp.min_eigenvalues(kernels_sphere.SphereLaplaceKernel, _sets([1]), torch.tensor([0.5, 2.0]))
    np.testing.assert_array_equal(calls["thetas"], [4.0, 0.25])


def test_a_list_of_unequal_sets_is_processed_set_by_set(stubbed):
    calls, table = stubbed
    table.update({1: [0.1, 0.2], 2: [0.3, 0.4], 3: [0.5, 0.6]})
    sets = [_sets([1], n=4)[0], _sets([2], n=6)[0], _sets([3], n=5)[0]]
    got = kp.min_eigenvalues(kernels_sphere.SphereGaussianKernel, sets, [1.0, 2.0])
    np.testing.assert_array_equal(got, [[0.1, 0.2], [0.3, 0.4], [0.5, 0.6]])
    assert calls["eig"] == 3
    got = kp.min_eigenvalues(kernels_sphere.SphereGaussianKernel, [s[:4] for s in sets], [1.0, 2.0])      # equal sizes: stacked, one launch
    np.testing.assert_array_equal(got, [[0.1, 0.2], [0.3, 0.4], [0.5, 0.6]])
    assert calls["eig"] == 4


def test_smallest_pd_parameter():
    params = [0.1, 0.2, 0.4, 0.8, 1.6]
    assert kp.smallest_pd_parameter(params, [0.0, 0.5, 1.0, 1.0, 1.0]) == 0.4
    assert kp.smallest_pd_parameter(params, [1.0, 1.0, 1.0, 1.0, 1.0]) == 0.1
    # a non-monotone table: a parameter that qualifies below one that does not is not "from there on"
    assert kp.smallest_pd_parameter(params, [1.0, 1.0, 0.9, 1.0, 1.0]) == 0.8
    assert kp.smallest_pd_parameter(params, [1.0, 1.0, 0.9, 1.0, 1.0], required=0.9) == 0.1
    # nothing qualifies when the largest parameter does not
    assert kp.smallest_pd_parameter(params, [1.0, 1.0, 1.0, 1.0, 0.95]) is None
    assert kp.smallest_pd_parameter(params, [0.0] * 5) is None
    # the order of the parameters does not matter
    assert kp.smallest_pd_parameter([1.6, 0.1, 0.8, 0.4, 0.2], [1.0, 0.0, 1.0, 1.0, 0.5]) == 0.4
    with pytest.raises(ValueError):
        kp.smallest_pd_parameter(params, [1.0, 1.0])
