"""What the joint posterior and the sampler decide on the host: gabo_gp_posterior_joint and gabo_mvn_sample (csrc/gp_posterior.hip) refuse
malformed calls before any HIP call, the workspace follows the padding stated in the header, models.MultivariateNormal is plain algebra around
one launch (stubbed here), and tests/golden/letters_gp.npz is what tests/golden/make_golden_letters_gp.py wrote - none of it needs a GPU."""
import ctypes
import hashlib
import os
import re

import numpy as np
import pytest
import torch

from gabotorch_amd import _lib, models, ops
from tests import _cpu_gp_posterior as cpu
from tests.conftest import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", autouse=True)
def _built_library():
    if not os.path.exists(_lib.LIB_PATH):
        from gabotorch_amd import _build
        _build.build()


def _p(a):
    return None if a is None else ctypes.c_void_p(a)


def _joint(lib, kstar=8, cov=16, linv=24, alpha=32, m=5, n=3, mean_out=40, var_out=48, ws=64, ws_bytes=None):
    """made-up addresses that are never touched: the verdict on the arguments comes first"""
    if ws_bytes is None:
        ws_bytes = lib.gabo_gp_posterior_joint_workspace_bytes(m, n)
    return lib.gabo_gp_posterior_joint(_p(kstar), _p(cov), _p(linv), _p(alpha), m, n, 0.0, 1.0, _p(mean_out), _p(var_out), _p(ws), ws_bytes, None)


def _sample(lib, mean=8, cov=16, m=5, samples=2, base=None, out=24, tril=None, status=32):
    return lib.gabo_mvn_sample(_p(mean), _p(cov), m, samples, ctypes.c_uint64(1), _p(base), _p(out), _p(tril), _p(status), None)


def test_malformed_joint_calls_are_refused_before_any_hip_call():
    lib = _lib.load()
    assert _joint(lib, n=_lib.GABO_GP_MLL_LARGE_MAX_N + 1, ws_bytes=1 << 30) == _lib.GABO_ERR_DIM
    assert _joint(lib, n=_lib.GABO_GP_MLL_LARGE_MAX_N + 1, kstar=None, ws_bytes=1 << 30) == _lib.GABO_ERR_DIM
    assert _joint(lib, m=_lib.GABO_GP_POSTERIOR_MAX_M + 1, ws_bytes=1 << 40) == _lib.GABO_ERR_DIM
    for bad in (dict(kstar=None), dict(cov=None), dict(linv=None), dict(alpha=None), dict(mean_out=None), dict(var_out=None), dict(ws=None),
                dict(m=0, ws_bytes=1 << 20), dict(m=-4, ws_bytes=1 << 20), dict(n=0, ws_bytes=1 << 20), dict(n=-1, ws_bytes=1 << 20)):
        assert _joint(lib, **bad) == _lib.GABO_ERR_ARG, bad
    need = lib.gabo_gp_posterior_joint_workspace_bytes(5, 3)
    assert _joint(lib, ws_bytes=need - 1) == _lib.GABO_ERR_ARG
    assert _joint(lib, ws_bytes=0) == _lib.GABO_ERR_ARG


def test_malformed_sampler_calls_are_refused_before_any_hip_call():
    lib = _lib.load()
    assert _sample(lib, m=_lib.GABO_MVN_SAMPLE_MAX_M + 1) == _lib.GABO_ERR_DIM
    assert _sample(lib, m=_lib.GABO_MVN_SAMPLE_MAX_M + 1, cov=None) == _lib.GABO_ERR_DIM
    for bad in (dict(mean=None), dict(cov=None), dict(status=None), dict(out=None), dict(m=0), dict(m=-2), dict(samples=-1)):
        assert _sample(lib, **bad) == _lib.GABO_ERR_ARG, bad
    assert lib.gabo_mvn_base_samples(None, 3, 5, ctypes.c_uint64(1), None) == _lib.GABO_ERR_ARG
    assert lib.gabo_mvn_base_samples(_p(8), 3, 0, ctypes.c_uint64(1), None) == _lib.GABO_ERR_ARG
    assert lib.gabo_mvn_base_samples(_p(8), -1, 5, ctypes.c_uint64(1), None) == _lib.GABO_ERR_ARG
    assert lib.gabo_mvn_base_samples(None, 0, 5, ctypes.c_uint64(1), None) == _lib.GABO_OK       # nothing to draw, nothing launched


@pytest.mark.parametrize("m,n", [(1, 1), (64, 16), (65, 17), (100, 79), (4096, 96), (130, 161), (1, 2048)])
def test_workspace_is_v_padded_to_the_tiles(m, n):
    lib = _lib.load()
    assert lib.gabo_gp_posterior_joint_workspace_bytes(m, n) == ((m + 63) // 64 * 64) * ((n + 15) // 16 * 16) * 8


def test_workspace_of_a_refused_call_is_zero():
    lib = _lib.load()
    for args in ((0, 5), (5, 0), (-1, 5), (5, _lib.GABO_GP_MLL_LARGE_MAX_N + 1), (_lib.GABO_GP_POSTERIOR_MAX_M + 1, 5)):
        assert lib.gabo_gp_posterior_joint_workspace_bytes(*args) == 0, args


def test_constants_match_the_header():
    text = open(os.path.join(ROOT, "include", "gabo_hip.h")).read()
    for name in ("GABO_GP_POSTERIOR_MAX_M", "GABO_MVN_SAMPLE_MAX_M", "GABO_GP_MLL_LARGE_MAX_N", "GABO_ERR_NOT_SPD"):
        value = re.search(rf"#define {name} \(?(-?\d+)\)?", text)
        assert value is not None and int(value.group(1)) == getattr(_lib, name), name
    assert _lib.GABO_MVN_JITTER_LADDER == cpu.LADDER == (0.0, 1e-8, 1e-7, 1e-6)
    assert "0x6d766e7a" in text and cpu.MVN_TAG == 0x6D766E7A
    assert cpu.MVN_TAG not in (0x6761626F, 0x73656C65, 0x73706872)          # the three streams the library had


def test_the_fused_sampler_fits_a_compute_unit():
    """the LDS arithmetic of csrc/gp_posterior.hip: triangle + (1 + 4 waves) padded vectors + 16 doubles; the switch point is the one of
    gabo_gram_extreme_eig's LDS form (three 64-column groups per row)"""
    def doubles(m):
        return m * (m + 1) // 2 + 5 * ((m + 63) // 64 * 64) + 16
    assert doubles(_lib.GABO_MVN_SAMPLE_MAX_M) * 8 <= 160 * 1024
    assert _lib.GABO_MVN_SAMPLE_MAX_M == _lib.GABO_GRAM_EIG_LDS_MAX_N == 3 * 64


# ---- MultivariateNormal on CPU tensors, the launch stubbed -----------------------------------------------------------------------------------
@pytest.fixture
def stubbed(monkeypatch):
    calls = []

    def mvn_sample(mean, cov, sample_shape=(), seed=None, base_samples=None, return_scale_tril=False):
        calls.append(dict(shape=tuple(sample_shape), seed=seed, base=base_samples))
        L = torch.linalg.cholesky(cov + 1e-8 * torch.eye(cov.shape[0], dtype=cov.dtype))
        z = base_samples if base_samples is not None else torch.ones(tuple(sample_shape) + (cov.shape[0],), dtype=cov.dtype)
        return mean + z @ L.T, L, torch.tensor(1, dtype=torch.int32)

    monkeypatch.setattr(ops, "mvn_sample", mvn_sample)
    monkeypatch.setattr(ops, "_device_for", lambda *ts: torch.device("cpu"))
    return calls


def _dist():
    cov = torch.tensor([[4.0, 1.0, 0.0], [1.0, 9.0, 0.0], [0.0, 0.0, -1e-17]], dtype=torch.float64)
    return models.MultivariateNormal(torch.tensor([1.0, 2.0, 3.0], dtype=torch.float64), cov), cov


def test_multivariate_normal_fields():
    d, cov = _dist()
    assert d.covariance_matrix is cov and torch.equal(d.mean, torch.tensor([1.0, 2.0, 3.0], dtype=torch.float64)) and d.loc is d.mean
    assert torch.equal(d.variance, torch.tensor([4.0, 9.0, 0.0], dtype=torch.float64))       # the diagonal, clamped at 0
    assert torch.equal(d.stddev, torch.tensor([2.0, 3.0, 0.0], dtype=torch.float64))
    lo, hi = d.confidence_region()
    assert torch.equal(lo, torch.tensor([-3.0, -4.0, 3.0], dtype=torch.float64)) and torch.equal(hi, torch.tensor([5.0, 8.0, 3.0], dtype=torch.float64))
    assert tuple(d.event_shape) == (3,)
    given = models.MultivariateNormal(d.mean, cov, variance=torch.tensor([4.0, 9.0, -2.0], dtype=torch.float64))
    assert torch.equal(given.variance, torch.tensor([4.0, 9.0, 0.0], dtype=torch.float64))
    for mean, c in ((torch.zeros(2, dtype=torch.float64), cov), (torch.zeros(1, 3, dtype=torch.float64), cov), (torch.zeros(3, dtype=torch.float64), cov[None])):
        with pytest.raises(ValueError):
            models.MultivariateNormal(mean, c)


def test_multivariate_normal_sampling_is_one_launch_per_call(stubbed):
    d, cov = _dist()
    z = torch.arange(6, dtype=torch.float64).reshape(2, 3)
    out = d.sample(torch.Size([2]), base_samples=z)
    assert len(stubbed) == 1 and stubbed[0]["shape"] == (2,) and stubbed[0]["base"] is z
    assert out.shape == (2, 3) and d.jitter_used == 1e-8 and len(stubbed) == 1          # (the factor of the last draw is kept)
    np.testing.assert_allclose((d.scale_tril @ d.scale_tril.T).numpy(), (cov + 1e-8 * torch.eye(3, dtype=torch.float64)).numpy(), atol=1e-15)
    assert d.rsample(torch.Size([4, 2]), seed=11).shape == (4, 2, 3) and stubbed[-1]["seed"] == 11 and stubbed[-1]["shape"] == (4, 2)
    assert d.sample().shape == (3,) and stubbed[-1]["shape"] == ()
    fresh, _ = _dist()
    assert fresh.scale_tril.shape == (3, 3) and stubbed[-1]["shape"] == (0,)            # a factor without samples


def test_plugin_export():
    from gabotorch_amd.plugin_api import gpytorch as gp
    from gabotorch_amd import _compat
    if not _compat.HAVE_GPYTORCH:
        assert gp.distributions.MultivariateNormal is models.MultivariateNormal
    assert callable(gp.distributions.MultivariateNormal)
    assert hasattr(models.SingleTaskGP, "forward") and hasattr(models.ExactGP, "forward")
    assert models.SingleTaskGP.forward is not torch.nn.Module.forward and models.ExactGP.forward is not torch.nn.Module.forward


def test_forward_refuses_a_batch_of_test_sets_before_any_launch():
    with pytest.raises(ValueError, match="one test set"):
        models._joint_posterior(None, 1.0, None, None, None, 0.0, torch.zeros(2, 4, 3))


def test_python_wrappers_refuse_host_tensors():
    z = torch.zeros(3, 3, dtype=torch.float64)
    with pytest.raises(ValueError, match="HIP device"):
        ops.gp_posterior_joint(z, z, z, z[0], 0.0, 1.0)
    with pytest.raises(ValueError, match="HIP device"):
        ops.mvn_sample(z[0], z, (2,))


# ---- the fixture ------------------------------------------------------------------------------------------------------------------------------
LETTERS = {
    "beta": ("float64", (1,), "3a782dc88acafd2e210287a7ccbcefda"),
    "dist_test_test": ("float64", (100, 100), "c87dcbd81a7368b4c601f4d7720dae45"),
    "dist_test_train": ("float64", (100, 79), "b2911f149a4be9a51f673a75d804e36c"),
    "dist_train_train": ("float64", (79, 79), "0cece617e558878e001750660e63f4d7"),
    "mean": ("float64", (1,), "af5570f5a1810b7af78caf4bc70a660f"),
    "noise": ("float64", (1,), "3f710ac088db33363087de2b9a657541"),
    "outputscale": ("float64", (1,), "64fa92a0745fda69503e42b2fcff78ae"),
    "train_idx": ("int64", (79,), "ce6d98e007e85777e621fd30fcc21443"),
    "x_test": ("float64", (100, 3), "6018f1291df5a9e5a7b56cc02217e8f0"),
    "y_test": ("float64", (100,), "2eb27737d5f0421f9ea9adf106f63273"),
    "y_train": ("float64", (79,), "7405f0cd51001a6658a1d10aa7a68f7c"),
}


def test_letters_fixture_is_pinned():
    g = load_golden("letters_gp.npz")
    assert sorted(g.files) == sorted(LETTERS)
    for name, (dtype, shape, digest) in LETTERS.items():
        a = np.ascontiguousarray(np.atleast_1d(g[name]))
        assert str(a.dtype) == dtype and a.shape == shape, name
        assert hashlib.sha256(a.tobytes()).hexdigest()[:32] == digest, name
    assert (float(g["beta"]), float(g["outputscale"]), float(g["noise"]), float(g["mean"])) == (1.3, 2000.0, 2.0, 0.0)
    keep = np.delete(np.arange(100), np.hstack((np.arange(24, 37), np.arange(68, 76))))
    assert np.array_equal(g["train_idx"], keep) and np.array_equal(g["y_train"], g["y_test"][keep])
    assert np.array_equal(g["dist_test_train"], g["dist_test_test"][:, keep]) or np.allclose(g["dist_test_train"], g["dist_test_test"][:, keep], atol=1e-12)


def test_letters_problem_needs_the_first_rung_of_the_ladder():
    """numpy on the fixture: the posterior covariance is indefinite by rounding only, so Cholesky fails as it stands and passes with 1e-8"""
    g = load_golden("letters_gp.npz")
    _, cov, cond = cpu.gaussian_posterior(g["dist_train_train"], g["dist_test_train"], g["dist_test_test"], g["y_train"], 1.3, 2000.0, 2.0, 0.0)
    cov = 0.5 * (cov + cov.T)
    lam = np.linalg.eigvalsh(cov)
    assert 3e4 < cond < 5e4 and -1e-10 < lam[0] < 0.0 and 200.0 < lam[-1] < 300.0
    with pytest.raises(np.linalg.LinAlgError):
        np.linalg.cholesky(cov)
    np.linalg.cholesky(cov + 1e-8 * np.eye(100))


def test_normals_of_the_helper_are_standard():
    z = cpu.mvn_normals(12345, 400, 51)
    assert z.shape == (400, 51) and abs(z.mean()) < 0.03 and abs(z.std() - 1.0) < 0.03
    assert np.array_equal(cpu.mvn_normals(12345, 400, 50), z[:, :50])           # coordinates 2k, 2k + 1 from draw k whatever m is
    assert not np.array_equal(cpu.mvn_normals(12346, 400, 51), z)
