"""The three one-call fit entries (gabo_nested_sphere_fit_evaluate, gabo_nested_sphere_fit_evaluate_series, gabo_nested_spd_fit_evaluate) called
directly through _lib with seeded inputs, against the out_host vectors recorded from the build before the entries shared one host chain
(tests/golden/nested_fit_entries.npz).  Every entry returned identical bytes on five calls of that build, so the comparison is exact.
The three cases on the tiled likelihood (n = 190, 190, 170) were recorded again, five identical calls each, when gabo_gp_mll_large began to take
its pivot blocks in Cholesky-factored form (csrc/gp_mll_large.hip; judged by tests/test_gpu_gp_ill_conditioned.py): they moved by at most 1.5e-11
of an entry and 3.5e-14 of the largest entry of their vector.  The host chain around that launch is pinned by the other ten.

Shapes - the smallest at which the host chain takes another path: n = 65 is one row past a wave, n = 190 / 170 the tiled likelihood above
GABO_GP_MLL_MAX_N = 160, n = 1 the degenerate Gram matrix; (21, 18) has 18 projection levels."""
import ctypes
import functools
import math
import os

import numpy as np
import pytest
import torch

from gabotorch_amd import _lib, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "nested_fit_entries.npz")

SPHERE_SHAPES = [(5, 2, 12), (21, 18, 65), (12, 10, 190), (5, 2, 1)]                    # (D, levels, n)
SPD_SHAPES = [(5, 2, 10), (10, 3, 65), (12, 4, 170), (5, 2, 1)]                         # (D, d, n)
# (entry, shape, series) - series = (nu, levels of the series) or None
CASES = ([("gauss", s, None) for s in SPHERE_SHAPES] + [("series", s, (2.5, 32)) for s in SPHERE_SHAPES] + [("series", SPHERE_SHAPES[0], (math.inf, 1))]
         + [("spd", s, None) for s in SPD_SHAPES])
NPD_CASES = [("gauss", SPHERE_SHAPES[0], None), ("series", SPHERE_SHAPES[0], (2.5, 32)), ("spd", SPD_SHAPES[0], None)]
SCALARS = (0.6, 1.3, 0.1, 0.15)              # beta / kappa / theta, outputscale, noise, mean
NPD_NOISE = -10.0


def case_id(case):
    entry, shape, series = case
    return "{}-{}-{}-n{}".format(entry, *shape) + ("" if series is None else "-nu{}-L{}".format(*series))


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _unit_rows(a):
    return a / np.sqrt((a * a).sum(axis=1, keepdims=True))


@functools.lru_cache(maxsize=None)
def _inputs(entry, shape):
    """the device and host arrays of a shape, drawn once (numpy's default_rng; the SPD points by ops.spd_sample with a fixed seed)"""
    D, L, n = shape
    rng = np.random.default_rng(1000 * D + 10 * L + n)
    dev = torch.device(DEV)
    y = torch.tensor(rng.standard_normal(n), device=dev)
    if entry == "spd":
        xv = ops.spd_sample(n, D, 0.5, 2.0, 7 + D, dev, mandel=True)
        W = rng.standard_normal((D, L))
        for c in range(L):                   # Gram-Schmidt, in plain sums: a point of the Grassmannian
            for b in range(c):
                W[:, c] -= (W[:, c] * W[:, b]).sum() * W[:, b]
            W[:, c] /= math.sqrt((W[:, c] * W[:, c]).sum())
        return xv, ops.mandel_to_matrix(xv).contiguous(), y, np.ascontiguousarray(W)
    x = torch.tensor(_unit_rows(rng.standard_normal((n, D))), device=dev)
    axes = np.concatenate([_unit_rows(rng.standard_normal((1, D - k)))[0] for k in range(L)])
    return x, y, np.ascontiguousarray(axes), np.full(L, math.pi / 2)


def evaluate(case, want_grad, noise=SCALARS[2]):
    """one call of the case's entry -> (status, out_host)"""
    entry, shape, series = case
    D, L, n = shape
    lib = _lib.load()
    dev = torch.device(DEV)
    theta, outputscale, _, mean = SCALARS
    stream = ops._stream_ptr(dev)
    with torch.cuda.device(dev):
        if entry == "spd":
            xv, xm, y, W = _inputs(entry, shape)
            ws = torch.empty(int(lib.gabo_nested_spd_fit_workspace_bytes(n, D, L)), dtype=torch.uint8, device=dev)
            pinned = torch.empty(2 * D * L + 7, dtype=torch.float64).pin_memory()
            out = np.full(7 + D * L, np.nan)
            rc = lib.gabo_nested_spd_fit_evaluate(xv.data_ptr(), xm.data_ptr(), y.data_ptr(), _ptr(W), n, D, L, theta, outputscale, noise, mean,
                                                  want_grad, _ptr(out), ws.data_ptr(), ws.numel(), pinned.data_ptr(), pinned.numel(), stream)
            return rc, out
        x, y, axes, dists = _inputs(entry, shape)
        total = axes.size
        out = np.full(7 + total, np.nan)
        if entry == "gauss":
            ws = torch.empty(int(lib.gabo_nested_sphere_fit_workspace_bytes(n, D, L)), dtype=torch.uint8, device=dev)
            pinned = torch.empty(2 * total + L + 7, dtype=torch.float64).pin_memory()
            rc = lib.gabo_nested_sphere_fit_evaluate(x.data_ptr(), y.data_ptr(), _ptr(axes), _ptr(dists), n, D, L, theta, outputscale, noise, mean,
                                                     want_grad, _ptr(out), ws.data_ptr(), ws.numel(), pinned.data_ptr(), pinned.numel(), stream)
            return rc, out
        p, dp, _ = ops.sphere_matern_coefficients_and_derivative(D - L, theta, series[0], series[1])
        assert p.size == series[1] + 1
        ws = torch.empty(int(lib.gabo_nested_sphere_fit_series_workspace_bytes(n, D, L, p.size)), dtype=torch.uint8, device=dev)
        pinned = torch.empty(2 * total + L + 1 + 4 * p.size + 7, dtype=torch.float64).pin_memory()
        rc = lib.gabo_nested_sphere_fit_evaluate_series(x.data_ptr(), y.data_ptr(), _ptr(axes), _ptr(dists), n, D, L, _ptr(p), _ptr(dp), int(p.size),
                                                        outputscale, noise, mean, want_grad, _ptr(out), ws.data_ptr(), ws.numel(), pinned.data_ptr(),
                                                        pinned.numel(), stream)
        return rc, out


@functools.lru_cache(maxsize=None)
def _golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_entry_returns_the_recorded_vector(case):
    rc1, with_grad = evaluate(case, 1)
    rc0, values = evaluate(case, 0)
    assert rc1 == _lib.GABO_OK and rc0 == _lib.GABO_OK
    assert with_grad[5] == 0.0 and np.isfinite(with_grad).all()
    # want_grad = 0: the same six numbers, bit for bit, and zeros behind them
    np.testing.assert_array_equal(values[:6], with_grad[:6])
    assert values[6] == 0.0 and not values[7:].any()
    golden = _golden()
    np.testing.assert_array_equal(with_grad, golden[case_id(case) + "-g1"])
    np.testing.assert_array_equal(values, golden[case_id(case) + "-g0"])


@pytest.mark.parametrize("case", NPD_CASES, ids=case_id)
def test_covariance_that_is_not_positive_definite_is_flagged(case):
    """noise = -10: outputscale K + noise I has negative eigenvalues; the call returns GABO_OK and out[5] carries the flag"""
    rc, out = evaluate(case, 1, noise=NPD_NOISE)
    assert rc == _lib.GABO_OK
    flag = _golden()[case_id(case) + "-npd"]
    assert flag.shape == (1,) and flag[0] != 0.0
    assert out[5] == flag[0]
