"""Host side of the three one-call fit entries (no GPU): gabo_nested_spd_fit_evaluate, gabo_nested_sphere_fit_evaluate and
gabo_nested_sphere_fit_evaluate_series through _lib alone - which error each argument check returns, in which order, all of them before the
first HIP call, and the values of the three *_workspace_bytes functions on a grid (tests/golden/nested_fit_workspace_bytes.json)."""
import ctypes
import json
import math
import os

import pytest

from gabotorch_amd import _lib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "nested_fit_workspace_bytes.json")
NS = (1, 12, 65, 160, 161, 190, 2048)
SPHERE_SHAPES = ((5, 2), (21, 18), (51, 47), (12, 10))          # (D, levels)
SERIES_COEFFS = (1, 2, 33, 129)
SPD_SHAPES = ((5, 2), (10, 3), (12, 4), (32, 31))               # (D, d)
DIM, ARG = _lib.GABO_ERR_DIM, _lib.GABO_ERR_ARG


@pytest.fixture(scope="module", autouse=True)
def _built_library():
    if not os.path.exists(_lib.LIB_PATH):
        from gabotorch_amd import _build
        _build.build()


_buf = (ctypes.c_double * 4096)()
PTR = ctypes.addressof(_buf)


def _sphere_call(n=12, D=5, levels=2, beta=1.0, ws=None, pinned=None, skip=None, null=False):
    lib = _lib.load()
    total = levels * D - levels * (levels - 1) // 2
    ws = lib.gabo_nested_sphere_fit_workspace_bytes(n, D, levels) if ws is None else ws
    pinned = 2 * total + levels + 7 if pinned is None else pinned
    args = [PTR, PTR, PTR, PTR, n, D, levels, beta, 1.0, 0.1, 0.0, 1, PTR, PTR, ws, PTR, pinned, None]
    if null:
        args = [None if a == PTR else a for a in args]
    if skip is not None:
        args[skip] = None
    return lib.gabo_nested_sphere_fit_evaluate(*args)


def _spd_call(n=12, D=5, d=2, theta=1.0, ws=None, pinned=None, skip=None, null=False):
    lib = _lib.load()
    ws = lib.gabo_nested_spd_fit_workspace_bytes(n, D, d) if ws is None else ws
    pinned = 2 * D * d + 7 if pinned is None else pinned
    args = [PTR, PTR, PTR, PTR, n, D, d, theta, 1.0, 0.1, 0.0, 1, PTR, PTR, ws, PTR, pinned, None]
    if null:
        args = [None if a == PTR else a for a in args]
    if skip is not None:
        args[skip] = None
    return lib.gabo_nested_spd_fit_evaluate(*args)


POINTERS = (0, 1, 2, 3, 12, 13, 15)          # positions of the pointer arguments in both signatures


def test_sphere_entry_dimension_errors():
    for null in (False, True):               # (with null pointers too: the dimension error wins over the argument error)
        assert _sphere_call(D=1, levels=1, null=null) == DIM
        assert _sphere_call(D=5, levels=0, null=null) == DIM and _sphere_call(D=5, levels=5, null=null) == DIM
        assert _sphere_call(D=80, levels=10, null=null) == DIM                # latent dimension 70 > 64
        assert _sphere_call(n=0, null=null) == DIM and _sphere_call(n=_lib.GABO_GP_MLL_LARGE_MAX_N + 1, null=null) == DIM
    assert _sphere_call(D=1, levels=1, beta=0.0, ws=0, pinned=0) == DIM
    assert _sphere_call(n=0, beta=math.nan, ws=0, pinned=0) == DIM


def test_spd_entry_dimension_errors():
    for null in (False, True):
        assert _spd_call(D=1, d=1, null=null) == DIM
        assert _spd_call(D=5, d=0, null=null) == DIM and _spd_call(D=5, d=5, null=null) == DIM
        assert _spd_call(D=_lib.GABO_SPD_MAX_DIM + 1, d=2, null=null) == DIM
        assert _spd_call(n=0, null=null) == DIM and _spd_call(n=_lib.GABO_GP_MLL_LARGE_MAX_N + 1, null=null) == DIM
    assert _spd_call(D=_lib.GABO_SPD_MAX_DIM + 1, d=2, theta=0.0, ws=0, pinned=0) == DIM
    assert _spd_call(n=0, theta=math.nan, ws=0, pinned=0) == DIM


@pytest.mark.parametrize("call,shape", [(_sphere_call, dict(D=5, levels=2)), (_sphere_call, dict(D=21, levels=18)), (_spd_call, dict(D=5, d=2)),
                                        (_spd_call, dict(D=12, d=4))], ids=["sphere-5-2", "sphere-21-18", "spd-5-2", "spd-12-4"])
def test_argument_errors(call, shape):
    lib = _lib.load()
    assert call(null=True, **shape) == ARG
    for skip in POINTERS:                     # each pointer null in turn, every other argument valid
        assert call(skip=skip, **shape) == ARG, skip
    for bad in (0.0, -1.0, math.nan):         # beta / theta
        assert call(**{"beta" if call is _sphere_call else "theta": bad}, **shape) == ARG, bad
    if call is _sphere_call:
        D, L = shape["D"], shape["levels"]
        need_ws, need_pinned = lib.gabo_nested_sphere_fit_workspace_bytes(12, D, L), 2 * (L * D - L * (L - 1) // 2) + L + 7
    else:
        D, d = shape["D"], shape["d"]
        need_ws, need_pinned = lib.gabo_nested_spd_fit_workspace_bytes(12, D, d), 2 * D * d + 7
    assert need_ws > 0
    assert call(ws=need_ws - 1, **shape) == ARG and call(pinned=need_pinned - 1, **shape) == ARG
    assert call(ws=0, **shape) == ARG and call(pinned=0, **shape) == ARG


def _grid(lib):
    out = {}
    for n in NS:
        for D, L in SPHERE_SHAPES:
            out[f"sphere:{n}:{D}:{L}"] = int(lib.gabo_nested_sphere_fit_workspace_bytes(n, D, L))
            for nc in SERIES_COEFFS:
                out[f"series:{n}:{D}:{L}:{nc}"] = int(lib.gabo_nested_sphere_fit_series_workspace_bytes(n, D, L, nc))
        for D, d in SPD_SHAPES:
            out[f"spd:{n}:{D}:{d}"] = int(lib.gabo_nested_spd_fit_workspace_bytes(n, D, d))
    return out


def test_workspace_bytes_on_the_recorded_grid():
    with open(GOLDEN) as fh:
        want = json.load(fh)
    got = _grid(_lib.load())
    assert len(got) == len(NS) * (len(SPHERE_SHAPES) * (1 + len(SERIES_COEFFS)) + len(SPD_SHAPES)) and sorted(got) == sorted(want)
    assert all(v > 0 and v % 256 == 0 for v in got.values())
    wrong = {k: (got[k], want[k]) for k in got if got[k] != want[k]}
    assert not wrong, wrong


def test_workspace_bytes_are_zero_for_rejected_arguments():
    lib = _lib.load()
    sphere, series, spd = lib.gabo_nested_sphere_fit_workspace_bytes, lib.gabo_nested_sphere_fit_series_workspace_bytes, lib.gabo_nested_spd_fit_workspace_bytes
    for n, D, L in ((0, 5, 2), (-1, 5, 2), (12, 1, 1), (12, 5, 0), (12, 5, 5), (12, 5, -1)):
        assert sphere(n, D, L) == 0, (n, D, L)
        assert series(n, D, L, 33) == 0, (n, D, L)
    for nc in (0, -1, 130):
        assert series(12, 5, 2, nc) == 0, nc
    for n, D, d in ((0, 5, 2), (-1, 5, 2), (12, 1, 1), (12, 5, 0), (12, 5, 5), (12, 5, 6)):
        assert spd(n, D, d) == 0, (n, D, d)
