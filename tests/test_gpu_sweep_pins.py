"""Twelve tiny native sweeps (native_sweep.py: six through the SPD driver, six through the sphere driver) against what the same sweeps returned
before the drivers moved into that module: tests/golden/sweep_pins.npz, written by tests/golden/make_golden_sweep_pins.py, which also holds the
cases.  Exact: the candidate's bytes, the log's costs, iteration counts, constraint values, picks, key set and flags, the warnings' categories,
and where numpy's and torch's global generators stand afterwards.  Needs an MI355X."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _module():
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "make_golden_sweep_pins.py")
    spec = importlib.util.spec_from_file_location("make_golden_sweep_pins", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


PINS = _module()


@pytest.mark.parametrize("name", list(PINS.CASES))
def test_sweep_returns_what_it_returned_before_the_drivers_moved(golden, name):
    want = golden("sweep_pins.npz")
    keys = PINS.HOST_KEYS + (() if name in want["host_only"] else PINS.DEVICE_KEYS)      # (host_only: device bytes that differed between the recorder's own runs)
    got = PINS.run_case(name)
    for key in keys:
        print(name, key, got[key].tolist())
    for key in keys:
        w = want[f"{name}/{key}"]
        assert got[key].dtype == w.dtype and got[key].shape == w.shape, key
        assert got[key].tobytes() == w.tobytes(), key
    if name.startswith("sphere_constrained"):
        assert got["final_constraints"].shape == (PINS.RESTARTS, 2)
    if name == "spd_selection_flag_fallback":
        assert got["warnings"].tolist() == ["BadInitialCandidatesWarning"] and "device_selection" in got["log_false"]
    assert len(PINS.CASES) == 12 and len(want["host_only"]) <= 2 and set(want["host_only"].tolist()) <= set(PINS.CASES)
