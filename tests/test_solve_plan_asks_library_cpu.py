"""BatchedTrustRegions._solve_device chooses the single-launch solve on the library's word (gabo_spd_tr_solve_supported), whatever the dimension: it
holds no dimension limit of its own.  The library is replaced by a stub here, so no GPU is needed: with a stub that says yes at d = 10 the single
launch is chosen, with one that says no the propose / update launches are - and the question reaches the library with the problem's restart count,
dimension and number of constraints."""
import functools
import types

import pytest
import torch

from gabotorch_amd import _lib
from gabotorch_amd.manifold_optimization import batched_trust_regions as btr
from gabotorch_amd.Riemannian_utils import spd_constraints_utils_torch as scut


class _Library:
    def __init__(self, solve_supported):
        self.answer, self.asked = solve_supported, []

    def gabo_spd_tr_propose_supported(self, flags, d):
        return 1

    def gabo_spd_tr_solve_supported(self, acq, r, d, n_constraints, lift_dim):
        self.asked.append((r, d, n_constraints, lift_dim))
        return self.answer


def _choose(monkeypatch, d, supported, constraints):
    lib = _Library(supported)
    monkeypatch.setattr(btr, "_library", lambda: lib)
    solver = btr.BatchedTrustRegions(maxiter=3)
    chosen = []
    monkeypatch.setattr(solver, "_single_launch_solve", lambda *a: chosen.append("single_launch"))
    monkeypatch.setattr(solver, "_propose_update_launches", lambda *a: chosen.append("propose_update"))
    monkeypatch.setattr(solver, "_tcg_launches", lambda *a: chosen.append("tcg_launches"))
    fused = types.SimpleNamespace(family="spd", single_launch=True, mode=_lib.GABO_OUT_GAUSSIAN, metric=_lib.GABO_METRIC_AFFINE_INVARIANT,
                                  acq_params=lambda: _lib.AcqParams())
    problem = types.SimpleNamespace(fused=fused)
    x = torch.eye(d, dtype=torch.float64).repeat(7, 1, 1)
    solver._solve_device(problem, x, [], constraints, 1, 5, 10.0, 1.0, 1e-6)
    return chosen, lib.asked


@pytest.mark.parametrize("d", [5, 8, 10, 12])
def test_the_single_launch_is_chosen_on_the_librarys_word_at_any_dimension(monkeypatch, d):
    box = [functools.partial(scut.max_eigenvalue_constraint_torch, maximum_eigenvalue=2.6),
           functools.partial(scut.min_eigenvalue_constraint_torch, minimum_eigenvalue=0.3)]
    for cons in ([], box):
        chosen, asked = _choose(monkeypatch, d, 1, cons)
        assert chosen == ["single_launch"] and asked == [(7, d, len(cons), 0)]
        chosen, asked = _choose(monkeypatch, d, 0, cons)
        assert chosen == ["propose_update"] and asked == [(7, d, len(cons), 0)]


def test_a_host_callable_keeps_the_launch_per_iteration_plans_without_asking(monkeypatch):
    chosen, asked = _choose(monkeypatch, 10, 1, [lambda m: scut.max_eigenvalue_constraint_torch(m, 2.6)])
    assert chosen == ["propose_update"] and asked == []
