"""The host side of the sweep's initial conditions, without a GPU and without the library: gen_batch_initial_conditions_manifold on CPU tensors
with a plain Python acquisition callable.  What it picks, how often it calls manifold.rand and where it leaves numpy's and torch's global
generators are behaviour that the native sweep drivers share (one host sampler, one retry loop): every figure below is a literal recorded before
those steps were stated once."""
import warnings

import numpy as np
import pytest
import torch

from gabotorch_amd import manifolds, models
from gabotorch_amd.manifold_optimization import manifold_optimize as mo

RAW = 6


def _nonneg(X):
    return X[:, 0, 0].clamp_min(0.0) ** 2 + 0.01 * (X[:, 0, 1] > 0)


def _signed(X):
    return X[:, 0, 0] + 0.5 * X[:, 0, 1]


def _zero(X):
    return torch.zeros(X.shape[0], dtype=X.dtype)


def _run(acq, num_restarts, options):
    man = manifolds.Sphere(3)
    calls, rand = [0], man.rand

    def counted():
        calls[0] += 1
        return rand()
    man.rand = counted
    np.random.seed(11)
    torch.manual_seed(11)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        chosen = mo.gen_batch_initial_conditions_manifold(acq, man, None, None, num_restarts, RAW, options=options)
    after = (int(np.random.randint(2 ** 31)), int(torch.randint(2 ** 31, (1,))))
    bad = [w for w in caught if issubclass(w.category, models.BadInitialCandidatesWarning)]
    assert len(bad) == len(caught)
    return chosen, calls[0], after, len(bad)


def _rows(chosen, total, batched):
    """indices of the chosen points among the `total` samples of the attempt they came from, redrawn from the same seed"""
    np.random.seed(11)
    man = manifolds.Sphere(3)
    pts = None
    for attempt in range(1, total // RAW + 1):
        pts = man.rand_batch(RAW * attempt) if batched else np.stack([man.rand() for _ in range(RAW * attempt)])
    out = []
    for row in chosen[:, 0].numpy():
        hit = np.nonzero((pts == row).all(1))[0]
        assert len(hit) == 1
        out.append(int(hit[0]))
    return out


# (acquisition, num_restarts, options) -> (rows, total of the attempt they came from, manifold.rand calls, (next numpy, next torch), warnings)
CASES = {
    "nonneg": (_nonneg, 2, {"nonnegative": True}),
    "signed": (_signed, 2, {}),
    "nonneg_all_rows": (_nonneg, 6, {"nonnegative": True}),
    "signed_all_rows": (_signed, 6, {}),
    "nonneg_batched_rand": (_nonneg, 2, {"nonnegative": True, "batched_rand": True}),
    "signed_batched_rand": (_signed, 2, {"batched_rand": True}),
    "zero_everywhere": (_zero, 2, {"nonnegative": True}),
    "zero_everywhere_signed": (_zero, 2, {}),
}
EXPECTED = {
    "nonneg": ([2, 0], 6, 6, (239116623, 707468379), 0),
    "signed": ([1, 0], 6, 6, (239116623, 707468379), 0),
    "nonneg_all_rows": ([0, 1, 2, 3, 4, 5], 6, 6, (239116623, 707468379), 0),
    "signed_all_rows": ([0, 1, 2, 3, 4, 5], 6, 6, (239116623, 707468379), 0),
    "nonneg_batched_rand": ([1, 2], 6, 0, (293375679, 707468379), 0),
    "signed_batched_rand": ([1, 0], 6, 0, (293375679, 707468379), 0),
    "zero_everywhere": ([11, 17], 24, 60, (530413876, 451723847), 1),          # 6 + 12 + 18 + 24 draws
    "zero_everywhere_signed": ([11, 17], 24, 60, (530413876, 451723847), 1),
}
EXPECTED_EMPTY = {False: 54893165, True: 293375679}          # batched_rand -> the next np.random.randint(2 ** 31) after an empty draw


@pytest.mark.parametrize("name", list(CASES))
def test_initial_conditions_rows_rand_calls_and_generator_state(name):
    acq, num_restarts, options = CASES[name]
    rows, total, rand_calls, after, n_warnings = EXPECTED[name]
    chosen, calls, got_after, got_warnings = _run(acq, num_restarts, options)
    assert chosen.shape == (num_restarts, 1, 3) and chosen.dtype == torch.float64
    assert _rows(chosen, total, bool(options.get("batched_rand"))) == rows
    assert calls == rand_calls
    assert got_after == after
    assert got_warnings == n_warnings


def test_zero_acquisition_makes_four_attempts_of_growing_size(monkeypatch):
    totals = []
    score = mo._score_raw_samples
    monkeypatch.setattr(mo, "_score_raw_samples", lambda acq, X, post, options: (totals.append(X.shape[0]), score(acq, X, post, options))[1])
    with pytest.warns(models.BadInitialCandidatesWarning) as caught:
        mo.gen_batch_initial_conditions_manifold(_zero, manifolds.Sphere(3), None, None, 2, RAW, options={"nonnegative": True})
    assert totals == [6, 12, 18, 24] and len(caught) == 1


@pytest.mark.parametrize("batched", [False, True])
def test_draw_of_an_empty_shard(batched):
    """count = 0 under world = 1: the loop form calls manifold.rand once for the point shape (and consumes that draw); rand_batch(0) draws its seed"""
    man = manifolds.Sphere(3)
    calls, rand = [0], man.rand

    def counted():
        calls[0] += 1
        return rand()
    man.rand = counted
    np.random.seed(11)
    pts = mo._draw_raw_samples(man, 6, 0, 0, {"batched_rand": batched}, torch.float64)
    assert pts.shape == (0, 1, 3) and pts.dtype == torch.float64
    assert calls[0] == (0 if batched else 1)
    assert int(np.random.randint(2 ** 31)) == EXPECTED_EMPTY[batched]

