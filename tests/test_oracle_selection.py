"""The oracle of the device-side restart selection (oracle/selection.py): its Philox4x32-10 against the known-answer vectors published with the
generator (Random123 kat_vectors: philox4x32, 10 rounds), and the heuristic's invariants."""
import numpy as np
import pytest

from oracle import selection as osel
from tests import _spd_sampler_cases as cases


def test_philox4x32_10_known_answers():
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff, 0xffffffff), (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for ctr, key, want in kat:
        got = osel.philox4x32_10(np.array(ctr, dtype=np.uint32), np.array(key, dtype=np.uint32))
        assert tuple(int(v) for v in got) == want


def test_selection_invariants():
    rng = np.random.default_rng(3)
    y = np.maximum(rng.standard_normal(2048), 0.0) * np.exp(rng.standard_normal(2048))
    for n in (1, 64, 512):
        picked, keys = osel.select_nonneg(y, n, seed=12345)
        assert picked.shape == (n,) and len(set(picked.tolist())) == n
        assert int(np.argmax(y)) in picked
        assert (keys[picked[:-1]] >= 0).all()
    u = osel.selection_uniforms(7, 100000)
    assert 0.0 < u.min() and u.max() <= 1.0 and abs(u.mean() - 0.5) < 5e-3
    assert osel.select_nonneg(-np.ones(8), 2, 1)[0] is None
    assert osel.select_nonneg(np.array([1.0, 0.0, 0.0, 0.0]), 2, 1)[0] is None
    # frequencies of a single draw follow the weights
    yy = np.array([1.0, 0.8, 0.5, 0.2])
    w = np.exp(2.0 * (yy / yy.max() - 1.0))
    counts = np.zeros(4)
    for seed in range(4000):
        counts[osel.select_nonneg(yy, 1, seed, eta=2.0, alpha=1e-9)[0][0]] += 1
    # (the arg-max is forced in when n = 1 misses it: a single draw always returns index 0 - so test the race itself through the keys)
    wins = np.zeros(4)
    for seed in range(4000):
        wins[int(np.argmax(osel.select_nonneg(yy, 1, seed, eta=2.0, alpha=1e-9)[1]))] += 1
    np.testing.assert_allclose(wins / 4000, w / w.sum(), atol=0.03)


def test_sphere_sampler_oracle_is_uniform_on_the_sphere():
    """oracle.selection.sphere_samples (what sphere_sample_kernel draws): unit rows, reproducible per (seed, index), independent of how many are drawn,
    and the distribution of [3P] Sphere.rand - coordinates with mean 0 and variance 1 / dim, no preferred direction."""
    a = osel.sphere_samples(99, 4096, 10)
    np.testing.assert_allclose(np.linalg.norm(a, axis=1), 1.0, rtol=0, atol=1e-15)
    np.testing.assert_array_equal(a[:100], osel.sphere_samples(99, 100, 10))          # addressed by sample index
    assert np.abs(a - osel.sphere_samples(100, 4096, 10)).max() > 0.1                  # another seed, another draw
    assert np.abs(a.mean(0)).max() < 0.02 and np.abs(a.var(0) - 0.1).max() < 0.01
    cov = a.T @ a / 4096
    assert np.abs(cov - np.eye(10) / 10).max() < 0.01
    odd = osel.sphere_samples(5, 1000, 7)                                              # odd dimension: the second deviate of the last pair is dropped
    np.testing.assert_allclose(np.linalg.norm(odd, axis=1), 1.0, rtol=0, atol=1e-15)
    assert odd.shape == (1000, 7) and np.abs(odd.mean(0)).max() < 0.06


@pytest.mark.parametrize("d", cases.ORDERS)
def test_spd_sampler_oracle_has_the_spectrum_it_drew(d):
    """oracle.selection.spd_samples at every order the device sampler takes, both seeds of the device test: X is symmetric with the eigenvalues
    lam (so Q is orthogonal to the working precision), lam lies in [min_eig, max_eig], kappa >= 1 (= 1 exactly when there is one column)"""
    for seed in cases.SEEDS:
        X, lam, kappa = cases.oracle(seed, 0, cases.N, d)
        assert X.shape == (cases.N, d, d) and lam.shape == (cases.N, d) and kappa.shape == (cases.N,)
        np.testing.assert_array_equal(X, X.transpose(0, 2, 1))
        assert lam.min() >= cases.LO and lam.max() <= cases.HI
        np.testing.assert_allclose(np.linalg.eigvalsh(X), np.sort(lam, axis=1), rtol=0, atol=cases.spectrum_bound(d))
        assert kappa.min() >= 1.0 and np.isfinite(kappa).all() and (d > 1 or (kappa == 1.0).all())
    # equal bounds: every sample is that multiple of the identity
    X, lam, _ = cases.oracle(cases.SEEDS[0], 0, 5, d, 2.0, 2.0)
    np.testing.assert_array_equal(lam, 2.0)
    np.testing.assert_allclose(X, np.broadcast_to(2.0 * np.eye(d), X.shape), rtol=0, atol=16 * d * cases.EPS * 2.0)


def test_spd_sampler_oracle_is_addressed_by_seed_and_sample_index():
    """sample i depends on (64-bit seed, 64-bit index first + i) only: overlapping ranges agree bit for bit, also across the counter's low word; the
    high word of the counter and the high word of the key each change the draw"""
    seed = cases.SEEDS[1]
    for d in (3, 10):
        whole = cases.oracle(seed, 0, cases.N, d)
        part = osel.spd_samples(seed, 37, 50, d, cases.LO, cases.HI)
        for a, b in zip(whole, part):
            np.testing.assert_array_equal(a[37:87], b)
        high = cases.oracle(seed, cases.FIRST_HIGH, 8, d)                   # indices 2^32 - 3 ... 2^32 + 4
        tail = osel.spd_samples(seed, 2 ** 32 + 1, 6, d, cases.LO, cases.HI)    # 2^32 + 1 ... 2^32 + 6
        for a, b in zip(high, tail):
            np.testing.assert_array_equal(a[4:8], b[:4])
        # index 2^32 + i is not index i (a counter cut to its low word would say so)
        assert np.abs(high[0][3:8] - whole[0][0:5]).max() > 0.1 and np.abs(high[1][3:8] - whole[1][0:5]).max() > 0.01
        # nor is seed + 2^32 the seed (a key cut to its low word), nor the low word alone
        for other in (seed ^ (1 << 32), seed & 0xFFFFFFFF, seed ^ (1 << 63)):
            assert np.abs(osel.spd_samples(other, 0, 5, d, cases.LO, cases.HI)[0] - whole[0][:5]).max() > 0.1
    assert np.abs(cases.oracle(0, 0, cases.N, 4)[0] - cases.oracle(1 << 32, 0, cases.N, 4)[0]).max() > 0.1


def test_spd_sampler_oracle_in_double_stays_within_a_quarter_of_the_device_bound():
    """The reference against itself: the same statements in plain double with numpy's libm (log, cos, sin a few ulp from the correctly rounded values,
    like the device's) against the extended-precision run, for EVERY case the device is compared on - per sample within a quarter of the bound the
    device gets, 16 d eps kappa_i max_eig / 4.  (Where np.longdouble is no wider than double the two runs differ by libm's 2 pi only.)"""
    worst = 0.0
    for seed, first, count, d in cases.CASES:
        X, lam, kappa = cases.oracle(seed, first, count, d)
        Xd, lamd, kappad = osel.spd_samples(seed, first, count, d, cases.LO, cases.HI, work=np.float64)
        err = np.abs(Xd - X).reshape(count, -1).max(1)
        ratio = err / (0.25 * cases.bound(d, kappa))
        worst = max(worst, float(ratio.max()))
        assert (ratio <= 1.0).all(), (hex(seed), first, d, int(np.argmax(ratio)), float(ratio.max()), float(kappa[np.argmax(ratio)]))
        np.testing.assert_allclose(lamd, lam, rtol=0, atol=4 * cases.EPS * cases.HI)
        np.testing.assert_allclose(kappad, kappa, rtol=1e-6)
    print(f"double-precision oracle against the extended one: worst error / (bound / 4) = {worst:.3f}")
