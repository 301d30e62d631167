"""Checks of the reference that judges the GP dense-algebra launches on nearly singular matrices (tests/_cpu_gp_dense.py), none of which needs a
GPU: the longdouble route against mpmath at 50 digits, the conditions every input of tests/test_gpu_gp_ill_conditioned.py has to meet - stated
as conditions, not as measurements - and the construction of the matrices that are not positive definite."""
import numpy as np
import pytest

from tests import _cpu_gp_dense as cpu

LD = np.longdouble
WINDOW = {"benign": (0.0, 1e4), "mid": (1e6, 1e10), "hard": (1e7, 1e13)}          # cond_2(Ky) of a level


def test_longdouble_is_the_extended_format():
    """the bounds below (2^-64) and the margin over the fp64 tolerances assume the 64-bit significand of x87"""
    assert np.finfo(LD).eps <= 2.0 ** -63


@pytest.mark.parametrize("gram", [False, True])
@pytest.mark.parametrize("level", list(cpu.LEVELS))
@pytest.mark.parametrize("n", [5, 30, 40])
def test_longdouble_reference_agrees_with_mpmath(n, level, gram):
    """the five outputs within 64 cond 2^-64 x (sum of absolute terms), alpha within 64 cond 2^-64 max |alpha|: 256 times below the smallest
    tolerance (4 cond 2^-53 ...) an fp64 result is held to against it"""
    e, y, theta, outputscale, noise, mean = cpu.case(n, level)
    ref = cpu.case_reference(n, level, gram)
    want, want_alpha = cpu.reference_mp(cpu.gram_of(n, level) if gram else e, y, theta, outputscale, noise, mean, gram=gram)
    tol = 64.0 * ref.cond * cpu.U_LD * ref.scale
    err = np.array([float(abs(ref.out[i] - cpu.mp_to_longdouble(want[i]))) for i in range(5)])
    alpha = np.array([cpu.mp_to_longdouble(v) for v in want_alpha])
    tol_alpha = 64.0 * ref.cond * cpu.U_LD * float(np.max(np.abs(alpha)))
    err_alpha = float(np.max(np.abs(ref.alpha - alpha)))
    print(f"n {n} {level} gram {gram}: cond {ref.cond:.3e}; error / tolerance "
          + ", ".join(f"{name} {a / b:.3g}" for name, a, b in zip(cpu.NAMES, err, tol) if b > 0.0) + f", alpha {err_alpha / tol_alpha:.3g}")
    for i in range(5):
        assert err[i] <= tol[i], (cpu.NAMES[i], err[i], tol[i])
    assert err_alpha <= tol_alpha
    if gram:
        assert ref.out[1] == 0.0 and ref.scale[1] == 0.0 and want[1] == 0


ALL_CASES = sorted(set(cpu.MLL_CASES + cpu.FACTOR_CASES + [(n, "benign") for n in cpu.FLAG_POSITIONS] + [cpu.REPEAT_CASE]))


@pytest.mark.parametrize("n,level", ALL_CASES)
def test_inputs_meet_the_conditions_the_device_tests_rely_on(n, level):
    """cond_2(Ky) lies in the window of the level, and the smallest pivot is at least 64 n 2^-53 ||Ky||_2: positive definite beyond the rounding
    of any fp64 elimination, so that `must not be flagged` is a fair demand"""
    _, _, _, outputscale, noise, _ = cpu.case(n, level)
    for gram in (False, True):
        ref = cpu.case_reference(n, level, gram)
        lo, hi = WINDOW[level]
        assert lo <= ref.cond < hi, (ref.cond, lo, hi)
        ky = outputscale * cpu.gram_of(n, level) + noise * np.eye(n)
        floor = 64.0 * n * cpu.U * np.linalg.norm(ky, 2)
        print(f"n {n} {level} gram {gram}: cond {ref.cond:.3e}, smallest pivot {float(ref.pivots.min()):.3e} >= {floor:.3e}")
        assert float(ref.pivots.min()) >= floor
        assert (level == "benign") == (noise == 0.05)
        assert np.array_equal(ref.kinv, ref.kinv.T) and np.array_equal(ref.W, ref.W.T) and np.array_equal(ref.linv, np.tril(ref.linv))


@pytest.mark.parametrize("n", cpu.LIMIT_SIZES)
def test_the_cases_at_the_size_limit_are_benign(n):
    e, _, theta, outputscale, noise, _ = cpu.case(n, "benign")
    cond = np.linalg.cond(outputscale * np.exp(-theta * e) + noise * np.eye(n))
    assert cond < WINDOW["benign"][1], cond


def test_numpy_route_constant_is_below_the_project_constant():
    """c of tests/test_gpu_gp_ill_conditioned.py on the cases that cost nothing here (its own import evaluates the whole table)"""
    worst = cpu.numpy_route_constant([(n, level) for n, level in cpu.MLL_CASES if n <= 42])
    print(f"|numpy route - reference| <= {worst:.3f} cond 2^-53 scale for n <= 42")
    assert 0.0 < 4.0 * worst <= 8.0


@pytest.mark.parametrize("n,pos", [(n, pos) for n, positions in cpu.ZERO_POSITIONS.items() if n <= 161 for pos in positions])
def test_zero_pivot_at_gives_an_exact_zero_and_leaves_the_rest_positive_definite(n, pos):
    _, _, _, outputscale, _, _ = cpu.case(n, "benign")
    bad, noise = cpu.zero_pivot_at(cpu.gram_of(n, "benign"), outputscale, pos)
    assert outputscale * bad[pos, pos] + noise == 0.0 and float(LD(outputscale) * LD(bad[pos, pos]) + LD(noise)) == 0.0      # rounded twice or once
    assert not bad[pos, :pos].any() and not bad[pos + 1:, pos].any() and np.array_equal(bad, bad.T)
    ky = LD(outputscale) * bad.astype(LD) + LD(noise) * np.eye(n, dtype=LD)
    with pytest.raises(np.linalg.LinAlgError) as info:
        cpu.ld_cholesky(ky)
    assert info.value.args[0] == pos
    rest = np.delete(np.delete(ky, pos, 0), pos, 1)
    assert float((np.diagonal(cpu.ld_cholesky(rest)) ** 2).min()) >= 64.0 * n * cpu.U * np.linalg.norm(rest.astype(np.float64), 2)


@pytest.mark.parametrize("n,pos", [(n, pos) for n, positions in cpu.FLAG_POSITIONS.items() for pos in positions])
def test_indefinite_at_moves_one_pivot_below_zero_and_none_before_it(n, pos):
    _, y, _, outputscale, noise, _ = cpu.case(n, "benign")
    k = cpu.gram_of(n, "benign")
    bad = cpu.indefinite_at(k, y, outputscale, noise, pos)
    assert np.array_equal(bad[:pos, :pos], k[:pos, :pos]) and np.array_equal(bad, bad.T)
    ky = LD(outputscale) * bad.astype(LD) + LD(noise) * np.eye(n, dtype=LD)
    with pytest.raises(np.linalg.LinAlgError) as info:
        cpu.ld_cholesky(ky)
    assert info.value.args[0] == pos                               # the first pivot that is not positive is pivot pos
    pivots = cpu.case_reference(n, "benign", True).pivots
    lead = np.diagonal(cpu.ld_cholesky(ky[:pos, :pos])) ** 2 if pos else np.zeros(0, dtype=LD)
    assert np.all(np.abs(lead - pivots[:pos]) <= 1e-12 * pivots[:pos])
    # pivot pos itself: Ky'[pos, pos] - Ky[pos, pos] + pivots[pos] = -0.1 up to the rounding of the fp64 entry
    shifted = float(ky[pos, pos] - (LD(outputscale) * LD(k[pos, pos]) + LD(noise)) + pivots[pos])
    assert abs(shifted + 0.1) <= 8.0 * cpu.U * (abs(outputscale * k[pos, pos]) + 0.1 + float(pivots[pos]))
    with pytest.raises(np.linalg.LinAlgError):
        np.linalg.cholesky(outputscale * bad + noise * np.eye(n))
