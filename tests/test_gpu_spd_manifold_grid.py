"""Every two-operand SPD-manifold operation (gabo_spd_manifold_op: exp, log, dist, inner, norm, egrad2rgrad, ehess2rhess) at every order class and
in every launch shape, against a 50-digit truth; and the sphere operations (gabo_sphere_manifold_op) against longdouble evaluations of their formulas.

Launch shapes.  The C entry chooses among three instantiations (csrc/spd_manifold.hip, gabo_spd_manifold_op: `if (d > 12 && n < 1024)` ... `else if
(d >= kWaveEighMinDim)` ... `else`, kWaveEighMinDim = 5 in wave_eigh.hpp):
    spd_manifold_kernel<64, false>   Jacobi                    d < 5
    spd_manifold_kernel<64, true>    one wave, wave_eigh       d >= 5, unless the next row applies
    spd_manifold_kernel<256, true>   four waves, barriers live d > 12 and n < 1024
The small batch here is the fixture's four cases of an order (n = 4: rows 1, 2, 3 by d); the large one, for d > 12, is the same four cases tiled to
n = 1028 >= 1024 (row 2).  WHOEVER CHANGES THE RULE MOVES THESE SIZES (SMALL_N, LARGE_N, the order lists of tests/_cpu_spd_manifold.py).

Truth and tolerances.  tests/golden/spd_manifold_grid.npz (make_golden_spd_manifold_grid.py, mpmath at 50 digits, not needed here) holds, per order
d in 1..12, 13, 16, 17, 24, 31, 32, four point pairs - A well-conditioned, B base point of condition 1e8, C a hair apart (M = I + 1e-6 S), D far
apart (eigenvalues of M over exp(+-6)) - with Log_X(Y), Exp_X(U), dist, inner, norm rounded once from 50 digits, and eref(op, family): the worst
relative error over all orders of two fp64 CPU routes (the oracle's functions; plain-numpy Cholesky whitening) against that truth.  The device is held to
    tol(op, family) = max(10 x eref(op, family), 1e-12),         error = max|got - truth| / max|truth|
(10: the project's margin over a reference's own fp64 uncertainty; 1e-12: the bar of the eigen-solver's logm), and the two polynomial operations to
1e-11 of max|truth| against np.longdouble products.  test_spd_manifold_grid_cpu.py asserts on the references alone that every tol is <= 1e-7 and that
the families are in their regimes.  eref as generated:
              A         B         C         D
    log    6.02e-15  6.35e-11  5.38e-10  6.84e-12
    exp    1.55e-15  1.06e-11  1.40e-15  6.12e-15
    dist   1.16e-15  4.60e-09  1.93e-10  4.95e-13
    inner  4.71e-16  3.83e-09  1.16e-14  3.06e-16
    norm   3.21e-16  1.21e-09  2.16e-16  3.99e-16

Worst device error / bound on an MI355X, per (operation, family) and launch shape (every order that takes the shape):
                   <64,false>  d = 1..4, n = 4           <64,true>  d = 5..12, n = 4 and          <256,true>  d = 13..32, n = 4
                                                         d = 13..32, n = 1028
                     A       B       C       D          A       B       C       D           A       B       C       D
    log           3.4e-03 2.5e-03 1.3e-01 6.1e-04    6.6e-03 8.7e-02 9.3e-02 3.1e-02     6.6e-03 8.7e-02 6.5e-02 3.1e-02
    exp           8.1e-04 6.6e-03 6.0e-04 2.4e-03    1.0e-03 4.5e-02 1.4e-03 3.2e-03     1.0e-03 3.0e-02 8.9e-04 2.5e-03
    dist          2.1e-03 5.5e-02 7.6e-02 9.7e-04    6.4e-04 1.3e-02 2.2e-02 5.5e-02     6.4e-04 3.1e-03 1.4e-02 1.6e-02
    inner         2.3e-04 7.2e-02 2.3e-04 4.0e-04    1.5e-03 1.6e-02 8.1e-03 1.3e-03     1.2e-03 1.5e-03 3.0e-03 1.3e-03
    norm          1.8e-04 1.1e-01 1.4e-04 1.8e-04    1.1e-03 1.5e-02 7.3e-04 5.1e-04     1.1e-03 2.3e-03 7.3e-04 5.1e-04
    egrad2rgrad   2.4e-05 9.0e-06 2.8e-05 2.9e-05    3.1e-05 9.1e-05 3.9e-05 3.2e-05     3.1e-05 9.1e-05 3.4e-05 3.2e-05
    ehess2rhess   1.8e-05 1.5e-05 1.6e-05 3.5e-05    3.8e-05 3.5e-05 3.5e-05 3.3e-05     2.6e-05 3.5e-05 3.5e-05 3.3e-05
    exp(log) = Y  6.7e-04 1.3e-04 8.7e-08 2.7e-05    4.8e-04 1.8e-03 1.3e-07 2.5e-05     4.5e-04 5.1e-04 9.7e-08 2.5e-05
Sphere, worst over every dim and n: proj 1.6e-02, retr 2.1e-02, ehess2rhess 1.6e-02, exp 2.9e-02 (tangent norm 1e-15: 5.3e-03, 1e-17: 7.1e-04);
dist / log on generic pairs 8.1e-03 / 1.8e-02, at angle 1e-4 1.4e-01 / 5.3e-03 (most of it the longdouble acos of the truth), at pi - 1e-4
5.2e-06 / 1.7e-01, at 1e-9 (absolute 3e-8) 8.8e-03 / 2.1e-09.  With the acos form the sphere kernel had before this test (emulated in fp64 on the
CPU) dist at angle 1e-4 and log at pi - 1e-4 are 2 to 18 x over their bounds at every dim from 2 to 65, and log(x, x) is not 0 wherever <x, x>
rounds below 1 (18 % of random unit vectors at dim 2, 45 % at dim 512): SOP_LOG / SOP_DIST now take the angle from the chord (sphere_angle,
csrc/spd_manifold.hip).
"""
import numpy as np
import pytest
import torch

from gabotorch_amd import _lib, manifolds, ops
from tests import _cpu_spd_manifold as cpu

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SMALL_N, LARGE_N = 4, 1028                   # LARGE_N = 257 copies of the four cases: >= 1024, the one-wave shape at d > 12
BAD_SMALL, BAD_LARGE = 2, 777                # where the status-word tests put their negative-definite base point
NF = len(cpu.FAMILIES)
OP = {"exp": _lib.GABO_SPD_EXP, "log": _lib.GABO_SPD_LOG, "dist": _lib.GABO_SPD_DIST, "inner": _lib.GABO_SPD_INNER, "norm": _lib.GABO_SPD_NORM,
      "egrad2rgrad": _lib.GABO_SPD_EGRAD2RGRAD, "ehess2rhess": _lib.GABO_SPD_EHESS2RHESS}


def t(x):
    return torch.tensor(np.ascontiguousarray(x), dtype=torch.float64, device=DEV)


def launch_shape(d, n):
    if d > 12 and n < 1024:
        return "<256,true>"
    return "<64,true>" if d >= 5 else "<64,false>"


def batches(d):
    return [SMALL_N] + ([LARGE_N] if d > 12 else [])


def tile(a, n):
    """the four cases repeated to n rows, interleaved: row i is case i % 4"""
    return np.tile(a, (n // NF,) + (1,) * (a.ndim - 1))


def first_copy(out, what):
    """the first four rows of a tiled batch's result, after checking that every later copy equals them bit for bit (a matrix is its own block)"""
    copies = out.reshape((out.shape[0] // NF, NF) + tuple(out.shape[1:]))
    assert torch.equal(copies, copies[:1].expand_as(copies)), f"{what}: copies of one case differ within a batch"
    return out[:NF].cpu().numpy()


def report(d, n, what, errs, bounds):
    ratios = [e / b for e, b in zip(errs, bounds)]
    print(f"RATIO d={d} n={n} shape={launch_shape(d, n)} op={what} " + " ".join(f"{f}={r:.3e}" for f, r in zip(cpu.FAMILIES, ratios)))
    for f, e, b in zip(cpu.FAMILIES, errs, bounds):
        assert e <= b, f"{what} d={d} n={n} {launch_shape(d, n)} family {f}: error {e:.3e} > bound {b:.3e}"


@pytest.mark.parametrize("d", cpu.ORDERS)
def test_two_operand_operations_against_the_50_digit_truth(golden, d):
    g = golden(cpu.FIXTURE)
    X, Y, U = g[f"X_{d}"], g[f"Y_{d}"], g[f"log_{d}"]
    G, H = cpu.poly_inputs(d, NF)
    poly = {"egrad2rgrad": cpu.egrad2rgrad_ld(X, G), "ehess2rhess": cpu.ehess2rhess_ld(X, G, H, U)}
    for n in batches(d):
        x, y, u, gg, hh = (t(tile(a, n)) for a in (X, Y, U, G, H))
        got = {"exp": ops.spd_manifold_op(OP["exp"], x, u), "log": ops.spd_manifold_op(OP["log"], x, y),
               "dist": ops.spd_manifold_op(OP["dist"], x, y), "inner": ops.spd_manifold_op(OP["inner"], x, u, y),
               "norm": ops.spd_manifold_op(OP["norm"], x, u), "egrad2rgrad": ops.spd_manifold_op(OP["egrad2rgrad"], x, gg),
               "ehess2rhess": ops.spd_manifold_op(OP["ehess2rhess"], x, gg, hh, u)}
        ops.check_deferred()
        for name in ("exp", "log"):
            assert torch.equal(got[name], got[name].transpose(-1, -2)), f"{name} d={d} n={n}: not exactly symmetric"
        for name in cpu.OPS:
            out = first_copy(got[name], f"{name} d={d} n={n}")
            report(d, n, name, [cpu.rel_err(out[f], g[f"{name}_{d}"][f]) for f in range(NF)], [cpu.tol(g, name, f) for f in cpu.FAMILIES])
        for name, want in poly.items():
            out = first_copy(got[name], f"{name} d={d} n={n}").astype(np.longdouble)
            errs = [float(np.max(np.abs(out[f] - want[f])) / np.max(np.abs(want[f]))) for f in range(NF)]
            report(d, n, name, errs, [cpu.POLY_TOL] * NF)


@pytest.mark.parametrize("d", cpu.ORDERS)
def test_identities_and_the_round_trip(golden, d):
    g = golden(cpu.FIXTURE)
    X, Y = g[f"X_{d}"], g[f"Y_{d}"]
    A = 0
    for n in batches(d):
        x, y = t(tile(X, n)), t(tile(Y, n))
        zero = torch.zeros_like(x)
        xmax = float(np.abs(X[A]).max())
        log_xx = first_copy(ops.spd_manifold_op(OP["log"], x, x), "log(X, X)")
        dist_xx = first_copy(ops.spd_manifold_op(OP["dist"], x, x), "dist(X, X)")
        exp_x0 = first_copy(ops.spd_manifold_op(OP["exp"], x, zero), "exp(X, 0)")
        norm_x0 = ops.spd_manifold_op(OP["norm"], x, zero)
        print(f"EXACT d={d} n={n} log(X,X)/max|X|={np.abs(log_xx[A]).max() / xmax:.2e} dist(X,X)/sqrt(d)={dist_xx[A] / np.sqrt(d):.2e} "
              f"|exp(X,0)-X|/max|X|={np.abs(exp_x0[A] - X[A]).max() / xmax:.2e}")
        assert np.abs(log_xx[A]).max() <= 1e-13 * xmax
        assert 0.0 <= dist_xx[A] <= 1e-13 * np.sqrt(d)
        assert np.abs(exp_x0[A] - X[A]).max() <= 1e-13 * xmax
        assert bool((norm_x0 == 0.0).all())                     # every family: the norm of the zero tangent is 0 exactly
        back = first_copy(ops.spd_manifold_op(OP["exp"], x, ops.spd_manifold_op(OP["log"], x, y)), "exp(X, log(X, Y))")
        report(d, n, "exp(log)", [cpu.rel_err(back[f], Y[f]) for f in range(NF)],
               [2.0 * cpu.tol(g, "log", f) + cpu.tol(g, "exp", f) for f in cpu.FAMILIES])
        ops.check_deferred()


@pytest.mark.parametrize("d", [4, 5, 13, 32])
def test_positive_definite_wrappers_add_no_arithmetic(golden, d):
    g = golden(cpu.FIXTURE)
    X, Y, U = g[f"X_{d}"], g[f"Y_{d}"], g[f"log_{d}"]
    man = manifolds.PositiveDefinite(d)
    x, y, u = t(X), t(Y), t(U)
    assert np.array_equal(man.exp(X, U), ops.spd_manifold_op(OP["exp"], x, u).cpu().numpy())
    assert np.array_equal(man.log(X, Y), ops.spd_manifold_op(OP["log"], x, y).cpu().numpy())
    assert np.array_equal(man.dist(X, Y), ops.spd_manifold_op(OP["dist"], x, y).cpu().numpy())
    assert np.array_equal(man.inner(X, U, Y), ops.spd_manifold_op(OP["inner"], x, u, y).cpu().numpy())
    assert np.array_equal(man.norm(X, U), ops.spd_manifold_op(OP["norm"], x, u).cpu().numpy())


@pytest.mark.parametrize("d,n,bad", [(d, SMALL_N, BAD_SMALL) for d in cpu.ORDERS] + [(13, LARGE_N, BAD_LARGE), (32, LARGE_N, BAD_LARGE)])
def test_status_word_names_the_matrix_in_each_launch_shape(golden, raising, d, n, bad):
    """A negative-definite base point at a known index of the batch: the kernel's Cholesky reports it in the status word and goes on"""
    g = golden(cpu.FIXTURE)
    X, U = tile(g[f"X_{d}"], n), tile(g[f"log_{d}"], n)
    good_x, u = t(X), t(U)
    X[bad] = -X[bad]
    with raising(f"input matrix #{bad} is not positive definite"):
        ops.spd_manifold_op(OP["exp"], t(X), u)
    out = ops.spd_manifold_op(OP["exp"], good_x, u)           # the next clean call passes, and nothing is left pending
    ops.check_deferred()
    assert bool(torch.isfinite(out).all())


# ------------------------------------------------------------------------------------------------------------------ sphere
U53 = 2.0 ** -53
SPH_DIMS = (1, 2, 3, 16, 64, 65, 512)
SPH_NS = (1, 255, 257)                       # the 256-thread block edge
ACOS_ABS = 3e-8                              # the project's allowance for acos next to +-1 (test_sphere_golden)
LD = np.longdouble


def _rows_max(a):
    return np.max(np.abs(a), axis=-1)


def _unit(rng, n, dim):
    x = rng.standard_normal((n, dim)).astype(LD)
    return (x / np.sqrt(np.sum(x * x, axis=-1, keepdims=True))).astype(np.float64)


def _tangent(rng, x, norm=None):
    """a random vector projected onto the tangent space at x in longdouble (scaled to `norm` where given), rounded to fp64"""
    xl = x.astype(LD)
    h = rng.standard_normal(x.shape).astype(LD)
    h = h - np.sum(xl * h, axis=-1, keepdims=True) * xl
    if norm is not None:
        length = np.sqrt(np.sum(h * h, axis=-1, keepdims=True))
        h = np.where(length > 0, h / np.where(length > 0, length, 1), 0) * np.asarray(norm, dtype=LD)
    return h.astype(np.float64)


def _at_angle(rng, x, theta):
    """points at angle theta from x: x cos(theta) + v sin(theta), v a unit tangent, in longdouble, rounded to fp64"""
    v = _tangent(rng, x, 1.0).astype(LD)
    return (x.astype(LD) * np.cos(LD(theta)) + v * np.sin(LD(theta))).astype(np.float64)


def _on_sphere(x):
    """The point of the sphere an fp64 vector stands for: normalised in longdouble.  An fp64 'unit' vector has norm 1 + O(2^-53), and acos(<x, y>) turns
    that into an angle error of 2^-53 / sin t - as large as the rounding the bounds below allow the KERNEL, so the truth must not carry it."""
    x = x.astype(LD)
    return x / np.sqrt(np.sum(x * x, axis=-1, keepdims=True))


def _ip(x, y):
    return np.clip(np.sum(_on_sphere(x) * _on_sphere(y), axis=-1), LD(-1), LD(1))


def sph_exp_ld(x, u):
    x, u = x.astype(LD), u.astype(LD)
    nu = np.sqrt(np.sum(u * u, axis=-1, keepdims=True))
    safe = np.where(nu > 0, nu, LD(1))
    return np.where(nu > 0, x * np.cos(nu) + u * (np.sin(safe) / safe), x)


def sph_log_ld(x, y):
    th = np.arccos(_ip(x, y))[..., None]
    x, y = _on_sphere(x), _on_sphere(y)
    safe = np.where(th > 0, th, LD(1))
    return np.where(th > 0, (y - x * np.cos(th)) * (safe / np.sin(safe)), LD(0))


def sph(op, *args):
    return ops.sphere_manifold_op(op, *[t(a) for a in args]).cpu().numpy()


def check_rows(what, got, want, bound):
    """per row: max|got - want| <= bound (bound already holds the row's scale)"""
    err = _rows_max((got.astype(LD) - want).reshape(len(got), -1)).astype(np.float64)
    bound = np.asarray(bound, dtype=np.float64)
    worst = int(np.argmax(err - bound))
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.nanmax(np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0)))
    print(f"SPHERE {what} rows={len(got)} worst error/bound={ratio:.3e}")
    assert np.all(err <= bound), f"{what}: row {worst}: error {err[worst]:.3e} > bound {bound[worst]:.3e}"


@pytest.mark.parametrize("dim", SPH_DIMS)
def test_sphere_operations_against_longdouble(dim):
    """proj, retr, ehess2rhess, exp within 64 dim 2^-53 of max|truth| (per point); dist and log within 64 dim 2^-53 (1 + 1 / max(sin t, 2^-26)) of
    max|truth|, t the angle: the factor by which acos of an inner product rounded at 2^-53 is conditioned; pairs at angle 1e-9 within the absolute 3e-8.
    The truth is the header's formula (acos of the clipped inner product) in longdouble, for dist and log on the inputs normalised in longdouble
    (_on_sphere); the kernel takes the angle from the chord, so the two share no arithmetic.  Where the kernel branches the statements are exact:
    exp(x, 0) = x, log(x, x) = 0, dist(x, x) = 0."""
    rng = np.random.default_rng([cpu.SEED, dim, 2])
    eps = 64.0 * dim * U53
    for n in SPH_NS:
        tag = f"dim={dim} n={n}"
        x = _unit(rng, n, dim)
        xl = x.astype(LD)
        # proj, retr, ehess2rhess.  The bounds are relative to the RESULT, so the inputs keep the result from cancelling: ambient vectors are a tangent
        # part of norm in [0.5, 2] plus a normal part c x with |c| <= 1 (a vector next to the normal direction would project to rounding noise), and the
        # tangent of ehess2rhess points away from the projected Hessian term it is added to
        def ambient():
            return _tangent(rng, x, rng.uniform(0.5, 2.0, (n, 1))) + rng.uniform(-1.0, 1.0, (n, 1)) * x
        h, eg, eh = ambient(), ambient(), ambient()
        hl, egl, ehl = h.astype(LD), eg.astype(LD), eh.astype(LD)
        want = hl - np.sum(xl * hl, axis=-1, keepdims=True) * xl
        got = sph(_lib.GABO_SPH_PROJ, x, h)
        if dim == 1:
            assert np.all(got == 0.0), "dim = 1: the tangent space is {0}"
        else:
            check_rows(f"proj {tag}", got, want, eps * _rows_max(want))
        tg = _tangent(rng, x, rng.uniform(0.5, 2.0, (n, 1)))
        step = 0.1 * tg
        want = xl + step.astype(LD)
        want = want / np.sqrt(np.sum(want * want, axis=-1, keepdims=True))
        check_rows(f"retr {tag}", sph(_lib.GABO_SPH_RETR, x, step), want, eps * _rows_max(want))
        first = eh - np.sum(x * eh, axis=-1, keepdims=True) * x
        second = -np.sum(x * eg, axis=-1, keepdims=True) * tg
        tg = tg * np.where(np.sum(first * second, axis=-1, keepdims=True) < 0, -1.0, 1.0)
        want = ehl - np.sum(xl * ehl, axis=-1, keepdims=True) * xl - np.sum(xl * egl, axis=-1, keepdims=True) * tg.astype(LD)
        got = sph(_lib.GABO_SPH_EHESS2RHESS, x, eg, eh, tg)
        if dim == 1:
            assert np.all(got == 0.0), "dim = 1: the tangent space is {0}"
        else:
            check_rows(f"ehess2rhess {tag}", got, want, eps * _rows_max(want))
        # exp: ordinary tangents, and the norms around the kernel's 1e-16 switch
        for label, norm in (("generic", rng.uniform(0.1, 3.0, (n, 1))), ("1e-15", 1e-15), ("1e-17", 1e-17), ("zero", 0.0)):
            u = _tangent(rng, x, norm) if label != "zero" else np.zeros_like(x)
            got = sph(_lib.GABO_SPH_EXP, x, u)
            want = sph_exp_ld(x, u)
            check_rows(f"exp {label} {tag}", got, want, eps * _rows_max(want))
            if label == "zero" or dim == 1:
                assert np.array_equal(got, x), "exp(x, 0) is x bit for bit"
        # dist, log
        assert np.array_equal(sph(_lib.GABO_SPH_LOG, x, x), np.zeros_like(x)), "log(x, x) is 0 bit for bit"
        assert np.array_equal(sph(_lib.GABO_SPH_DIST, x, x), np.zeros(n)), "dist(x, x) is 0 bit for bit"
        if dim == 1:
            y = x * rng.choice([-1.0, 1.0], size=(n, 1))
            d1 = sph(_lib.GABO_SPH_DIST, x, y)
            assert np.array_equal(d1, np.where(y[:, 0] == x[:, 0], 0.0, np.pi)), "dim = 1: dist is 0 or pi"
            continue
        pairs = [("generic", _unit(rng, n, dim), False), ("1e-9", _at_angle(rng, x, 1e-9), True), ("1e-4", _at_angle(rng, x, 1e-4), False),
                 ("pi-1e-4", _at_angle(rng, x, np.pi - 1e-4), False)]
        for label, y, absolute in pairs:
            th = np.arccos(_ip(x, y))
            cond = (1.0 + 1.0 / np.maximum(np.sin(th).astype(np.float64), 2.0 ** -26))
            want_log = sph_log_ld(x, y)
            if absolute:
                b_dist, b_log = np.full(n, ACOS_ABS), np.full(n, ACOS_ABS)
            else:
                b_dist, b_log = eps * cond * th.astype(np.float64), eps * cond * _rows_max(want_log).astype(np.float64)
            check_rows(f"dist {label} {tag}", sph(_lib.GABO_SPH_DIST, x, y), th, b_dist)
            check_rows(f"log {label} {tag}", sph(_lib.GABO_SPH_LOG, x, y), want_log, b_log)
