"""The constrained sphere sweep drivers (gabo_sphere_sweep_solve_constrained / _run_constrained, gabo_sphere_sample; csrc/spd_sweep.hip) refuse a
malformed constraint set on the host, before any HIP call - so these checks need no GPU - and size their workspace from the unconstrained layout."""
import ctypes

import numpy as np
import pytest

from gabotorch_amd import _lib

LO, UP, BALL = _lib.GABO_SPHERE_CONSTRAINT_COORD_LOWER, _lib.GABO_SPHERE_CONSTRAINT_COORD_UPPER, _lib.GABO_SPHERE_CONSTRAINT_GEODESIC_BALL
DIM, R, RAW = 3, 4, 16


@pytest.fixture(scope="module", autouse=True)
def _built_library():
    import os
    if not os.path.exists(_lib.LIB_PATH):
        from gabotorch_amd import _build
        _build.build()


def _cons(n, neq=0, kinds=(), idx=(), n_centres=0, centres=None):
    c = _lib.SphereSweepConstraints()
    c.n_constraints, c.n_equalities = n, neq
    for k, v in enumerate(kinds):
        c.kind[k] = v
    for k, v in enumerate(idx):
        c.index[k] = v
    for k in range(8):
        c.bound[k] = 0.1
    c.centres, c.n_centres, c.strict, c.delta_cons = centres, n_centres, 0, 1e-6
    return c


def _cfg():
    cfg = _lib.SphereSweepConfig()
    cfg.acq = _lib.SphereAcqParams(8, 8, 8, 8, 8, 12, DIM, 1.0, 0, 0.0, 1.0, 1.0, 0.0, _lib.GABO_ACQ_POSTERIOR_MEAN, 1, -1.0)
    cfg.delta_bar, cfg.delta0, cfg.theta, cfg.kappa, cfg.mininner, cfg.maxinner, cfg.exact_hessian = 1.0, 0.1, 1.0, 0.1, 1, DIM, 1
    cfg.rho_prime, cfg.rho_regularization, cfg.mingradnorm, cfg.maxiter = 0.1, 1e3, 1e-6, 10
    return cfg


class _Calls:
    """both drivers with every other argument well-formed (host buffers of the right sizes, a made-up workspace address that is never touched:
    the verdict on the constraint set comes first)"""

    def __init__(self):
        self.lib = _lib.load()
        self.cfg = _cfg()
        self.picked = np.arange(R, dtype=np.int64)
        self.raw = np.zeros((RAW, DIM))
        self.best, self.iters, self.fallback = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int(0)
        self.value = ctypes.c_double(0.0)
        self.ptrs = [ctypes.c_void_p() for _ in range(5)]

    def solve(self, cons):
        p = self.ptrs
        return self.lib.gabo_sphere_sweep_solve_constrained(ctypes.byref(self.cfg), self.picked.ctypes.data, R, RAW, ctypes.byref(self.best),
                                                            ctypes.byref(self.value), ctypes.byref(self.iters), ctypes.byref(p[0]), ctypes.byref(p[1]),
                                                            ctypes.byref(p[2]), None if cons is None else ctypes.byref(cons), ctypes.byref(p[4]),
                                                            ctypes.c_void_p(256), 1 << 30, None)

    def run(self, cons, host_points=True):
        p = self.ptrs
        return self.lib.gabo_sphere_sweep_run_constrained(ctypes.byref(self.cfg), RAW, R, self.raw.ctypes.data if host_points else None, 7, 1.0, 1e-4, 11,
                                                          ctypes.byref(self.best), ctypes.byref(self.value), ctypes.byref(self.iters), ctypes.byref(p[0]),
                                                          ctypes.byref(p[1]), ctypes.byref(p[2]), ctypes.byref(p[3]), ctypes.byref(self.fallback),
                                                          None if cons is None else ctypes.byref(cons), ctypes.byref(p[4]), ctypes.c_void_p(256), 1 << 30,
                                                          None)


@pytest.mark.parametrize("what,cons", [
    ("nine constraints", _cons(9, kinds=[LO] * 8, idx=[0] * 8)),
    ("an unknown kind", _cons(1, kinds=[3], idx=[0])),
    ("a coordinate index >= dim", _cons(1, kinds=[LO], idx=[DIM])),
    ("a negative coordinate index", _cons(1, kinds=[UP], idx=[-1])),
    ("a ball without centres", _cons(1, kinds=[BALL], idx=[0], n_centres=1, centres=None)),
    ("a ball outside its centres", _cons(1, kinds=[BALL], idx=[2], n_centres=2, centres=8)),
    ("more equalities than constraints", _cons(2, neq=3, kinds=[LO, UP], idx=[0, 1])),
    ("a negative count", _cons(-1)),
])
def test_malformed_constraint_sets_are_refused_before_any_hip_call(what, cons):
    calls = _Calls()
    assert calls.solve(cons) == _lib.GABO_ERR_ARG, what
    assert calls.run(cons) == _lib.GABO_ERR_ARG, what
    assert calls.run(cons, host_points=False) == _lib.GABO_ERR_ARG, what


def test_missing_struct_bad_dimension_and_device_sampling_on_an_equality():
    calls = _Calls()
    assert calls.solve(None) == _lib.GABO_ERR_ARG and calls.run(None) == _lib.GABO_ERR_ARG
    # NULL raw points = draw on the device: not ON an equality constraint (the caller's host sampler draws there)
    assert calls.run(_cons(2, neq=1, kinds=[LO, UP], idx=[1, 0]), host_points=False) == _lib.GABO_ERR_ARG
    calls.cfg.acq.dim = 1
    assert calls.solve(_cons(1, kinds=[LO], idx=[0])) == _lib.GABO_ERR_DIM
    assert calls.run(_cons(1, kinds=[LO], idx=[0])) == _lib.GABO_ERR_DIM


def test_the_sampler_alone_validates_on_the_host():
    lib = _lib.load()
    ints = lambda *v: (ctypes.c_int * 9)(*v)              # noqa: E731
    dbl = (ctypes.c_double * 9)(*([0.1] * 9))

    def sample(n, neq, kinds, idx, count=0, dim=DIM, n_centres=0, centres=None):
        # (count = 0: a well-formed call returns GABO_OK without a launch)
        return lib.gabo_sphere_sample(None, count, dim, 7, n, neq, kinds, idx, dbl, centres, n_centres, None, None)
    assert sample(0, 0, None, None) == _lib.GABO_OK and sample(8, 0, ints(*[LO] * 8), ints(*[2] * 8)) == _lib.GABO_OK
    assert sample(2, 0, ints(BALL, UP), ints(1, 0), n_centres=2, centres=ctypes.c_void_p(8)) == _lib.GABO_OK
    assert sample(9, 0, ints(*[LO] * 9), ints(*[0] * 9)) == _lib.GABO_ERR_ARG
    assert sample(1, 1, ints(LO), ints(1)) == _lib.GABO_ERR_ARG                        # inequalities only
    assert sample(1, 0, ints(LO), ints(DIM)) == _lib.GABO_ERR_ARG
    assert sample(1, 0, ints(BALL), ints(0)) == _lib.GABO_ERR_ARG
    assert sample(1, 0, ints(5), ints(0)) == _lib.GABO_ERR_ARG
    assert sample(0, 0, None, None, dim=1) == _lib.GABO_ERR_DIM and sample(0, 0, None, None, dim=513) == _lib.GABO_ERR_DIM
    assert sample(0, 0, None, None, count=4) == _lib.GABO_ERR_ARG                      # no output, no flag
    assert _lib.GABO_SPHERE_SAMPLE_MAX_TRIES == 256


@pytest.mark.parametrize("dim,raw,r", [(3, 64, 16), (10, 2048, 512), (65, 50, 7)])
def test_workspace_is_the_unconstrained_one_plus_what_the_constraints_need(dim, raw, r):
    lib = _lib.load()
    plain = lib.gabo_sphere_sweep_workspace_bytes(dim, raw, r)
    sizes = [lib.gabo_sphere_sweep_workspace_bytes_constrained(dim, raw, r, c) for c in range(9)]
    assert plain > 0 and sizes[0] >= plain
    assert all(b > a for a, b in zip(sizes, sizes[1:])), sizes
    # the final constraint values (r x c doubles) and the trust-region workspace of c constraints are in it
    for c in (1, 8):
        grown = lib.gabo_sphere_tr_workspace_bytes(r, dim, c) - lib.gabo_sphere_tr_workspace_bytes(r, dim, 0)
        assert sizes[c] - sizes[0] >= r * c * 8 + grown - 512, (c, sizes[c] - sizes[0], grown)
    assert lib.gabo_sphere_sweep_workspace_bytes_constrained(dim, raw, r, 9) == 0 and lib.gabo_sphere_sweep_workspace_bytes_constrained(dim, raw, r, -1) == 0
    assert lib.gabo_sphere_sweep_workspace_bytes_constrained(1, raw, r, 0) == 0
