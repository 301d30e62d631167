"""joint_optimize_manifold through the native sweep drivers of csrc/spd_sweep.hip: the decision whether a sweep can take them (_native_sweep_plan), the
device state they keep between sweeps, and one driver per manifold (_native_sweep, _native_sweep_sphere).  The host steps both paths share - the host sampler, the
selection heuristic and its retry loop - are manifold_optimize's; that module imports this one, so this one reaches it from inside its functions."""
import ctypes
import time
import warnings

import numpy as np
import torch

from .. import _lib, _status, ops
from ..fused_acquisition import FusedAcquisition
from .batched_trust_regions import BatchedTrustRegions, default_limits


def _native_sweep_plan(acq_function, manifold, solver, q, num_restarts, raw_samples, bounds, sample_type, options, inequality_constraints,
                       equality_constraints, pre_processing_manifold, post_processing_manifold, approx_hessian, solver_init_conds):
    """The sweep through a native driver (csrc/spd_sweep.hip: gabo_spd_sweep_score_rows / _select_rows / _solve_rows, or the sphere's
    gabo_sphere_sweep_score / _solve / _run and their _constrained forms) when EVERY launch of it would be one the driver issues - built-in surrogate
    evaluated in one launch, constraints the library's own built with functools.partial (or none), the whole solve one launch.  Returns what the
    driver needs, with the driver itself under "driver", or None: then the Python path of joint_optimize_manifold runs, launch for launch the same
    work.  options={"native_sweep": False} keeps the Python path."""
    from ..manifolds import PositiveDefinite, Sphere
    from ..Riemannian_utils import spd_utils_torch
    from ..Riemannian_utils.spd_constraints_utils_torch import builtin_constraint
    from . import manifold_optimize as mo
    device = options.get("device")
    if not (options.get("native_sweep", True) and device is not None):
        return None
    # (every plan option at its default, all restarts in one batch: both manifolds' drivers)
    if (any(options.get(k, True) is False for k in ("fused_acquisition", "device_tcg", "device_outer", "device_iteration", "device_solve"))
            or options.get("batch_limit", num_restarts) < num_restarts or num_restarts < 1 or raw_samples < 1):
        return None
    if not (q == 1 and bounds is None and not solver_init_conds and sample_type == torch.float64 and isinstance(solver, BatchedTrustRegions)
            and not solver.use_rand and solver.maxtime >= 1000 and solver.trace is None):
        return None
    dev = torch.device(device)
    if dev.type != "cuda":
        return None
    if isinstance(manifold, Sphere):
        # exact or FD Hessian, no constraints or the library's own sphere constraints (coordinate bounds, great circle, geodesic ball built with functools.partial:
        # what the solve launch evaluates itself); any other constraint is a host callable and keeps the Python path, which also shards the sweep: this driver does not
        if mo._dist() is not None or pre_processing_manifold is not None or post_processing_manifold is not None:
            return None
        as_list = lambda c: list(c) if isinstance(c, (list, tuple)) else ([c] if c else [])       # noqa: E731  (BatchedTrustRegions._solve's reading)
        eqs, ineqs = as_list(equality_constraints), as_list(inequality_constraints)
        group = None
        if eqs or ineqs:
            from ..Riemannian_utils.sphere_constraints_utils_torch import builtin_sphere_group
            group = builtin_sphere_group(eqs + ineqs, int(manifold._n), dev)
            if group is None:
                return None
        fused = FusedAcquisition.build(acq_function, None, dev)
        if fused is None or not (fused.family == "sphere" and fused.one_launch):
            return None
        return {"driver": _native_sweep_sphere, "fused": fused, "device": dev, "manifold": manifold, "exact_hessian": not approx_hessian, "sphere_group": group,
                "n_equalities": len(eqs)}
    if not (isinstance(manifold, PositiveDefinite) and manifold._n >= 2 and approx_hessian and not equality_constraints):
        return None       # (how far up the drivers go is the library's to say: gabo_spd_tr_solve_supported below)
    device_rand = bool(options.get("device_rand")) and hasattr(manifold, "rand_batch_device")
    if device_rand and not (type(manifold).rand_batch_device is PositiveDefinite.rand_batch_device and "rand_batch_device" not in vars(manifold)
                            and hasattr(manifold, "min_eig") and hasattr(manifold, "max_eig")):
        return None       # (a sampler of the caller's own on the device: the Python path calls it)
    if pre_processing_manifold is not spd_utils_torch.vector_to_symmetric_matrix_mandel_torch:
        return None
    cons = list(inequality_constraints or [])
    builtins = [builtin_constraint(c) for c in cons]
    if len(cons) > 8 or any(b is None or len(b) != 2 or b[0] not in (_lib.GABO_CONSTRAINT_MAX_EIGENVALUE, _lib.GABO_CONSTRAINT_MIN_EIGENVALUE)
                            for b in builtins):
        return None
    fused = FusedAcquisition.build(acq_function, post_processing_manifold, dev)
    if fused is None or not (fused.family == "spd" and fused.flavour in ("ai", "le") and fused.single_launch and fused.matrix_input):
        return None       # (affine-invariant and log-Euclidean surrogates: the metrics gabo_spd_tr_solve iterates)
    if not _lib.load().gabo_spd_tr_solve_supported(ctypes.byref(fused.acq_params()), int(num_restarts), int(manifold._n), len(builtins), 0):
        return None       # (e.g. the log-Euclidean surrogate at d = 7, 8 beyond its LDS-resident form: the propose / update launches run)
    return {"driver": _native_sweep, "fused": fused, "device": dev, "manifold": manifold, "builtins": builtins, "device_rand": device_rand}


def _trust_region_fields(cfg, solver, limits):
    """fills the trust-region fields SweepConfig and SphereSweepConfig have in common from the solver and default_limits(manifold); returns Delta_cons"""
    mininner, maxinner, delta_bar, delta0, delta_cons = limits
    cfg.delta_bar, cfg.delta0 = float(delta_bar), float(delta0)
    cfg.theta, cfg.kappa, cfg.mininner, cfg.maxinner = float(solver.theta), float(solver.kappa), int(mininner), int(maxinner)
    cfg.rho_prime, cfg.rho_regularization = float(solver.rho_prime), float(solver.rho_regularization)
    cfg.mingradnorm, cfg.maxiter = float(solver.mingradnorm), int(solver.maxiter)
    return delta_cons


def _sweep_log(iterations, per_restart_iterations, final_cost, time0, device_selection):
    """the keys of solver.log both drivers write: those of the Python path's single-launch solve that a driver knows"""
    return {"iterations": iterations, "per_restart_iterations": per_restart_iterations, "final_cost": final_cost, "final_gradnorm": None, "cost_evals": 0,
            "grad_evals": 0, "time": time.time() - time0, "one_launch_solve": True, "native_sweep": True, "device_selection": device_selection}


_sweep_workspaces = {}          # (family, device index, stream) -> "spd": _RowsState, "sphere": the uint8 workspace of the sphere driver


def _all_gather_rows(dist, full, block):
    """full (world * rows, width) <- every rank's block (rows, width): ONE collective; backends without all_gather_into_tensor take the list form"""
    try:
        dist.all_gather_into_tensor(full, block)
    except (RuntimeError, NotImplementedError, AttributeError):
        parts = [torch.empty_like(block) for _ in range(dist.get_world_size())]
        dist.all_gather(parts, block)
        full.copy_(torch.cat(parts))


class _RowsState:
    """What one (device, stream) keeps between SPD sweeps: the device workspace of the native driver (its two tables as tensors) and a block of PAGE-LOCKED
    host memory the kernels write straight into (scores, result rows) and read from (picked rows) - no copy launch, no pageable staging; the host
    looks at it through numpy once the stream has drained.  Keyed by what fixes the tables (d, rows, restarts, constraints); the number of training
    points only sizes the solver's scratch behind them, so a BO loop whose training set grows by one point per iteration keeps its state and lets the
    workspace grow when it has to."""

    def __init__(self, lib, dev, n_train, d, max_rows, restarts, n_constraints):
        self.key = (d, max_rows, restarts, n_constraints)
        self.dev = dev
        dv = d * (d + 1) // 2
        self.ws, self.wsb = None, 0
        self.fit(lib, n_train)
        self.pinned = torch.zeros(3 + max_rows + restarts + restarts * (2 + dv), dtype=torch.float64).pin_memory()
        host = self.pinned.numpy()
        self.err = host[:3].view(np.int32)                  # mirrors of (score status, solve status, selection flag): int32[2] each
        self.values = host[3:3 + max_rows]
        self.picked = host[3 + max_rows:3 + max_rows + restarts].view(np.int64)
        self.results = host[3 + max_rows + restarts:].reshape(restarts, 2 + dv)
        base = self.pinned.data_ptr()
        self.err_ptr = (base, base + 8, base + 16)
        self.values_ptr, self.picked_ptr, self.results_ptr = base + 24, base + 8 * (3 + max_rows), base + 8 * (3 + max_rows + restarts)
        self.status = torch.zeros(3, 2, dtype=torch.int32, device=dev)      # the device words behind the mirrors (only a failing launch writes them)
        self.status_ptr = tuple(self.status.data_ptr() + 8 * k for k in range(3))
        self.picked_dev = torch.zeros(restarts, dtype=torch.int64, device=dev)      # device selection: this rank's rows
        self.samples_dev = None                                                     # ... and every restart's sample index (sized on first use)

    def fit(self, lib, n_train):
        """the workspace for a surrogate on n_train points: grown when the one held is too small (the tables sit at its start, at offsets that do not
        depend on n_train)"""
        d, max_rows, restarts, n_constraints = self.key
        dv = d * (d + 1) // 2
        need = int(lib.gabo_spd_sweep_rows_workspace_bytes(n_train, d, max_rows, restarts, n_constraints))
        if self.ws is not None and need <= self.wsb:
            return
        self.wsb = need + need // 4           # (room for a few more training points before the next growth)
        self.ws = torch.empty(self.wsb // 8 + 1, dtype=torch.float64, device=self.dev)
        raw_p, res_p = ctypes.c_void_p(), ctypes.c_void_p()
        if lib.gabo_spd_sweep_rows_tables(self.ws.data_ptr(), n_train, d, max_rows, restarts, n_constraints, ctypes.byref(raw_p), ctypes.byref(res_p)) != 0:
            raise RuntimeError("gabo_spd_sweep_rows_tables refused the workspace")
        o_raw, o_res = (raw_p.value - self.ws.data_ptr()) // 8, (res_p.value - self.ws.data_ptr()) // 8
        self.raw = self.ws[o_raw:o_raw + max_rows * (1 + dv)].view(max_rows, 1 + dv)
        self.res = self.ws[o_res:o_res + restarts * (2 + dv)].view(restarts, 2 + dv)

    def raise_if_failed(self, which, what):
        """after the stream has drained: did a launch of call `which` (0 score, 1 solve) report a non-SPD matrix?  Host memory only."""
        e = self.err[2 * which:2 * which + 2]
        if e[0] != 0:
            st = [int(e[0]), int(e[1])]
            e[:] = 0
            self.status[which].zero_()
            raise RuntimeError(_status._not_spd_message(what)(st))


def _rows_state(lib, dev, stream, n_train, d, max_rows, restarts, n_constraints):
    key = ("spd", dev.index, stream)
    st = _sweep_workspaces.get(key)
    if st is None or st.key != (d, max_rows, restarts, n_constraints):
        st = _sweep_workspaces[key] = _RowsState(lib, dev, n_train, d, max_rows, restarts, n_constraints)
    else:
        st.fit(lib, n_train)
    return st


class _SpdSweep:
    """The steps of one SPD sweep (_native_sweep).  Raw sample i of an attempt's `total` belongs to rank i // per and sits in row 1 + i % per of that
    rank's block of the raw-row table; row 0 of a block is its header (the rank's proposal for the selection seed; rank 0's is used).  Restart k
    belongs to rank k % world (trust-region iteration counts vary: interleaved).  The ranks meet in exactly two all_gathers, of the raw-row table
    and of the result rows, none inside the library."""

    def __init__(self, mo, plan, acq_function, solver, num_restarts, raw_samples, options):
        self.mo, self.plan, self.options, self.raw_samples, self.lib = mo, plan, options, raw_samples, _lib.load()
        self.dev, man = plan["device"], plan["manifold"]
        self.d, self.R, self.dist = man._n, int(num_restarts), mo._dist()
        self.rank, self.world = (self.dist.get_rank(), self.dist.get_world_size()) if self.dist is not None else (0, 1)
        self.r_loc, self.r_per = len(range(self.rank, self.R, self.world)), (self.R + self.world - 1) // self.world
        self.n_train = int(plan["fused"].train.shape[0])
        cfg = self.cfg = _lib.SweepConfig()
        cfg.acq, cfg.d = plan["fused"].acq_params(), self.d
        cfg.min_eig, cfg.max_eig = (float(man.min_eig), float(man.max_eig)) if plan["device_rand"] else (0.0, 0.0)
        cfg.n_constraints, cfg.strict = len(plan["builtins"]), 1 if solver.strict_constraints else 0
        for k, b in enumerate(plan["builtins"]):
            cfg.constraint_kind[k], cfg.constraint_bound[k] = int(b[0]), float(b[1])
        cfg.delta_cons = _trust_region_fields(cfg, solver, default_limits(man))
        self.cfg_ref = ctypes.byref(cfg)
        self.nonneg, self.eta, self.alpha = mo._selection(acq_function, options)
        self.checking = _status.error_checking() is not False
        # the selection on the device (gabo_spd_sweep_select_rows) when it is botorch's non-negative heuristic on a table the kernel takes
        self.on_device = bool(options.get("device_selection", True)) and self.nonneg and bool(self.lib.gabo_spd_sweep_select_supported(raw_samples, self.R))

    def score(self, total):
        """One attempt, nothing waits: this rank draws its share of the `total` raw samples and scores them into its block of the table, takes the
        selection seed and - several ranks - all_gathers the table, the seed in its block's header row.  Returns the seed this rank proposes."""
        mo, plan, rank, world, d = self.mo, self.plan, self.rank, self.world, self.d
        per = self.per = (total + world - 1) // world
        lo = min(rank * per, total)
        cnt = min(lo + per, total) - lo
        st = self.st = _rows_state(self.lib, self.dev, self.stream, self.n_train, d, world * (per + 1), max(self.r_per, 1), self.cfg.n_constraints)
        sample_seed, raw = 0, None
        with mo._rank_stream(rank, world if not plan["device_rand"] else 1):
            if plan["device_rand"]:
                sample_seed = int(np.random.randint(0, 2 ** 63 - 1, dtype=np.int64))       # (the draw of manifolds.PositiveDefinite.rand_batch_device)
            else:
                raw = mo._host_samples(plan["manifold"], cnt, self.options, (d, d))
        mo._mark(self.options, "-> score")
        self.pending = ops.prefetch_deferred()           # (the GP's set-up launches: their status words travel while the scoring launches run)
        if cnt:
            to_host = world == 1 and not self.on_device          # one rank, selection on the host: the values go straight to page-locked memory
            _lib.check(self.lib.gabo_spd_sweep_score_rows(
                self.cfg_ref, lo, rank * (per + 1) + 1, cnt, world * (per + 1), max(self.r_per, 1), sample_seed & 0xFFFFFFFFFFFFFFFF, None if raw is None else raw.ctypes.data,
                st.values_ptr if to_host else None, st.ws.data_ptr(), st.wsb, st.status_ptr[0], st.err_ptr[0], 1 if to_host else 0, self.stream), "gabo_spd_sweep_score_rows")
        mo._mark(self.options, "<- score")
        seed = mo._selection_seed()
        if world > 1:
            block = st.raw[rank * (per + 1):(rank + 1) * (per + 1)]
            block[0, 0] = float(seed)           # < 2^52: exact in a double
            _all_gather_rows(self.dist, st.raw, block.clone())          # every rank's block -> the whole table, in place on every rank
        return seed

    def select_on_device(self, total, seed):
        """the selection kernel behind the scoring on the stream (with several ranks it reads rank 0's seed from the table); no wait"""
        st, world, R = self.st, self.world, self.R
        if st.samples_dev is None or st.samples_dev.numel() < R:
            st.samples_dev = torch.zeros(R, dtype=torch.int64, device=self.dev)
        st.err[4] = -1
        _lib.check(self.lib.gabo_spd_sweep_select_rows(st.raw.data_ptr(), self.d, total, self.per, R, self.eta, self.alpha, seed, 1 if world > 1 else 0,
                                                       self.rank, world, st.picked_dev.data_ptr(), st.samples_dev.data_ptr(), st.status_ptr[2],
                                                       st.err_ptr[2], self.stream), "gabo_spd_sweep_select_rows")

    def scored_attempt(self, total):
        """one attempt of the host heuristic: (values of the `total` raw samples, selection seed) on the host once the scoring has drained"""
        seed, st = self.score(total), self.st
        if self.world == 1:
            y = st.values[:total]
        else:
            col = st.raw[:, 0].cpu().numpy().reshape(self.world, self.per + 1)         # (this copy waits for the stream)
            seed, y = int(col[0, 0]), np.ascontiguousarray(col[:, 1:].reshape(-1)[:total])
        ops.check_prefetched(self.pending)
        if self.checking:
            st.raise_if_failed(0, "gabo_spd_sweep_score_rows")
        self.mo._mark(self.options, "<- checks")
        return y, seed

    def select_on_host(self):
        """the host heuristic with its retries; this rank's picks (sample indices) -> rows of the last attempt's table"""
        picked, _ = self.mo._retry_selection(self.scored_attempt, self.raw_samples, self.R, self.nonneg, self.eta, self.alpha)
        mine, per = picked[self.rank::self.world], self.per
        self.st.picked[:self.r_loc] = (mine // per) * (per + 1) + 1 + mine % per

    def solve(self):
        st, world, r_loc = self.st, self.world, self.r_loc
        if world > 1 and r_loc < self.r_per:
            st.res[r_loc:, 0] = float("inf")             # (a rank with one restart fewer: its padding row loses every argmax)
        if r_loc:
            _lib.check(self.lib.gabo_spd_sweep_solve_rows(
                self.cfg_ref, st.picked_dev.data_ptr() if self.on_device else st.picked_ptr, r_loc, world * (self.per + 1), st.results_ptr if world == 1 else None,
                st.status_ptr[2] if self.on_device else None, st.ws.data_ptr(), st.wsb, st.status_ptr[1], st.err_ptr[1], 1 if world == 1 else 0, self.stream),
                "gabo_spd_sweep_solve_rows")
        self.mo._mark(self.options, "<- solve")

    def result_rows(self):
        """(cost, iterations, candidate) of every restart, in restart order, as a host array"""
        st, world, r_per, width = self.st, self.world, self.r_per, 2 + self.d * (self.d + 1) // 2
        if world == 1:
            return st.results[:self.R]           # (page-locked memory the solve writes: valid once the stream has drained)
        gathered = torch.empty(world * r_per, width, dtype=torch.float64, device=self.dev)
        _all_gather_rows(self.dist, gathered, st.res[:r_per].clone())
        # rank r's row j is restart j * world + r           (the copy to the host waits for the stream)
        return gathered.cpu().numpy().reshape(world, r_per, width).transpose(1, 0, 2).reshape(world * r_per, width)[:self.R]

    def result(self, rows, solver, time0):
        """solver.log and the winner's row"""
        st, dv, cost = self.st, self.d * (self.d + 1) // 2, rows[:, 0]
        best = int(np.argmin(cost))          # torch.argmax(-cost): the first of equal values; a NaN wins (numpy's argmin returns the first NaN too)
        solver.log = _sweep_log(int(rows[:, 1].max()), torch.from_numpy(rows[:, 1].astype(np.int64)), torch.from_numpy(cost.copy()), time0, self.on_device)
        solver.log["world_size"] = self.world
        if self.on_device and self.options.get("log_picked"):
            solver.log["picked_samples"] = st.samples_dev[:self.R].cpu().numpy()
        if self.world == 1:
            return st.res[best, 2:].clone().reshape(1, dv)          # (the winner's row of the device table: no host -> device copy)
        return torch.from_numpy(rows[best, 2:].copy()).reshape(1, dv).to(self.dev)


def _native_sweep(plan, acq_function, solver, num_restarts, raw_samples, options):
    """joint_optimize_manifold on S^d_++ through gabo_spd_sweep_score_rows -> selection -> gabo_spd_sweep_solve_rows -> argmin: five launches per sweep
    on one GPU and, with the selection on the device (gabo_spd_sweep_select_rows, the default), one host wait.  The draws from numpy's and torch's
    generators and every statement executed on the device are those of the Python path.  With options["device_selection"] = False the selection is
    the Python path's too (select_rows), and a seeded sweep returns its candidate bit for bit; the selection kernel picks from the library's own
    random stream, and the Python path returns the same candidate only when handed the same picks (options["log_picked"] records them;
    tests/test_gpu_native_sweep.py covers both)."""
    from . import manifold_optimize as mo
    sweep = _SpdSweep(mo, plan, acq_function, solver, num_restarts, raw_samples, options)
    time0 = time.time()
    with torch.cuda.device(sweep.dev):
        sweep.stream = ops._stream_ptr(sweep.dev)
        if sweep.on_device:
            sweep.select_on_device(raw_samples, sweep.score(raw_samples))
        else:
            sweep.select_on_host()
        mo._mark(options, "<- selection")
        sweep.solve()
        rows = sweep.result_rows()
        if sweep.on_device:
            ops.check_prefetched(sweep.pending)
            if sweep.checking:
                sweep.st.raise_if_failed(0, "gabo_spd_sweep_score_rows")
            if sweep.st.err[4] != 0:
                # the heuristic needs its random fall-backs (no positive value among the raw samples, or fewer than restarts), a value is NaN - or the
                # flag never arrived; the launches behind the selection did no work (gabo_spd_sweep_solve_rows' skip_flag).  The host heuristic decides
                return _native_sweep(plan, acq_function, solver, num_restarts, raw_samples, dict(options, device_selection=False))
        if sweep.checking:
            sweep.st.raise_if_failed(1, "gabo_spd_sweep_solve_rows")
    out = sweep.result(rows, solver, time0)
    mo._mark(options, "<- result")
    return out


class _SphereSweep:
    """The steps of one sphere sweep (_native_sweep_sphere), without constraints or with the library's own sphere constraints (plan["sphere_group"]: the
    _constrained entry points, the constraints evaluated inside the solve launch)."""

    def __init__(self, mo, plan, acq_function, solver, num_restarts, raw_samples, options):
        self.mo, self.solver, self.options, self.raw_samples, self.lib = mo, solver, options, raw_samples, _lib.load()
        self.dev, self.man, self.dim, self.R = plan["device"], plan["manifold"], int(plan["manifold"]._n), int(num_restarts)
        cfg = self.cfg = _lib.SphereSweepConfig()
        cfg.acq = plan["fused"].sphere_acq_params()
        delta_cons = _trust_region_fields(cfg, solver, default_limits(self.man))
        cfg.exact_hessian = 1 if plan["exact_hessian"] else 0
        group, neq = plan["sphere_group"], int(plan["n_equalities"])
        self.cons, self.C = None, 0
        if group is not None:
            kinds, indices, bounds, centres = group
            cons, self.C = _lib.SphereSweepConstraints(), len(kinds)
            cons.n_constraints, cons.n_equalities = self.C, neq
            for k in range(self.C):
                cons.kind[k], cons.index[k], cons.bound[k] = int(kinds[k]), int(indices[k]), float(bounds[k])
            cons.centres, cons.n_centres = (None, 0) if centres is None else (centres.data_ptr(), int(centres.shape[0]))       # (the group keeps the tensor alive)
            cons.strict, cons.delta_cons = (1 if solver.strict_constraints else 0), float(delta_cons)
            self.cons = cons
        self.nonneg, self.eta, self.alpha = mo._selection(acq_function, options)
        # with constraints the selection kernel is opt-in; the device sampler on top of it needs inequalities only (see _native_sweep_sphere)
        self.device_selection = bool(options.get("device_selection", True)) if group is None else options.get("device_selection") is True
        self.device_rand = bool(options.get("device_rand")) and (group is None or (self.device_selection and neq == 0))
        self.time0 = time.time()

    def workspace(self, total):
        """the (device, stream)'s workspace, grown to hold a sweep over `total` raw samples"""
        self.wsb = int(self.lib.gabo_sphere_sweep_workspace_bytes(self.dim, total, self.R) if self.cons is None
                       else self.lib.gabo_sphere_sweep_workspace_bytes_constrained(self.dim, total, self.R, self.C))
        key = ("sphere", self.dev.index, self.stream)
        self.ws = _sweep_workspaces.get(key)
        if self.ws is None or self.ws.numel() < self.wsb:
            self.ws = _sweep_workspaces[key] = torch.empty(self.wsb, dtype=torch.uint8, device=self.dev)

    def call(self, name, head, *more):
        """entry point `name`(*head, the out-parameters every entry point has, *more, workspace, stream) - with constraints `name`_constrained, which
        takes them and the pointer to their final values before the workspace.  Returns the out-parameters."""
        best, value, iters = ctypes.c_int64(0), ctypes.c_double(0.0), ctypes.c_int64(0)
        cand, cost, its, cv = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
        args = head + tuple(ctypes.byref(p) for p in (best, value, iters, cand, cost, its)) + more
        if self.cons is not None:
            name, args = name + "_constrained", args + (ctypes.byref(self.cons), ctypes.byref(cv))
        _lib.check(getattr(self.lib, name)(*args, self.ws.data_ptr(), self.wsb, self.stream), name)
        return best, iters, cand, cost, its, cv

    def view(self, ptr, count, dtype):
        return self.ws[int(ptr.value) - self.ws.data_ptr():][:8 * count].view(dtype)

    def result(self, outs, device_selection, picked):
        """solver.log - the keys of _sweep_log, "final_constraints" (R x C constraint values at the final iterates, equalities first; None without constraints),
        "lds_resident" (which instantiation of the solve kernel ran), with options["log_picked"] the restarts' raw samples picked() - and the winner's row"""
        (best, iters, cand, cost, its, cv), R, C = outs, self.R, self.C
        lds = self.lib.gabo_sphere_tr_solve_lds_resident(ctypes.byref(self.cfg.acq), R, C)
        log = self.solver.log = _sweep_log(int(iters.value), self.view(its, R, torch.int64).clone(), self.view(cost, R, torch.float64).clone(),
                                           self.time0, device_selection)
        log["final_constraints"] = self.view(cv, R * C, torch.float64).reshape(R, C).clone() if (self.cons is not None and cv.value) else None
        log["lds_resident"] = bool(lds) if lds >= 0 else None
        if self.options.get("log_picked"):
            log["picked"] = picked()
        return self.view(cand, R * self.dim, torch.float64).reshape(R, self.dim)[int(best.value)].reshape(1, self.dim).clone()

    def one_call(self):
        """gabo_sphere_sweep_run[_constrained]: scoring -> selection kernel -> solve -> arg-max with one host wait, the raw samples from the host sampler
        or - device_rand - drawn on the device.  Returns the candidate, or None when the run reports that the heuristic needs its random fall-backs
        or that the constrained device sampler ran out of tries (a feasible set of measure ~1e-3 of the sphere or less: one warning)."""
        total, R = self.raw_samples, self.R
        self.workspace(total)
        raw = None if self.device_rand else self.mo._host_samples(self.man, total, self.options, (self.dim,))
        sample_seed = int(np.random.randint(0, 2 ** 63 - 1, dtype=np.int64)) if raw is None else 0
        picked, fallback = ctypes.c_void_p(), ctypes.c_int(0)
        outs = self.call("gabo_sphere_sweep_run", (ctypes.byref(self.cfg), total, R, None if raw is None else raw.ctypes.data, sample_seed,
                                                   float(self.eta), float(self.alpha), self.mo._selection_seed()), ctypes.byref(picked), ctypes.byref(fallback))
        ops.check_deferred()
        if not fallback.value:
            return self.result(outs, True, lambda: self.view(picked, R, torch.int64).cpu().numpy().copy())
        if fallback.value == 2 and not getattr(_native_sweep_sphere, "_warned_exhausted", False):          # (once per process)
            _native_sweep_sphere._warned_exhausted = True
            warnings.warn(f"the device sampler found no feasible point for some raw sample in {_lib.GABO_SPHERE_SAMPLE_MAX_TRIES} tries (the "
                          "inequality constraints leave too small a part of the sphere): the raw samples come from manifold.rand on the host")
        return None

    def scored_attempt(self, total):
        """one attempt of the host heuristic: `total` points of the host sampler and their values, then the selection seed"""
        self.workspace(total)
        raw = self.mo._host_samples(self.man, total, self.options, (self.dim,))
        y = np.empty(total, dtype=np.float64)
        _lib.check(self.lib.gabo_sphere_sweep_score(ctypes.byref(self.cfg), total, total, self.R, raw.ctypes.data, y.ctypes.data, self.ws.data_ptr(),
                                                    self.wsb, self.stream), "gabo_sphere_sweep_score")
        ops.check_deferred()
        return y, self.mo._selection_seed()

    def two_calls(self):
        """gabo_sphere_sweep_score, select_rows on the host with its retries, gabo_sphere_sweep_solve[_constrained]"""
        picked, total = self.mo._retry_selection(self.scored_attempt, self.raw_samples, self.R, self.nonneg, self.eta, self.alpha)
        idx = np.ascontiguousarray(picked, dtype=np.int64)
        return self.result(self.call("gabo_sphere_sweep_solve", (ctypes.byref(self.cfg), idx.ctypes.data, self.R, total)), False, idx.copy)


def _native_sweep_sphere(plan, acq_function, solver, num_restarts, raw_samples, options):
    """joint_optimize_manifold on the sphere through the native driver (csrc/spd_sweep.hip).  ONE call with the selection heuristic as a kernel on the
    library's own random stream: the default WITHOUT constraints; with constraints only for options["device_selection"] = True (seeded constrained
    sweeps keep the candidates they returned when the sweep around the solve was Python).  Reproducible for a seed, but the Python path returns the
    same candidate only when handed the same picks (options["log_picked"] records them).  options["device_rand"] draws the raw samples of that call
    on the device; with constraints the device sampler rejects into the INEQUALITY constraints (gabo_sphere_sample) and cannot draw ON an equality:
    then the host sampler (`manifold.rand` / `rand_batch`, in the reference's constrained examples a sampler of feasible points) is used.
    Otherwise - also for acquisition functions that can be negative, more raw samples than the kernel holds, or when the one call gives up - TWO
    calls around select_rows on the host: numpy's and torch's generators are consumed exactly as on the Python path and the device executes its
    statements, so a seeded sweep returns the Python path's candidate, costs and iteration counts bit for bit."""
    from . import manifold_optimize as mo
    sweep = _SphereSweep(mo, plan, acq_function, solver, num_restarts, raw_samples, options)
    with torch.cuda.device(sweep.dev):
        sweep.stream = ops._stream_ptr(sweep.dev)
        one_call = sweep.device_selection and sweep.nonneg and sweep.lib.gabo_spd_sweep_select_supported(raw_samples, sweep.R)
        out = sweep.one_call() if one_call else None
        return sweep.two_calls() if out is None else out
