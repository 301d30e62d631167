"""Multi-start acquisition maximisation on a manifold - same entry points and keyword arguments as the reference
(BoManifolds/manifold_optimization/manifold_optimize.py:36-321), re-organised for the MI355X:

  * the `raw_samples` candidates are scored in one batched acquisition call (as the reference does, :297-309); with
    torch.distributed initialised they are drawn and scored sharded by sample index, one all_gather of (value, sample);
  * the `num_restarts` local solves run in LOCK STEP (BatchedTrustRegions) instead of the sequential loop at :207;
  * with torch.distributed initialised, restart r is owned by rank r % world (interleaved: trust-region iteration counts
    vary), each rank optimises its share on its own GPU, and ONE all_gather of (acquisition value, candidate) per restart
    followed by a local argmax replaces get_best_candidates (:118-120).  Ties go to the lowest global restart index on
    every rank, so all ranks return the same candidate.
"""
import warnings

import numpy as np
import torch

from ..distributed import row_block
from ..models import BadInitialCandidatesWarning, get_best_candidates, initialize_q_batch, initialize_q_batch_nonneg, is_nonnegative      # noqa: F401
from ..fused_acquisition import FusedAcquisition
from .batched_trust_regions import BatchedProblem, BatchedTrustRegions
# the native drivers: joint_optimize_manifold looks the plan up here; the other names stay reachable here for bench.py, tools/ and tests/
from .native_sweep import _all_gather_rows, _native_sweep, _native_sweep_plan, _native_sweep_sphere, _RowsState, _sweep_workspaces       # noqa: F401


def _dist():
    import torch.distributed as dist
    return dist if (dist.is_available() and dist.is_initialized()) else None


def _mark(options, label):
    """development hook: options["timeline"] = [] collects (label, perf_counter) pairs of the sweep's host phases (tools/sweep_native_phases.py)"""
    tl = options.get("timeline")
    if tl is not None:
        import time
        tl.append((label, time.perf_counter()))


def shard_restarts(num_restarts, rank, world):
    """Indices of the restarts rank `rank` owns (interleaved)."""
    return list(range(rank, num_restarts, world))


def gather_best(candidates_local, values_local, owned, num_restarts):
    """all_gather of per-restart (value, candidate) and argmax.  candidates_local: r_local x q x d, values_local:
    r_local.  Returns (best candidate q x d, all candidates R x q x d, all values R) - identical on every rank."""
    dist = _dist()
    if dist is None or dist.get_world_size() == 1:
        return get_best_candidates(candidates_local, values_local), candidates_local, values_local
    world = dist.get_world_size()
    per = (num_restarts + world - 1) // world
    q, d = candidates_local.shape[-2:]
    dev, dt = candidates_local.device, candidates_local.dtype
    packed = torch.full((per, 1 + q * d), float("-inf"), dtype=dt, device=dev)     # padded slots lose every argmax
    n = len(owned)
    if n:
        packed[:n, 0] = values_local.reshape(-1).to(dt)
        packed[:n, 1:] = candidates_local.reshape(n, -1)
    gathered = [torch.empty_like(packed) for _ in range(world)]
    dist.all_gather(gathered, packed)
    values = torch.full((num_restarts,), float("-inf"), dtype=dt, device=dev)
    cands = torch.zeros(num_restarts, q, d, dtype=dt, device=dev)
    for r in range(world):
        idx = shard_restarts(num_restarts, r, world)
        if idx:
            values[idx] = gathered[r][:len(idx), 0]
            cands[idx] = gathered[r][:len(idx), 1:].reshape(len(idx), q, d)
    return get_best_candidates(cands, values), cands, values


def joint_optimize_manifold(acq_function, manifold, solver, q, num_restarts, raw_samples, bounds, sample_type=torch.float64,
                            options=None, inequality_constraints=None, equality_constraints=None, pre_processing_manifold=None,
                            post_processing_manifold=None, approx_hessian=False, solver_init_conds=False):
    """Returns the `q x d` best candidate (manifold_optimize.py:36-120)."""
    options = options or {}
    analytic = getattr(acq_function, "is_analytic", True)
    _mark(options, "-> plan")
    plan = _native_sweep_plan(acq_function, manifold, solver, q if not analytic else 1, num_restarts, raw_samples, bounds, sample_type, options,
                              inequality_constraints, equality_constraints, pre_processing_manifold, post_processing_manifold, approx_hessian,
                              solver_init_conds)
    _mark(options, "<- plan")
    if plan is not None:
        return plan["driver"](plan, acq_function, solver, num_restarts, raw_samples, options)
    batch_initial_conditions = gen_batch_initial_conditions_manifold(
        acq_function=acq_function, manifold=manifold, bounds=bounds, q=None if analytic else q, num_restarts=num_restarts,
        raw_samples=raw_samples, sample_type=sample_type, options=options, post_processing_manifold=post_processing_manifold)
    dist = _dist()
    rank, world = (dist.get_rank(), dist.get_world_size()) if dist is not None else (0, 1)
    # (no broadcast: every rank selected the same initial conditions from the all_gathered raw samples)
    owned = shard_restarts(num_restarts, rank, world)
    batch_limit = options.get("batch_limit", num_restarts)
    cand_list, val_list = [], []
    start = 0
    while start < len(owned):
        idx = owned[start:start + batch_limit]
        c, v = gen_candidates_manifold(
            initial_conditions=batch_initial_conditions[idx], acquisition_function=acq_function, manifold=manifold,
            solver=solver, pre_processing_manifold=pre_processing_manifold, post_processing_manifold=post_processing_manifold,
            lower_bounds=None if bounds is None else bounds[0], upper_bounds=None if bounds is None else bounds[1],
            options={k: v for k, v in options.items() if k not in ("batch_limit", "nonnegative")},   # "hip_graphs", "device" pass through
            inequality_constraints=inequality_constraints, equality_constraints=equality_constraints,
            approx_hessian=approx_hessian, solver_init_conds=solver_init_conds)
        cand_list.append(c)
        val_list.append(v)
        start += batch_limit
    if cand_list:
        cands, vals = torch.cat(cand_list), torch.cat(val_list)
    else:
        cands = batch_initial_conditions[:0]
        vals = torch.zeros(0, dtype=batch_initial_conditions.dtype, device=batch_initial_conditions.device)
    best, _, _ = gather_best(cands, vals, owned, num_restarts)
    return best


def sequential_optimize_manifold(acq_function, manifold, solver, q, num_restarts, raw_samples, bounds, sample_type=torch.float64,
                                 options=None, inequality_constraints=None, equality_constraints=None, pre_processing_manifold=None,
                                 post_processing_manifold=None, approx_hessian=False, solver_init_conds=False):
    """A batch of q proposals, `q x d` in the order chosen, by greedy "Kriging believer" selection (Ginsbourger et al. 2010; not in the
    reference, whose analytic acquisitions ignore q): row 0 is joint_optimize_manifold's candidate; row k is the same sweep on
    ExpectedImprovement over the model conditioned on rows 0 ... k - 1 with the believer's targets (the posterior mean at each of them:
    models.*.condition_on_observations - bordered updates of the prediction cache on the device, no new factorisation), best_f and maximize
    unchanged.  Every sweep is a joint_optimize_manifold call with the arguments given here, so it takes whatever plan that function picks.
    acq_function: models.ExpectedImprovement over models.ExactGP or models.SingleTaskGP; the rows are the model's input vectors."""
    from .. import models
    if isinstance(acq_function, models.PosteriorMean):
        raise ValueError("sequential_optimize_manifold: the believer's observation does not change the posterior mean, so every row would be the "
                         "same point; use ExpectedImprovement")
    if type(acq_function) is not models.ExpectedImprovement or type(getattr(acq_function, "model", None)) not in (models.ExactGP, models.SingleTaskGP):
        raise NotImplementedError("sequential_optimize_manifold supports models.ExpectedImprovement over models.ExactGP or models.SingleTaskGP, got "
                                  f"{type(acq_function).__name__} over {type(getattr(acq_function, 'model', None)).__name__}")
    q = int(q)
    if q < 1:
        raise ValueError(f"sequential_optimize_manifold: q = {q}")
    acq, rows = acq_function, []
    for k in range(q):
        rows.append(joint_optimize_manifold(acq, manifold, solver, 1, num_restarts, raw_samples, bounds, sample_type=sample_type, options=options,
                                            inequality_constraints=inequality_constraints, equality_constraints=equality_constraints,
                                            pre_processing_manifold=pre_processing_manifold, post_processing_manifold=post_processing_manifold,
                                            approx_hessian=approx_hessian, solver_init_conds=solver_init_conds))
        if k + 1 < q:
            x = rows[-1].detach().reshape(1, -1).to(acq.model.train_x.device, torch.float64)
            acq = models.ExpectedImprovement(acq.model.condition_on_observations(x), best_f=acq_function.best_f, maximize=acq_function.maximize)
    return rows[0] if q == 1 else torch.cat([r.reshape(1, -1) for r in rows])


def _library_constraint(con):
    """functools.partial over one of the library's eigenvalue constraints (plain or stated in the original space of a nested
    SPD mapping) or sphere constraints (coordinate bounds, geodesic ball): torch code without host synchronisation, safe to capture
    into the hipGraphs of the trust-region iteration."""
    import functools

    from ..nested_mappings import nested_spd_constraints_utils as nested
    from ..Riemannian_utils import spd_constraints_utils_torch as plain
    from ..Riemannian_utils import sphere_constraints_utils_torch as sphere
    if not isinstance(con, functools.partial):
        return False
    if con.func in (sphere.coordinate_lower_bound_constraint_torch, sphere.coordinate_upper_bound_constraint_torch,
                    sphere.geodesic_ball_constraint_torch):
        return sphere.builtin_sphere_constraint(con) is not None       # (all parameters by keyword: the device evaluates those itself)
    return con.func in (plain.max_eigenvalue_constraint_torch, plain.min_eigenvalue_constraint_torch,
                        nested.max_eigenvalue_nested_spd_constraint, nested.min_eigenvalue_nested_spd_constraint)


def gen_candidates_manifold(initial_conditions, acquisition_function, manifold, solver, pre_processing_manifold=None,
                            post_processing_manifold=None, lower_bounds=None, upper_bounds=None, inequality_constraints=None,
                            equality_constraints=None, approx_hessian=False, solver_init_conds=False, options=None):
    """Optimise every initial condition (R x 1 x d) and return (candidates R x 1 x d, acquisition values R)
    (manifold_optimize.py:124-228).  `solver` is one of this package's trust-region classes (TrustRegions, ConstrainedTrustRegions,
    StrictConstrainedTrustRegions = BatchedTrustRegions: all restarts in lock step); any other object exposing pymanopt's
    `solve(problem, x=...)` is driven restart by restart (`_gen_candidates_pointwise`)."""
    x0 = initial_conditions.detach()
    if x0.shape[1] != 1:
        raise NotImplementedError("q != 1 is not handled (neither does the reference: manifold_optimize.py:206)")
    x0 = x0[:, 0]
    if pre_processing_manifold is not None:
        x0 = pre_processing_manifold(x0)

    def cost(x):
        if post_processing_manifold is not None:
            x = post_processing_manifold(x)
        x = x[:, None].double()                     # R x (q=1) x d: a t-batch per restart  (:182-184)
        return -acquisition_function(x)

    def precon(x, d):                               # (:190-193)
        flat = d.reshape(d.shape[0], -1)
        zero = flat.sum(1) == 0
        return torch.where(zero.reshape((-1,) + (1,) * (d.dim() - 1)), d + 1e-30, d)

    from .augmented_lagrange_method import AugmentedLagrangeMethod
    if (isinstance(solver, AugmentedLagrangeMethod) and isinstance(getattr(solver, "inner_solver", None), BatchedTrustRegions)
            and not solver_init_conds and (equality_constraints is not None or inequality_constraints is not None)
            and (options or {}).get("batched_alm", True) and getattr(solver, "_logverbosity", 0) <= 0):
        # The augmented-Lagrangian method around this package's trust regions - the default solver of the reference's constrained sphere
        # examples - on all restarts in lock step: the per-restart updates of the reference's loop with the inner solves batched
        # (augmented_lagrange_method.py: solve_batched; options={"batched_alm": False} drives it restart by restart as the reference does).
        fused = FusedAcquisition.build(acquisition_function, post_processing_manifold, x0.device) if (x0.is_cuda and (options or {}).get("fused_acquisition", True)) else None
        problem = BatchedProblem(manifold, cost, approx_hessian=True, precon=precon, fused=fused)
        opt_x = solver.solve_batched(problem, x0.double(), eq_constraints=equality_constraints, ineq_constraints=inequality_constraints)
        candidates = opt_x if post_processing_manifold is None else post_processing_manifold(opt_x)
        candidates = candidates[:, None]
        with torch.no_grad():
            batch_acquisition = -problem.cost(opt_x) if fused is not None else acquisition_function(candidates)
        return candidates.detach(), batch_acquisition.detach()
    if not isinstance(solver, BatchedTrustRegions):
        return _gen_candidates_pointwise(x0, acquisition_function, manifold, solver, post_processing_manifold, inequality_constraints,
                                         equality_constraints, approx_hessian, solver_init_conds)
    fused = None
    if (options or {}).get("fused_acquisition", True) and x0.is_cuda:
        # built-in surrogate + kernel + Mandel post-processing: value and gradient as a fixed chain of HIP launches
        fused = FusedAcquisition.build(acquisition_function, post_processing_manifold, x0.device)
    problem = BatchedProblem(manifold, cost, approx_hessian=approx_hessian, precon=precon,
                             use_hip_graphs=bool((options or {}).get("hip_graphs", False)), fused=fused)
    problem.reference_precon = True          # `precon` above is the one csrc/spd_tcg.hip implements
    problem.device_tcg = bool((options or {}).get("device_tcg", True))
    problem.device_outer = bool((options or {}).get("device_outer", True))
    problem.device_iteration = bool((options or {}).get("device_iteration", True))
    problem.device_solve = bool((options or {}).get("device_solve", True))
    # the constraint callables are user code: they run eagerly between graph replays unless the caller states they are capturable -
    # or they are this library's own eigenvalue / sphere constraints with their parameters bound by functools.partial (sync-free by construction)
    cons = list(equality_constraints or []) + list(inequality_constraints or [])
    problem.capture_constraints = bool((options or {}).get("capture_constraints", bool(cons) and all(_library_constraint(c) for c in cons)))
    if solver_init_conds:
        x0 = torch.stack([torch.as_tensor(manifold.rand()) for _ in range(x0.shape[0])]).to(x0)
    if equality_constraints is not None or inequality_constraints is not None:
        opt_x = solver.solve(problem, x0.double(), eq_constraints=equality_constraints, ineq_constraints=inequality_constraints)
    else:
        opt_x = solver.solve(problem, x0.double())
    candidates = opt_x
    if post_processing_manifold is not None:
        candidates = post_processing_manifold(candidates)
    candidates = candidates[:, None]
    with torch.no_grad():
        final = getattr(solver, "log", None) or {}
        if fused is not None and final.get("one_launch_solve") and final.get("final_cost") is not None and final["final_cost"].shape[0] == opt_x.shape[0]:
            # the single-launch solve ended with the cost of every restart's final iterate in its state (evaluated by the same device
            # function the fused chain calls): no further launch
            batch_acquisition = -final["final_cost"]
        elif fused is not None:
            batch_acquisition = -fused.cost(opt_x)          # same values through the fused chain (one launch for the SPD kernels)
        else:
            batch_acquisition = acquisition_function(candidates)
    if candidates.is_cuda:
        from .. import ops as _ops
        _ops.check_deferred()          # (no-op unless a deferred launch check is still queued: then one 8-byte read-back)
    return candidates.detach(), batch_acquisition.detach()


def _gen_candidates_pointwise(x0, acquisition_function, manifold, solver, post_processing_manifold, inequality_constraints,
                              equality_constraints, approx_hessian, solver_init_conds):
    """The reference's own loop (manifold_optimize.py:175-228) for a solver that is not one of this package's lock-step trust regions:
    any object with pymanopt's `solve(problem, x=ndarray[, eq_constraints=, ineq_constraints=])`.  One pymanopt-style `Problem` on
    single points (autograd through the acquisition function, whose kernel evaluations are still the HIP kernels), restarts one
    after the other on the host."""
    import types

    from ..pymanopt_addons.problem import Problem
    from .approximate_hessian import get_hessianfd

    def cost(x):                                     # (:177-185)
        if post_processing_manifold is not None:
            x = post_processing_manifold(x)
        return -acquisition_function(x[None].double()).sum()

    def precon(x, d):                                # (:189-192)
        if np.sum(d) == 0.0:
            d += 1e-30
        return d

    problem = Problem(manifold=manifold, cost=cost, verbosity=0, arg=torch.Tensor(), precon=precon)
    if approx_hessian:
        problem._hess = types.MethodType(get_hessianfd, problem)
    constrained = equality_constraints is not None or inequality_constraints is not None
    points = []
    for i in range(x0.shape[0]):
        if solver_init_conds:
            opt_x = solver.solve(problem)
        elif constrained:
            opt_x = solver.solve(problem, x=x0[i].detach().cpu().numpy(), eq_constraints=equality_constraints,
                                 ineq_constraints=inequality_constraints)
        else:
            opt_x = solver.solve(problem, x=x0[i].detach().cpu().numpy())
        points.append(torch.as_tensor(np.asarray(opt_x), dtype=torch.float64))
    candidates = torch.stack(points).to(x0.device)
    if post_processing_manifold is not None:
        candidates = post_processing_manifold(candidates)
    candidates = candidates[:, None]
    with torch.no_grad():
        batch_acquisition = acquisition_function(candidates)
    return candidates.detach(), batch_acquisition.detach()


class _rank_stream:
    """Host draws of one rank's shard of the raw samples.  Single process: numpy's global stream as it is (the reference's draw order,
    pinned by golden vectors).  Several ranks: every rank takes ONE integer from the global stream - identically seeded ranks stay in
    step, which the GP fit's numpy candidates and every later draw rely on - and draws its shard from a temporary state seeded with
    (that integer, rank); the global state is put back afterwards.  The shards of different ranks are then distinct streams whatever the
    seeding of the processes, and nobody has to reseed numpy per rank."""

    def __init__(self, rank, world):
        self.rank, self.world, self.saved = rank, world, None

    def __enter__(self):
        if self.world > 1:
            base = int(np.random.randint(0, 2 ** 31 - 1))
            self.saved = np.random.get_state()
            np.random.seed([base, self.rank])
        return self

    def __exit__(self, *exc):
        if self.saved is not None:
            np.random.set_state(self.saved)
        return False


def _host_samples(manifold, count, options, shape=None):
    """`count` points of the host sampler as one float64 array, (count,) + point shape: one vectorised draw with options["batched_rand"] (same
    distribution, not numpy's draw order of `count` manifold.rand() calls), else manifold.rand() point by point.  shape: the point shape the caller
    expects, checked; a caller that does not know it (None) learns it from the array, for which an empty draw takes one point from the sampler."""
    if options.get("batched_rand") and hasattr(manifold, "rand_batch"):
        raw = manifold.rand_batch(count)
    elif count:
        raw = np.stack([np.asarray(manifold.rand()) for _ in range(count)])
    else:
        raw = np.zeros((0,) + shape) if shape is not None else np.asarray(manifold.rand())[None][:0]
    raw = np.ascontiguousarray(raw, dtype=np.float64)
    if shape is not None and raw.shape != (count,) + shape:
        raise RuntimeError(f"manifold.rand returned points of shape {raw.shape[1:]}, expected {shape}")
    return raw


def _draw_raw_samples(manifold, total, first, count, options, sample_type, rank=0, world=1):
    """Raw samples first ... first + count - 1 of the `total` of one attempt, count x 1 x (point shape) (manifold_optimize.py:288).
    `manifold.rand` stays a host callable (callers monkey-patch it); two opt-in faster routes draw the same distribution."""
    device = options.get("device")
    if options.get("device_rand") and device is not None and hasattr(manifold, "rand_batch_device"):
        # drawn on the device, stream addressed by the global sample index: the shards of ranks with a common numpy seed are
        # exactly the samples one rank would have drawn
        return manifold.rand_batch_device(total, device, first=first, count=count)[:, None].to(sample_type)
    with _rank_stream(rank, world):
        pts = torch.from_numpy(_host_samples(manifold, count, options))[:, None].to(sample_type)
    return pts if device is None else pts.to(device)


def _score_raw_samples(acq_function, X_rnd, post_processing_manifold, options):
    """(post-processed samples, acquisition values) of a block of raw samples, no gradients (manifold_optimize.py:291-309)."""
    fused = None
    if options.get("fused_acquisition", True) and X_rnd.is_cuda and X_rnd.shape[1] == 1:
        fused = FusedAcquisition.build(acq_function, post_processing_manifold, X_rnd.device)
    with torch.no_grad():
        if fused is not None:          # built-in surrogate: one launch of the fused chain for the SPD kernels, same values
            Y = -fused.cost(X_rnd[:, 0].contiguous()) if X_rnd.shape[0] else X_rnd.new_zeros(0, dtype=torch.float64)
            X = X_rnd if post_processing_manifold is None else post_processing_manifold(X_rnd)
            return X, Y
        X = X_rnd if post_processing_manifold is None else post_processing_manifold(X_rnd)
        step = options.get("batch_limit") or max(X.shape[0], 1)
        parts = [acq_function(X[s:s + step]) for s in range(0, X.shape[0], step)]
        Y = torch.cat(parts).to(X) if parts else X.new_zeros(0)
    return X, Y


def _gather_raw_samples(X_loc, Y_loc, total, seed):
    """ONE all_gather that assembles the sample-index shards of every rank - rows [row_block(total, r, world)) from rank r - and
    carries each rank's proposal for the selection seed; rank 0's is the one every rank uses.  Returns (X, Y, seed), identical on
    every rank (raw-sample scoring sharded by sample index)."""
    dist = _dist()
    if dist is None or dist.get_world_size() == 1:
        return X_loc, Y_loc, seed
    world = dist.get_world_size()
    per = (total + world - 1) // world
    feat = X_loc[0].numel() if X_loc.shape[0] else int(np.prod(X_loc.shape[1:]))
    packed = torch.zeros(per + 1, 1 + feat, dtype=torch.float64, device=X_loc.device)
    packed[0, 0] = float(seed)                      # < 2^52: exact in a double
    n = X_loc.shape[0]
    packed[1:1 + n, 0] = Y_loc.reshape(-1).double()
    packed[1:1 + n, 1:] = X_loc.reshape(n, -1).double()
    parts = [torch.empty_like(packed) for _ in range(world)]
    dist.all_gather(parts, packed)
    counts = [row_block(total, r, world) for r in range(world)]
    X = torch.cat([parts[r][1:1 + hi - lo, 1:] for r, (lo, hi) in enumerate(counts)]).reshape((total,) + tuple(X_loc.shape[1:])).to(X_loc.dtype)
    Y = torch.cat([parts[r][1:1 + hi - lo, 0] for r, (lo, hi) in enumerate(counts)]).to(Y_loc.dtype)
    if world > 1 and counts[1][1] - counts[1][0] == counts[0][1] and counts[0][1] > 0 and torch.equal(parts[0][1:], parts[1][1:]) \
            and float(parts[0][0, 0]) == float(parts[1][0, 0]) and not getattr(_gather_raw_samples, "_warned", False):
        _gather_raw_samples._warned = True
        warnings.warn("ranks 0 and 1 drew identical raw samples: manifold.rand does not read numpy's global generator (whose per-rank "
                      "streams are derived internally) - make the sampler rank-aware, or draw on the device (options['device_rand']), "
                      "whose stream is addressed by sample index.  Do NOT reseed numpy per rank: the GP fit draws from it on every rank")
    return X, Y, int(parts[0][0, 0].item())


def _selection(acq_function, options):
    """(nonneg, eta, alpha) of the botorch heuristic gen_batch_initial_conditions_manifold applies to the scored raw samples:
    initialize_q_batch_nonneg for acquisition functions that are non-negative (or options["nonnegative"]), initialize_q_batch otherwise
    (manifold_optimize.py:296-317), with their keyword arguments from `options`."""
    nonneg = bool(options.get("nonnegative") or is_nonnegative(acq_function))
    return nonneg, float(options.get("eta", 1.0)), float(options.get("alpha", 1e-4))


def select_rows(y, n, generator, nonneg, eta=1.0, alpha=1e-4):
    """Which n of the scored raw samples become restarts: models.initialize_q_batch_nonneg / initialize_q_batch ([3P] botorch.optim.initializers)
    stated on ROW INDICES, for values that are already on the host.  y: (total,) float64 numpy array.  Returns (int64 index array of length n,
    bad) - bad: the heuristic had to pick at random (botorch's BadInitialCandidatesWarning; the caller retries with more samples).
    The comparisons and index bookkeeping are numpy; everything that feeds the random draw (the weights, torch.multinomial / torch.randperm on
    `generator`) is the torch arithmetic of the functions it restates, so the rows picked are theirs, draw for draw (tests/test_selection_cpu.py).
    Rounds 4-5 called those functions on torch tensors: a dozen tiny CPU-tensor operations, 0.16-0.25 ms of a 1.4-ms sweep."""
    total = int(y.shape[0])
    if n > total:
        raise RuntimeError(f"n ({n}) cannot be larger than the number of provided samples ({total})")
    if n == total:
        return np.arange(total, dtype=np.int64), False
    if not nonneg:
        Y = torch.from_numpy(y)
        Ystd = Y.std()
        if Ystd == 0:
            return torch.randperm(n=total, generator=generator)[:n].numpy().astype(np.int64), True
        max_idx = int(torch.max(Y, dim=0)[1])
        etaZ = eta * ((Y - Y.mean()) / Ystd)
        weights = torch.exp(etaZ)
        while torch.isinf(weights).any():
            etaZ *= 0.5
            weights = torch.exp(etaZ)
        idcs = torch.multinomial(weights, n, generator=generator).numpy().astype(np.int64)
        if max_idx not in idcs:
            idcs[-1] = max_idx
        return idcs, False
    max_idx = int(np.argmax(y))                 # (first maximum; a NaN wins, as in torch.max)
    max_val = float(y[max_idx])
    if max_val != max_val:
        raise RuntimeError("select_rows: the acquisition values of the raw samples contain NaN")       # (botorch's loop below would never end)
    if max_val <= 0:
        return torch.randperm(n=total, generator=generator)[:n].numpy().astype(np.int64), True
    pos = y > 0
    num_pos = int(pos.sum())
    if num_pos < n:
        remaining = n - num_pos
        rand_idx = torch.randperm(total - num_pos, generator=generator)[:remaining].numpy()
        both = np.concatenate([np.nonzero(pos)[0], np.nonzero(~pos)[0][rand_idx]])
        return both[torch.randperm(n, generator=generator).numpy()].astype(np.int64), False
    alpha_pos = y >= alpha * max_val
    while alpha_pos.sum() < n:
        alpha = 0.1 * alpha
        alpha_pos = y >= alpha * max_val
    pool = np.nonzero(alpha_pos)[0]
    weights = torch.exp(eta * (torch.from_numpy(y[alpha_pos]) / max_val - 1))
    idcs = pool[torch.multinomial(weights, n, generator=generator).numpy()].astype(np.int64)
    if max_idx not in idcs:
        idcs[-1] = max_idx
    return idcs, False


def _selection_seed():
    return int(torch.randint(0, 2 ** 52, (1,)).item())          # from torch's global generator, like botorch's own multinomial draw; < 2^52: exact in a double


def _retry_selection(scored_attempt, raw_samples, num_restarts, nonneg, eta, alpha):
    """The reference's retry loop (manifold_optimize.py:283-320): attempts 1 ... 4 on raw_samples x attempt samples, as long as the heuristic reports that
    it had to pick at random; after the fourth, its warning.  scored_attempt(total) draws and scores `total` raw samples, then takes _selection_seed() -
    with several ranks rank 0's, which the all_gather of the scores carries - and returns (values on the host: (total,) float64 numpy, seed).  The rows
    are selected on a fresh generator with that seed: identical on every rank.  Returns (rows, total of the attempt they index)."""
    for attempt in range(1, 5):                     # the reference's factor = 1 ... max_factor - 1
        total = raw_samples * attempt
        y, seed = scored_attempt(total)
        picked, bad = select_rows(y, num_restarts, torch.Generator().manual_seed(seed), nonneg, eta, alpha)
        if not bad:
            return picked, total
    warnings.warn("Unable to find non-zero acquisition function values - initial conditions are being selected randomly.",
                  BadInitialCandidatesWarning)
    return picked, total


def gen_batch_initial_conditions_manifold(acq_function, manifold, bounds, q, num_restarts, raw_samples,
                                          sample_type=torch.float64, options=None, post_processing_manifold=None):
    """`num_restarts x q x d` initial conditions chosen among `raw_samples` random manifold points by the botorch
    heuristics (manifold_optimize.py:232-321), with the reference's retries (_retry_selection).

    With torch.distributed initialised the raw samples are sharded BY SAMPLE INDEX: rank r draws and scores rows
    row_block(total, r, world) only, one all_gather assembles (Y, X), and every rank runs the selection on identical data with an
    identical random stream - so all ranks hold the same initial conditions without a broadcast."""
    options = options or {}
    q = 1 if q is None else q
    nonneg, eta, alpha = _selection(acq_function, options)
    dist = _dist()
    rank, world = (dist.get_rank(), dist.get_world_size()) if dist is not None else (0, 1)
    samples = []

    def scored_attempt(total):
        lo, hi = row_block(total, rank, world) if world > 1 else (0, total)
        X_loc, Y_loc = _score_raw_samples(acq_function, _draw_raw_samples(manifold, total, lo, hi - lo, options, sample_type, rank, world),
                                          post_processing_manifold, options)
        X_rnd, Y_rnd, seed = _gather_raw_samples(X_loc, Y_loc, total, _selection_seed())
        samples[:] = [X_rnd]
        # The selection heuristic is a dozen data-dependent decisions on `total` scalars: on the device every one of them is a launch and a read-back (0.85 ms of
        # the 4.4-ms config-4 sweep, tools/sweep_phases2.py); the values come to the host in ONE copy, select_rows picks ROW INDICES there, the rows are gathered on the device
        y_host = Y_rnd.detach().double().cpu().numpy()          # (the host waits for the scores here anyway: deferred launch checks cost nothing now)
        if Y_rnd.is_cuda:
            from .. import ops as _ops
            _ops.check_deferred()
        return np.ascontiguousarray(y_host.reshape(-1)), seed
    picked, _ = _retry_selection(scored_attempt, raw_samples * q, num_restarts, nonneg, eta, alpha)
    return samples[0].index_select(0, torch.from_numpy(picked).to(samples[0].device))
