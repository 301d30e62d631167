"""Constraints on the sphere with the reference's module name (BoManifolds/Riemannian_utils/sphere_constraints_utils_torch.py:12-25 holds
`post_processing_init_sphere_torch`) plus the constraint functions of the reference's three constrained sphere examples as library functions:
the coordinate bounds of gabo_sphere_bound_constraints.py:94-121 (and, as an equality, the great circle of
gabo_sphere_equality_constraints.py:106-107) and the geodesic ball of gabo_sphere_inequality_constraints.py.

The functions are plain torch code for one point (dim,) or a batch (R, dim), differentiable, on any device.  Bound with functools.partial
(every parameter by keyword) they are recognised by `builtin_sphere_constraint`, and the trust-region kernels of csrc/sphere_tr.hip
evaluate them themselves (gabo_sphere_constraints_eval, gabo_sphere_tr_solve_constrained)."""
import torch

from .. import _lib


def post_processing_init_sphere_torch(x):
    """rows of x (N x d) scaled to unit norm"""
    return x / torch.linalg.vector_norm(x, dim=-1, keepdim=True)


def coordinate_lower_bound_constraint_torch(x, index, lower_bound):
    """x[..., index] - lower_bound  (>= 0 when satisfied; as an equality constraint: the circle x[index] = lower_bound)"""
    return x[..., index] - lower_bound


def coordinate_upper_bound_constraint_torch(x, index, upper_bound):
    """upper_bound - x[..., index]  (>= 0 when satisfied)"""
    return upper_bound - x[..., index]


def geodesic_ball_constraint_torch(x, center, angle):
    """angle - acos(clip(<x, center>, -1, 1))  (>= 0 inside the geodesic ball of half-angle `angle` around `center`).

    The gradient is DEFINED as zero where |<x, center>| >= 1: the clip is flat outside [-1, 1] and acos has no finite derivative at +-1
    (autograd through clip and acos gives inf or nan there).  The device form (csrc/sphere_tr.hip: sph_cons_eval) does the same."""
    c = (x * center.to(x)).sum(-1)
    inside = c.abs() < 1
    smooth = torch.acos(torch.where(inside, c, torch.zeros_like(c)))           # (the branch not taken sees acos(0): a finite derivative to mask)
    flat = torch.acos(torch.clamp(c.detach(), -1.0, 1.0))
    return angle - torch.where(inside, smooth, flat)


def builtin_sphere_constraint(con):
    """(kind, index, bound) for the coordinate kinds, (kind, None, bound, center) for the ball, when `con` is a constraint the library can
    evaluate inside its sphere kernels, else None (the contract of spd_constraints_utils_torch.builtin_constraint): a functools.partial over
    one of the three functions above with ALL parameters bound by keyword.  A tensor bound must have one element; `center` must be a
    one-dimensional tensor that does not require grad (its length is compared with the dimension by the caller)."""
    import functools
    if not isinstance(con, functools.partial) or con.args:
        return None

    def scalar(v):
        if torch.is_tensor(v):
            return float(v.item()) if v.numel() == 1 and not v.requires_grad else None
        return float(v) if isinstance(v, (int, float)) and not isinstance(v, bool) else None

    kw = con.keywords
    for fn, name, kind in ((coordinate_lower_bound_constraint_torch, "lower_bound", _lib.GABO_SPHERE_CONSTRAINT_COORD_LOWER),
                           (coordinate_upper_bound_constraint_torch, "upper_bound", _lib.GABO_SPHERE_CONSTRAINT_COORD_UPPER)):
        if con.func is fn:
            if set(kw) != {"index", name}:
                return None
            index, bound = kw["index"], scalar(kw[name])
            if isinstance(index, bool) or not isinstance(index, int) or bound is None:
                return None
            return (kind, index, bound)
    if con.func is geodesic_ball_constraint_torch:
        if set(kw) != {"center", "angle"}:
            return None
        center, bound = kw["center"], scalar(kw["angle"])
        if bound is None or not torch.is_tensor(center) or center.dim() != 1 or center.requires_grad or not center.dtype.is_floating_point:
            return None
        return (_lib.GABO_SPHERE_CONSTRAINT_GEODESIC_BALL, None, bound, center)
    return None


_groups = {}          # ids of the constraints -> (the constraints, dim, device, packed): see builtin_sphere_group


def builtin_sphere_group(constraints, dim, device):
    """(kinds, indices, bounds, centres) - what ops.sphere_constraints_eval and ops.SphereTr.solve take - when EVERY constraint is a built-in
    of a sphere of ambient dimension `dim` (at most 8 of them), else None.  centres: the balls' centres as one (n_centres x dim) fp64 tensor
    on `device` (None without a ball); a negative coordinate index counts from the end, as it does in torch.  Remembered per constraint list
    (the solvers ask once per outer iteration, possibly under graph capture, where nothing may be copied from the host)."""
    cons = list(constraints)
    if not cons or len(cons) > 8:
        return None
    key = tuple(id(c) for c in cons)
    held = _groups.get(key)
    if held is not None and all(a is b for a, b in zip(held[0], cons)) and held[1] == dim and held[2] == torch.device(device):
        return held[3]
    kinds, indices, bounds, centres = [], [], [], []
    packed = ()
    for info in (builtin_sphere_constraint(c) for c in cons):
        if info is None:
            packed = None
            break
        index = info[1]
        if len(info) == 4:
            if info[3].shape[0] != dim:
                packed = None
                break
            index = len(centres)
            centres.append(info[3].detach().to(device=device, dtype=torch.float64))
        elif not -dim <= index < dim:
            packed = None
            break
        kinds.append(info[0])
        indices.append(index % dim if len(info) == 3 else index)
        bounds.append(info[2])
    if packed is not None:
        packed = (kinds, indices, bounds, torch.stack(centres).contiguous() if centres else None)
    if len(_groups) > 64:
        _groups.clear()
    _groups[key] = (cons, dim, torch.device(device), packed)
    return packed
