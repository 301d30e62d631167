"""Host-side launch plumbing: torch tensors in, C-ABI calls on the current HIP stream, torch tensors out.

torch is used for device memory and stream ownership only; every number is produced by libgabo_hip.so.
Inputs living on the CPU are moved to the GPU, computed there and moved back (the reference's examples build CPU
tensors); without a GPU every call raises - there is no CPU implementation in this package.
"""
import math

import torch

from . import _lib, _status
from ._status import (_check_launch, _deferred, _not_spd_message, _raise_if_not_spd, _status_rings, _status_word,     # noqa: F401
                      check_deferred, check_prefetched, prefetch_deferred, set_error_checking)      # (device status words: ops.* as before)


def _device_for(*tensors):
    for t in tensors:
        if t.is_cuda:
            return t.device
    if not torch.cuda.is_available():
        raise RuntimeError("gabotorch_amd needs an MI355X: no HIP device is visible and there is no CPU fallback")
    return torch.device("cuda", torch.cuda.current_device())


def _stream_ptr(device):
    """raw hipStream_t of torch's current stream on `device` (torch.cuda.current_stream builds a Stream object around the same call: 4 us a time)"""
    idx = device.index if isinstance(device, torch.device) else torch.device(device).index
    return torch._C._cuda_getCurrentRawStream(torch.cuda.current_device() if idx is None else idx)


class _NoCtx:
    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False


_NO_CTX = _NoCtx()


def _on(device):
    """`with _on(dev):` = `with torch.cuda.device(dev):` when dev is not the current device, nothing otherwise (the guard object costs ~8 us)"""
    idx = device.index if isinstance(device, torch.device) else torch.device(device).index
    return _NO_CTX if (idx is None or idx == torch.cuda.current_device()) else torch.cuda.device(idx)


def _flatten_batch(x, tail_dims):
    """(..., tail) -> (tensor2d_or_3d contiguous, batch, batch_stride_in_elements).  A batch produced by
    `.expand()` (all batch strides 0) is passed as ONE shared set with batch stride 0."""
    shape = x.shape                   # (every read of .shape builds a torch.Size: once)
    bshape = shape[:-tail_dims]
    nb = math.prod(bshape)
    if len(bshape) > 0 and nb > 1 and all(st == 0 for st, sz in zip(x.stride()[:len(bshape)], bshape) if sz > 1):
        base = x[(0,) * len(bshape)].contiguous()
        return base, nb, 0
    return x.contiguous(), nb, math.prod(shape[-tail_dims:])


def _prep(x, device):
    if x.dtype != torch.float64:
        x = x.double()
    return x.to(device)


def _ptr(t):
    """the address of an optional tensor"""
    return None if t is None else t.data_ptr()


def _workspace(wsb, dev):
    """`wsb` bytes of device scratch as fp64 words (never an empty tensor: its address is handed over even when the entry asks for nothing)"""
    return torch.empty(max(wsb // 8, 1), dtype=torch.float64, device=dev)


def _pinned(n):
    """n fp64 words of page-locked host memory"""
    return torch.empty(n, dtype=torch.float64).pin_memory()


def _dense(x, *others):
    """One tensor in, one tensor of the same batch out: -> (the caller's device, the launch device, x as contiguous fp64 there).
    `others`: further tensor arguments that may decide the launch device."""
    dev = _device_for(x, *others)
    return x.device, dev, _prep(x, dev).contiguous()


def _check_two_sets(x1, x2, suffix=""):
    sh1, sh2 = x1.shape, x2.shape
    if sh1[:-2] != sh2[:-2] or sh1[-1] != sh2[-1]:
        raise RuntimeError(f"batch/feature shapes differ: {tuple(sh1)} vs {tuple(sh2)}{suffix}")


_NO_BROADCASTING = " (no broadcasting, as in the reference)"


def _two_sets(x1, x2, others=(), one_set=False):
    """The prologue of every launch on two point sets x1 (..., N1, f), x2 (..., N2, f) of one batch shape:
    -> (launch device, x1 flattened, x2 flattened, nb, N1, N2, batch stride of x1, of x2, batch shape), the sets as _flatten_batch lays them
    out (an expand()ed set once, stride 0).  `others`: further tensor arguments that may decide the device.
    one_set: x2 is x1 and the entry promises the same address for both."""
    dev = _device_for(x1, x2, *others)
    a2, nb, s1 = _flatten_batch(_prep(x1, dev), 2)
    b2, _, s2 = (a2, nb, s1) if one_set else _flatten_batch(_prep(x2, dev), 2)
    sh1 = x1.shape
    return dev, a2, b2, nb, sh1[-2], x2.shape[-2], s1, s2, sh1[:-2]


def _gram_sets(x1, x2, suffix="", one_set=False, diag=False):
    """_two_sets behind the shape check, with the fp64 output (..., N1, N2) - diag: (..., N, 1) - in place of the batch shape"""
    _check_two_sets(x1, x2, suffix)
    dev, a2, b2, nb, n1, n2, s1, s2, bshape = _two_sets(x1, x2, (), one_set)
    if diag and n1 != n2:
        raise RuntimeError("diag=True needs x1 and x2 of the same length")
    return dev, a2, b2, nb, n1, n2, s1, s2, torch.empty(bshape + ((n1, 1) if diag else (n1, n2)), dtype=torch.float64, device=dev)


def _wrt_roles(wrt, a2, b2, n1, n2, s1, s2, go_si, go_sj):
    """A gradient with respect to x2 is the one with respect to x1 of the launch with the two sets exchanged and grad_out read transposed:
    -> (first set, second set, their sizes, their batch strides, row and column stride of grad_out, sign).  The sign goes with the epsilon the
    flat metrics add to x1 - x2 (frobenius_pairwise); the affine-invariant distance is symmetric and ignores it."""
    if wrt == 1:
        return a2, b2, n1, n2, s1, s2, go_si, go_sj, 1.0
    return b2, a2, n2, n1, s2, s1, go_sj, go_si, -1.0


def _sum_shared_first_set(gx, nb, sf):
    """The flat gradients with the first set handed over as ONE expand()ed set (batch stride 0): the launch wrote one slice per batch entry;
    the caller gets their sum, expanded like the input."""
    if sf == 0 and nb > 1:
        return gx.reshape((nb,) + gx.shape[-2:]).sum(0).expand(gx.shape)
    return gx


def _require(dev, **tensors):
    """The pointer-taking wrappers below hand raw device addresses to the library: anything that is not a contiguous tensor on
    `dev` of the dtype the C ABI reads there would be reinterpreted silently.  fp64 unless the name says otherwise."""
    dev = torch.device(dev)
    for name, t in tensors.items():
        if t is None:
            continue
        want = (torch.uint8, torch.bool) if name in ("active", "invalid") else ((torch.int64,) if name == "iters" else (torch.float64,))
        on_dev = torch.is_tensor(t) and t.device.type == dev.type and (dev.index is None or t.device.index == dev.index)
        if not on_dev or t.dtype not in want or not t.is_contiguous():
            raise TypeError(f"{name}: expected a contiguous {want[0]} tensor on {dev}, got "
                            f"{getattr(t, 'dtype', type(t))} on {getattr(t, 'device', None)}"
                            f"{'' if not torch.is_tensor(t) or t.is_contiguous() else ' (not contiguous)'}")


def _out(t, out_device):
    """The result on the caller's device.  A caller that handed CPU tensors gets a CPU tensor back - a device -> host copy that waits for the
    stream anyway: the natural point to look at the status words of the launches behind it (deferred error checking: one more small copy)."""
    if t.device == out_device:
        return t
    r = t.to(out_device)
    if _status.error_checking() == "deferred" and out_device.type == "cpu":
        _status.check_deferred()
    return r


def _mandel_dim(dv):
    d = int((-1.0 + (1.0 + 8.0 * dv) ** 0.5) / 2.0)
    if d * (d + 1) // 2 != dv:
        raise RuntimeError(f"last dimension {dv} is not d(d+1)/2")
    return d


# The one scalar parameter of a kernel (beta, lengthscale): a Python number or a one-element tensor at the entry, an fp64 tensor for the
# autograd Function (a tensor keeps its shape), whose gradient goes back in the shape and on the device the parameter came in.
def _scalar_param(value, refusal):
    if torch.is_tensor(value):
        if value.numel() != 1:
            raise RuntimeError(refusal)
        return value.double()
    return torch.tensor(float(value), dtype=torch.float64)


def _note_param(ctx, param):
    ctx.param_like = (param.shape, param.device) if torch.is_tensor(param) else (None, None)


def _param_grad(ctx, grad):
    shape, device = ctx.param_like
    return grad.reshape(shape).to(device)


_ONE_SPD_LENGTHSCALE = "gabotorch_amd SPD kernels take a single lengthscale (batch_shape == ())"


def spd_ai_pairwise(x1, x2, beta=1.0, mode=_lib.GABO_OUT_GAUSSIAN, symmetric=False, return_dist=False):
    """x1 (..., N1, d_vec), x2 (..., N2, d_vec) Mandel vectors -> (..., N1, N2) on x1's device.
    return_dist=True also returns the distance matrix written by the same launch."""
    lib = _lib.load()
    out_device = x1.device
    dev, a2, b2, nb, n1, n2, s1, s2, out = _gram_sets(x1, x2, _NO_BROADCASTING)
    d = _mandel_dim(a2.shape[-1])
    dist = torch.empty_like(out) if return_dist else None
    if out.numel() == 0:
        return (out.to(out_device), dist.to(out_device)) if return_dist else out.to(out_device)
    wsb = lib.gabo_spd_ai_workspace_bytes(nb, n1, n2, d)
    ws = _workspace(wsb, dev)
    status = _status_word(dev)
    flags = int(mode) | (_lib.GABO_SYMMETRIC if symmetric else 0)
    with _on(dev):
        rc = lib.gabo_spd_ai_pairwise(a2.data_ptr(), b2.data_ptr(), out.data_ptr(), _ptr(dist), nb, n1, n2, d, s1, s2, float(beta), flags,
                                      ws.data_ptr(), wsb, status.data_ptr(), _stream_ptr(dev))
    _check_launch(rc, status, "gabo_spd_ai_pairwise")
    if return_dist:
        return _out(out, out_device), dist.to(out_device)
    return _out(out, out_device)


def spd_ai_backward(x1, x2, grad_out, beta=1.0, mode=_lib.GABO_OUT_GAUSSIAN, wrt=1):
    """Gradient of sum(grad_out * spd_ai_pairwise(x1, x2)) with respect to x1 (wrt=1) or x2 (wrt=2), Mandel layout.
    grad_out (..., N1, N2).  Returns a tensor shaped like the differentiated argument."""
    lib = _lib.load()
    out_device = (x1 if wrt == 1 else x2).device
    dev, a2, b2, nb, n1, n2, s1, s2, bshape = _two_sets(x1, x2, (grad_out,))
    g = _prep(grad_out, dev).contiguous()
    d = _mandel_dim(a2.shape[-1])
    first, second, m1, m2, sf, ss, go_si, go_sj, _ = _wrt_roles(wrt, a2, b2, n1, n2, s1, s2, n2, 1)
    gx = torch.zeros(bshape + (m1, a2.shape[-1]), dtype=torch.float64, device=dev)
    if gx.numel() == 0 or m2 == 0:
        return _out(gx, out_device)
    wsb = lib.gabo_spd_ai_workspace_bytes(nb, m1, m2, d)
    ws = _workspace(wsb, dev)
    status = _status_word(dev)
    with _on(dev):
        rc = lib.gabo_spd_ai_backward(first.data_ptr(), second.data_ptr(), g.data_ptr(), gx.data_ptr(), nb, m1, m2, d, sf, ss,
                                      n1 * n2, go_si, go_sj, float(beta), int(mode), ws.data_ptr(), wsb, status.data_ptr(),
                                      _stream_ptr(dev))
    _lib.check(rc, "gabo_spd_ai_backward")
    _raise_if_not_spd(status, "gabo_spd_ai_backward")
    # (a set handed over as ONE expand()ed set, batch stride 0: the result is still the gradient with respect to the expanded tensor, one slice
    # per batch entry - autograd's ExpandBackward sums them for the base tensor; summing here as well would count the batch twice)
    return _out(gx, out_device)


def spd_ai_backward2(x1, x2, grad_out, u, beta=1.0, mode=_lib.GABO_OUT_GAUSSIAN, want_dgrad_out=True, want_mixed=False):
    """Second-order terms of the kernel (gabo_spd_ai_backward2): with grad_out fixed and u a direction shaped like x1, returns (hv, dg, mixed):
    hv = d/dt spd_ai_backward(x1 + t u, x2, grad_out)|_0 (shaped like x1), dg[..., i, j] = <u_i, dK_ij/dx1_i> (or None) and
    mixed = d <spd_ai_backward(x1, x2, grad_out), u> / d x2 (shaped like x2, or None)."""
    lib = _lib.load()
    out_device = x1.device
    dev, a2, b2, nb, n1, n2, s1, s2, bshape = _two_sets(x1, x2, (grad_out, u))
    g, uu = _prep(grad_out, dev).contiguous(), _prep(u, dev).contiguous()
    if uu.shape != x1.shape:
        raise RuntimeError(f"direction {tuple(uu.shape)} is not shaped like x1 {tuple(x1.shape)}")
    dv = a2.shape[-1]
    d = _mandel_dim(dv)
    if s1 == 0 and nb > 1:                       # an expand()ed x1 with per-batch directions: give every batch its own copy
        a2, s1 = a2.expand(nb, n1, dv).contiguous(), n1 * dv
    hv = torch.zeros(bshape + (n1, dv), dtype=torch.float64, device=dev)
    dg = torch.zeros(bshape + (n1, n2), dtype=torch.float64, device=dev) if want_dgrad_out else None
    mx = torch.zeros(bshape + (n2, dv), dtype=torch.float64, device=dev) if want_mixed else None
    if hv.numel() == 0 or n2 == 0:
        return _out(hv, out_device), (None if dg is None else dg.to(out_device)), (None if mx is None else mx.to(x2.device))
    wsb = lib.gabo_spd_ai_backward2_workspace_bytes(nb, n1, n2, d)
    ws = _workspace(wsb, dev)
    status = _status_word(dev)
    with _on(dev):
        rc = lib.gabo_spd_ai_backward2(a2.data_ptr(), b2.data_ptr(), g.data_ptr(), uu.data_ptr(), hv.data_ptr(), _ptr(dg), _ptr(mx), nb, n1, n2, d,
                                       s1, s2, n1 * n2, n2, 1, float(beta), int(mode), ws.data_ptr(), wsb, status.data_ptr(), _stream_ptr(dev))
    _lib.check(rc, "gabo_spd_ai_backward2")
    _raise_if_not_spd(status, "gabo_spd_ai_backward2")
    # (x2 as one expand()ed set: mx stays per batch entry, like spd_ai_backward's result - ExpandBackward does the sum)
    return _out(hv, out_device), (None if dg is None else dg.to(out_device)), (None if mx is None else mx.to(x2.device))


class _SpdAiGradFunction(torch.autograd.Function):
    """The first-order gradient of sum(grad_out * K(x1, x2)) with respect to x1 (wrt = 1) or x2 (wrt = 2) as a differentiable function of
    (x1, x2, grad_out, beta): the node a second autograd pass runs through (create_graph=True; pymanopt_addons/tools/autodiff/_pytorch.py:103-116
    builds exact Hessian-vector products that way).  Its own backward is gabo_spd_ai_backward2: the diagonal block of the Hessian, the mixed
    block and the directional derivative of K for grad_out; for wrt = 2 the same call with the two sets exchanged (d(A, B) = d(B, A)).
    The mixed derivative with beta comes from the same launch: dK/dx = -beta K d(d^2)/dx (Gaussian), so d/dbeta (dK/dx) = (1/beta - d^2) dK/dx and
    d <g, u> / dbeta = sum_ij grad_out_ij (1/beta - d_ij^2) <u_i, dK_ij/dx_i>  (Laplace: d instead of d^2; distance output: 0)."""

    @staticmethod
    def forward(ctx, x1, x2, grad_out, beta, mode, wrt):
        bval = float(beta)
        ctx.save_for_backward(x1, x2, grad_out)
        ctx.bval, ctx.mode, ctx.wrt = bval, mode, wrt
        _note_param(ctx, beta)
        return spd_ai_backward(x1, x2, grad_out, bval, mode, wrt=wrt).to((x1 if wrt == 1 else x2).dtype)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, u):
        x1, x2, grad_out = ctx.saved_tensors
        need1, need2, needg, needb = ctx.needs_input_grad[:4]
        needb = needb and ctx.mode != _lib.GABO_OUT_DISTANCE
        if ctx.wrt == 1:
            hv, dg, mx = spd_ai_backward2(x1, x2, grad_out, u, ctx.bval, ctx.mode, want_dgrad_out=needg or needb, want_mixed=need2)
            d1, d2 = hv, mx
        else:
            hv, dg, mx = spd_ai_backward2(x2, x1, grad_out.transpose(-1, -2), u, ctx.bval, ctx.mode, want_dgrad_out=needg or needb, want_mixed=need1)
            d1, d2 = mx, hv
            dg = None if dg is None else dg.transpose(-1, -2)
        gb = None
        if ctx.needs_input_grad[3]:
            if needb:
                dist = spd_ai_pairwise(x1, x2, 1.0, _lib.GABO_OUT_DISTANCE).to(dg.device)
                w = dist * dist if ctx.mode == _lib.GABO_OUT_GAUSSIAN else dist
                gb = (grad_out.to(dg.device) * dg * (1.0 / ctx.bval - w)).sum()
            else:
                gb = torch.zeros((), dtype=torch.float64, device=grad_out.device)
            gb = _param_grad(ctx, gb)
        return (d1.to(x1.dtype) if need1 else None), (d2.to(x2.dtype) if need2 else None), (dg.to(grad_out.dtype) if needg else None), gb, None, None


class _SpdAiKernelFunction(torch.autograd.Function):
    """K(x1, x2; beta) with the HIP forward and the HIP closed-form backward.  The gradient with respect to x1 is itself differentiable
    and so is the one with respect to x2 (in x1, x2 and the upstream gradient: _SpdAiGradFunction), which is what exact Hessian-vector
    products of a cost built on the kernel need (approx_hessian=False; the reference's SPD examples run with approx_hessian=True,
    manifold_optimize.py:198-202); so is the gradient with respect to beta (second order in x1, x2, beta and the upstream gradient)."""

    @staticmethod
    def forward(ctx, x1, x2, beta, mode):
        bval = float(beta)
        need = x1.requires_grad or x2.requires_grad or (torch.is_tensor(beta) and beta.requires_grad)
        if need:
            out, dist = spd_ai_pairwise(x1, x2, bval, mode, return_dist=True)
            ctx.save_for_backward(x1, x2, out, dist, beta)
        else:
            same = x1.data_ptr() == x2.data_ptr() and x1.shape == x2.shape and x1.stride() == x2.stride() and x1.dim() == 2
            out = spd_ai_pairwise(x1, x2, bval, mode, symmetric=same)
        ctx.bval, ctx.mode = bval, mode
        _note_param(ctx, beta)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        x1, x2, out, dist, beta = ctx.saved_tensors
        g1 = g2 = gb = None
        second = torch.is_grad_enabled()              # create_graph=True: this pass is being recorded
        second = second and (x1.requires_grad or x2.requires_grad or grad_out.requires_grad or beta.requires_grad)
        if ctx.needs_input_grad[0]:
            if second:
                g1 = _SpdAiGradFunction.apply(x1, x2, grad_out, beta, ctx.mode, 1)
            else:
                g1 = spd_ai_backward(x1, x2, grad_out, ctx.bval, ctx.mode, wrt=1).to(x1.dtype)
        if ctx.needs_input_grad[1]:
            if second:
                g2 = _SpdAiGradFunction.apply(x1, x2, grad_out, beta, ctx.mode, 2)
            else:
                g2 = spd_ai_backward(x1, x2, grad_out, ctx.bval, ctx.mode, wrt=2).to(x2.dtype)
        if ctx.needs_input_grad[2]:
            if ctx.mode == _lib.GABO_OUT_DISTANCE:
                gb = torch.zeros((), dtype=grad_out.dtype, device=grad_out.device)
            elif second:
                # A recorded pass: dK/dbeta = -d^2 K (Gaussian) / -d K (Laplace) must itself be a function of (x1, x2, beta, grad_out), so it
                # is rebuilt from two differentiable evaluations (kernel value and distance) instead of the saved, constant matrices - the
                # marginal likelihood's Hessian in beta and the x-beta blocks then come out complete (third derivatives are not provided:
                # the nodes created here are first / second order like every other one).
                kk = _SpdAiKernelFunction.apply(x1, x2, beta, ctx.mode)
                dd = _SpdAiKernelFunction.apply(x1, x2, beta, _lib.GABO_OUT_DISTANCE)
                gb = -(grad_out * kk * (dd * dd if ctx.mode == _lib.GABO_OUT_GAUSSIAN else dd)).sum()
            else:
                go = grad_out.detach()
                if ctx.mode == _lib.GABO_OUT_GAUSSIAN:
                    gb = -(go * out * dist * dist).sum()      # dK/dbeta = -d^2 K
                else:
                    gb = -(go * out * dist).sum()             # dK/dbeta = -d K
            gb = _param_grad(ctx, gb)
        return g1, g2, gb, None


def spd_ai_kernel(x1, x2, beta, mode=_lib.GABO_OUT_GAUSSIAN):
    """Differentiable entry point used by the kernel classes.  beta: python float or a one-element tensor."""
    beta = _scalar_param(beta, "gabotorch_amd SPD kernels take a single beta (batch_shape == ()), as every reference example does")
    return _SpdAiKernelFunction.apply(x1, x2, beta, int(mode))


def sphere_pairwise(x1, x2, beta=1.0, mode=_lib.GABO_OUT_GAUSSIAN, diag=False, symmetric=False):
    """x1 (..., N1, dim), x2 (..., N2, dim) -> (..., N1, N2)   [diag: (..., N, 1)]."""
    lib = _lib.load()
    out_device = x1.device
    dev, a2, b2, nb, n1, n2, s1, s2, out = _gram_sets(x1, x2, diag=diag)
    dim = a2.shape[-1]
    if out.numel() == 0:
        return _out(out, out_device)
    flags = int(mode) | (_lib.GABO_SYMMETRIC if symmetric and not diag else 0)
    with _on(dev):
        stream = _stream_ptr(dev)
        ktable = None
        # (not while a hipGraph is being captured: a build recorded into the graph would not have run for eager launches that find it cached)
        if lib.gabo_sphere_pairwise_uses_ktable(nb, n1, n2, dim, float(beta), flags, 1 if diag else 0) and not torch.cuda.is_current_stream_capturing():
            ktable = _sphere_ktable(lib, dev, stream, float(beta))
        rc = lib.gabo_sphere_pairwise_cached(a2.data_ptr(), b2.data_ptr(), out.data_ptr(), nb, n1, n2, dim, s1, s2, float(beta), flags,
                                             1 if diag else 0, _ptr(ktable), stream)
    _lib.check(rc, "gabo_sphere_pairwise")
    return _out(out, out_device)


_sphere_ktables = {}


def _sphere_ktable(lib, dev, stream, beta):
    """The kernel-value table of the large sphere Gram launches for this beta, built once per (device, stream, beta) by gabo_sphere_ktable_build
    and handed to gabo_sphere_pairwise_cached: a BO iteration evaluates every kernel matrix with the one fitted beta, so the 3-us table build
    leaves the prologue of each launch.  Keyed by the stream the build was enqueued on (stream order makes it visible to the launches behind it)."""
    key = (dev.type, dev.index, stream if isinstance(stream, int) else getattr(stream, "value", stream))
    ent = _sphere_ktables.get(key)
    if ent is None or ent[0] != beta:
        table = ent[1] if ent is not None else torch.empty(int(lib.gabo_sphere_ktable_doubles()), dtype=torch.float64, device=dev)
        if len(_sphere_ktables) > 16 and ent is None:
            _sphere_ktables.clear()
        _lib.check(lib.gabo_sphere_ktable_build(beta, table.data_ptr(), stream), "gabo_sphere_ktable_build")
        _sphere_ktables[key] = (beta, table)
        return table
    return ent[1]


def sphere_from_inner(inner, beta, mode, order):
    """Element-wise f^(order)(c) on an inner-product tensor (any shape)."""
    lib = _lib.load()
    out_device, dev, c = _dense(inner)
    out = torch.empty_like(c)
    with _on(dev):
        _lib.check(lib.gabo_sphere_from_inner(c.data_ptr(), out.data_ptr(), c.numel(), float(beta), int(mode), int(order),
                                              _stream_ptr(dev)), "gabo_sphere_from_inner")
    return _out(out, out_device)


class _SphereFromInner(torch.autograd.Function):
    """f^(order)(c), differentiable in c up to order 2 (value -> gradient -> Hessian-vector product) and, at order 0, in beta."""

    @staticmethod
    def forward(ctx, c, beta, mode, order):
        bval = float(beta)
        out = sphere_from_inner(c, bval, mode, order)
        ctx.save_for_backward(c, out)
        ctx.bval, ctx.mode, ctx.order = bval, mode, order
        _note_param(ctx, beta)
        return out

    @staticmethod
    def backward(ctx, g):
        c, out = ctx.saved_tensors
        gc = gb = None
        if ctx.needs_input_grad[0]:
            if ctx.order >= 2:
                raise RuntimeError("gabotorch_amd sphere kernels are differentiable twice in x, not three times")
            gc = g * _SphereFromInner.apply(c, torch.tensor(ctx.bval, dtype=torch.float64), ctx.mode, ctx.order + 1)
        if ctx.needs_input_grad[1]:
            if ctx.order != 0:
                raise RuntimeError("mixed x/beta second derivatives of the sphere kernels are not provided")
            with torch.no_grad():
                th = sphere_from_inner(c, 1.0, _lib.GABO_OUT_DISTANCE, 0)
                if ctx.mode == _lib.GABO_OUT_GAUSSIAN:
                    gb = -(g * out * th * th).sum()
                elif ctx.mode == _lib.GABO_OUT_LAPLACE:
                    gb = -(g * out * th).sum()
                else:
                    gb = torch.zeros((), dtype=g.dtype, device=g.device)
                gb = _param_grad(ctx, gb)
        return gc, gb, None, None


def sphere_kernel(x1, x2, beta, mode=_lib.GABO_OUT_GAUSSIAN, diag=False):
    """Differentiable entry point of the sphere kernels.  Without autograd: one fused pairwise launch.  With autograd: the
    inner products are a plain batched GEMM (torch.matmul -> rocBLAS) followed by the element-wise HIP kernel, which keeps the
    expression differentiable twice in x1/x2."""
    beta = _scalar_param(beta, "gabotorch_amd sphere kernels take a single beta (batch_shape == ())")
    need = torch.is_grad_enabled() and (x1.requires_grad or x2.requires_grad or beta.requires_grad)
    if not need:
        # (no automatic GABO_SYMMETRIC here: the sphere launch is so short that the mirror pass costs more than it saves)
        return sphere_pairwise(x1, x2, float(beta), mode, diag=diag)
    dev = _device_for(x1, x2)
    a, b = x1.double().to(dev), x2.double().to(dev)
    if diag:
        c = (a * b).sum(-1, keepdim=True)
    else:
        c = a @ b.transpose(-1, -2)
    return _SphereFromInner.apply(c, beta, int(mode), 0).to(x1.device)


# ---- Riemannian Matern / heat kernels on the sphere: zonal series with non-negative coefficients (csrc/sphere_zonal.hip) ----------
SPHERE_ZONAL_MAX_LEVELS = 128


def _zonal_derivative(coeff, series_dim):
    """d/dc of sum_k coeff[k] P_k^(d): coefficients coeff[k] k (k + d - 1) / d, k >= 1, of the series in dimension d + 2"""
    import numpy as np
    k = np.arange(1, len(coeff), dtype=np.float64)
    out = coeff[1:] * (k * (k + (series_dim - 1.0))) / float(series_dim)
    return (out if len(out) else np.zeros(1)), series_dim + 2


def sphere_matern_coefficients(dim, lengthscale, nu, num_levels, order=0, wrt_lengthscale=False):
    """Coefficients of the Riemannian Matern kernel (nu = math.inf: the heat kernel) on the unit sphere of R^dim (Borovitskiy et al. 2020),
    truncated at `num_levels`, as a zonal series  k(x, y) = sum_n p_n P_n(<x, y>):  with d = dim - 1, lambda_n = n (n + d - 1), m_n the number of
    spherical harmonics of level n,  p_n = Phi(lambda_n) m_n / sum_k Phi(lambda_k) m_k,
        Phi = (2 nu / kappa^2 + lambda)^(-nu - d/2)   or   exp(-kappa^2 lambda / 2),   kappa = lengthscale.
    p_n >= 0 and sum p_n = 1: positive definite for every kappa, k(x, x) = 1.  A lengthscale well below 1 / num_levels is not resolved.
    order = 1, 2: the series of the first / second derivative in c = <x, y>; wrt_lengthscale: of the derivative in kappa (order 0: they sum to 0).
    -> (numpy float64 coefficients, series_dim) for sphere_zonal_from_inner / sphere_zonal_pairwise.  Host arithmetic only: the weights are
    formed in log space (m_n from exact integers) relative to the largest one, so nothing overflows at dim 64 or 128 levels."""
    import numpy as np
    order = int(order)
    if order not in (0, 1, 2):
        raise ValueError(f"sphere_matern_coefficients: order = {order} outside 0, 1, 2")
    p, rate, series_dim = _sphere_matern_weights(*_sphere_matern_arguments(dim, lengthscale, nu, num_levels))
    if wrt_lengthscale:
        p = p * (rate - (p * rate).sum())
    for _ in range(order):
        p, series_dim = _zonal_derivative(p, series_dim)
    return np.ascontiguousarray(p, dtype=np.float64), series_dim


def sphere_matern_coefficients_and_derivative(dim, lengthscale, nu, num_levels):
    """(p, dp / dkappa, series_dim): sphere_matern_coefficients(...) and its wrt_lengthscale=True form, bit for bit, from one pass over the
    weights - what one evaluation of gp_mll_series takes."""
    import numpy as np
    p, rate, series_dim = _sphere_matern_weights(*_sphere_matern_arguments(dim, lengthscale, nu, num_levels))
    return np.ascontiguousarray(p, dtype=np.float64), np.ascontiguousarray(p * (rate - (p * rate).sum()), dtype=np.float64), series_dim


def _sphere_matern_arguments(dim, lengthscale, nu, num_levels):
    dim, L = int(dim), int(num_levels)
    kappa, nu = float(lengthscale), float(nu)
    if dim < 2:
        raise ValueError(f"sphere_matern_coefficients: dim = {dim}; the sphere S^(dim-1) needs dim >= 2")
    if not 1 <= L <= SPHERE_ZONAL_MAX_LEVELS:
        raise ValueError(f"sphere_matern_coefficients: num_levels = {num_levels} outside 1 ... {SPHERE_ZONAL_MAX_LEVELS}")
    if not nu > 0.0:
        raise ValueError(f"sphere_matern_coefficients: nu = {nu} must be positive (math.inf: the heat kernel)")
    if not (kappa > 0.0 and math.isfinite(kappa)):
        raise ValueError(f"sphere_matern_coefficients: lengthscale = {kappa} must be positive and finite")
    return dim, kappa, nu, L


_sphere_level_logm = {}


def _sphere_matern_weights(dim, kappa, nu, L):
    """(p_n, Phi'(lambda_n) / Phi(lambda_n) in kappa, d) of sphere_matern_coefficients for validated arguments.  The log multiplicities
    log m_n - exact integers, a Python loop - do not depend on kappa: kept per (dim, num_levels)."""
    import numpy as np
    d = dim - 1
    n = np.arange(L + 1, dtype=np.float64)
    lam = n * (n + (d - 1.0))
    logm = _sphere_level_logm.get((dim, L))
    if logm is None:
        if len(_sphere_level_logm) > 64:
            _sphere_level_logm.clear()
        logm = np.array([0.0] + [math.log(math.comb(k + d, d) - math.comb(k + d - 2, d)) for k in range(1, L + 1)])
        logm.setflags(write=False)
        _sphere_level_logm[(dim, L)] = logm
    if math.isinf(nu):
        logphi = -(kappa * kappa) * lam / 2.0
        rate = -kappa * lam                                            # Phi' / Phi
    else:
        base = 2.0 * nu / (kappa * kappa) + lam
        logphi = -(nu + d / 2.0) * np.log(base)
        rate = (nu + d / 2.0) * (4.0 * nu / kappa ** 3) / base
    logw = logphi + logm
    w = np.exp(logw - logw.max())
    return w / w.sum(), rate, d


def sphere_zonal_table(coeff, series_dim):
    """The series f = sum_k coeff[k] P_k^(series_dim) with its first and second derivative in c as the table gabo_sphere_acq_params.series points
    to: numpy (3, len(coeff), 2) of (coefficient, B_k) pairs, order o in series dimension series_dim + 2 o (B_k = (k - 1) / (k + d - 2), B_0 = B_1 = 0),
    the shorter derivative series zero-padded.  The derivative coefficients are those of sphere_matern_coefficients(order=1, 2)."""
    import numpy as np
    p = np.ascontiguousarray(coeff, dtype=np.float64).reshape(-1)
    L, sd = int(p.size), int(series_dim)
    if not 1 <= L <= SPHERE_ZONAL_MAX_LEVELS + 1:
        raise ValueError(f"sphere_zonal_table: {L} levels outside 1 ... {SPHERE_ZONAL_MAX_LEVELS + 1}")
    if sd < 1:
        raise ValueError(f"sphere_zonal_table: series dimension {series_dim} must be at least 1")
    table = np.zeros((3, L, 2))
    k = np.arange(2, L, dtype=np.float64)
    for order in range(3):
        table[order, :min(p.size, L), 0] = p[:L]
        table[order, 2:, 1] = (k - 1.0) / (k + float(sd) - 2.0)       # (one IEEE division each, as zonal_series of csrc/sphere_zonal.hip)
        p, sd = _zonal_derivative(p, sd)
    return table


def _zonal_coeff(coeff):
    import numpy as np
    a = np.ascontiguousarray(coeff, dtype=np.float64).reshape(-1)
    return a, a.ctypes.data, int(a.size)


def sphere_zonal_from_inner(inner, coeff, series_dim):
    """Element-wise sum_k coeff[k] P_k(c) on an inner-product tensor (any shape); coeff: host float64 (see sphere_matern_coefficients)."""
    lib = _lib.load()
    out_device, dev, c = _dense(inner)
    out = torch.empty_like(c)
    a, ptr, na = _zonal_coeff(coeff)
    with _on(dev):
        _lib.check(lib.gabo_sphere_zonal_from_inner(c.data_ptr(), out.data_ptr(), c.numel(), ptr, na, int(series_dim), _stream_ptr(dev)),
                   "gabo_sphere_zonal_from_inner")
    return _out(out, out_device)


def sphere_zonal_pairwise(x1, x2, coeff, series_dim, diag=False, symmetric=False):
    """x1 (..., N1, dim), x2 (..., N2, dim) -> (..., N1, N2)   [diag: (..., N, 1)]:  sum_k coeff[k] P_k(<x1_i, x2_j>) in one launch."""
    lib = _lib.load()
    out_device = x1.device
    dev, a2, b2, nb, n1, n2, s1, s2, out = _gram_sets(x1, x2, diag=diag)
    dim = a2.shape[-1]
    ca, ptr, na = _zonal_coeff(coeff)
    if out.numel() == 0:
        return _out(out, out_device)
    flags = _lib.GABO_SYMMETRIC if symmetric and not diag else 0
    with _on(dev):
        rc = lib.gabo_sphere_zonal_pairwise(a2.data_ptr(), b2.data_ptr(), out.data_ptr(), nb, n1, n2, dim, s1, s2, ptr, na, int(series_dim),
                                            flags, 1 if diag else 0, _stream_ptr(dev))
    _lib.check(rc, "gabo_sphere_zonal_pairwise")
    return _out(out, out_device)


class _SphereMaternFromInner(torch.autograd.Function):
    """f^(order)(c) of the Riemannian Matern series, differentiable in c up to order 2 (value -> gradient -> Hessian-vector product) and, at
    order 0, in the lengthscale."""

    @staticmethod
    def forward(ctx, c, lengthscale, dim, nu, num_levels, order):
        lval = float(lengthscale)
        coeff, sd = sphere_matern_coefficients(dim, lval, nu, num_levels, order)
        out = sphere_zonal_from_inner(c, coeff, sd)
        ctx.save_for_backward(c)
        ctx.lval, ctx.spec, ctx.order = lval, (dim, nu, num_levels), order
        _note_param(ctx, lengthscale)
        return out

    @staticmethod
    def backward(ctx, g):
        c, = ctx.saved_tensors
        dim, nu, num_levels = ctx.spec
        gc = gl = None
        if ctx.needs_input_grad[0]:
            if ctx.order >= 2:
                raise RuntimeError("gabotorch_amd sphere kernels are differentiable twice in x, not three times")
            gc = g * _SphereMaternFromInner.apply(c, torch.tensor(ctx.lval, dtype=torch.float64), dim, nu, num_levels, ctx.order + 1)
        if ctx.needs_input_grad[1]:
            if ctx.order != 0:
                raise RuntimeError("mixed x/lengthscale second derivatives of the sphere kernels are not provided")
            with torch.no_grad():
                coeff, sd = sphere_matern_coefficients(dim, ctx.lval, nu, num_levels, 0, wrt_lengthscale=True)
                gl = _param_grad(ctx, (g * sphere_zonal_from_inner(c, coeff, sd)).sum())
        return gc, gl, None, None, None, None


def sphere_matern_kernel(x1, x2, lengthscale, nu, num_levels, diag=False):
    """Differentiable entry point of the Riemannian Matern kernel on the sphere (nu = math.inf: heat kernel), shaped like sphere_kernel.
    Without autograd: one fused launch (the symmetric one when x1 is x2).  With autograd: the inner products are a plain batched GEMM followed
    by the element-wise series, differentiable twice in x1 / x2 and once in the lengthscale."""
    lengthscale = _scalar_param(lengthscale, "gabotorch_amd sphere kernels take a single lengthscale (batch_shape == ())")
    dim = x1.shape[-1]
    need = torch.is_grad_enabled() and (x1.requires_grad or x2.requires_grad or lengthscale.requires_grad)
    if not need:
        coeff, sd = sphere_matern_coefficients(dim, float(lengthscale), nu, num_levels)
        return sphere_zonal_pairwise(x1, x2, coeff, sd, diag=diag, symmetric=x1 is x2)
    dev = _device_for(x1, x2)
    a, b = x1.double().to(dev), x2.double().to(dev)
    if diag:
        c = (a * b).sum(-1, keepdim=True)
    else:
        c = a @ b.transpose(-1, -2)
    return _SphereMaternFromInner.apply(c, lengthscale, dim, float(nu), int(num_levels), 0).to(x1.device)


def mandel_to_matrix(vec):
    """(..., d_vec) -> (..., d, d)."""
    lib = _lib.load()
    out_device, dev, v = _dense(vec)
    dv = v.shape[-1]
    d = _mandel_dim(dv)
    n = v.numel() // dv if dv else 0
    out = torch.empty(v.shape[:-1] + (d, d), dtype=torch.float64, device=dev)
    with _on(dev):
        _lib.check(lib.gabo_mandel_to_matrix(v.data_ptr(), out.data_ptr(), n, d, _stream_ptr(dev)), "gabo_mandel_to_matrix")
    return _out(out, out_device)


def matrix_to_mandel(mat):
    """(..., d, d) -> (..., d_vec), averaging the two triangles."""
    lib = _lib.load()
    out_device, dev, m = _dense(mat)
    d = m.shape[-1]
    if m.shape[-2] != d:
        raise RuntimeError("last two dimensions must be square")
    n = m.numel() // (d * d)
    out = torch.empty(m.shape[:-2] + (d * (d + 1) // 2,), dtype=torch.float64, device=dev)
    with _on(dev):
        _lib.check(lib.gabo_matrix_to_mandel(m.data_ptr(), out.data_ptr(), n, d, _stream_ptr(dev)), "gabo_matrix_to_mandel")
    return _out(out, out_device)


# ------------------------------------------------------------------------------------------ batched manifold operations
def _mats(dev, *xs):
    """Bring (…, d, d) inputs to contiguous fp64 device tensors of one common batch shape."""
    ts = [None if x is None else _prep(torch.as_tensor(x), dev) for x in xs]
    shape = None
    for t_ in ts:
        if t_ is not None:
            shape = t_.shape if shape is None else torch.broadcast_shapes(shape, t_.shape)
    return [None if t_ is None else t_.expand(shape).contiguous() for t_ in ts], shape


def spd_manifold_op(op, a, b=None, c=None, e=None, want_grad=False):
    """Batched SPD-manifold operation `op` (one of _lib.GABO_SPD_*) on (..., d, d) tensors; see include/gabo_hip.h."""
    lib = _lib.load()
    # the maximiser's own calls: contiguous fp64 tensors of one shape on one HIP device - nothing to convert, broadcast or move (the general
    # route below spends ~0.1 ms of host time on that per call, two calls in front of every 4-ms sweep's solve launch)
    if (torch.is_tensor(a) and a.is_cuda and a.dtype == torch.float64 and a.is_contiguous() and a.dim() >= 2
            and all(x is None or (torch.is_tensor(x) and x.dtype == torch.float64 and x.device == a.device and x.shape == a.shape
                                  and x.is_contiguous()) for x in (b, c, e))):
        out_device = dev = a.device
        (A, B, C, E), shape = (a, b, c, e), a.shape
    else:
        first = torch.as_tensor(a)
        out_device = first.device
        dev = _device_for(*[torch.as_tensor(x) for x in (a, b, c, e) if x is not None])
        (A, B, C, E), shape = _mats(dev, a, b, c, e)
    d = shape[-1]
    n = A.numel() // (d * d) if d else 0
    scalar = op in (_lib.GABO_SPD_INNER, _lib.GABO_SPD_NORM, _lib.GABO_SPD_DIST, _lib.GABO_SPD_EIGMAX, _lib.GABO_SPD_EIGMIN)
    out = torch.empty(shape[:-2] if scalar else shape, dtype=torch.float64, device=dev)
    matfun = op in (_lib.GABO_SPD_LOGM, _lib.GABO_SPD_EXPM, _lib.GABO_SPD_SQRTM)
    out2 = None
    if want_grad and scalar:
        out2 = torch.empty(shape, dtype=torch.float64, device=dev)               # v v^T of the extreme eigenvalue
    elif want_grad and matfun:
        out2 = torch.empty(shape[:-2] + (d * d + d,), dtype=torch.float64, device=dev)      # V and the eigenvalues, for the backward
    status = _status_word(dev)
    with _on(dev):
        rc = lib.gabo_spd_manifold_op(int(op), _ptr(A), _ptr(B), _ptr(C), _ptr(E), out.data_ptr(), _ptr(out2), n, d, status.data_ptr(),
                                      _stream_ptr(dev))
    _check_launch(rc, status, "gabo_spd_manifold_op")
    if out2 is not None:
        return _out(out, out_device), (out2 if matfun else out2.to(out_device))
    return _out(out, out_device)


class _SpdMatFun(torch.autograd.Function):
    """logm / expm / sqrtm of symmetric (SPD) matrices with the divided-difference adjoint as backward (first order)."""

    @staticmethod
    def forward(ctx, a, op):
        # the forward launch hands its eigen-decomposition (device-resident) to the backward: no second eigen-solve
        out, eig = spd_manifold_op(int(op), a, want_grad=True)
        ctx.save_for_backward(eig)
        ctx.op, ctx.shape, ctx.device, ctx.dtype = int(op), tuple(a.shape), a.device, a.dtype
        return out.to(a.dtype)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        (eig,) = ctx.saved_tensors
        lib = _lib.load()
        dev = eig.device
        d = ctx.shape[-1]
        G = _prep(g, dev).expand(eig.shape[:-1] + (d, d)).contiguous()
        out = torch.empty_like(G)
        with _on(dev):
            _lib.check(lib.gabo_spd_matfun_backward_eig(ctx.op, eig.data_ptr(), G.data_ptr(), out.data_ptr(), G.numel() // (d * d), d,
                                                        _stream_ptr(dev)), "gabo_spd_matfun_backward_eig")
        return out.reshape(ctx.shape).to(ctx.device, ctx.dtype), None


def spd_matrix_function(a, op):
    """Differentiable GABO_SPD_LOGM / GABO_SPD_EXPM / GABO_SPD_SQRTM on (..., d, d) matrices."""
    return _SpdMatFun.apply(a, int(op)) if a.requires_grad else spd_manifold_op(int(op), a)


class NestedSpdReconstruction:
    """Reconstruction cost of the nested-SPD mapping for a FIXED data set, value and gradient in one launch
    (gabo_nested_spd_reconstruction; nested_spd_optimization.py:23-92).  metric: _lib.GABO_RECON_LOG_EUCLIDEAN / _AFFINE_INVARIANT.
    Built once per optimisation: logm X_n (or chol(X_n)^-1), Y_n^1/2 and the staging buffers stay on the device."""

    def __init__(self, x_data, x_data_projected, projection_matrix, metric, sqrt_low=None):
        lib = _lib.load()
        self.metric = int(metric)
        dev = self.device = _device_for(x_data, x_data_projected, projection_matrix)
        X = _prep(x_data, dev).contiguous()
        self.y = _prep(x_data_projected, dev).contiguous()
        self.w = _prep(projection_matrix, dev).contiguous()
        self.N, self.D, self.d = int(X.shape[0]), int(X.shape[-1]), int(self.w.shape[1])
        self.m = self.D - self.d
        if X.dim() != 3 or X.shape[1] != self.D or tuple(self.y.shape) != (self.N, self.d, self.d) or self.w.shape[0] != self.D:
            raise RuntimeError(f"shapes: x_data {tuple(X.shape)}, x_data_projected {tuple(self.y.shape)}, projection_matrix {tuple(self.w.shape)}")
        self.sqrt_y = (spd_manifold_op(_lib.GABO_SPD_SQRTM, self.y) if sqrt_low is None else _prep(sqrt_low, dev)).contiguous()
        self.data = torch.empty_like(X)
        status = _status_word(dev)
        with _on(dev):
            _lib.check(lib.gabo_nested_spd_reconstruction_prepare(X.data_ptr(), self.data.data_ptr(), self.N, self.D, self.metric,
                                                                  status.data_ptr(), _stream_ptr(dev)), "gabo_nested_spd_reconstruction_prepare")
        _raise_if_not_spd(status, "gabo_nested_spd_reconstruction_prepare")
        self.sizes = (self.D * self.m, self.m * self.m, self.d * self.m)
        self._buffers = {}

    def _staging(self, P):
        ent = self._buffers.get(P)
        if ent is None:
            lib = _lib.load()
            nV, nC, nK = self.sizes
            npar = nV + nC + nK
            ws = max(int(lib.gabo_nested_spd_reconstruction_workspace_bytes(P, max(self.N, 1), self.D, self.d)), 16)
            host_in, host_out = _pinned(P * npar), _pinned(P * (1 + npar))
            dev_in = torch.empty(P * npar, dtype=torch.float64, device=self.device)
            dev_out = torch.empty(P * (1 + npar), dtype=torch.float64, device=self.device)
            o1, o2, o3 = P, P + P * nV, P + P * (nV + nC)
            ent = self._buffers[P] = dict(
                host_in=host_in, dev_in=dev_in, host_out=host_out, dev_out=dev_out, ws=torch.empty(ws, dtype=torch.uint8, device=self.device),
                # views made once: an evaluation is host-bound (one launch of ~0.14 ms), every Python-level slice on its path counts
                hin=host_in.numpy(), hout=host_out.numpy(), v=dev_in[:P * nV], c=dev_in[P * nV:P * (nV + nC)], k=dev_in[P * (nV + nC):],
                cost=dev_out[:P], gv=dev_out[o1:o2], gc=dev_out[o2:o3], gk=dev_out[o3:], ho_cost=host_out[:P], do_cost=dev_out[:P],
                stream=torch.cuda.current_stream(self.device))
        return ent

    def launch(self, v, c, k, cost, gv, gc, gk, P, ws):
        """Raw launch on contiguous fp64 device tensors (gv = gc = gk = None: values only)."""
        lib = _lib.load()
        with torch.cuda.device(self.device):
            _lib.check(lib.gabo_nested_spd_reconstruction(self.data.data_ptr(), self.y.data_ptr(), self.sqrt_y.data_ptr(), self.w.data_ptr(),
                                                          v.data_ptr(), c.data_ptr(), k.data_ptr(), cost.data_ptr(), _ptr(gv), _ptr(gc), _ptr(gk), None,
                                                          None, P, self.N, self.D, self.d, self.metric, ws.data_ptr(), ws.numel(),
                                                          _stream_ptr(self.device)),
                       "gabo_nested_spd_reconstruction")

    def evaluate_host(self, V, C, K, grad=True):
        """numpy in, numpy out: V (P, D, m) or (D, m), C, K likewise -> cost (P,) [, gV, gC, gK].  One pinned host-to-device copy, one
        launch, one copy back: what an evaluation of the augmented-Lagrangian line search costs."""
        import numpy as np
        V, C, K = (np.asarray(a, dtype=np.float64) for a in (V, C, K))
        single = V.ndim == 2
        P = 1 if single else V.shape[0]
        ent = self._staging(P)
        nV, nC, nK = self.sizes
        hin = ent["hin"]
        hin[:P * nV] = V.ravel()
        hin[P * nV:P * (nV + nC)] = C.ravel()
        hin[P * (nV + nC):] = K.ravel()
        ent["dev_in"].copy_(ent["host_in"], non_blocking=True)
        if grad:
            self.launch(ent["v"], ent["c"], ent["k"], ent["cost"], ent["gv"], ent["gc"], ent["gk"], P, ent["ws"])
            ent["host_out"].copy_(ent["dev_out"], non_blocking=True)
        else:
            self.launch(ent["v"], ent["c"], ent["k"], ent["cost"], None, None, None, P, ent["ws"])
            ent["ho_cost"].copy_(ent["do_cost"], non_blocking=True)
        torch.cuda.current_stream(self.device).synchronize()
        hout = ent["hout"]
        costs = hout[:P].copy()
        if not grad:
            return costs[0] if single else costs
        o1, o2, o3 = P, P + P * nV, P + P * (nV + nC)
        gV = hout[o1:o2].reshape(V.shape).copy()
        gC = hout[o2:o3].reshape(C.shape).copy()
        gK = hout[o3:].reshape(K.shape).copy()
        return (costs[0] if single else costs), gV, gC, gK

    def __call__(self, V, C, K):
        """Differentiable (first order) torch form: V (D, m), C (m, m), K (d, m) tensors -> 0-dim cost."""
        return _NestedSpdReconstructionFn.apply(self, V, C, K)

    def solve_host(self, V, C, unit, raw, options):
        """The augmented-Lagrangian / conjugate-gradient run from the start point (V, C, unit, raw) as ONE call of the native host loop
        (gabo_nested_spd_reconstruction_solve): numpy in, numpy out -> (V, C, unit, raw, log dict).  options: _lib.ReconSolveOptions."""
        import ctypes

        import numpy as np
        lib = _lib.load()
        ent = self._buffers.get("solve")
        if ent is None:
            dev_bytes, pin_doubles = ctypes.c_size_t(0), ctypes.c_size_t(0)
            lib.gabo_nested_spd_reconstruction_solve_workspace_bytes(self.N, self.D, self.d, ctypes.byref(dev_bytes), ctypes.byref(pin_doubles))
            ent = self._buffers["solve"] = dict(ws=torch.empty(max(dev_bytes.value, 16), dtype=torch.uint8, device=self.device),
                                                pinned=_pinned(pin_doubles.value),
                                                w_host=np.ascontiguousarray(self.w.cpu().numpy(), dtype=np.float64))
        v, c, u = (np.array(a, dtype=np.float64, order="C") for a in (V, C, unit))
        r = np.array([float(np.asarray(raw).reshape(-1)[0])], dtype=np.float64)
        if v.shape != (self.D, self.m) or c.shape != (self.m, self.m) or u.size != self.d * self.m:
            raise RuntimeError(f"start point shapes: V {v.shape}, C {c.shape}, unit {u.shape}")
        log = _lib.ReconSolveLog()
        ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)   # noqa: E731
        with torch.cuda.device(self.device):
            code = lib.gabo_nested_spd_reconstruction_solve(
                self.data.data_ptr(), self.y.data_ptr(), self.sqrt_y.data_ptr(), self.w.data_ptr(), ptr(ent["w_host"]), ptr(v), ptr(c), ptr(u),
                ptr(r), self.N, self.D, self.d, self.metric, ent["ws"].data_ptr(), ent["ws"].numel(), ent["pinned"].data_ptr(),
                ent["pinned"].numel(), ctypes.byref(options), ctypes.byref(log), _stream_ptr(self.device))
        _lib.check(code, "gabo_nested_spd_reconstruction_solve")
        return v, c, u, r, _recon_log(log)


def _recon_log(log):
    return {"iterations": int(log.outer_iterations), "inner_iterations": int(log.inner_iterations), "evaluations": int(log.evaluations),
            "launches": int(log.launches), "stop_reason": _lib.GABO_RECON_STOP[log.stop_reason], "violation": float(log.violation),
            "rho": float(log.rho), "gammas": [float(log.gamma)], "final_cost": float(log.final_cost), "time": float(log.seconds),
            "time_in_evaluator": float(log.seconds_evaluator), "host_threads": int(log.host_threads)}


def nested_spd_reconstruction_solve_with(evaluate, w_host, V, C, unit, raw, options):
    """The same native loop around a host callable  evaluate(V (P, D, m), C (P, m, m), K (P, d, m)) -> (cost (P,), gV, gC, gK)  in numpy
    (gabo_nested_spd_reconstruction_solve_with): a user-supplied cost function, or a test's.  -> (V, C, unit, raw, log dict)."""
    import ctypes

    import numpy as np
    lib = _lib.load()
    w = np.ascontiguousarray(w_host, dtype=np.float64)
    D, d = w.shape
    m = D - d
    v, c, u = (np.array(a, dtype=np.float64, order="C") for a in (V, C, unit))
    r = np.array([float(np.asarray(raw).reshape(-1)[0])], dtype=np.float64)
    npar = D * m + m * m + d * m
    staging = np.empty(_lib.GABO_RECON_MAX_LOOKAHEAD * (2 * npar + 1 + m + m * m))
    failure = []

    def trampoline(_ctx, P, pv, pc, pk, pcost, pgv, pgc, pgk):
        try:
            as_np = lambda q, *shape: np.ctypeslib.as_array(q, shape=(int(np.prod(shape)),)).reshape(shape)   # noqa: E731
            cost, gv, gc, gk = evaluate(as_np(pv, P, D, m).copy(), as_np(pc, P, m, m).copy(), as_np(pk, P, d, m).copy())
            as_np(pcost, P)[:] = np.asarray(cost, dtype=np.float64).reshape(P)
            as_np(pgv, P, D, m)[:] = gv
            as_np(pgc, P, m, m)[:] = gc
            as_np(pgk, P, d, m)[:] = gk
            return _lib.GABO_OK
        except Exception as exc:          # nothing may propagate through the C frames: the loop stops on the code, the error is raised below
            failure.append(exc)
            return _lib.GABO_ERR_ARG

    log = _lib.ReconSolveLog()
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)   # noqa: E731
    code = lib.gabo_nested_spd_reconstruction_solve_with(_lib.ReconEvalFn(trampoline), None, ptr(w), ptr(v), ptr(c), ptr(u), ptr(r), D, d,
                                                         ptr(staging), staging.size, ctypes.byref(options), ctypes.byref(log))
    if failure:
        raise failure[0]
    _lib.check(code, "gabo_nested_spd_reconstruction_solve_with")
    return v, c, u, r, _recon_log(log)


class _NestedSpdReconstructionFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, rec, V, C, K):
        dev = rec.device
        v, c, k = (_prep(t_.detach(), dev).contiguous() for t_ in (V, C, K))
        need = any(t_.requires_grad for t_ in (V, C, K))
        cost = torch.empty(1, dtype=torch.float64, device=dev)
        gv, gc, gk = (torch.empty_like(t_) for t_ in (v, c, k)) if need else (None, None, None)
        rec.launch(v, c, k, cost, gv, gc, gk, 1, rec._staging(1)["ws"])
        if need:
            ctx.save_for_backward(gv, gc, gk)
        ctx.meta = [(t_.device, t_.dtype) for t_ in (V, C, K)]
        return cost[0].to(V.device, V.dtype)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        out = [None]
        for grad, (dev, dt), need in zip(ctx.saved_tensors, ctx.meta, ctx.needs_input_grad[1:]):
            out.append((grad * g.to(grad.device)).to(dev, dt) if need else None)
        return tuple(out)


def nested_spd_lift_prepare(w, v, c, k):
    """(x0, p) of gabo_nested_spd_lift_prepare for the mapping (W, V, C, K) on w's device (detached fp64)."""
    lib = _lib.load()
    dev = _device_for(w, v, c, k)
    W, V, C, K = (_prep(t_.detach(), dev).contiguous() for t_ in (w, v, c, k))
    D, d = int(W.shape[0]), int(W.shape[1])
    if tuple(V.shape) != (D, D - d) or tuple(C.shape) != (D - d, D - d) or tuple(K.shape) != (d, D - d):
        raise RuntimeError(f"nested SPD mapping shapes: W {tuple(W.shape)}, V {tuple(V.shape)}, C {tuple(C.shape)}, K {tuple(K.shape)}")
    x0 = torch.empty(D, D, dtype=torch.float64, device=dev)
    p = torch.empty(D, d, dtype=torch.float64, device=dev)
    with _on(dev):
        _lib.check(lib.gabo_nested_spd_lift_prepare(V.data_ptr(), C.data_ptr(), K.data_ptr(), x0.data_ptr(), p.data_ptr(), D, d, _stream_ptr(dev)),
                   "gabo_nested_spd_lift_prepare")
    return W, x0, p


def nested_spd_extreme_eigenvalues(y, w, p, x0, want_grad=False):
    """y (..., d, d) latent points -> lam (..., 2) = (lambda_max, lambda_min) of the lifted points [, grad (..., 2, d, d)]."""
    lib = _lib.load()
    dev = w.device
    Y = _prep(y, dev).contiguous()
    D, d = int(w.shape[0]), int(w.shape[1])
    if Y.shape[-2:] != (d, d):
        raise RuntimeError(f"latent points must be (..., {d}, {d}), got {tuple(Y.shape)}")
    R = Y.numel() // (d * d)
    lam = torch.empty(Y.shape[:-2] + (2,), dtype=torch.float64, device=dev)
    grad = torch.empty(Y.shape[:-2] + (2, d, d), dtype=torch.float64, device=dev) if want_grad else None
    with _on(dev):
        _lib.check(lib.gabo_nested_spd_extreme_eigenvalues(Y.data_ptr(), w.data_ptr(), p.data_ptr(), x0.data_ptr(), lam.data_ptr(),
                                                           _ptr(grad), R, D, d, _stream_ptr(dev)),
                   "gabo_nested_spd_extreme_eigenvalues")
    return (lam, grad) if want_grad else lam


class _NestedSpdExtremes(torch.autograd.Function):
    """(lambda_max, lambda_min) of the lifted latent point, differentiable (first order) in the latent point."""

    @staticmethod
    def forward(ctx, y, w, p, x0):
        if not y.requires_grad:
            return nested_spd_extreme_eigenvalues(y, w, p, x0).to(y.device, y.dtype)
        lam, grad = nested_spd_extreme_eigenvalues(y, w, p, x0, want_grad=True)
        ctx.save_for_backward(grad)
        return lam.to(y.device, y.dtype)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        (grad,) = ctx.saved_tensors
        gy = (g.to(grad.device)[..., None, None] * grad).sum(-3)
        return gy.to(g.device, g.dtype), None, None, None


def nested_spd_extremes(y, w, p, x0):
    return _NestedSpdExtremes.apply(y, w, p, x0)


def spd_project(x_mandel, w):
    """(..., D_vec) Mandel, w (D, dl) -> (..., dl_vec) Mandel of W^T X W."""
    lib = _lib.load()
    out_device = x_mandel.device
    dev = _device_for(x_mandel, w)
    x = _prep(x_mandel, dev).contiguous()
    W = _prep(w, dev).contiguous()
    D = _mandel_dim(x.shape[-1])
    if W.dim() != 2 or W.shape[0] != D:
        raise RuntimeError(f"projection matrix must be ({D}, d_latent), got {tuple(W.shape)}")
    dl = W.shape[1]
    n = x.numel() // x.shape[-1]
    out = torch.empty(x.shape[:-1] + (dl * (dl + 1) // 2,), dtype=torch.float64, device=dev)
    with _on(dev):
        _lib.check(lib.gabo_spd_project(x.data_ptr(), W.data_ptr(), out.data_ptr(), n, D, dl, _stream_ptr(dev)), "gabo_spd_project")
    return _out(out, out_device)


class _SpdProject(torch.autograd.Function):
    """Mandel(W^T X W), differentiable in X (adjoint = the same kernel with W^T) and in W (2 sum_n X_n W G_n)."""

    @staticmethod
    def forward(ctx, x, w):
        ctx.save_for_backward(x, w)
        return spd_project(x, w)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        gx = gw = None
        if ctx.needs_input_grad[0]:
            gx = spd_project(g, w.t().contiguous()).to(x.dtype)
        if ctx.needs_input_grad[1]:
            dev = _device_for(x, w, g)
            X = mandel_to_matrix(_prep(x, dev)).reshape(-1, w.shape[0], w.shape[0])
            G = mandel_to_matrix(_prep(g, dev)).reshape(-1, w.shape[1], w.shape[1])
            gw = 2.0 * torch.einsum("nab,bc,ncd->ad", X, _prep(w, dev), G).to(w.device, w.dtype)
        return gx, gw


def spd_project_diff(x_mandel, w):
    """Differentiable spd_project."""
    if x_mandel.requires_grad or w.requires_grad:
        return _SpdProject.apply(x_mandel, w)
    return spd_project(x_mandel, w)


def _nested_spd_gram(entry, x1, x2, w, *scalars):
    """The two nested Gram entries: the library's `entry` on dense sets (it takes no batch strides; `x2 is x1`: the set once, the same
    address twice) and the projection matrix, `scalars` between the sizes and the workspace."""
    lib = _lib.load()
    _check_two_sets(x1, x2, _NO_BROADCASTING)
    out_device = x1.device
    dev = _device_for(x1, x2, w)
    a = _prep(x1, dev).contiguous()
    b = a if x2 is x1 else _prep(x2, dev).contiguous()
    W = _prep(w, dev).contiguous()
    D = _mandel_dim(a.shape[-1])
    if W.dim() != 2 or W.shape[0] != D:
        raise RuntimeError(f"projection matrix must be ({D}, d_latent), got {tuple(W.shape)}")
    dl = int(W.shape[1])
    n1, n2 = a.shape[-2], b.shape[-2]
    nb = math.prod(a.shape[:-2])
    out = torch.empty(a.shape[:-2] + (n1, n2), dtype=torch.float64, device=dev)
    if out.numel() == 0:
        return _out(out, out_device)
    wsb = lib.gabo_nested_spd_gram_workspace_bytes(nb, n1, n2, dl)
    ws = _workspace(wsb, dev)
    status = _status_word(dev)
    with _on(dev):
        rc = getattr(lib, entry)(a.data_ptr(), b.data_ptr(), W.data_ptr(), out.data_ptr(), nb, n1, n2, D, dl, *scalars, ws.data_ptr(), wsb,
                                 status.data_ptr(), _stream_ptr(dev))
    _check_launch(rc, status, entry)
    return _out(out, out_device)


def nested_spd_gram(x1, x2, w, beta, metric=_lib.GABO_METRIC_AFFINE_INVARIANT, mode=_lib.GABO_OUT_GAUSSIAN):
    """Gram matrix of the nested SPD kernels in two launches, no gradient (gabo_nested_spd_gram): x1 (..., N1, D_vec), x2 (..., N2, D_vec) Mandel
    vectors of the ORIGINAL space, w (D, d_latent) with 2 <= d_latent <= 4 -> (..., N1, N2).  metric: _lib.GABO_METRIC_AFFINE_INVARIANT
    (exp(-beta d_AI^2) of the projected points) or _lib.GABO_METRIC_LOG_EUCLIDEAN (exp(-beta ||logm - logm + 1e-15||_F^2))."""
    return _nested_spd_gram("gabo_nested_spd_gram", x1, x2, w, int(metric), float(beta), int(mode))


def nested_spd_matern_gram(x1, x2, w, lengthscale, nu):
    """Gram matrix of NestedSpdLogEuclideanMaternKernel in two launches, no gradient (gabo_nested_spd_matern_gram): shapes as nested_spd_gram;
    out = k_nu(||logm Y1 - logm Y2 + 1e-15||_F; lengthscale) of the projected points, nu in {0.5, 1.5, 2.5}, gpytorch's MaternKernel
    parametrisation.  With `x2 is x1` the set is projected once and the matrix is symmetric to the last bit."""
    nu2, lval = _matern_nu2(nu), _matern_lengthscale(lengthscale)
    return _nested_spd_gram("gabo_nested_spd_matern_gram", x1, x2, w, lval, nu2)


def nested_spd_gram_applicable(x1, x2, w, *params):
    """the fused two-launch Gram serves evaluations that nobody differentiates, latent dimensions 2 ... 4 and dense, equally batched inputs"""
    if torch.is_grad_enabled() and any(torch.is_tensor(t_) and t_.requires_grad for t_ in (x1, x2, w) + params):
        return False
    if w.dim() != 2 or not (2 <= w.shape[1] <= 4) or w.shape[0] > _lib.GABO_SPD_MAX_DIM or x1.dim() < 2 or x1.shape[:-2] != x2.shape[:-2]:
        return False
    D = w.shape[0]
    if x1.shape[-1] != D * (D + 1) // 2 or x2.shape[-1] != x1.shape[-1]:
        return False
    dv = w.shape[1] * (w.shape[1] + 1) // 2
    return (D * w.shape[1] + dv * x1.shape[-1]) * 8 <= 48 * 1024 and (x1.is_cuda or torch.cuda.is_available())


def spd_logm_mandel(x_mandel):
    lib = _lib.load()
    out_device, dev, x = _dense(x_mandel)
    d = _mandel_dim(x.shape[-1])
    out = torch.empty_like(x)
    with _on(dev):
        _lib.check(lib.gabo_spd_logm_mandel(x.data_ptr(), out.data_ptr(), x.numel() // x.shape[-1], d, _stream_ptr(dev)),
                   "gabo_spd_logm_mandel")
    return _out(out, out_device)


def frobenius_pairwise(x1, x2, beta=1.0, mode=_lib.GABO_OUT_GAUSSIAN):
    """Mandel vectors x1 (..., N1, d_vec), x2 (..., N2, d_vec) -> (..., N1, N2) Frobenius distance / kernel."""
    lib = _lib.load()
    out_device = x1.device
    dev, a2, b2, nb, n1, n2, s1, s2, out = _gram_sets(x1, x2)
    d = _mandel_dim(a2.shape[-1])
    with _on(dev):
        _lib.check(lib.gabo_frobenius_pairwise(a2.data_ptr(), b2.data_ptr(), out.data_ptr(), nb, n1, n2, d, s1, s2, float(beta),
                                               int(mode), _stream_ptr(dev)), "gabo_frobenius_pairwise")
    return _out(out, out_device)


def spd_logm_mandel_backward(x_mandel, grad_y):
    """Gradient w.r.t. x (Mandel) of a loss whose gradient w.r.t. spd_logm_mandel(x) is grad_y."""
    lib = _lib.load()
    out_device, dev, x = _dense(x_mandel, grad_y)
    g = _prep(grad_y, dev).expand(x.shape).contiguous()
    d = _mandel_dim(x.shape[-1])
    out = torch.empty_like(x)
    with _on(dev):
        _lib.check(lib.gabo_spd_logm_mandel_backward(x.data_ptr(), g.data_ptr(), out.data_ptr(), x.numel() // x.shape[-1], d,
                                                     _stream_ptr(dev)), "gabo_spd_logm_mandel_backward")
    return _out(out, out_device)


class _SpdLogmMandel(torch.autograd.Function):
    """Mandel(logm(X)) with the Daleckii-Krein adjoint as backward (first order)."""

    @staticmethod
    def forward(ctx, x):
        ctx.save_for_backward(x)
        return spd_logm_mandel(x)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        return spd_logm_mandel_backward(x, g).to(x.dtype)


def spd_logm_mandel_diff(x_mandel):
    """Differentiable spd_logm_mandel."""
    return _SpdLogmMandel.apply(x_mandel) if x_mandel.requires_grad else spd_logm_mandel(x_mandel)


def frobenius_backward(x1, x2, grad_out, beta=1.0, mode=_lib.GABO_OUT_GAUSSIAN, wrt=1):
    """Gradient of sum(grad_out * frobenius_pairwise(x1, x2)) with respect to x1 (wrt=1) or x2 (wrt=2)."""
    lib = _lib.load()
    out_device = (x1 if wrt == 1 else x2).device
    dev, a2, b2, nb, n1, n2, s1, s2, bshape = _two_sets(x1, x2, (grad_out,))
    g = _prep(grad_out, dev).contiguous()
    d = _mandel_dim(a2.shape[-1])
    first, second, m1, m2, sf, ss, go_si, go_sj, sgn = _wrt_roles(wrt, a2, b2, n1, n2, s1, s2, n2, 1)
    gx = torch.zeros(bshape + (m1, a2.shape[-1]), dtype=torch.float64, device=dev)
    if gx.numel() == 0 or m2 == 0:
        return _out(gx, out_device)
    with _on(dev):
        _lib.check(lib.gabo_frobenius_backward(first.data_ptr(), second.data_ptr(), g.data_ptr(), gx.data_ptr(), nb, m1, m2, d, sf,
                                               ss, n1 * n2, go_si, go_sj, float(beta), int(mode), sgn, _stream_ptr(dev)),
                   "gabo_frobenius_backward")
    return _out(_sum_shared_first_set(gx, nb, sf), out_device)


class _FrobeniusKernelFunction(torch.autograd.Function):
    """frobenius_pairwise(x1, x2; beta) with HIP forward and backward (first order), differentiable in x1, x2 and beta."""

    @staticmethod
    def forward(ctx, x1, x2, beta, mode):
        bval = float(beta)
        out = frobenius_pairwise(x1, x2, bval, mode)
        ctx.save_for_backward(x1, x2, out)
        ctx.bval, ctx.mode = bval, mode
        _note_param(ctx, beta)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        x1, x2, out = ctx.saved_tensors
        g1 = g2 = gb = None
        if ctx.needs_input_grad[0]:
            g1 = frobenius_backward(x1, x2, grad_out, ctx.bval, ctx.mode, wrt=1).to(x1.dtype)
        if ctx.needs_input_grad[1]:
            g2 = frobenius_backward(x1, x2, grad_out, ctx.bval, ctx.mode, wrt=2).to(x2.dtype)
        if ctx.needs_input_grad[2]:
            if ctx.mode == _lib.GABO_OUT_DISTANCE:
                gb = torch.zeros((), dtype=grad_out.dtype, device=grad_out.device)
            else:       # K = exp(-beta t) with t = d^2 (Gaussian) or d (Laplace): dK/dbeta = -t K
                dist = frobenius_pairwise(x1, x2, 1.0, _lib.GABO_OUT_DISTANCE).to(out.device)
                t = dist * dist if ctx.mode == _lib.GABO_OUT_GAUSSIAN else dist
                gb = -(grad_out * out * t).sum()
            gb = _param_grad(ctx, gb)
        return g1, g2, gb, None


def frobenius_kernel(x1, x2, beta, mode=_lib.GABO_OUT_GAUSSIAN):
    """Differentiable entry point used by SpdFrobeniusGaussianKernel / SpdLogEuclideanGaussianKernel."""
    return _FrobeniusKernelFunction.apply(x1, x2, _scalar_param(beta, _ONE_SPD_LENGTHSCALE), int(mode))


# ---- Matern kernels on the flat SPD metrics (csrc/flat_matern.hip): features are Mandel vectors, the distance is frobenius_pairwise's ----
def _matern_nu2(nu):
    """2 nu for nu in {0.5, 1.5, 2.5} (ValueError otherwise): the smoothness the C entries take"""
    try:
        nu2 = int(round(2.0 * float(nu)))
    except (TypeError, ValueError, OverflowError):
        nu2 = -1
    if nu2 not in (1, 3, 5) or float(nu) * 2.0 != nu2:
        raise ValueError(f"nu must be 0.5, 1.5 or 2.5, got {nu!r}")
    return nu2


def _matern_lengthscale(lengthscale):
    """the lengthscale as a positive finite Python float (ValueError otherwise), as the C entries check it"""
    if torch.is_tensor(lengthscale) and lengthscale.numel() != 1:
        raise RuntimeError(_ONE_SPD_LENGTHSCALE)
    value = float(lengthscale)
    if not (value > 0.0 and math.isfinite(value)):
        raise ValueError(f"the lengthscale must be positive and finite, got {value!r}")
    return value


def flat_matern_pairwise(x1, x2, lengthscale, nu):
    """Mandel vectors x1 (..., N1, d_vec), x2 (..., N2, d_vec) -> (..., N1, N2) Matern kernel k_nu(r; lengthscale) of the distance r of
    frobenius_pairwise, nu in {0.5, 1.5, 2.5}, in gpytorch's MaternKernel parametrisation (x = sqrt(2 nu) r / lengthscale).  With
    `x2 is x1` the matrix is symmetric to the last bit."""
    lib = _lib.load()
    nu2, lval = _matern_nu2(nu), _matern_lengthscale(lengthscale)
    out_device = x1.device
    # (one point set: the same pointer, and with it an exactly symmetric matrix)
    dev, a2, b2, nb, n1, n2, s1, s2, out = _gram_sets(x1, x2, one_set=x2 is x1)
    d = _mandel_dim(a2.shape[-1])
    with _on(dev):
        _lib.check(lib.gabo_flat_matern_pairwise(a2.data_ptr(), b2.data_ptr(), out.data_ptr(), nb, n1, n2, d, s1, s2, lval, nu2,
                                                 _stream_ptr(dev)), "gabo_flat_matern_pairwise")
    return _out(out, out_device)


def flat_matern_backward(x1, x2, grad_out, lengthscale, nu, wrt=1):
    """Gradient of sum(grad_out * flat_matern_pairwise(x1, x2)) with respect to x1 (wrt=1) or x2 (wrt=2); grad_out may be strided."""
    lib = _lib.load()
    nu2, lval = _matern_nu2(nu), _matern_lengthscale(lengthscale)
    if wrt not in (1, 2):
        raise ValueError(f"wrt must be 1 or 2, got {wrt!r}")
    out_device = (x1 if wrt == 1 else x2).device
    dev, a2, b2, nb, n1, n2, s1, s2, bshape = _two_sets(x1, x2, (grad_out,))
    g = _prep(grad_out, dev)
    d = _mandel_dim(a2.shape[-1])
    if g.dim() == 2 and tuple(g.shape) == (n1, n2) and nb == 1 and min(g.stride()) >= 0:
        go_b, go_i, go_j = 0, g.stride(0), g.stride(1)          # (a strided matrix - a transpose, a slice - is read in place)
    else:
        g = g.expand(bshape + (n1, n2)).contiguous()
        go_b, go_i, go_j = n1 * n2, n2, 1
    first, second, m1, m2, sf, ss, go_i, go_j, sgn = _wrt_roles(wrt, a2, b2, n1, n2, s1, s2, go_i, go_j)
    gx = torch.zeros(bshape + (m1, a2.shape[-1]), dtype=torch.float64, device=dev)
    if gx.numel() == 0 or m2 == 0:
        return _out(gx, out_device)
    with _on(dev):
        _lib.check(lib.gabo_flat_matern_backward(first.data_ptr(), second.data_ptr(), g.data_ptr(), gx.data_ptr(), nb, m1, m2, d, sf, ss,
                                                 go_b, go_i, go_j, lval, nu2, sgn, _stream_ptr(dev)), "gabo_flat_matern_backward")
    return _out(_sum_shared_first_set(gx, nb, sf), out_device)


def flat_matern_from_distance(r, lengthscale, nu, order=0):
    """Element-wise on a distance tensor (any shape): order 0 the Matern kernel k_nu(r; lengthscale), order 1 its derivative in the lengthscale."""
    lib = _lib.load()
    nu2, lval = _matern_nu2(nu), _matern_lengthscale(lengthscale)
    if order not in (0, 1):
        raise ValueError(f"order must be 0 or 1, got {order!r}")
    out_device, dev, c = _dense(r)
    out = torch.empty_like(c)
    with _on(dev):
        _lib.check(lib.gabo_flat_matern_from_distance(c.data_ptr(), out.data_ptr(), c.numel(), lval, nu2, int(order), _stream_ptr(dev)),
                   "gabo_flat_matern_from_distance")
    return _out(out, out_device)


class _FlatMaternKernelFunction(torch.autograd.Function):
    """flat_matern_pairwise(x1, x2; lengthscale) with HIP forward and backward (first order), differentiable in x1, x2 and the lengthscale."""

    @staticmethod
    def forward(ctx, x1, x2, lengthscale, nu, same):
        lval = _matern_lengthscale(lengthscale)
        out = flat_matern_pairwise(x1, x1 if same else x2, lval, nu)
        ctx.save_for_backward(x1, x2)
        ctx.lval, ctx.nu = lval, nu
        _note_param(ctx, lengthscale)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        x1, x2 = ctx.saved_tensors
        g1 = g2 = gl = None
        if ctx.needs_input_grad[0]:
            g1 = flat_matern_backward(x1, x2, grad_out, ctx.lval, ctx.nu, wrt=1).to(x1.dtype)
        if ctx.needs_input_grad[1]:
            g2 = flat_matern_backward(x1, x2, grad_out, ctx.lval, ctx.nu, wrt=2).to(x2.dtype)
        if ctx.needs_input_grad[2]:      # sum_ij g_ij dk_ij/dl: the distance launch, then the element-wise one
            dist = frobenius_pairwise(x1, x2, 1.0, _lib.GABO_OUT_DISTANCE).to(grad_out.device)
            gl = _param_grad(ctx, (grad_out * flat_matern_from_distance(dist, ctx.lval, ctx.nu, order=1)).sum())
        return g1, g2, gl, None, None


def flat_matern_kernel(x1, x2, lengthscale, nu):
    """Differentiable entry point used by SpdFrobeniusMaternKernel / SpdLogEuclideanMaternKernel (first order in x1, x2 and the lengthscale)."""
    _matern_nu2(nu)
    return _FlatMaternKernelFunction.apply(x1, x2, _scalar_param(lengthscale, _ONE_SPD_LENGTHSCALE), float(nu), x2 is x1)


# ---- Matern / heat kernels of the affine-invariant SPD metric by random phase features (csrc/spd_ai_spectral.hip) ----
# a(Z) = 2 log diag chol(Z);  rho_k = (d + 1 - 2k) / 4;  for feature l with spectral point lam_l, weight w_l and Haar matrix H_l:
# a_il = a(H_l^T X_i H_l),  F_i = [sqrt(w_l) exp(-rho . a_il) cos(lam_l . a_il) | ... sin ...],  k(X_i, Y_j) = <F_i, F_j> / (|F_i| |F_j|).


def _spectral_nu(nu):
    """nu as a float: positive, or math.inf for the heat kernel (ValueError otherwise)"""
    if isinstance(nu, bool) or not isinstance(nu, (int, float)) or not (nu > 0.0) or math.isnan(nu):
        raise ValueError(f"nu must be a positive number or math.inf, got {nu!r}")
    return float(nu)


def _spectral_rho(d, device=None):
    return (d - 1 - 2.0 * torch.arange(d, dtype=torch.float64, device=device)) / 4.0


def spd_ai_spectral_base(dim, num_features, nu, seed):
    """The lengthscale-independent random draw behind the features -> (e, gamma, H): numpy arrays (L, d), (L,) or None (nu = inf), (L, d, d).
    Host only, numpy.random.Generator(PCG64(seed)), drawn in this order:
      1. standard_normal((L, d, d)) = G;  e = eigvalsh((G + G^T) / 2), density prop. to prod |e_i - e_j| exp(-|e|^2 / 2);
      2. Generator.permuted(e, axis=1): the d entries of every row in random order;
      3. finite nu only: gamma(shape nu, scale 1, L);
      4. standard_normal((L, d, d)) = Q R;  H = Q with its columns multiplied by sign(diag R): Haar on O(d)."""
    import numpy as np
    nu = _spectral_nu(nu)
    if not (isinstance(dim, int) and dim >= 2) or not (isinstance(num_features, int) and num_features >= 1):
        raise ValueError(f"dim must be an integer >= 2 and num_features an integer >= 1, got {dim!r}, {num_features!r}")
    rng = np.random.Generator(np.random.PCG64(seed))
    g = rng.standard_normal((num_features, dim, dim))
    e = rng.permuted(np.linalg.eigvalsh(0.5 * (g + g.transpose(0, 2, 1))), axis=1)
    gamma = None if math.isinf(nu) else rng.gamma(nu, 1.0, num_features)
    q, r = np.linalg.qr(rng.standard_normal((num_features, dim, dim)))
    return e, gamma, q * np.sign(np.diagonal(r, axis1=-2, axis2=-1))[:, None, :]


def spd_ai_spectral_points(base, lengthscale, nu):
    """(e, gamma, H) and a lengthscale kappa -> (lam (L, d), w (L,)), torch fp64 on the lengthscale's device, differentiable in the lengthscale:
    lam = e / kappa (nu = inf) or e sqrt((nu / kappa^2 + |rho|^2 / 2) / gamma), |rho|^2 = d (d^2 - 1) / 48;
    w = prod_{i<j} tanh(pi |lam_i - lam_j|) in (0, 1], the part of the Plancherel density the draw of e leaves out (an importance weight)."""
    nu = _spectral_nu(nu)
    ls = _scalar_param(lengthscale, _ONE_SPD_LENGTHSCALE).reshape(())
    e, gamma = (torch.as_tensor(t, dtype=torch.float64, device=ls.device) if t is not None else None for t in base[:2])
    d = e.shape[-1]
    if math.isinf(nu):
        lam = e / ls
    else:
        lam = e * torch.sqrt((nu / (ls * ls) + d * (d * d - 1) / 96.0) / gamma).unsqueeze(-1)
    i, j = torch.triu_indices(d, d, 1, device=ls.device)
    w = torch.tanh(math.pi * (lam[:, i] - lam[:, j]).abs()).prod(-1)
    return lam, w


_phases_held = None


def _spectral_phases(phases, dev, d):
    """(L, d, d) -> the entry-major (d, d, L) copy on `dev` that the launches read (a wave's loads are contiguous), remembered for the last
    tensor handed in: a kernel object calls with the same one every time"""
    global _phases_held
    if phases.dim() != 3 or phases.shape[-1] != d or phases.shape[-2] != d:
        raise RuntimeError(f"phases must be (L, {d}, {d}), got {tuple(phases.shape)}")
    key = (phases.data_ptr(), phases._version, tuple(phases.shape), phases.device, phases.dtype, dev)
    if _phases_held is None or _phases_held[0] != key:
        _phases_held = (key, _prep(phases.detach(), dev).permute(1, 2, 0).contiguous(), phases)      # (holding `phases` keeps its address its own)
    return _phases_held[1]


def _spectral_points_input(x, what):
    if x.dim() != 2:
        raise RuntimeError(f"{what}: x must be (N, d(d+1)/2) Mandel vectors (no batch dimensions), got {tuple(x.shape)}")
    return _mandel_dim(x.shape[-1])


def spd_ai_logdiag(x, phases):
    """x (N, d(d+1)/2) Mandel vectors, phases (L, d, d) orthogonal matrices -> a (N, L, d), a[i, l] = 2 log diag chol(H_l^T X_i H_l): one
    launch (gabo_spd_ai_logdiag), 2 <= d <= 10, no gradient.  N L d 8 bytes.  A NaN or non-SPD row gives NaN in its own rows of `a`."""
    lib = _lib.load()
    d = _spectral_points_input(x, "spd_ai_logdiag")
    out_device = x.device
    dev = _device_for(x, phases)
    xc = _prep(x.detach(), dev).contiguous()
    ht = _spectral_phases(phases, dev, d)
    n, L = xc.shape[0], ht.shape[-1]
    out = torch.empty(n, L, d, dtype=torch.float64, device=dev)
    with _on(dev):
        _lib.check(lib.gabo_spd_ai_logdiag(xc.data_ptr(), ht.data_ptr(), out.data_ptr(), n, L, d, _stream_ptr(dev)), "gabo_spd_ai_logdiag")
    return _out(out, out_device)


def _spectral_features_torch(a, lam, weight):
    """the features from log-diagonals a (N, L, d) by element-wise torch operations: differentiable in a, lam and weight"""
    d = a.shape[-1]
    amp = torch.sqrt(weight) * torch.exp(-(a * _spectral_rho(d, a.device)).sum(-1))
    theta = (a * lam).sum(-1)
    f = torch.cat([amp * torch.cos(theta), amp * torch.sin(theta)], dim=-1)
    return f / torch.sqrt((f * f).sum(-1, keepdim=True))


def _spectral_logdiag_torch(x, phases):
    """a(H^T X H) as a plain torch composition (torch.linalg.cholesky on N L matrices): differentiable in x, first order, slow"""
    d = _mandel_dim(x.shape[-1])
    r, c = torch.tril_indices(d, d, device=x.device)
    order = torch.argsort((r - c) * d + c, stable=True)          # Mandel order: the diagonal, then sub-diagonal 1, 2, ...
    r, c = r[order], c[order]
    scale = torch.ones(len(r), dtype=x.dtype, device=x.device).masked_fill(r != c, 0.5 ** 0.5)
    mat = torch.zeros(x.shape[:-1] + (d, d), dtype=x.dtype, device=x.device)
    mat = mat.index_put((torch.arange(x.shape[0], device=x.device)[:, None], r[None, :], c[None, :]), x * scale)
    mat = mat + torch.tril(mat, -1).transpose(-1, -2)
    s = torch.einsum("lba,nbc,lcd->nlad", phases, mat, phases)
    return 2.0 * torch.log(torch.diagonal(torch.linalg.cholesky(0.5 * (s + s.transpose(-1, -2))), dim1=-2, dim2=-1))


def _spectral_features_launch(x, phases, lam, weight, d):
    """the fused forward launch: no gradient"""
    lib = _lib.load()
    out_device = x.device
    dev = _device_for(x, phases, lam, weight)
    xc = _prep(x.detach(), dev).contiguous()
    ht = _spectral_phases(phases, dev, d)
    n, L = xc.shape[0], ht.shape[-1]
    lc, wc = _prep(lam.detach(), dev).contiguous(), _prep(weight.detach(), dev).contiguous()
    if tuple(lc.shape) != (L, d) or tuple(wc.shape) != (L,):
        raise RuntimeError(f"lam must be ({L}, {d}) and weight ({L},), got {tuple(lc.shape)} and {tuple(wc.shape)}")
    out = torch.empty(n, 2 * L, dtype=torch.float64, device=dev)
    with _on(dev):
        _lib.check(lib.gabo_spd_ai_spectral_features(xc.data_ptr(), ht.data_ptr(), lc.data_ptr(), wc.data_ptr(), out.data_ptr(), n, L, d,
                                                     _stream_ptr(dev)), "gabo_spd_ai_spectral_features")
    return _out(out, out_device)


_spectral_backward_ws = {}


def spd_ai_spectral_features_backward(x, phases, lam, fhat, grad_out):
    """The x-gradient of the normalised features, the launch alone (gabo_spd_ai_spectral_features_backward: the factorisations once more
    and one small congruence per point, no tape): x (N, d(d+1)/2), phases (L, d, d), lam (L, d), fhat (N, 2 L) =
    spd_ai_spectral_features(x, phases, lam, weight), grad_out (N, 2 L) the upstream gradient of fhat -> d <grad_out, fhat> / d x (N, d(d+1)/2)
    on x's device.  The weights cancel.  2 <= d <= 10, no gradient of its own.  A NaN or non-SPD row of x gives NaN in its own row.  The
    workspace is kept per (device, N, L, d)."""
    if x.dim() != 2:
        raise RuntimeError(f"spd_ai_spectral_features_backward: x must be (N, d(d+1)/2) Mandel vectors (no batch dimensions), got {tuple(x.shape)}")
    d = _mandel_dim(x.shape[-1])
    if phases.dim() != 3 or tuple(phases.shape[1:]) != (d, d):
        raise RuntimeError(f"spd_ai_spectral_features_backward: phases must be (L, {d}, {d}), got {tuple(phases.shape)}")
    n, L = x.shape[0], phases.shape[0]
    if tuple(lam.shape) != (L, d):
        raise RuntimeError(f"spd_ai_spectral_features_backward: lam must be ({L}, {d}), got {tuple(lam.shape)}")
    if tuple(fhat.shape) != (n, 2 * L) or tuple(grad_out.shape) != (n, 2 * L):
        raise RuntimeError(f"spd_ai_spectral_features_backward: fhat and grad_out must be ({n}, {2 * L}), got {tuple(fhat.shape)} and "
                           f"{tuple(grad_out.shape)}")
    lib = _lib.load()
    out_device = x.device
    dev = _device_for(x, phases, lam, fhat, grad_out)
    xc = _prep(x.detach(), dev).contiguous()
    ht = _spectral_phases(phases, dev, d)
    lc, fc, gc = (_prep(t.detach(), dev).contiguous() for t in (lam, fhat, grad_out))
    gx = (torch.zeros if L == 0 else torch.empty)(n, x.shape[-1], dtype=torch.float64, device=dev)          # (no feature: no launch)
    key = (dev, n, L, d)
    ws = _spectral_backward_ws.get(key)
    if ws is None:
        if len(_spectral_backward_ws) > 4:
            _spectral_backward_ws.clear()
        # (0 bytes for a shape that the call below refuses)
        ws = _spectral_backward_ws[key] = _workspace(int(lib.gabo_spd_ai_spectral_features_backward_workspace_bytes(n, L, d)), dev)
    with _on(dev):
        _lib.check(lib.gabo_spd_ai_spectral_features_backward(xc.data_ptr(), ht.data_ptr(), lc.data_ptr(), fc.data_ptr(), gc.data_ptr(),
                                                              gx.data_ptr(), ws.data_ptr(), ws.numel() * 8, n, L, d, _stream_ptr(dev)),
                   "gabo_spd_ai_spectral_features_backward")
    return _out(gx, out_device)


class _SpectralFeaturesFunction(torch.autograd.Function):
    """The fused feature launch with the backward launch as its x-gradient: first order, gradients for x only."""

    @staticmethod
    def forward(ctx, x, phases, lam, weight, d):
        fhat = _spectral_features_launch(x, phases, lam, weight, d)
        ctx.save_for_backward(x, fhat)
        ctx.phases, ctx.lam = phases, lam.detach()
        return fhat

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        x, fhat = ctx.saved_tensors
        return spd_ai_spectral_features_backward(x, ctx.phases, ctx.lam, fhat, grad_out).to(x.dtype), None, None, None, None


def spd_ai_spectral_features(x, phases, lam, weight, logdiag=None, x_grad="launch"):
    """Normalised random phase features F (N, 2 L) of the points x (N, d(d+1)/2), |F_i| = 1, for phases (L, d, d), spectral points lam (L, d)
    and weights (L,).  The cheapest route that supports the gradients asked for:
      - nothing requires grad, no `logdiag`: ONE fused launch (gabo_spd_ai_spectral_features); the log-diagonals are never stored;
      - `logdiag` (= spd_ai_logdiag(x, phases)) given: element-wise torch operations on it, differentiable in lam and weight (so in the
        lengthscale they come from); x is not looked at;
      - x requires grad and neither lam nor weight does: the fused launch, with spd_ai_spectral_features_backward (one launch pair) as its
        gradient - first order, nothing kept but x and F;
      - x requires grad together with lam or weight, or x_grad="torch": a plain torch composition through torch.linalg.cholesky of the N L
        matrices H^T X H - first order, and slow."""
    if x_grad not in ("launch", "torch"):
        raise ValueError(f"x_grad must be 'launch' or 'torch', got {x_grad!r}")
    if logdiag is not None:
        return _spectral_features_torch(logdiag, lam.to(logdiag), weight.to(logdiag))
    d = _spectral_points_input(x, "spd_ai_spectral_features")
    if torch.is_grad_enabled() and x.requires_grad:
        if x_grad == "launch" and not (lam.requires_grad or weight.requires_grad):
            return _SpectralFeaturesFunction.apply(x, phases, lam, weight, d)
        xd = x.double()
        return _spectral_features_torch(_spectral_logdiag_torch(xd, phases.to(xd)), lam.to(xd), weight.to(xd))
    if torch.is_grad_enabled() and (lam.requires_grad or weight.requires_grad):
        return _spectral_features_torch(spd_ai_logdiag(x, phases).to(lam.device), lam.double(), weight.double())
    return _spectral_features_launch(x, phases, lam, weight, d)


def spd_ai_matern_kernel(x1, x2, phases, lam, weight, logdiag1=None, logdiag2=None, diag=False, x_grad="launch"):
    """k(x1_i, x2_j) = <F(x1_i), F(x2_j)> (N1, N2) with F = spd_ai_spectral_features (routes and gradients, `x_grad` among them: see there): a
    Monte-Carlo approximation, error O(1 / sqrt L), of the Riemannian Matern / heat kernel of the affine-invariant metric that is positive
    semi-definite for every sample.  `x2 is x1`: one feature call, and the matrix is exactly symmetric with an exactly unit diagonal.
    diag=True: the diagonal (N1 == N2), exactly 1 when x2 is x1."""
    f1 = spd_ai_spectral_features(x1, phases, lam, weight, logdiag=logdiag1, x_grad=x_grad)
    if x2 is x1:
        k = torch.mm(f1, f1.t())
        dg = k.diagonal()
        unit = dg / dg                      # exactly 1, or NaN for a row of NaN features
        if diag:
            return unit
        k = 0.5 * (k + k.t())
        return torch.where(torch.eye(k.shape[0], dtype=torch.bool, device=k.device), unit.unsqueeze(-1).expand_as(k), k)
    f2 = spd_ai_spectral_features(x2, phases, lam, weight, logdiag=logdiag2, x_grad=x_grad).to(f1.device)
    return (f1 * f2).sum(-1) if diag else torch.mm(f1, f2.t())


_spectral_base_held = None


def _spectral_base_on(base, dev):
    """(e, gamma or None) of a base draw as fp64 tensors on `dev`, uploaded once per base object and remembered for the last one"""
    global _spectral_base_held
    key = (id(base[0]), None if base[1] is None else id(base[1]), dev)
    if _spectral_base_held is None or _spectral_base_held[0] != key:
        e = torch.as_tensor(base[0], dtype=torch.float64).contiguous().to(dev)
        gamma = None if base[1] is None else torch.as_tensor(base[1], dtype=torch.float64).contiguous().to(dev)
        _spectral_base_held = (key, e, gamma, base[:2])      # (holding the arrays keeps their ids their own)
    return _spectral_base_held[1], _spectral_base_held[2]


def spd_ai_spectral_points_dkappa(base, lengthscale, nu, device=None):
    """(e, gamma, H) and a lengthscale kappa (a number) -> (lam (L, d), w (L,), q (L,), c ()) on the device, one launch
    (gabo_spd_ai_spectral_points_dkappa): lam and w as spd_ai_spectral_points, q = (d log w / d kappa) / 2 and the scalar c with
    d lam / d kappa = c lam.  No gradient: q and c ARE the derivative."""
    lib = _lib.load()
    nu = _spectral_nu(nu)
    dev = torch.device(device) if device is not None else _device_for()
    e, gamma = _spectral_base_on(base, dev)
    if gamma is None and not math.isinf(nu):
        raise ValueError("a base draw without gamma belongs to the heat kernel (nu = math.inf)")
    L, d = e.shape
    lam = torch.empty(L, d, dtype=torch.float64, device=dev)
    w, q, c = (torch.empty(s, dtype=torch.float64, device=dev) for s in ((L,), (L,), ()))
    with _on(dev):
        _lib.check(lib.gabo_spd_ai_spectral_points_dkappa(e.data_ptr(), _ptr(gamma), L, d, float(lengthscale), nu, lam.data_ptr(), w.data_ptr(),
                                                          q.data_ptr(), c.data_ptr(), _stream_ptr(dev)), "gabo_spd_ai_spectral_points_dkappa")
    return lam, w, q, c


def spd_ai_spectral_features_dkappa(logdiag, lam, weight, q, c):
    """The normalised features and their lengthscale derivative from stored log-diagonals, one launch (gabo_spd_ai_spectral_features_dkappa):
    logdiag (N, L, d) = spd_ai_logdiag(x, phases), lam (L, d), weight (L,), q (L,), c (a number or a one-element tensor) as
    spd_ai_spectral_points_dkappa returns them -> (F (N, 2 L), dF / d kappa (N, 2 L)).  F has the bits of spd_ai_spectral_features(x, phases,
    lam, weight).  No gradient."""
    lib = _lib.load()
    if logdiag.dim() != 3:
        raise RuntimeError(f"spd_ai_spectral_features_dkappa: logdiag must be (N, L, d), got {tuple(logdiag.shape)}")
    out_device = logdiag.device
    dev = _device_for(logdiag, lam, weight)
    a = _prep(logdiag.detach(), dev).contiguous()
    n, L, d = a.shape
    lc, wc, qc = (_prep(t.detach(), dev).contiguous() for t in (lam, weight, q))
    cc = _prep(c.detach() if torch.is_tensor(c) else torch.tensor(float(c), dtype=torch.float64), dev).reshape(1)
    if tuple(lc.shape) != (L, d) or tuple(wc.shape) != (L,) or tuple(qc.shape) != (L,):
        raise RuntimeError(f"lam must be ({L}, {d}), weight and q ({L},), got {tuple(lc.shape)}, {tuple(wc.shape)} and {tuple(qc.shape)}")
    f = torch.empty(n, 2 * L, dtype=torch.float64, device=dev)
    g = torch.empty(n, 2 * L, dtype=torch.float64, device=dev)
    if n > 0:
        with _on(dev):
            _lib.check(lib.gabo_spd_ai_spectral_features_dkappa(a.data_ptr(), lc.data_ptr(), wc.data_ptr(), qc.data_ptr(), cc.data_ptr(),
                                                                f.data_ptr(), g.data_ptr(), n, L, d, _stream_ptr(dev)),
                       "gabo_spd_ai_spectral_features_dkappa")
    return _out(f, out_device), _out(g, out_device)


def spd_ai_feature_gram(f):
    """f (N, k) -> f f^T (N, N) on the fp64 matrix pipe (gabo_spd_ai_feature_gram): exactly symmetric, the diagonal exactly 1 for rows of unit
    norm (v / v: NaN for a row with a NaN); the bits of an entry depend on its two rows alone.  N <= GABO_GP_MLL_LARGE_MAX_N.  No gradient."""
    lib = _lib.load()
    if f.dim() != 2:
        raise RuntimeError(f"spd_ai_feature_gram: f must be (N, k), got {tuple(f.shape)}")
    out_device, dev, fc = _dense(f.detach())
    n, k = fc.shape
    ws = _workspace(int(lib.gabo_spd_ai_feature_gram_workspace_bytes(n, k)), dev)
    out = torch.empty(n, n, dtype=torch.float64, device=dev)
    with _on(dev):
        _lib.check(lib.gabo_spd_ai_feature_gram(fc.data_ptr(), out.data_ptr(), n, k, ws.data_ptr(), ws.numel() * 8, _stream_ptr(dev)),
                   "gabo_spd_ai_feature_gram")
    return _out(out, out_device)


def gp_acquisition(kstar, alpha, linv, linv_t, mean, outputscale, kxx, best_f, kind, maximize, out_sign=1.0, need_grad=True):
    """Fused GP posterior + acquisition on the strip kstar (R x n, base kernel values): -> (value R, d value / d kstar R x n or None).
    All tensors fp64 on one HIP device."""
    lib = _lib.load()
    dev = kstar.device
    ks = kstar.contiguous()
    r, n = ks.shape
    value = torch.empty(r, dtype=torch.float64, device=dev)
    grad = torch.empty_like(ks) if need_grad else None
    with _on(dev):
        _lib.check(lib.gabo_gp_acquisition(ks.data_ptr(), alpha.data_ptr(), _ptr(linv), _ptr(linv_t), value.data_ptr(), _ptr(grad), r, n,
                                           float(mean), float(outputscale), float(kxx), float(best_f), int(kind), 1 if maximize else 0,
                                           float(out_sign), _stream_ptr(dev)), "gabo_gp_acquisition")
    return value, grad


_GP_FACTOR_MESSAGE = "gabo_gp_factor: the training covariance outputscale * K + noise * I is not positive definite (Cholesky pivot <= 0)"


def gp_factor(kbase, y, outputscale, noise, mean, defer_check=False, on_fail=None, want_kinv=False):
    """Prediction cache of the exact GP in one launch (gabo_gp_factor): kbase n x n BASE kernel matrix of the training set, y its targets ->
    (L^-1, L^-T, alpha) with L = chol(outputscale kbase + noise I), alpha = (outputscale kbase + noise I)^-1 (y - mean); n <= GABO_GP_FACTOR_MAX_N.
    Raises like torch.linalg.cholesky when the matrix is not positive definite - at once, or (defer_check=True) at the next check_deferred();
    on_fail: called before that error is raised (the caller drops whatever it built on the factor).  All tensors fp64 on one HIP device."""
    lib = _lib.load()
    dev = kbase.device
    kb, yy = kbase.contiguous(), y.to(dev, torch.float64).contiguous()
    n = kb.shape[-1]
    _require(dev, kbase=kb, y=yy)
    linv = torch.empty(n, n, dtype=torch.float64, device=dev)
    linv_t = torch.empty(n, n, dtype=torch.float64, device=dev)
    alpha = torch.empty(n, dtype=torch.float64, device=dev)
    kinv = torch.empty(n, n, dtype=torch.float64, device=dev) if want_kinv else None
    status = _status_word(dev, force=True)
    with _on(dev):
        rc = lib.gabo_gp_factor(kb.data_ptr(), yy.data_ptr(), n, float(outputscale), float(noise), float(mean), linv.data_ptr(), linv_t.data_ptr(),
                                alpha.data_ptr(), None if kinv is None else kinv.data_ptr(), status.data_ptr(), _stream_ptr(dev))
    _lib.check(rc, "gabo_gp_factor")
    # The status is read back whatever set_error_checking says (torch.linalg.cholesky would raise here too, and a silent garbage factor would
    # poison every acquisition value) - but not HERE: the read-back would park the host behind the launch (~0.1 ms of a 4-ms sweep) while it
    # has the rest of the sweep's launches to issue.  It is registered and checked at the caller's next natural synchronisation point
    # (check_deferred: after the raw samples' scores have been copied to the host, after a solve, or whenever error checking reads a status).
    _raise_if_not_spd(status, "gabo_gp_factor", message=_GP_FACTOR_MESSAGE, on_fail=on_fail, force=True)
    if defer_check is False:
        check_deferred()
    if want_kinv:          # (+ the symmetric inverse L^-T L^-1: what the fused SPD acquisition kernels take in place of the two factors)
        return linv, linv_t, alpha, kinv
    return linv, linv_t, alpha


_gp_prepare_ws = {}


def spd_gp_prepare(train_mandel, y, beta, mode, outputscale, noise, mean, want_factors=True, on_fail=None):
    """Everything an acquisition sweep needs from a fitted exact GP with an affine-invariant kernel, from ONE host call (gabo_spd_gp_prepare):
    the training Gram matrix, (L^-1, L^-T, alpha) of gp_factor, the entry-major training factors of spd_acq_prepare_train (d_vec x n, or None) and
    the symmetric inverse A = L^-T L^-1 -> (linv, linv_t, alpha, factors, kinv).
    The Cholesky status is checked at the next check_deferred() (as gp_factor(defer_check=True)); on_fail as there."""
    lib = _lib.load()
    dev = train_mandel.device
    x = train_mandel if train_mandel.is_contiguous() else train_mandel.contiguous()
    yy = y if (y.device == dev and y.dtype == torch.float64 and y.is_contiguous()) else y.to(dev, torch.float64).contiguous()
    if not (x.is_cuda and x.dtype == torch.float64 and x.dim() == 2 and yy.numel() == x.shape[0]):
        raise TypeError("spd_gp_prepare: train_mandel must be an n x d_vec fp64 tensor on a HIP device and y its n targets")
    n, dv = x.shape
    d = _mandel_dim(dv)
    # one allocation for the outputs: [L^-1 | L^-T | alpha | A = L^-T L^-1 | factors]
    nn = n * n
    flat = torch.empty(3 * nn + n + (dv * n if want_factors else 0), dtype=torch.float64, device=dev)
    base = flat.data_ptr()
    stream = _stream_ptr(dev)
    key = (dev.index, stream, n, d)
    ent = _gp_prepare_ws.get(key)
    if ent is None:
        if len(_gp_prepare_ws) > 16:
            _gp_prepare_ws.clear()
        wsb = int(lib.gabo_spd_gp_prepare_workspace_bytes(n, d))
        ent = _gp_prepare_ws[key] = (torch.empty(wsb, dtype=torch.uint8, device=dev), wsb)
    ws, wsb = ent
    status, fstatus = _status_word(dev), _status_word(dev, force=True)
    with _on(dev):
        rc = lib.gabo_spd_gp_prepare(x.data_ptr(), yy.data_ptr(), n, d, beta, mode, outputscale, noise, mean, base, base + 8 * nn, base + 16 * nn,
                                     base + 8 * (2 * nn + n), base + 8 * (3 * nn + n) if want_factors else None, ws.data_ptr(), wsb,
                                     status.data_ptr(), fstatus.data_ptr(), stream)
    _check_launch(rc, status, "gabo_spd_gp_prepare", on_fail=on_fail)
    _raise_if_not_spd(fstatus, "gabo_gp_factor", message=_GP_FACTOR_MESSAGE, on_fail=on_fail, force=True)
    linv, linv_t, alpha = flat[:nn].view(n, n), flat[nn:2 * nn].view(n, n), flat[2 * nn:2 * nn + n]
    kinv = flat[2 * nn + n:3 * nn + n].view(n, n)
    factors = flat[3 * nn + n:].view(dv, n) if want_factors else None
    return linv, linv_t, alpha, factors, kinv


_mll_large_ws = {}


def _gp_mll_large(e, y, theta, outputscale, noise, mean, gram, want_w):
    """gabo_gp_mll_large on contiguous device tensors -> (out (6,) device tensor, W or None); the workspace is kept per (device, n)."""
    lib = _lib.load()
    dev, n = e.device, e.shape[-1]
    key = (dev, n)
    ws = _mll_large_ws.get(key)
    if ws is None:
        if len(_mll_large_ws) > 4:
            _mll_large_ws.clear()
        ws = _mll_large_ws[key] = torch.empty(int(lib.gabo_gp_mll_large_workspace_bytes(n)) // 8 + 1, dtype=torch.float64, device=dev)
    out = torch.empty(6, dtype=torch.float64, device=dev)
    w = torch.empty(n, n, dtype=torch.float64, device=dev) if want_w else None
    with _on(dev):
        _lib.check(lib.gabo_gp_mll_large(e.data_ptr(), y.data_ptr(), n, float(theta), float(outputscale), float(noise), float(mean),
                                         1 if gram else 0, out.data_ptr(), _ptr(w), ws.data_ptr(),
                                         ws.numel() * 8, _stream_ptr(dev)), "gabo_gp_mll_large")
    return out, w


_mll_host_out = {}


def _mll_host(dev):
    """The page-locked result buffer of the small likelihood launches, one per device, which the kernel addresses itself: -> (tensor, its
    numpy view).  An L-BFGS evaluation is the launch and a stream wait - no device buffer, no copy back (a surrogate fit is ~35 of these;
    worth 4 % of it: 1.57 -> 1.51 ms on 5 ... 20 observations - the rest is scipy's L-BFGS-B and the Python chain rule around the launch)."""
    ent = _mll_host_out.get(dev.index)
    if ent is None:
        host = _pinned(8).zero_()
        ent = _mll_host_out[dev.index] = (host, host.numpy())
    return ent


def _mll_wait_and_read(dev, host_np):
    """after the launch that was handed _mll_host's buffer: the six results as Python floats"""
    torch.cuda.current_stream(dev).synchronize()
    return host_np[:6].tolist()


def gp_mll(e, y, theta, outputscale, noise, mean):
    """One evaluation of the exact-GP marginal log likelihood with K = outputscale * exp(-theta * e) + noise * I (gabo_gp_mll; the tiled
    gabo_gp_mll_large beyond GABO_GP_MLL_MAX_N points): -> [ll, dll/dtheta, dll/doutputscale, dll/dnoise, dll/dmean,
    not_positive_definite] as Python floats (one device->host copy).  e: n x n fp64 on a HIP device (n <= GABO_GP_MLL_LARGE_MAX_N), y: n."""
    lib = _lib.load()
    dev = e.device
    n = e.shape[-1]
    if e.dim() != 2 or e.shape[0] != n or y.numel() != n or not e.is_contiguous() or not y.is_contiguous():
        raise RuntimeError("gp_mll: e must be a contiguous n x n matrix and y a contiguous vector of n targets")
    if n > _lib.GABO_GP_MLL_MAX_N:
        return _gp_mll_large(e, y, theta, outputscale, noise, mean, False, False)[0].tolist()
    # (the inner loop of a fit: _mll_host only when this device has no buffer yet, and _mll_wait_and_read written out - the two calls measured
    # 0.1 us on the 22.8 us of an evaluation at n = 20)
    host, host_np = _mll_host_out.get(dev.index) or _mll_host(dev)
    with _on(dev):
        stream = _stream_ptr(dev)
        _lib.check(lib.gabo_gp_mll(e.data_ptr(), y.data_ptr(), n, float(theta), float(outputscale), float(noise), float(mean),
                                   host.data_ptr(), stream), "gabo_gp_mll")
        torch.cuda.current_stream(dev).synchronize()
    return host_np[:6].tolist()


def gp_mll_gram(k, y, outputscale, noise, mean, want_w=True):
    """gabo_gp_mll_gram: exact-GP marginal log likelihood for Ky = outputscale * k + noise * I with k an arbitrary base Gram matrix
    (n x n fp64 on a HIP device, n <= GABO_GP_MLL_LARGE_MAX_N).  -> (out (6,) device tensor: ll, 0, dll/doutputscale, dll/dnoise,
    dll/dmean, not-positive-definite flag;  W = alpha alpha^T - Ky^-1 (n x n) or None).  No host synchronisation."""
    lib = _lib.load()
    dev = k.device
    n = k.shape[-1]
    if k.dim() != 2 or k.shape[0] != n or y.numel() != n:
        raise RuntimeError("gp_mll_gram: k must be an n x n matrix and y a vector of n targets")
    k, y = k.contiguous(), y.contiguous()
    if n > _lib.GABO_GP_MLL_MAX_N:
        return _gp_mll_large(k, y, 0.0, outputscale, noise, mean, True, want_w)
    out = torch.empty(6, dtype=torch.float64, device=dev)
    w = torch.empty(n, n, dtype=torch.float64, device=dev) if want_w else None
    with _on(dev):
        _lib.check(lib.gabo_gp_mll_gram(k.data_ptr(), y.data_ptr(), n, float(outputscale), float(noise), float(mean), out.data_ptr(), _ptr(w),
                                        _stream_ptr(dev)), "gabo_gp_mll_gram")
    return out, w


def gp_mll_series(c, y, coeff, dcoeff, series_dim, outputscale, noise, mean):
    """One evaluation of the exact-GP marginal log likelihood with K = outputscale * sum_k coeff[k] P_k^(series_dim)(c) + noise * I, the
    zonal series evaluated inside the launch (gabo_gp_mll_series): -> [ll, dll/dkappa, dll/doutputscale, dll/dnoise, dll/dmean,
    not_positive_definite] as Python floats, dll/dkappa from the series dcoeff of d coeff / d kappa (None: 0).  c: the n x n inner products,
    fp64 on a HIP device, y: n; coeff, dcoeff: host float64 (sphere_matern_coefficients_and_derivative).  Beyond GABO_GP_MLL_MAX_N points (up
    to GABO_GP_MLL_LARGE_MAX_N) the same numbers are composed from the element-wise series, gabo_gp_mll_large and one reduction."""
    lib = _lib.load()
    dev = c.device
    n = c.shape[-1]
    if c.dim() != 2 or c.shape[0] != n or y.numel() != n or not c.is_contiguous() or not y.is_contiguous():
        raise RuntimeError("gp_mll_series: c must be a contiguous n x n matrix and y a contiguous vector of n targets")
    a, ptr, na = _zonal_coeff(coeff)
    da, dptr, nda = _zonal_coeff(dcoeff) if dcoeff is not None else (None, None, na)
    if nda != na:
        raise RuntimeError(f"gp_mll_series: {na} coefficients but {nda} derivative coefficients")
    if n > _lib.GABO_GP_MLL_MAX_N:
        out, w = _gp_mll_large(sphere_zonal_from_inner(c, a, series_dim), y, 0.0, outputscale, noise, mean, True, da is not None)
        if da is not None:
            d_kappa = (0.5 * float(outputscale)) * (w * sphere_zonal_from_inner(c, da, series_dim)).sum()
            out[1] = torch.where(out[5] == 0, d_kappa, torch.zeros_like(d_kappa))
        return out.tolist()
    host, host_np = _mll_host(dev)                 # (as gp_mll: one launch, one stream wait)
    with _on(dev):
        stream = _stream_ptr(dev)
        _lib.check(lib.gabo_gp_mll_series(c.data_ptr(), y.data_ptr(), n, ptr, dptr, na, int(series_dim), float(outputscale), float(noise),
                                          float(mean), host.data_ptr(), stream), "gabo_gp_mll_series")
        return _mll_wait_and_read(dev, host_np)


def gp_mll_matern(r, y, lengthscale, nu, outputscale, noise, mean):
    """One evaluation of the exact-GP marginal log likelihood with K = outputscale * k_nu(r; lengthscale) + noise * I, the Matern function of
    flat_matern_from_distance evaluated inside the launch (gabo_gp_mll_matern): -> [ll, dll/dlengthscale, dll/doutputscale, dll/dnoise,
    dll/dmean, not_positive_definite] as Python floats.  r: the n x n distance matrix (frobenius_pairwise with GABO_OUT_DISTANCE), fp64 on a
    HIP device, y: n; nu in {0.5, 1.5, 2.5}.  Beyond GABO_GP_MLL_MAX_N points (up to GABO_GP_MLL_LARGE_MAX_N) the same numbers are composed
    from the element-wise launches, gabo_gp_mll_large and one reduction."""
    lib = _lib.load()
    nu2, lval = _matern_nu2(nu), _matern_lengthscale(lengthscale)
    dev = r.device
    n = r.shape[-1]
    if r.dim() != 2 or r.shape[0] != n or y.numel() != n or not r.is_contiguous() or not y.is_contiguous():
        raise RuntimeError("gp_mll_matern: r must be a contiguous n x n matrix and y a contiguous vector of n targets")
    if n > _lib.GABO_GP_MLL_MAX_N:
        out, w = _gp_mll_large(flat_matern_from_distance(r, lval, nu, 0), y, 0.0, outputscale, noise, mean, True, True)
        d_l = (0.5 * float(outputscale)) * (w * flat_matern_from_distance(r, lval, nu, 1)).sum()
        out[1] = torch.where(out[5] == 0, d_l, torch.zeros_like(d_l))
        return out.tolist()
    host, host_np = _mll_host(dev)                 # (as gp_mll: one launch, one stream wait)
    with _on(dev):
        stream = _stream_ptr(dev)
        _lib.check(lib.gabo_gp_mll_matern(r.data_ptr(), y.data_ptr(), n, lval, nu2, float(outputscale), float(noise), float(mean),
                                          host.data_ptr(), stream), "gabo_gp_mll_matern")
        return _mll_wait_and_read(dev, host_np)


_mll_spectral_ws = {}


def gp_mll_spd_ai_spectral(logdiag, y, base, lengthscale, nu, outputscale, noise, mean):
    """One evaluation of the exact-GP marginal log likelihood with K = outputscale * k(kappa) + noise * I, k the random-phase-feature Matern /
    heat kernel of the affine-invariant SPD metric (spd_ai_matern_kernel) at the lengthscale kappa, as ONE host call
    (gabo_gp_mll_spd_ai_spectral): -> [ll, dll/dkappa, dll/doutputscale, dll/dnoise, dll/dmean, not_positive_definite] as Python floats.
    logdiag: (n, L, d) = spd_ai_logdiag(x, phases) of the training points, contiguous fp64 on a HIP device, which is fixed during a fit; y: n;
    base = (e, gamma, H) of spd_ai_spectral_base, e and gamma uploaded once per base object.  n <= GABO_GP_MLL_LARGE_MAX_N, d <= 10.  The
    workspace and the page-locked result buffer are kept per (device, n, L, d)."""
    lib = _lib.load()
    nu = _spectral_nu(nu)
    dev = logdiag.device
    if logdiag.dim() != 3 or y.numel() != logdiag.shape[0] or not logdiag.is_contiguous() or not y.is_contiguous():
        raise RuntimeError("gp_mll_spd_ai_spectral: logdiag must be a contiguous (n, L, d) tensor and y a contiguous vector of n targets")
    _require(dev, logdiag=logdiag, y=y)
    n, L, d = logdiag.shape
    e, gamma = _spectral_base_on(base, dev)
    if tuple(e.shape) != (L, d) or (gamma is None) != math.isinf(nu):
        raise RuntimeError(f"gp_mll_spd_ai_spectral: the base draw has e {tuple(e.shape)} and {'no ' if gamma is None else ''}gamma; "
                           f"logdiag is {(n, L, d)} and nu = {nu}")
    key = (dev, n, L, d)
    ent = _mll_spectral_ws.get(key)
    if ent is None:
        wsb = int(lib.gabo_gp_mll_spd_ai_spectral_workspace_bytes(n, L, d))
        if wsb == 0:
            raise RuntimeError(f"gp_mll_spd_ai_spectral: (n, L, d) = {(n, L, d)} is outside 1 <= n <= {_lib.GABO_GP_MLL_LARGE_MAX_N}, 2 <= d <= 10")
        if len(_mll_spectral_ws) > 4:
            _mll_spectral_ws.clear()
        import ctypes
        ent = _mll_spectral_ws[key] = (_workspace(wsb, dev), _pinned(8).zero_(), (ctypes.c_double * 7)())
    ws, host, out = ent
    with _on(dev):
        _lib.check(lib.gabo_gp_mll_spd_ai_spectral(logdiag.data_ptr(), y.data_ptr(), e.data_ptr(), _ptr(gamma), n, L, d, nu, float(lengthscale),
                                                   float(outputscale), float(noise), float(mean), out, ws.data_ptr(), ws.numel() * 8,
                                                   host.data_ptr(), 8, _stream_ptr(dev)), "gabo_gp_mll_spd_ai_spectral")
    return [out[0], out[6], out[2], out[3], out[4], out[5]]


def gram_extreme_eigenvalues(e, thetas):
    """gabo_gram_extreme_eig: {lambda_min, lambda_max} of K = exp(-theta * e), entry by entry, for every matrix of e and every theta in one
    launch (the kernel-parameter studies of examples/kernels/*/..._kernel_parameters.py; kernel_utils.kernel_parameters builds e).
    e: (..., n, n) fp64 on a HIP device, symmetric (the lower triangle and the diagonal are read), n <= GABO_GRAM_EIG_MAX_N;
    thetas: (P,) tensor or sequence.  -> (..., P, 2) on e's device.  A non-finite entry of a matrix or a non-finite theta gives NaN for
    the pairs it touches, no error.  The workspace is allocated here; no host synchronisation."""
    lib = _lib.load()
    if not torch.is_tensor(e) or not e.is_cuda or e.dtype != torch.float64:
        raise ValueError("gram_extreme_eigenvalues: e must be an fp64 tensor on a HIP device")
    if e.dim() < 2 or e.shape[-1] != e.shape[-2]:
        raise ValueError(f"gram_extreme_eigenvalues: e must be (..., n, n), got {tuple(e.shape)}")
    dev, n = e.device, e.shape[-1]
    if not 1 <= n <= _lib.GABO_GRAM_EIG_MAX_N:
        raise ValueError(f"gram_extreme_eigenvalues: n = {n} outside 1 ... {_lib.GABO_GRAM_EIG_MAX_N}")
    th = thetas if torch.is_tensor(thetas) else torch.as_tensor(thetas, dtype=torch.float64)
    if th.dim() != 1 or th.numel() < 1:
        raise ValueError(f"gram_extreme_eigenvalues: thetas must be (P,) with P >= 1, got {tuple(th.shape)}")
    th = th.to(device=dev, dtype=torch.float64).contiguous()
    bshape, nt = tuple(e.shape[:-2]), th.numel()
    nb = math.prod(bshape)
    if nb < 1:
        raise ValueError(f"gram_extreme_eigenvalues: empty batch {tuple(e.shape)}")
    ec = e.contiguous()
    out = torch.empty(bshape + (nt, 2), dtype=torch.float64, device=dev)
    wsb = int(lib.gabo_gram_extreme_eig_workspace_bytes(nb, n, nt))
    ws = _workspace(wsb, dev) if wsb else None
    with _on(dev):
        _lib.check(lib.gabo_gram_extreme_eig(ec.data_ptr(), nb, n, th.data_ptr(), nt, out.data_ptr(), _ptr(ws), wsb, _stream_ptr(dev)),
                   "gabo_gram_extreme_eig")
    return out


def gp_posterior_joint(kstar, kss, linv, alpha, mean, outputscale, inplace=True):
    """Joint posterior of the latent f over a test set in two launches (gabo_gp_posterior_joint): kstar m x n and kss m x m BASE kernel values
    (test x train, test x test; the lower triangle and the diagonal of kss are read), linv = L^-1 with L L^T = outputscale k + noise I and
    alpha = Ky^-1 (y - mean) from the prediction cache -> (mean (m,), variance (m,), covariance m x m, exactly symmetric; its diagonal is
    the variance bit for bit).  kss is overwritten with the covariance and returned unless inplace=False.  All tensors fp64 on one HIP
    device, n <= GABO_GP_MLL_LARGE_MAX_N; dense m x m memory.  No host synchronisation."""
    lib = _lib.load()
    for name, t in (("kstar", kstar), ("kss", kss), ("linv", linv), ("alpha", alpha)):
        if not torch.is_tensor(t) or not t.is_cuda or t.dtype != torch.float64:
            raise ValueError(f"gp_posterior_joint: {name} must be an fp64 tensor on a HIP device")
    if kstar.dim() != 2 or kss.dim() != 2:
        raise ValueError(f"gp_posterior_joint: kstar must be m x n and kss m x m (one test set), got {tuple(kstar.shape)} and {tuple(kss.shape)}")
    dev = kstar.device
    m, n = kstar.shape
    if tuple(kss.shape) != (m, m) or tuple(linv.shape) != (n, n) or alpha.numel() != n:
        raise ValueError(f"gp_posterior_joint: kstar {tuple(kstar.shape)}, kss {tuple(kss.shape)}, linv {tuple(linv.shape)} and alpha "
                         f"{tuple(alpha.shape)} do not belong together")
    if not (1 <= m <= _lib.GABO_GP_POSTERIOR_MAX_M and 1 <= n <= _lib.GABO_GP_MLL_LARGE_MAX_N):
        raise ValueError(f"gp_posterior_joint: m = {m}, n = {n} outside 1 ... {_lib.GABO_GP_POSTERIOR_MAX_M}, 1 ... {_lib.GABO_GP_MLL_LARGE_MAX_N}")
    ks, li, al = kstar.contiguous(), linv.contiguous(), alpha.contiguous()
    cov = kss if (inplace and kss.is_contiguous()) else kss.clone(memory_format=torch.contiguous_format)
    _require(dev, kstar=ks, kss=cov, linv=li, alpha=al)
    out = torch.empty(2, m, dtype=torch.float64, device=dev)
    wsb = int(lib.gabo_gp_posterior_joint_workspace_bytes(m, n))
    ws = _workspace(wsb, dev)
    with _on(dev):
        _lib.check(lib.gabo_gp_posterior_joint(ks.data_ptr(), cov.data_ptr(), li.data_ptr(), al.data_ptr(), m, n, float(mean), float(outputscale),
                                               out[0].data_ptr(), out[1].data_ptr(), ws.data_ptr(), wsb, _stream_ptr(dev)),
                   "gabo_gp_posterior_joint")
    if inplace and cov is not kss:
        kss.copy_(cov)
        cov = kss
    return out[0], out[1], cov


def _gp_condition_message(st):
    return (f"gabo_gp_condition: the covariance extended by new point #{st[1]} is not positive definite (lambda^2 = outputscale k(x, x) + noise "
            f"- l.l <= 0 or not finite)")


def gp_condition(linv, alpha, kcross, knew, y_new=None, outputscale=1.0, noise=1e-2, mean=0.0, kinv=None, want_linv_t=True, on_fail=None):
    """The prediction cache (linv = L^-1 n x n, alpha = Ky^-1 (y - mean), kinv = Ky^-1 or None) extended by t new points without a new
    factorisation (gabo_gp_condition: bordered O(n^2) updates, 1 + 3 t launches, no host synchronisation): kcross t x n and knew t x t BASE
    kernel values (new x train, new x new; the lower triangle and the diagonal of knew are read), y_new the t targets or None for the
    believer (the current posterior mean at each new point in turn: alpha[:n] is then copied untouched and alpha[n:] = 0)
    -> (linv, linv_t or None, alpha, kinv or None, y_used (t,)) for the n + t points, new tensors.  t <= GABO_GP_CONDITION_MAX_T,
    n + t <= GABO_GP_MLL_LARGE_MAX_N.  All tensors fp64 on one HIP device.  A new point that leaves the matrix not positive definite
    raises RuntimeError at the next check_deferred(), as gp_factor(defer_check=True) does; on_fail is called before that."""
    lib = _lib.load()
    given = [("linv", linv), ("alpha", alpha), ("kcross", kcross), ("knew", knew)] + ([("y_new", y_new)] if y_new is not None else []) \
        + ([("kinv", kinv)] if kinv is not None else [])
    for name, t_ in given:
        if not torch.is_tensor(t_) or not t_.is_cuda or t_.dtype != torch.float64:
            raise ValueError(f"gp_condition: {name} must be an fp64 tensor on a HIP device")
    dev = linv.device
    if any(t_.device != dev for _, t_ in given):
        raise ValueError("gp_condition: all tensors must be on one HIP device")
    if kcross.dim() != 2 or knew.dim() != 2 or linv.dim() != 2:
        raise ValueError(f"gp_condition: linv must be n x n, kcross t x n and knew t x t (one set of new points), got {tuple(linv.shape)}, "
                         f"{tuple(kcross.shape)} and {tuple(knew.shape)}")
    t, n = kcross.shape
    if tuple(linv.shape) != (n, n) or tuple(knew.shape) != (t, t) or alpha.numel() != n or (y_new is not None and y_new.numel() != t) \
            or (kinv is not None and tuple(kinv.shape) != (n, n)):
        raise ValueError(f"gp_condition: linv {tuple(linv.shape)}, alpha {tuple(alpha.shape)}, kcross {tuple(kcross.shape)}, knew {tuple(knew.shape)}"
                         f"{'' if y_new is None else f', y_new {tuple(y_new.shape)}'}{'' if kinv is None else f', kinv {tuple(kinv.shape)}'} "
                         f"do not belong together")
    if not (1 <= n and 1 <= t <= _lib.GABO_GP_CONDITION_MAX_T and n + t <= _lib.GABO_GP_MLL_LARGE_MAX_N):
        raise ValueError(f"gp_condition: n = {n}, t = {t} outside 1 <= n, 1 <= t <= {_lib.GABO_GP_CONDITION_MAX_T}, "
                         f"n + t <= {_lib.GABO_GP_MLL_LARGE_MAX_N}")
    li, al, kc, kn = linv.contiguous(), alpha.contiguous(), kcross.contiguous(), knew.contiguous()
    yn = None if y_new is None else y_new.reshape(-1).contiguous()
    ki = None if kinv is None else kinv.contiguous()
    m = n + t
    # one allocation for the outputs and the workspace: [L^-1 | L^-T | A | alpha | y_used | workspace]
    wsb = int(lib.gabo_gp_condition_workspace_bytes(n, t))
    parts = [m * m, m * m if want_linv_t else 0, m * m if ki is not None else 0, m, t, wsb // 8]
    flat = torch.empty(sum(parts), dtype=torch.float64, device=dev)
    cuts = [0]
    for p in parts:
        cuts.append(cuts[-1] + p)
    linv_o, linv_t_o, kinv_o, alpha_o, y_used, ws = (flat[a:b] if b > a else None for a, b in zip(cuts[:-1], cuts[1:]))
    linv_o, linv_t_o, kinv_o = (None if v is None else v.view(m, m) for v in (linv_o, linv_t_o, kinv_o))
    status = _status_word(dev, force=True)
    with _on(dev):
        rc = lib.gabo_gp_condition(li.data_ptr(), al.data_ptr(), _ptr(ki), n, kc.data_ptr(), kn.data_ptr(), _ptr(yn), t, float(outputscale),
                                   float(noise), float(mean), linv_o.data_ptr(), _ptr(linv_t_o), alpha_o.data_ptr(), _ptr(kinv_o),
                                   y_used.data_ptr(), ws.data_ptr(), wsb, status.data_ptr(), _stream_ptr(dev))
    _lib.check(rc, "gabo_gp_condition")
    # (read back whatever set_error_checking says, at the caller's next synchronisation point: as gp_factor(defer_check=True))
    _raise_if_not_spd(status, "gabo_gp_condition", message=_gp_condition_message, on_fail=on_fail, force=True)
    return linv_o, linv_t_o, alpha_o, kinv_o, y_used


_MVN_MESSAGE = ("gabo_mvn_sample: the covariance matrix is not positive definite (no Cholesky factor with a jitter of 0, 1e-8, 1e-7 or 1e-6 "
                "on the diagonal)")


def _mvn_seed(seed):
    if seed is None:
        import numpy as np
        seed = int(np.random.randint(0, 2 ** 63 - 1, dtype=np.int64))
    return int(seed) & 0xFFFFFFFFFFFFFFFF


def mvn_base_samples(samples, m, seed, device=None):
    """samples x m standard normals of the stream gabo_mvn_sample draws from when it is given no base samples (Philox, key = seed, item = sample
    index, draw k -> coordinates 2k and 2k + 1, stream tag "mvnz"): the same seed gives the same normals here and there."""
    lib = _lib.load()
    dev = _device_for() if device is None else torch.device(device)
    samples, m = int(samples), int(m)
    if samples < 0 or m < 1:
        raise ValueError(f"mvn_base_samples: samples = {samples}, m = {m}")
    out = torch.empty(samples, m, dtype=torch.float64, device=dev)
    with _on(dev):
        _lib.check(lib.gabo_mvn_base_samples(out.data_ptr(), samples, m, _mvn_seed(seed), _stream_ptr(dev)), "gabo_mvn_base_samples")
    return out


def mvn_sample(mean, cov, sample_shape=(), seed=None, base_samples=None, return_scale_tril=False):
    """Draws from N(mean, cov): sample_shape + (m,) on cov's device, out = mean + L z with L L^T = cov + j I for the first j of
    GABO_MVN_JITTER_LADDER that factors (gpytorch's psd_safe_cholesky for doubles [3P]).
    m <= GABO_MVN_SAMPLE_MAX_M: one launch (gabo_mvn_sample), no host synchronisation; a matrix that no rung factors raises
    RuntimeError("... not positive definite") through set_error_checking's machinery (at the call, or at the next check_deferred()).
    Larger m: the same ladder around torch.linalg.cholesky_ex (one host wait per rung) and a matrix product; the normals are the same
    stream either way (mvn_base_samples), so a seed gives the same draw on both paths.
    z: base_samples (sample_shape + (m,)) when given, else the stream `seed` (None: a seed from numpy's global generator).
    return_scale_tril: -> (samples, L m x m, rung) with rung a 0-d int32 device tensor indexing the ladder."""
    lib = _lib.load()
    if not torch.is_tensor(cov) or not cov.is_cuda or cov.dtype != torch.float64 or cov.dim() != 2 or cov.shape[0] != cov.shape[1]:
        raise ValueError("mvn_sample: cov must be an m x m fp64 tensor on a HIP device")
    dev, m = cov.device, cov.shape[-1]
    if m < 1:
        raise ValueError("mvn_sample: empty covariance")
    shape = tuple(int(s) for s in sample_shape)
    count = math.prod(shape)
    mu = _prep(torch.as_tensor(mean), dev).reshape(-1).contiguous()
    if mu.numel() != m:
        raise ValueError(f"mvn_sample: mean has {mu.numel()} entries, cov is {m} x {m}")
    cv = cov.contiguous()
    z = None
    if base_samples is not None:
        z = _prep(torch.as_tensor(base_samples), dev)
        if tuple(z.shape) != shape + (m,):
            raise ValueError(f"mvn_sample: base_samples must be {shape + (m,)}, got {tuple(z.shape)}")
        z = z.reshape(count, m).contiguous()
    if m > _lib.GABO_MVN_SAMPLE_MAX_M:
        if z is None:
            z = mvn_base_samples(count, m, seed, device=dev)
        eye = torch.eye(m, dtype=torch.float64, device=dev)
        for rung, jitter in enumerate(_lib.GABO_MVN_JITTER_LADDER):
            L, info = torch.linalg.cholesky_ex(cv if jitter == 0.0 else cv + jitter * eye)
            if int(info.item()) == 0 and bool(torch.isfinite(L).all()):
                break
        else:
            raise RuntimeError(_MVN_MESSAGE)
        out = (mu + z @ L.transpose(-1, -2)).reshape(shape + (m,))
        return (out, L, torch.tensor(rung, dtype=torch.int32, device=dev)) if return_scale_tril else out
    out = torch.empty(count, m, dtype=torch.float64, device=dev)
    tril = torch.empty(m, m, dtype=torch.float64, device=dev) if return_scale_tril else None
    status = torch.zeros(2, dtype=torch.int32, device=dev)       # (a word of its own: status[1], the rung, outlives the error check)
    with _on(dev):
        _lib.check(lib.gabo_mvn_sample(mu.data_ptr(), cv.data_ptr(), m, count, _mvn_seed(seed) if z is None else 0,
                                       _ptr(z), out.data_ptr(), _ptr(tril),
                                       status.data_ptr(), _stream_ptr(dev)), "gabo_mvn_sample")
    _raise_if_not_spd(status, "gabo_mvn_sample", message=_MVN_MESSAGE)
    out = out.reshape(shape + (m,))
    return (out, tril, status[1]) if return_scale_tril else out


def spd_acq_prepare_train(train_mandel):
    """Entry-major Cholesky factors of the training matrices for spd_acq_eval (d_vec x n)."""
    lib = _lib.load()
    x = train_mandel.contiguous()
    n, dv = x.shape
    d = _mandel_dim(dv)
    out = torch.empty(dv, n, dtype=torch.float64, device=x.device)
    status = _status_word(x.device)
    with _on(x.device):
        _lib.check(lib.gabo_spd_acq_prepare_train(x.data_ptr(), out.data_ptr(), n, d, status.data_ptr(), _stream_ptr(x.device)),
                   "gabo_spd_acq_prepare_train")
    _raise_if_not_spd(status, "gabo_spd_acq_prepare_train")
    return out


def spd_acq_eval(x_mandel, train_factors, alpha, linv, linv_t, beta, mode, mean, outputscale, kxx, best_f, kind, maximize,
                 out_sign=1.0, need_grad=True, active_ptr=None, out=None):
    """Single-launch acquisition value (R) and Euclidean gradient (R x d_vec, Mandel) at SPD candidates."""
    lib = _lib.load()
    dev = _device_for(train_factors, x_mandel)
    x = _prep(x_mandel, dev).contiguous()
    _require(dev, train_factors=train_factors, alpha=alpha, linv=linv, linv_t=linv_t)
    r, dv = x.shape
    n = train_factors.shape[1]
    if out is not None:           # (value, grad) buffers to update in place: masked candidates keep their previous entries
        value, grad = out
    else:
        value = torch.empty(r, dtype=torch.float64, device=dev)
        grad = torch.empty_like(x) if need_grad else None
    affine = (int(mode) & 24) == 0           # only the affine-invariant metric spills logm(M_j) to scratch
    scratch = torch.empty(r * dv * n, dtype=torch.float64, device=dev) if (need_grad and affine) else None
    status = _status_word(dev)
    ptr = lambda t_: None if t_ is None else t_.data_ptr()   # noqa: E731
    with _on(dev):
        _lib.check(lib.gabo_spd_acq_eval(x.data_ptr(), train_factors.data_ptr(), alpha.data_ptr(), ptr(linv), ptr(linv_t),
                                         value.data_ptr(), ptr(grad), ptr(scratch), r, n, _mandel_dim(dv), float(beta), int(mode),
                                         float(mean), float(outputscale), float(kxx), float(best_f), int(kind), 1 if maximize else 0,
                                         float(out_sign), active_ptr, status.data_ptr(), _stream_ptr(dev)), "gabo_spd_acq_eval")
    _raise_if_not_spd(status, "gabo_spd_acq_eval")
    return value, grad


def spd_sample(n, d, min_eig, max_eig, seed, device, mandel=False, first=0):
    """n random SPD matrices (n, d, d) - or Mandel vectors (n, d_vec) - drawn on the device with spd_sample's distribution: samples
    first ... first + n - 1 of the stream keyed by `seed` (a rank's shard of the raw samples when first > 0)."""
    lib = _lib.load()
    dev = torch.device(device)
    out = torch.empty((n, d * (d + 1) // 2) if mandel else (n, d, d), dtype=torch.float64, device=dev)
    with _on(dev):
        _lib.check(lib.gabo_spd_sample_range(out.data_ptr(), int(first), n, d, float(min_eig), float(max_eig), int(seed) & 0xFFFFFFFFFFFFFFFF,
                                             1 if mandel else 0, _stream_ptr(dev)), "gabo_spd_sample_range")
    return out


def nested_sphere_epilogue(rotated, dist_to_axis, mode=0):
    """Per-point part of the nested-sphere projection on already rotated points (..., d) -> (..., d-1) [mode 0] / (..., d) [mode 1]."""
    lib = _lib.load()
    out_device, dev, u = _dense(rotated)
    d = u.shape[-1]
    n = u.numel() // d
    out = torch.empty(u.shape[:-1] + ((d - 1) if mode == 0 else d,), dtype=torch.float64, device=dev)
    with _on(dev):
        _lib.check(lib.gabo_nested_sphere_epilogue(u.data_ptr(), out.data_ptr(), n, d, float(dist_to_axis), int(mode), _stream_ptr(dev)),
                   "gabo_nested_sphere_epilogue")
    return _out(out, out_device)


def nested_sphere_epilogue_backward(rotated, grad_out, dist_to_axis):
    lib = _lib.load()
    out_device, dev, u = _dense(rotated, grad_out)
    g = _prep(grad_out, dev).contiguous()
    d = u.shape[-1]
    gu = torch.empty_like(u)
    with _on(dev):
        _lib.check(lib.gabo_nested_sphere_epilogue_backward(u.data_ptr(), g.data_ptr(), gu.data_ptr(), u.numel() // d, d,
                                                            float(dist_to_axis), _stream_ptr(dev)), "gabo_nested_sphere_epilogue_backward")
    return _out(gu, out_device)


class _NestedSphereEpilogue(torch.autograd.Function):
    """mode-0 epilogue, differentiable (first order) in the rotated points."""

    @staticmethod
    def forward(ctx, u, dist):
        ctx.save_for_backward(u)
        ctx.dist = float(dist)
        return nested_sphere_epilogue(u, ctx.dist, 0).to(u.dtype)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        (u,) = ctx.saved_tensors
        return nested_sphere_epilogue_backward(u, g, ctx.dist).to(u.dtype), None


def pack_nested_sphere_axes(sphere_axes, dim):
    """[axis of S^(dim-1) (dim entries), axis of the next subsphere (dim - 1 entries), ...] -> one float64 numpy vector, level after level
    (the layout of gabo_nested_sphere_frames / _reconstruction / _fit_evaluate)."""
    import numpy as np
    parts = []
    for k, a in enumerate(sphere_axes):
        v = (a.detach().cpu().double().numpy() if torch.is_tensor(a) else np.asarray(a, dtype=np.float64)).reshape(-1)
        if v.size != dim - k:
            raise RuntimeError(f"nested-sphere axis of level {k} must have {dim - k} entries, got {v.size}")
        parts.append(v)
    return np.ascontiguousarray(np.concatenate(parts))


def _nested_sphere_frames(sphere_axes, sphere_distances, dim, dev):
    """(frames, distances) device tensors of the fused nested-sphere launches from the lists the reference's functions take."""
    lib = _lib.load()
    levels = len(sphere_axes)
    axes = torch.cat([a.detach().reshape(-1).to(dev, torch.float64) for a in sphere_axes])
    if axes.numel() != levels * dim - levels * (levels - 1) // 2:
        raise RuntimeError("nested-sphere axes: level k must have dim - k entries")
    dists = torch.cat([(d.detach().reshape(-1)[:1].to(dev, torch.float64) if torch.is_tensor(d)
                        else torch.tensor([float(d)], dtype=torch.float64, device=dev)) for d in sphere_distances])
    frames = torch.empty(axes.numel() + 2 * levels, dtype=torch.float64, device=dev)
    with _on(dev):
        _lib.check(lib.gabo_nested_sphere_frames(axes.data_ptr(), frames.data_ptr(), dim, levels, _stream_ptr(dev)), "gabo_nested_sphere_frames")
    return frames, dists


def _level_offsets(dim, levels):
    return [k * dim - k * (k - 1) // 2 for k in range(levels + 1)]


def nested_sphere_project_all(x, sphere_axes, sphere_distances):
    """projection_from_sphere_to_subsphere (nested_spheres_utils.py:117-146) in one launch, no autograd: x (N, D) -> the list
    [x, x_{D-1}, ..., x_{D-levels}] of the points on every nested subsphere."""
    lib = _lib.load()
    dev = _device_for(x)
    X = _prep(x, dev).contiguous()
    n, dim = int(X.shape[0]), int(X.shape[1])
    levels = len(sphere_axes)
    frames, dists = _nested_sphere_frames(sphere_axes, sphere_distances, dim, dev)
    off = _level_offsets(dim, levels)
    z = torch.empty(n, dim - levels, dtype=torch.float64, device=dev)
    store = torch.empty(n, off[-1], dtype=torch.float64, device=dev)
    with _on(dev):
        _lib.check(lib.gabo_nested_sphere_project(X.data_ptr(), frames.data_ptr(), dists.data_ptr(), z.data_ptr(), store.data_ptr(), n, dim, levels,
                                                  _stream_ptr(dev)), "gabo_nested_sphere_project")
    return [store[:, off[k]:off[k + 1]] for k in range(levels)] + [z]


def nested_sphere_lift_all(x_subsphere, sphere_axes, sphere_distances):
    """projection_from_subsphere_to_sphere (nested_spheres_utils.py:182-218) in one launch, no autograd: x_subsphere (N, D - levels) -> the
    list [x_subsphere, x_{D-levels+1}, ..., x_D] (the axes are used in reverse order, as in the reference)."""
    lib = _lib.load()
    dev = _device_for(x_subsphere)
    Z = _prep(x_subsphere, dev).contiguous()
    levels = len(sphere_axes)
    n, dim = int(Z.shape[0]), int(Z.shape[1]) + levels
    frames, dists = _nested_sphere_frames(sphere_axes, sphere_distances, dim, dev)
    off = _level_offsets(dim, levels)
    store = torch.empty(n, off[-1], dtype=torch.float64, device=dev)
    with _on(dev):
        _lib.check(lib.gabo_nested_sphere_lift(Z.data_ptr(), frames.data_ptr(), dists.data_ptr(), None, store.data_ptr(), n, dim, levels,
                                               _stream_ptr(dev)), "gabo_nested_sphere_lift")
    return [Z] + [store[:, off[k]:off[k + 1]] for k in range(levels - 1, -1, -1)]


class NestedSphereReconstruction:
    """min_error_reconstruction_cost (nested_spheres_optimization.py:20-38) for FIXED data, subsphere points and axes, as a function of the
    distances to the axes: value and gradient of P parameter sets in one launch (gabo_nested_sphere_reconstruction)."""

    def __init__(self, x_data, x_subsphere, sphere_axes):
        lib = _lib.load()
        dev = self.device = _device_for(x_data, x_subsphere)
        self.x = _prep(x_data, dev).contiguous()
        self.z = _prep(x_subsphere, dev).contiguous()
        self.N, self.D = int(self.x.shape[0]), int(self.x.shape[1])
        self.L = self.D - int(self.z.shape[1])
        if self.x.dim() != 2 or self.z.dim() != 2 or self.z.shape[0] != self.N or self.L < 1 or len(sphere_axes) != self.L:
            raise RuntimeError(f"shapes: x_data {tuple(self.x.shape)}, x_subsphere {tuple(self.z.shape)}, {len(sphere_axes)} axes")
        axes = torch.as_tensor(pack_nested_sphere_axes(sphere_axes, self.D), device=dev)
        self.frames = torch.empty(axes.numel() + 2 * self.L, dtype=torch.float64, device=dev)
        with _on(dev):
            _lib.check(lib.gabo_nested_sphere_frames(axes.data_ptr(), self.frames.data_ptr(), self.D, self.L, _stream_ptr(dev)), "gabo_nested_sphere_frames")
        self._buffers = {}

    def evaluate(self, distances, grad=True):
        """distances: (P, L) or (L,) numpy -> cost (P,) [, d cost / d distances (P, L)] as numpy (one copy in, one launch, one copy out)."""
        import numpy as np
        lib = _lib.load()
        r = np.asarray(distances, dtype=np.float64)
        single = r.ndim == 1
        r = np.ascontiguousarray(r.reshape(-1, self.L))
        P = r.shape[0]
        ent = self._buffers.get(P)
        if ent is None:
            ws = max(int(lib.gabo_nested_sphere_reconstruction_workspace_bytes(P, max(self.N, 1), self.D, self.L)), 16)
            ent = self._buffers[P] = dict(hin=_pinned(P * self.L), hout=_pinned(P * (1 + self.L)),
                                          din=torch.empty(P * self.L, dtype=torch.float64, device=self.device),
                                          dout=torch.empty(P * (1 + self.L), dtype=torch.float64, device=self.device),
                                          ws=torch.empty(ws, dtype=torch.uint8, device=self.device))
        ent["hin"].numpy()[:] = r.ravel()
        ent["din"].copy_(ent["hin"], non_blocking=True)
        dout = ent["dout"]
        with torch.cuda.device(self.device):
            _lib.check(lib.gabo_nested_sphere_reconstruction(self.x.data_ptr(), self.z.data_ptr(), self.frames.data_ptr(), ent["din"].data_ptr(),
                                                             dout.data_ptr(), dout[P:].data_ptr() if grad else None, P, self.N, self.D, self.L,
                                                             ent["ws"].data_ptr(), ent["ws"].numel(), _stream_ptr(self.device)),
                       "gabo_nested_sphere_reconstruction")
        ent["hout"].copy_(dout, non_blocking=True)
        torch.cuda.current_stream(self.device).synchronize()
        out = ent["hout"].numpy()
        cost = out[:P].copy()
        if not grad:
            return cost[0] if single else cost
        g = out[P:].reshape(P, self.L).copy()
        return (cost[0], g[0]) if single else (cost, g)


def nested_sphere_next(rotated, dist_to_axis):
    """Differentiable mode-0 epilogue."""
    if rotated.requires_grad:
        return _NestedSphereEpilogue.apply(rotated, float(dist_to_axis))
    return nested_sphere_epilogue(rotated, dist_to_axis, 0)


class SpdTcg:
    """Device-resident truncated CG of the SPD trust regions (gabo_spd_tcg_*): thin handle around the workspace."""

    def __init__(self, r, d, n_constraints, device):
        self.lib = _lib.load()
        self.r, self.d, self.c, self.dev = int(r), int(d), int(n_constraints), device
        self.wsb = self.lib.gabo_spd_tcg_workspace_bytes(self.r, self.d, self.c)
        self.ws = torch.zeros(self.wsb // 8 + 1, dtype=torch.float64, device=device)
        self.x_fd = torch.empty(self.r, d * (d + 1) // 2, dtype=torch.float64, device=device)
        self.any_running = torch.zeros(1, dtype=torch.int32, device=device)
        self.running_ptr = self.ws.data_ptr() + self.lib.gabo_spd_tcg_running_offset(self.r, self.d, self.c)
        self.status = torch.zeros(2, dtype=torch.int32, device=device)

    def begin(self, x, g, gc, fc, active, Delta):
        ptr = lambda t_: None if t_ is None else t_.data_ptr()   # noqa: E731
        self._keep = (x.contiguous(), g.contiguous(), None if gc is None else gc.contiguous(), None if fc is None else fc.contiguous(),
                      active.to(torch.uint8).contiguous(), Delta.contiguous())
        xx, gg, gcc, fcc, act, dl = self._keep
        with _on(self.dev):
            _lib.check(self.lib.gabo_spd_tcg_begin(xx.data_ptr(), gg.data_ptr(), ptr(gcc), ptr(fcc), act.data_ptr(), dl.data_ptr(),
                                                   self.ws.data_ptr(), self.wsb, self.r, self.d, self.c, self.status.data_ptr(),
                                                   _stream_ptr(self.dev)), "gabo_spd_tcg_begin")

    def begin_rand(self, eta0, heta0):
        """use_rand (robust_trust_regions.py:173-181, 407-452), after begin(): start from eta0 with heta0 = hess(x, eta0), no preconditioner."""
        self._keep_rand = (eta0.contiguous(), heta0.contiguous())
        _require(self.dev, eta0=self._keep_rand[0], heta0=self._keep_rand[1])
        with _on(self.dev):
            _lib.check(self.lib.gabo_spd_tcg_begin_rand(self.ws.data_ptr(), self._keep_rand[0].data_ptr(), self._keep_rand[1].data_ptr(),
                                                        self.r, self.d, self.c, _stream_ptr(self.dev)), "gabo_spd_tcg_begin_rand")

    def fd_point(self):
        with _on(self.dev):
            _lib.check(self.lib.gabo_spd_tcg_fd_point(self.ws.data_ptr(), self.x_fd.data_ptr(), self.r, self.d, self.c,
                                                      _stream_ptr(self.dev)), "gabo_spd_tcg_fd_point")
        return self.x_fd

    def step(self, egrad_mandel, neq, delta_cons, theta, kappa, mininner):
        eg = egrad_mandel.contiguous()
        with _on(self.dev):
            _lib.check(self.lib.gabo_spd_tcg_step(self.ws.data_ptr(), eg.data_ptr(), self.any_running.data_ptr(), self.r, self.d,
                                                  self.c, int(neq), float(delta_cons), float(theta), float(kappa), int(mininner),
                                                  _stream_ptr(self.dev)), "gabo_spd_tcg_step")

    def end(self):
        eta = torch.empty(self.r, self.d, self.d, dtype=torch.float64, device=self.dev)
        heta = torch.empty_like(eta)
        stop = torch.empty(self.r, dtype=torch.int32, device=self.dev)
        with _on(self.dev):
            _lib.check(self.lib.gabo_spd_tcg_end(self.ws.data_ptr(), eta.data_ptr(), heta.data_ptr(), stop.data_ptr(), self.r,
                                                 self.d, self.c, _stream_ptr(self.dev)), "gabo_spd_tcg_end")
        return eta, heta, stop.long()


class SpdTr:
    """Device-resident trust-region iteration (gabo_spd_tr_propose / gabo_spd_tr_update) on persistent state tensors."""

    def __init__(self, r, d, n_constraints, acq_params, n_train, device):
        import ctypes
        self.lib = _lib.load()
        self.r, self.d, self.c, self.n, self.dev = int(r), int(d), int(n_constraints), int(n_train), device
        self.acq = acq_params                      # _lib.AcqParams; the tensors it points to are owned by the caller
        self.acq_ref = ctypes.byref(self.acq)
        self.wsb = self.lib.gabo_spd_tr_workspace_bytes(self.r, self.d, self.c, self.n)
        self.ws = torch.zeros(self.wsb // 8 + 1, dtype=torch.float64, device=device)
        self.x_prop = torch.zeros(self.r, d, d, dtype=torch.float64, device=device)
        self.any_active = torch.ones(1, dtype=torch.int32, device=device)
        self.status = torch.zeros(2, dtype=torch.int32, device=device)

    def propose(self, x, g, Delta, active, gc, fc, neq, delta_cons, theta, kappa, mininner, maxinner):
        _require(self.dev, x=x, g=g, Delta=Delta, active=active, gc=gc, fc=fc)
        ptr = lambda t_: None if t_ is None else t_.data_ptr()   # noqa: E731
        with _on(self.dev):
            _lib.check(self.lib.gabo_spd_tr_propose(x.data_ptr(), g.data_ptr(), Delta.data_ptr(), active.data_ptr(), ptr(gc), ptr(fc),
                                                    self.acq_ref, self.ws.data_ptr(), self.wsb, self.x_prop.data_ptr(), self.r, self.d,
                                                    self.c, int(neq), float(delta_cons), float(theta), float(kappa), int(mininner),
                                                    int(maxinner), self.any_active.data_ptr(), self.status.data_ptr(),
                                                    _stream_ptr(self.dev)), "gabo_spd_tr_propose")
        return self.x_prop

    def solve(self, x, fx, g, ng, Delta, active, iters, kinds, bounds, strict, delta_cons, theta, kappa, mininner, maxinner, delta_bar,
              rho_prime, rho_regularization, mingradnorm, maxiter, lift=None, record=None):
        """The whole solve in one launch (built-in eigenvalue constraints `kinds`/`bounds`, or none).  lift: the (w, x0, p) of
        nested_spd_lift_prepare when some kinds are the nested ones (bounds stated in the original space of a nested SPD mapping).
        record: (K, r, d*d + 2) tensor pre-filled with NaN -> per-iteration record of the launch (gabo_tr_solve_record)."""
        _require(self.dev, x=x, fx=fx, g=g, ng=ng, Delta=Delta, active=active, iters=iters, record=record)
        import ctypes
        nc = len(kinds)
        ck = (ctypes.c_int * max(nc, 1))(*kinds)
        cb = (ctypes.c_double * max(nc, 1))(*bounds)
        if lift is not None:
            lw, lx0, lp = lift                         # (the order nested_spd_lift_prepare returns them in)
            _require(self.dev, lift_w=lw, lift_p=lp, lift_x0=lx0)
            self._lift_ref = lift                      # (keeps the buffers alive until the next solve)
            lift_args = (lw.data_ptr(), lp.data_ptr(), lx0.data_ptr(), int(lw.shape[0]))
        else:
            lift_args = (None, None, None, 0)
        with _on(self.dev):
            if record is not None:
                assert tuple(record.shape[1:]) == (self.r, self.d * self.d + 2)
                _lib.check(self.lib.gabo_tr_solve_record(record.data_ptr(), int(record.shape[0])), "gabo_tr_solve_record")
            _lib.check(self.lib.gabo_spd_tr_solve(x.data_ptr(), fx.data_ptr(), g.data_ptr(), ng.data_ptr(), Delta.data_ptr(),
                                                  active.data_ptr(), iters.data_ptr(), self.acq_ref, nc, ck, cb, 1 if strict else 0,
                                                  self.ws.data_ptr(), self.wsb, self.r, self.d, float(delta_cons), float(theta),
                                                  float(kappa), int(mininner), int(maxinner), float(delta_bar), float(rho_prime),
                                                  float(rho_regularization), float(mingradnorm), int(maxiter), *lift_args,
                                                  self.status.data_ptr(), _stream_ptr(self.dev)), "gabo_spd_tr_solve")

    def update(self, x, fx, g, ng, Delta, active, iters, invalid, delta_bar, rho_prime, rho_regularization, mingradnorm, maxiter):
        _require(self.dev, x=x, fx=fx, g=g, ng=ng, Delta=Delta, active=active, iters=iters, invalid=invalid)
        with _on(self.dev):
            _lib.check(self.lib.gabo_spd_tr_update(x.data_ptr(), fx.data_ptr(), g.data_ptr(), ng.data_ptr(), Delta.data_ptr(),
                                                   active.data_ptr(), iters.data_ptr(), None if invalid is None else invalid.data_ptr(),
                                                   self.x_prop.data_ptr(), self.ws.data_ptr(), self.r, self.d, self.c, self.n,
                                                   float(delta_bar), float(rho_prime), float(rho_regularization), float(mingradnorm),
                                                   int(maxiter), self.any_active.data_ptr(), _stream_ptr(self.dev)), "gabo_spd_tr_update")


def sphere_acq_eval(x, acq_params, need_grad=True):
    """Single-launch acquisition value (R) and Euclidean gradient (R x dim) at points of the sphere; acq_params: _lib.SphereAcqParams."""
    import ctypes
    lib = _lib.load()
    dev = _device_for(x)
    xx = _prep(x, dev).contiguous()           # a float32 / host tensor would otherwise be read as fp64 device memory
    r = xx.shape[0]
    value = torch.empty(r, dtype=torch.float64, device=dev)
    grad = torch.empty_like(xx) if need_grad else None
    with _on(dev):
        _lib.check(lib.gabo_sphere_acq_eval(xx.data_ptr(), ctypes.byref(acq_params), value.data_ptr(), None if grad is None else grad.data_ptr(),
                                            r, _stream_ptr(dev)), "gabo_sphere_acq_eval")
    return value, grad


class SphereTr:
    """Device-resident trust-region iteration on the sphere (gabo_sphere_tr_*): same interface as SpdTr."""

    def __init__(self, r, dim, n_constraints, acq_params, device, exact_hessian=False):
        import ctypes
        self.lib = _lib.load()
        self.r, self.d, self.c, self.dev = int(r), int(dim), int(n_constraints), device
        self.exact = 1 if exact_hessian else 0
        self.acq = acq_params
        self.acq_ref = ctypes.byref(self.acq)
        self.wsb = self.lib.gabo_sphere_tr_workspace_bytes(self.r, self.d, self.c)
        self.ws = torch.zeros(self.wsb // 8 + 1, dtype=torch.float64, device=device)
        self.x_prop = torch.zeros(self.r, dim, dtype=torch.float64, device=device)
        self.any_active = torch.ones(1, dtype=torch.int32, device=device)

    def propose(self, x, g, Delta, active, gc, fc, neq, delta_cons, theta, kappa, mininner, maxinner):
        _require(self.dev, x=x, g=g, Delta=Delta, active=active, gc=gc, fc=fc)
        ptr = lambda t_: None if t_ is None else t_.data_ptr()   # noqa: E731
        with _on(self.dev):
            _lib.check(self.lib.gabo_sphere_tr_propose(x.data_ptr(), g.data_ptr(), Delta.data_ptr(), active.data_ptr(), ptr(gc), ptr(fc),
                                                       self.acq_ref, self.ws.data_ptr(), self.wsb, self.x_prop.data_ptr(), self.r, self.c,
                                                       int(neq), float(delta_cons), float(theta), float(kappa), int(mininner),
                                                       int(maxinner), self.exact, self.any_active.data_ptr(), _stream_ptr(self.dev)),
                       "gabo_sphere_tr_propose")
        return self.x_prop

    def update(self, x, fx, g, ng, Delta, active, iters, invalid, delta_bar, rho_prime, rho_regularization, mingradnorm, maxiter):
        _require(self.dev, x=x, fx=fx, g=g, ng=ng, Delta=Delta, active=active, iters=iters, invalid=invalid)
        with _on(self.dev):
            _lib.check(self.lib.gabo_sphere_tr_update(x.data_ptr(), fx.data_ptr(), g.data_ptr(), ng.data_ptr(), Delta.data_ptr(),
                                                      active.data_ptr(), iters.data_ptr(), None if invalid is None else invalid.data_ptr(),
                                                      self.ws.data_ptr(), self.r, self.d, self.c, float(delta_bar), float(rho_prime),
                                                      float(rho_regularization), float(mingradnorm), int(maxiter),
                                                      self.any_active.data_ptr(), _stream_ptr(self.dev)), "gabo_sphere_tr_update")

    def solve(self, x, fx, g, ng, Delta, active, iters, kinds, bounds, strict, delta_cons, theta, kappa, mininner, maxinner, delta_bar,
              rho_prime, rho_regularization, mingradnorm, maxiter, record=None, indices=(), centres=None, n_equalities=0):
        """The whole solve in one launch, without constraints or with the library's own sphere constraints (`kinds` / `indices` / `bounds`
        and the balls' `centres` as sphere_constraints_utils_torch.builtin_sphere_group packs them, the `n_equalities` equalities first).
        record: (K, r, dim + 2) tensor pre-filled with NaN -> per-iteration record of the launch (gabo_tr_solve_record)."""
        _require(self.dev, x=x, fx=fx, g=g, ng=ng, Delta=Delta, active=active, iters=iters, record=record, centres=centres)
        import ctypes
        nc = len(kinds)
        if nc != self.c or len(indices) != nc or len(bounds) != nc:
            raise ValueError(f"{nc} constraint kinds, {len(indices)} indices and {len(bounds)} bounds for a workspace of {self.c} constraints")
        ck = (ctypes.c_int * max(nc, 1))(*kinds)
        ci = (ctypes.c_int * max(nc, 1))(*indices)
        cb = (ctypes.c_double * max(nc, 1))(*bounds)
        if centres is not None and (centres.dim() != 2 or centres.shape[1] != self.d):
            raise ValueError("centres: n_centres x dim")
        with _on(self.dev):
            if record is not None:                     # (K, r, dim + 2), pre-filled with NaN: gabo_tr_solve_record
                assert tuple(record.shape[1:]) == (self.r, self.d + 2)
                _lib.check(self.lib.gabo_tr_solve_record(record.data_ptr(), int(record.shape[0])), "gabo_tr_solve_record")
            _lib.check(self.lib.gabo_sphere_tr_solve_constrained(
                x.data_ptr(), fx.data_ptr(), g.data_ptr(), ng.data_ptr(), Delta.data_ptr(), active.data_ptr(), iters.data_ptr(), self.acq_ref,
                self.ws.data_ptr(), self.wsb, self.r, float(theta), float(kappa), int(mininner), int(maxinner), self.exact, float(delta_bar),
                float(rho_prime), float(rho_regularization), float(mingradnorm), int(maxiter), nc, int(n_equalities), ck, ci, cb,
                None if centres is None else centres.data_ptr(), 0 if centres is None else int(centres.shape[0]), 1 if strict else 0,
                float(delta_cons), _stream_ptr(self.dev)), "gabo_sphere_tr_solve_constrained")

    def lds_resident(self):
        """whether solve() keeps the surrogate and the restart's workspace in LDS (gabo_sphere_tr_solve_lds_resident)"""
        rc = self.lib.gabo_sphere_tr_solve_lds_resident(self.acq_ref, self.r, self.c)
        if rc < 0:
            _lib.check(rc, "gabo_sphere_tr_solve_lds_resident")
        return bool(rc)


def sphere_constraints_eval(x, kinds, indices, bounds, centres=None, want_grad=True):
    """Values (R x C) and, want_grad, Riemannian gradients (C x R x dim) of the library's own sphere constraints at the R points x (R x dim)
    in one launch (gabo_sphere_constraints_eval); the arguments as sphere_constraints_utils_torch.builtin_sphere_group packs them."""
    import ctypes
    lib = _lib.load()
    dev = _device_for(x)
    xx = _prep(x, dev).contiguous()
    if xx.dim() != 2:
        raise ValueError("x: R x dim")
    r, dim, nc = xx.shape[0], xx.shape[1], len(kinds)
    if len(indices) != nc or len(bounds) != nc:
        raise ValueError("kinds, indices and bounds: one entry per constraint")
    if centres is not None:
        centres = _prep(centres, dev).contiguous()
        if centres.dim() != 2 or centres.shape[1] != dim:
            raise ValueError("centres: n_centres x dim")
    values = torch.empty(r, nc, dtype=torch.float64, device=dev)
    grads = torch.empty(nc, r, dim, dtype=torch.float64, device=dev) if want_grad else None
    ck = (ctypes.c_int * max(nc, 1))(*kinds)
    ci = (ctypes.c_int * max(nc, 1))(*indices)
    cb = (ctypes.c_double * max(nc, 1))(*bounds)
    with _on(dev):
        _lib.check(lib.gabo_sphere_constraints_eval(xx.data_ptr(), r, dim, nc, ck, ci, cb, _ptr(centres),
                                                    0 if centres is None else int(centres.shape[0]), values.data_ptr(), _ptr(grads),
                                                    _stream_ptr(dev)), "gabo_sphere_constraints_eval")
    return (values, grads) if want_grad else values


def sphere_sample(count, dim, seed, constraints=None, device=None):
    """count points uniform on S^(dim-1) inside the library's INEQUALITY constraints, drawn on the device by rejection (gabo_sphere_sample: try t of
    sample i is item i + t * count of the library's Philox stream `seed`; without constraints the stream's first count points).  constraints: None, a
    list of the library's sphere constraints (functools.partial with every parameter by keyword) or the (kinds, indices, bounds, centres) that
    sphere_constraints_utils_torch.builtin_sphere_group packs.  Returns (points count x dim, exhausted): exhausted = some sample was still infeasible
    after GABO_SPHERE_SAMPLE_MAX_TRIES tries and holds its last try."""
    import ctypes
    lib = _lib.load()
    dev = _device_for() if device is None else torch.device(device)
    count, dim = int(count), int(dim)
    if constraints is None or len(constraints) == 0:
        kinds, indices, bounds, centres = [], [], [], None
    elif len(constraints) == 4 and isinstance(constraints[0], (list, tuple)) and not callable(constraints[0]):
        kinds, indices, bounds, centres = constraints
    else:
        from .Riemannian_utils.sphere_constraints_utils_torch import builtin_sphere_group
        group = builtin_sphere_group(list(constraints), dim, dev)
        if group is None:
            raise ValueError("sphere_sample: every constraint must be one of the library's sphere constraints with its parameters bound by keyword "
                             "(at most 8 of them)")
        kinds, indices, bounds, centres = group
    nc = len(kinds)
    if len(indices) != nc or len(bounds) != nc:
        raise ValueError("kinds, indices and bounds: one entry per constraint")
    if centres is not None:
        centres = _prep(centres, dev).contiguous()
        if centres.dim() != 2 or centres.shape[1] != dim:
            raise ValueError("centres: n_centres x dim")
    out = torch.empty(count, dim, dtype=torch.float64, device=dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    ck = (ctypes.c_int * max(nc, 1))(*kinds)
    ci = (ctypes.c_int * max(nc, 1))(*indices)
    cb = (ctypes.c_double * max(nc, 1))(*bounds)
    with _on(dev):
        _lib.check(lib.gabo_sphere_sample(out.data_ptr(), count, dim, int(seed) & 0xFFFFFFFFFFFFFFFF, nc, 0, ck, ci, cb,
                                          _ptr(centres), 0 if centres is None else int(centres.shape[0]), flag.data_ptr(), _stream_ptr(dev)),
                   "gabo_sphere_sample")
    return out, bool(flag.item())


def sphere_manifold_op(op, x, u, v=None, w=None):
    """Batched sphere-manifold operation (one of _lib.GABO_SPH_*) on (..., dim) tensors."""
    lib = _lib.load()
    first = torch.as_tensor(x)
    out_device = first.device
    dev = _device_for(*[torch.as_tensor(t_) for t_ in (x, u, v, w) if t_ is not None])
    ts = [None if t_ is None else _prep(torch.as_tensor(t_), dev) for t_ in (x, u, v, w)]
    shape = torch.broadcast_shapes(*[t_.shape for t_ in ts if t_ is not None])
    X, U, V, W = [None if t_ is None else t_.expand(shape).contiguous() for t_ in ts]
    dim = shape[-1]
    n = X.numel() // dim
    out = torch.empty(shape[:-1] if op == _lib.GABO_SPH_DIST else shape, dtype=torch.float64, device=dev)
    with _on(dev):
        _lib.check(lib.gabo_sphere_manifold_op(int(op), _ptr(X), _ptr(U), _ptr(V), _ptr(W), out.data_ptr(), n, dim, _stream_ptr(dev)),
                   "gabo_sphere_manifold_op")
    return _out(out, out_device)


# ------------------------------------------------------------------------------------------ Frechet / Karcher means
GABO_SPD_MEAN_FUSED_MAX_DIM = 10          # the fused kernels of csrc/riemannian_mean.hip; above: the composed device path


def _mean_args(x, weights, start, tail, dev):
    """(..., N, tail) points with optional (..., N) weights and (..., tail) start -> contiguous (B, N, tail), (B, N) | None, (B, tail) | None"""
    xs = _prep(torch.as_tensor(x), dev)
    if xs.dim() < 2 or xs.shape[-2] < 1:
        raise RuntimeError(f"a mean needs (..., N, {tail}) points with N >= 1, got {tuple(xs.shape)}")
    bshape = xs.shape[:-2]
    n = xs.shape[-2]
    xs = xs.reshape(-1, n, xs.shape[-1]).contiguous()
    w = s = None
    if weights is not None:
        w = _prep(torch.as_tensor(weights), dev)
        if w.shape != bshape + (n,):
            raise RuntimeError(f"weights {tuple(w.shape)} do not match the points {tuple(bshape + (n,))}")
        w = w.reshape(-1, n).contiguous()
    if start is not None:
        s = _prep(torch.as_tensor(start), dev)
        if s.shape != bshape + (xs.shape[-1],):
            raise RuntimeError(f"start {tuple(s.shape)} does not match the points {tuple(bshape + (xs.shape[-1],))}")
        s = s.reshape(-1, xs.shape[-1]).contiguous()
    return xs, w, s, bshape


def _spd_mean_message(nb, n):
    def message(st):
        if st[1] >= nb * n:
            return f"gabo_spd_frechet_mean: the start point / an iterate of set #{st[1] - nb * n} is not positive definite (Cholesky pivot <= 0)"
        return f"gabo_spd_frechet_mean: input matrix #{st[1]} is not positive definite (Cholesky pivot <= 0)"
    return message


def _spd_frechet_mean_composed(xs, w, s, iters, d):
    """The mean from the library's batched launches: whiten with torch, one logm launch over the N matrices, a weighted sum, one expm launch, the
    congruence - per iteration, nothing read back.  Serves 11 <= d <= GABO_SPD_MAX_DIM and is the second device implementation the fused kernels
    are compared with.  Returns (mean, residuals, status): a status word of the ring (taken after the inner launches have taken theirs), written on
    the device as gabo_spd_frechet_mean writes it - {GABO_ERR_NOT_SPD, index of the
    first data matrix that is not positive definite (a failed Cholesky pivot or a NaN entry), or B N + the set whose start point / iterate failed}."""
    nb, n = xs.shape[:2]
    X = mandel_to_matrix(xs)                                                     # (B, N, d, d)
    m = X[:, 0] if s is None else mandel_to_matrix(s)
    wn = torch.full((nb, n), 1.0 / n, dtype=torch.float64, device=xs.device) if w is None else w / w.sum(-1, keepdim=True)
    resid = torch.empty(nb, iters, dtype=torch.float64, device=xs.device)
    bad_x = ((torch.linalg.cholesky_ex(X).info != 0) | torch.isnan(xs).any(-1)).reshape(-1)
    bad_m = torch.zeros(nb, dtype=torch.bool, device=xs.device)
    for it in range(iters + 1):
        L, info = torch.linalg.cholesky_ex(m)                                   # (info stays on the device)
        bad_m |= (info != 0) | torch.isnan(m).any(-1).any(-1)
        if it == iters:
            break
        Y = torch.linalg.solve_triangular(L[:, None], X, upper=False)           # L^-1 X
        M = torch.linalg.solve_triangular(L[:, None], Y.transpose(-1, -2), upper=False)     # L^-1 (L^-1 X)^T = L^-1 X L^-T
        M = 0.5 * (M + M.transpose(-1, -2))
        logs = spd_manifold_op(_lib.GABO_SPD_LOGM, M)
        # (a point of weight 0 is skipped, as in the fused kernels: its logarithm - NaN included - stays out of the sum)
        S = torch.where((wn != 0)[:, :, None, None], wn[:, :, None, None] * logs, torch.zeros((), dtype=torch.float64, device=xs.device)).sum(1)
        resid[:, it] = torch.linalg.matrix_norm(S)
        E = spd_manifold_op(_lib.GABO_SPD_EXPM, S)
        m = torch.bmm(torch.bmm(L, E), L.transpose(-1, -2))
        m = 0.5 * (m + m.transpose(-1, -2))
    bad = torch.cat([bad_x, bad_m])
    first = bad.to(torch.int32).argmax().to(torch.int32)
    code = torch.where(bad.any(), torch.full_like(first, _lib.GABO_ERR_NOT_SPD), torch.zeros_like(first))
    mean = matrix_to_mandel(m)
    status = _status_word(xs.device)
    status.copy_(torch.stack([code, torch.where(bad.any(), first, torch.zeros_like(first))]))
    return mean, resid, status


def spd_frechet_mean(x_mandel, weights=None, iters=10, start=None, return_residual=False, fused=None):
    """Frechet mean under the affine-invariant metric of (N, d_vec) or (..., N, d_vec) Mandel vectors -> (d_vec,) or (..., d_vec), on the input's
    device (the reference's `mean` / `mean_mandel_vector`, spd_utils.py:235-287, for one or many sets).  weights (..., N): non-negative, normalised
    inside; start (..., d_vec): default the set's first point.  return_residual: also (..., iters), the norm of the mean tangent each iteration
    started from.  fused=None: the fused kernels for d <= 10, the composed device path for 11 <= d <= 32; fused=False forces the composed path."""
    lib = _lib.load()
    first = torch.as_tensor(x_mandel)
    out_device = first.device
    dev = _device_for(*[torch.as_tensor(t_) for t_ in (x_mandel, weights, start) if t_ is not None])
    iters = int(iters)
    if iters < 0:
        raise RuntimeError("iters must be >= 0")
    xs, w, s, bshape = _mean_args(x_mandel, weights, start, "d_vec", dev)
    d = _mandel_dim(xs.shape[-1])
    if d < 2 or d > _lib.GABO_SPD_MAX_DIM:
        raise RuntimeError(f"spd_frechet_mean: 2 <= d <= {_lib.GABO_SPD_MAX_DIM}, got {d}")
    nb, n = xs.shape[:2]
    if fused is None:
        fused = d <= GABO_SPD_MEAN_FUSED_MAX_DIM
    elif fused and d > GABO_SPD_MEAN_FUSED_MAX_DIM:
        raise RuntimeError(f"spd_frechet_mean: the fused kernels serve d <= {GABO_SPD_MEAN_FUSED_MAX_DIM}, got {d}")
    if nb == 0:
        mean, resid = xs.new_empty(0, xs.shape[-1]), xs.new_empty(0, iters)
    elif not fused:
        mean, resid, status = _spd_frechet_mean_composed(xs, w, s, iters, d)
        _raise_if_not_spd(status, "gabo_spd_frechet_mean", message=_spd_mean_message(nb, n))
    else:
        mean = torch.empty(nb, xs.shape[-1], dtype=torch.float64, device=dev)
        resid = torch.empty(nb, iters, dtype=torch.float64, device=dev) if return_residual else None
        wsb = lib.gabo_spd_frechet_mean_workspace_bytes(nb, n, d)
        ws = _workspace(wsb, dev)
        status = _status_word(dev)
        with _on(dev):
            rc = lib.gabo_spd_frechet_mean(xs.data_ptr(), _ptr(w), _ptr(s), mean.data_ptr(), _ptr(resid), nb, n, d, iters, ws.data_ptr(), wsb,
                                           status.data_ptr(), _stream_ptr(dev))
        _lib.check(rc, "gabo_spd_frechet_mean")
        _raise_if_not_spd(status, "gabo_spd_frechet_mean", message=_spd_mean_message(nb, n))
    mean = mean.reshape(bshape + (xs.shape[-1],))
    if return_residual:
        return _out(mean, out_device), resid.reshape(bshape + (iters,)).to(out_device)
    return _out(mean, out_device)


def sphere_karcher_mean(x, weights=None, iters=10, start=None, return_residual=False):
    """Karcher mean of (N, dim) or (..., N, dim) unit vectors -> (dim,) or (..., dim), on the input's device (the reference's
    `karcher_mean_sphere`, sphere_utils.py:126-149, for one or many sets; 2 <= dim <= 512).  weights, start, return_residual: as spd_frechet_mean."""
    lib = _lib.load()
    first = torch.as_tensor(x)
    out_device = first.device
    dev = _device_for(*[torch.as_tensor(t_) for t_ in (x, weights, start) if t_ is not None])
    iters = int(iters)
    if iters < 0:
        raise RuntimeError("iters must be >= 0")
    xs, w, s, bshape = _mean_args(x, weights, start, "dim", dev)
    nb, n, dim = xs.shape
    mean = torch.empty(nb, dim, dtype=torch.float64, device=dev)
    resid = torch.empty(nb, iters, dtype=torch.float64, device=dev) if return_residual else None
    if nb > 0:
        wsb = lib.gabo_sphere_karcher_mean_workspace_bytes(nb, n, dim)
        ws = _workspace(wsb, dev)
        with _on(dev):
            rc = lib.gabo_sphere_karcher_mean(xs.data_ptr(), _ptr(w), _ptr(s), mean.data_ptr(), _ptr(resid), nb, n, dim, iters, ws.data_ptr(), wsb,
                                              _stream_ptr(dev))
        _lib.check(rc, "gabo_sphere_karcher_mean")
    mean = mean.reshape(bshape + (dim,))
    if return_residual:
        return _out(mean, out_device), resid.reshape(bshape + (iters,)).to(out_device)
    return _out(mean, out_device)
