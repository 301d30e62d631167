"""The arguments the two-point-set wrappers of gabotorch_amd/ops.py hand to the library, pinned on the CPU: `_lib.load` is replaced by a stand-in
whose gabo_* entries record their positional arguments and return GABO_OK, the "device" is the CPU, the stream is 0 and the status words come
from a host ring.  Nothing here plays a kernel: outputs keep whatever their allocation held.  Pointers are compared with the data_ptr() of the
tensor they must belong to, never as numbers of their own."""
import numpy as np
import pytest
import torch

from gabotorch_amd import _lib, _status, ops

WSB = 4096                      # what every *_workspace_bytes entry of the stand-in answers
D, DV, N1, N2 = 2, 3, 3, 2      # d = 2 -> Mandel vectors of 3 entries
GAUSS, DIST, LAPLACE, SYM = _lib.GABO_OUT_GAUSSIAN, _lib.GABO_OUT_DISTANCE, _lib.GABO_OUT_LAPLACE, _lib.GABO_SYMMETRIC


class _AnyPointer:
    """a buffer the wrapper allocates and drops (the workspace): some address"""

    def __eq__(self, other):
        return isinstance(other, int) and other != 0

    def __repr__(self):
        return "<some pointer>"


SOME = _AnyPointer()


class _Library:
    def __init__(self):
        self.calls, self.sizes = [], []

    def __getattr__(self, name):
        if not name.startswith("gabo_"):
            raise AttributeError(name)
        if name.endswith("_workspace_bytes"):
            return lambda *args: self.sizes.append((name, args)) or WSB

        def entry(*args):
            self.calls.append((name, args))
            return _lib.GABO_OK
        return entry

    def only(self, name):
        assert [c[0] for c in self.calls] == [name], self.calls
        return self.calls[0][1]


class _Host:
    """what the fixture hands out: the recording library, the host ring and every tensor _prep returned (kept alive, so that a converted copy
    can be recognised by its address)"""

    def __init__(self, lib, ring, prepared):
        self.lib, self.ring, self.prepared = lib, ring, prepared

    def status(self):
        """the address of the word the last launch was handed"""
        return self.ring.buf[self.ring.next].data_ptr()

    def converted(self, ptr, source):
        """the fp64 copy of `source` that _prep made and that `ptr` is the address of"""
        hits = [t for t in self.prepared if t.data_ptr() == ptr and t.dtype == torch.float64]
        assert hits and source.data_ptr() != ptr
        assert torch.equal(hits[0].reshape(-1)[:source.numel()], source.double().reshape(-1))
        return hits[0]


@pytest.fixture
def host(monkeypatch):
    lib, prepared = _Library(), []
    ring = _status._StatusRing("cpu", None)
    key = ("host", 0)
    monkeypatch.setattr(_status, "_ring_key", lambda dev=None: key)
    monkeypatch.setitem(_status._status_rings, key, ring)
    monkeypatch.setattr(_lib, "load", lambda: lib)
    monkeypatch.setattr(ops, "_device_for", lambda *ts: torch.device("cpu"))
    monkeypatch.setattr(ops, "_stream_ptr", lambda dev: 0)
    real_prep = ops._prep

    def prep(x, device):
        prepared.append(real_prep(x, device))
        return prepared[-1]
    monkeypatch.setattr(ops, "_prep", prep)
    prev = _status.set_error_checking("deferred")
    yield _Host(lib, ring, prepared)
    _status.set_error_checking(prev)
    _status._deferred.clear()


def _sets(batch=(), n1=N1, n2=N2, dtype=torch.float64, expand2=False, feature=DV):
    g = torch.Generator().manual_seed(3)
    x1 = torch.rand(*batch, n1, feature, generator=g, dtype=torch.float64).to(dtype)
    if expand2:
        base = torch.rand(n2, feature, generator=g, dtype=torch.float64).to(dtype)
        return x1, base.expand(*batch, n2, feature), base
    return x1, torch.rand(*batch, n2, feature, generator=g, dtype=torch.float64).to(dtype), None


def _cpu64(t, shape):
    return t.dtype == torch.float64 and t.device.type == "cpu" and tuple(t.shape) == tuple(shape)


# ------------------------------------------------------------------------------------------------------------ forward entries
# name -> (call with (x1, x2), library entry, arguments after the nine common ones (x1, x2, out, nb, n1, n2, d, s1, s2), has status/workspace)
PAIRWISE = {
    "frobenius": (lambda a, b: ops.frobenius_pairwise(a, b, 0.7, LAPLACE), "gabo_frobenius_pairwise", (0.7, LAPLACE, 0)),
    "flat_matern": (lambda a, b: ops.flat_matern_pairwise(a, b, 0.9, 1.5), "gabo_flat_matern_pairwise", (0.9, 3, 0)),
}


def _common(x1p, x2p, out, nb, s1, s2, n1=N1, n2=N2):
    return (x1p, x2p, out.data_ptr(), nb, n1, n2, D, s1, s2)


@pytest.mark.parametrize("name", sorted(PAIRWISE))
def test_flat_pairwise_arguments(host, name):
    call, entry, tail = PAIRWISE[name]
    # no batch
    x1, x2, _ = _sets()
    out = call(x1, x2)
    assert _cpu64(out, (N1, N2))
    assert host.lib.only(entry) == _common(x1.data_ptr(), x2.data_ptr(), out, 1, N1 * DV, N2 * DV) + tail
    # a dense batch of 2
    host.lib.calls.clear()
    x1, x2, _ = _sets((2,))
    out = call(x1, x2)
    assert _cpu64(out, (2, N1, N2))
    assert host.lib.only(entry) == _common(x1.data_ptr(), x2.data_ptr(), out, 2, N1 * DV, N2 * DV) + tail
    # x2 one expand()ed set: the base tensor's address, batch stride 0
    host.lib.calls.clear()
    x1, x2, base = _sets((2,), expand2=True)
    out = call(x1, x2)
    assert _cpu64(out, (2, N1, N2))
    assert host.lib.only(entry) == _common(x1.data_ptr(), base.data_ptr(), out, 2, N1 * DV, 0) + tail
    # fp32 input: converted, fp64 out
    host.lib.calls.clear()
    x1, x2, _ = _sets(dtype=torch.float32)
    out = call(x1, x2)
    assert _cpu64(out, (N1, N2))
    args = host.lib.only(entry)
    host.converted(args[0], x1), host.converted(args[1], x2)
    assert args[2:] == _common(0, 0, out, 1, N1 * DV, N2 * DV)[2:] + tail


def test_one_point_set_shares_the_pointer_only_where_promised(host):
    x = _sets(dtype=torch.float32)[0]
    ops.flat_matern_pairwise(x, x, 0.9, 1.5)
    args = host.lib.only("gabo_flat_matern_pairwise")
    assert args[0] == args[1] and args[4:6] == (N1, N1) and args[7] == args[8] == N1 * DV
    host.converted(args[0], x)
    host.lib.calls.clear()
    xb = _sets((2,), dtype=torch.float32)[0]
    ops.flat_matern_pairwise(xb, xb, 0.9, 1.5)
    args = host.lib.only("gabo_flat_matern_pairwise")
    assert args[0] == args[1] and args[3] == 2 and args[7] == args[8] == N1 * DV
    for call, entry in ((lambda: ops.frobenius_pairwise(x, x), "gabo_frobenius_pairwise"),
                        (lambda: ops.spd_ai_pairwise(x, x), "gabo_spd_ai_pairwise"),
                        (lambda: ops.sphere_zonal_pairwise(x, x, np.ones(2), 3), "gabo_sphere_zonal_pairwise")):
        host.lib.calls.clear()
        call()
        args = host.lib.only(entry)
        assert args[0] != args[1]                       # two conversions, both alive during the call
        host.converted(args[0], x), host.converted(args[1], x)
    # fp64: nothing to convert, so the input's own address twice
    x = _sets()[0]
    for call, entry in ((lambda: ops.frobenius_pairwise(x, x), "gabo_frobenius_pairwise"),
                        (lambda: ops.flat_matern_pairwise(x, x, 0.9, 2.5), "gabo_flat_matern_pairwise")):
        host.lib.calls.clear()
        call()
        assert host.lib.only(entry)[:2] == (x.data_ptr(), x.data_ptr())


@pytest.mark.parametrize("name", sorted(PAIRWISE))
def test_flat_pairwise_launches_on_empty_sets(host, name):
    call, entry, tail = PAIRWISE[name]
    for n1, n2 in ((N1, 0), (0, N2)):
        host.lib.calls.clear()
        x1, x2, _ = _sets(n1=n1, n2=n2)
        out = call(x1, x2)
        assert _cpu64(out, (n1, n2))
        assert host.lib.only(entry)[3:9] == (1, n1, n2, D, n1 * DV, n2 * DV)


def test_spd_ai_pairwise_arguments(host):
    x1, x2, _ = _sets()
    out = ops.spd_ai_pairwise(x1, x2, 0.6, LAPLACE)
    assert _cpu64(out, (N1, N2))
    assert host.lib.only("gabo_spd_ai_pairwise") == _common(x1.data_ptr(), x2.data_ptr(), out, 1, N1 * DV, N2 * DV)[:3] + (
        None, 1, N1, N2, D, N1 * DV, N2 * DV, 0.6, LAPLACE, SOME, WSB, host.status(), 0)
    assert host.lib.sizes == [("gabo_spd_ai_workspace_bytes", (1, N1, N2, D))]
    # the distance matrix of the same launch, the symmetric flag, a batch with x2 one expand()ed set
    host.lib.calls.clear()
    x1, x2, base = _sets((2,), expand2=True)
    out, dist = ops.spd_ai_pairwise(x1, x2, 2, GAUSS, symmetric=True, return_dist=True)
    assert _cpu64(out, (2, N1, N2)) and _cpu64(dist, (2, N1, N2))
    args = host.lib.only("gabo_spd_ai_pairwise")
    assert args == (x1.data_ptr(), base.data_ptr(), out.data_ptr(), dist.data_ptr(), 2, N1, N2, D, N1 * DV, 0, 2.0, GAUSS | SYM, SOME, WSB,
                    host.status(), 0)
    assert isinstance(args[10], float) and host.lib.sizes[-1] == ("gabo_spd_ai_workspace_bytes", (2, N1, N2, D))
    # a dense batch
    host.lib.calls.clear()
    x1, x2, _ = _sets((2,))
    out = ops.spd_ai_pairwise(x1, x2, mode=DIST | SYM)
    assert host.lib.only("gabo_spd_ai_pairwise")[4:12] == (2, N1, N2, D, N1 * DV, N2 * DV, 1.0, DIST | SYM)
    # fp32
    host.lib.calls.clear()
    x1, x2, _ = _sets(dtype=torch.float32)
    out = ops.spd_ai_pairwise(x1, x2)
    assert _cpu64(out, (N1, N2))
    args = host.lib.only("gabo_spd_ai_pairwise")
    host.converted(args[0], x1), host.converted(args[1], x2)
    # empty: no launch, no workspace question
    for n1, n2 in ((N1, 0), (0, N2)):
        host.lib.calls.clear()
        del host.lib.sizes[:]
        x1, x2, _ = _sets(n1=n1, n2=n2)
        out, dist = ops.spd_ai_pairwise(x1, x2, return_dist=True)
        assert _cpu64(out, (n1, n2)) and _cpu64(dist, (n1, n2)) and host.lib.calls == [] and host.lib.sizes == []
        assert _cpu64(ops.spd_ai_pairwise(x1, x2), (n1, n2)) and host.lib.calls == []


def test_sphere_zonal_pairwise_arguments(host):
    coeff = np.array([0.5, 0.25, 0.25])
    x1, x2, _ = _sets()
    out = ops.sphere_zonal_pairwise(x1, x2, coeff, 4)
    assert _cpu64(out, (N1, N2))
    assert host.lib.only("gabo_sphere_zonal_pairwise") == (x1.data_ptr(), x2.data_ptr(), out.data_ptr(), 1, N1, N2, DV, N1 * DV, N2 * DV,
                                                           coeff.ctypes.data, 3, 4, 0, 0, 0)
    host.lib.calls.clear()
    out = ops.sphere_zonal_pairwise(x1, x2, coeff, 4, symmetric=True)
    assert host.lib.only("gabo_sphere_zonal_pairwise")[12:] == (SYM, 0, 0)
    # diag: (..., N, 1), never the symmetric flag; sets of unequal length are refused
    host.lib.calls.clear()
    xb, yb, base = _sets((2,), n2=N1, expand2=True)
    out = ops.sphere_zonal_pairwise(xb, yb, coeff, 4, diag=True, symmetric=True)
    assert _cpu64(out, (2, N1, 1))
    assert host.lib.only("gabo_sphere_zonal_pairwise") == (xb.data_ptr(), base.data_ptr(), out.data_ptr(), 2, N1, N1, DV, N1 * DV, 0,
                                                           coeff.ctypes.data, 3, 4, 0, 1, 0)
    host.lib.calls.clear()
    with pytest.raises(RuntimeError, match="diag=True needs x1 and x2 of the same length"):
        ops.sphere_zonal_pairwise(x1, x2, coeff, 4, diag=True)
    # fp32, and the empty output that is returned without a launch
    x32, y32, _ = _sets(dtype=torch.float32)
    out = ops.sphere_zonal_pairwise(x32, y32, coeff, 4)
    args = host.lib.only("gabo_sphere_zonal_pairwise")
    host.converted(args[0], x32), host.converted(args[1], y32)
    assert _cpu64(out, (N1, N2))
    for n1, n2 in ((N1, 0), (0, N2)):
        host.lib.calls.clear()
        x1, x2, _ = _sets(n1=n1, n2=n2)
        assert _cpu64(ops.sphere_zonal_pairwise(x1, x2, coeff, 4), (n1, n2)) and host.lib.calls == []
    assert _cpu64(ops.sphere_zonal_pairwise(x1, x1, coeff, 4, diag=True), (0, 1)) and host.lib.calls == []


NO_BROADCAST = " (no broadcasting, as in the reference)"


@pytest.mark.parametrize("call, suffix", [
    (lambda a, b: ops.spd_ai_pairwise(a, b), NO_BROADCAST),
    (lambda a, b: ops.sphere_pairwise(a, b), ""),
    (lambda a, b: ops.sphere_zonal_pairwise(a, b, np.ones(2), 3), ""),
    (lambda a, b: ops.frobenius_pairwise(a, b), ""),
    (lambda a, b: ops.flat_matern_pairwise(a, b, 1.0, 0.5), ""),
    (lambda a, b: ops.nested_spd_gram(a, b, torch.eye(2, dtype=torch.float64), 1.0), NO_BROADCAST),
    (lambda a, b: ops.nested_spd_matern_gram(a, b, torch.eye(2, dtype=torch.float64), 1.0, 0.5), NO_BROADCAST),
])
def test_shape_mismatch_texts(host, call, suffix):
    x1 = _sets((2,))[0]
    for x2 in (_sets()[1], _sets((2,), feature=6)[1]):
        with pytest.raises(RuntimeError) as err:
            call(x1, x2)
        assert str(err.value) == f"batch/feature shapes differ: {tuple(x1.shape)} vs {tuple(x2.shape)}{suffix}"
    assert host.lib.calls == []


# ------------------------------------------------------------------------------------------------------------ gradients
BACKWARD = {
    # name -> (call, library entry, arguments behind the three grad_out strides, has the sign of the exchange, has workspace and status)
    "spd_ai": (lambda a, b, g, wrt: ops.spd_ai_backward(a, b, g, 0.6, LAPLACE, wrt=wrt), "gabo_spd_ai_backward", (0.6, LAPLACE), False, True),
    "frobenius": (lambda a, b, g, wrt: ops.frobenius_backward(a, b, g, 0.7, GAUSS, wrt=wrt), "gabo_frobenius_backward", (0.7, GAUSS), True, False),
    "flat_matern": (lambda a, b, g, wrt: ops.flat_matern_backward(a, b, g, 0.9, 2.5, wrt=wrt), "gabo_flat_matern_backward", (0.9, 5), True,
                    False),
}


def _backward_expected(host, name, wrt, p1, p2, g, gx, nb, s1, s2, go, n1=N1, n2=N2):
    _, _, scalars, signed, checked = BACKWARD[name]
    go_b, go_i, go_j = go
    if wrt == 1:
        head = (p1, p2, g.data_ptr(), gx.data_ptr(), nb, n1, n2, D, s1, s2, go_b, go_i, go_j)
    else:
        head = (p2, p1, g.data_ptr(), gx.data_ptr(), nb, n2, n1, D, s2, s1, go_b, go_j, go_i)
    return head + scalars + ((1.0 if wrt == 1 else -1.0,) if signed else ()) + ((SOME, WSB, host.status()) if checked else ()) + (0,)


@pytest.mark.parametrize("wrt", [1, 2])
@pytest.mark.parametrize("name", sorted(BACKWARD))
def test_backward_arguments(host, name, wrt):
    call, entry = BACKWARD[name][:2]
    m1 = N1 if wrt == 1 else N2
    # no batch, contiguous grad_out: strides (n2, 1), read transposed - (1, n2) - for wrt = 2; the batch stride is n1 n2 for two of the three
    x1, x2, _ = _sets()
    g = torch.rand(N1, N2, dtype=torch.float64)
    gx = call(x1, x2, g, wrt)
    assert _cpu64(gx, (m1, DV))
    go_b = 0 if name == "flat_matern" else N1 * N2          # (a single matrix is read in place by flat_matern_backward: batch stride 0)
    assert host.lib.only(entry) == _backward_expected(host, name, wrt, x1.data_ptr(), x2.data_ptr(), g, gx, 1, N1 * DV, N2 * DV, (go_b, N2, 1))
    if BACKWARD[name][4]:
        assert host.lib.sizes == [("gabo_spd_ai_workspace_bytes", (1, m1, N1 + N2 - m1, D))]
    # a dense batch of 2
    host.lib.calls.clear()
    x1, x2, _ = _sets((2,))
    g = torch.rand(2, N1, N2, dtype=torch.float64)
    gx = call(x1, x2, g, wrt)
    assert _cpu64(gx, (2, m1, DV))
    assert host.lib.only(entry) == _backward_expected(host, name, wrt, x1.data_ptr(), x2.data_ptr(), g, gx, 2, N1 * DV, N2 * DV,
                                                      (N1 * N2, N2, 1))
    # fp32 sets and gradient
    host.lib.calls.clear()
    x1, x2, _ = _sets(dtype=torch.float32)
    g = torch.rand(N1, N2)
    gx = call(x1, x2, g, wrt)
    assert _cpu64(gx, (m1, DV))
    args = host.lib.only(entry)
    c1, c2, cg = host.converted(args[0 if wrt == 1 else 1], x1), host.converted(args[1 if wrt == 1 else 0], x2), host.converted(args[2], g)
    assert args == _backward_expected(host, name, wrt, c1.data_ptr(), c2.data_ptr(), cg, gx, 1, N1 * DV, N2 * DV, (go_b, N2, 1))


@pytest.mark.parametrize("wrt", [1, 2])
@pytest.mark.parametrize("name", sorted(BACKWARD))
def test_backward_with_x2_one_expanded_set(host, name, wrt):
    """Batch stride 0 and the base tensor's address.  As the FIRST set of the launch (wrt = 2) the two flat gradients come back summed over the
    batch and expanded again; the affine-invariant one stays one slice per batch entry (autograd's ExpandBackward does that sum)."""
    call, entry = BACKWARD[name][:2]
    m1 = N1 if wrt == 1 else N2
    x1, x2, base = _sets((2,), expand2=True)
    g = torch.rand(2, N1, N2, dtype=torch.float64)
    gx = call(x1, x2, g, wrt)
    assert _cpu64(gx, (2, m1, DV))
    args = host.lib.only(entry)
    summed = wrt == 2 and name != "spd_ai"
    launched = gx
    if summed:
        assert gx.stride() == (0, DV, 1) and args[3] != gx.data_ptr()
        launched = torch.empty(0)            # (the launch's own buffer is gone: its address is not compared)
        args = args[:3] + (launched.data_ptr(),) + args[4:]
    else:
        assert gx.stride() == (m1 * DV, DV, 1)
    assert args == _backward_expected(host, name, wrt, x1.data_ptr(), base.data_ptr(), g, launched, 2, N1 * DV, 0, (N1 * N2, N2, 1))


@pytest.mark.parametrize("wrt", [1, 2])
@pytest.mark.parametrize("name", sorted(BACKWARD))
def test_backward_of_an_empty_set_returns_zeros_without_a_launch(host, name, wrt):
    call = BACKWARD[name][0]
    for n1, n2 in ((N1, 0), (0, N2)):
        x1, x2, _ = _sets(n1=n1, n2=n2)
        gx = call(x1, x2, torch.zeros(n1, n2, dtype=torch.float64), wrt)
        assert _cpu64(gx, (n1 if wrt == 1 else n2, DV)) and not gx.any() and host.lib.calls == [] and host.lib.sizes == []


@pytest.mark.parametrize("wrt", [1, 2])
def test_flat_matern_backward_reads_a_strided_matrix_in_place(host, wrt):
    x1, x2, _ = _sets()
    g = torch.rand(N2, N1, dtype=torch.float64).t()          # (N1, N2) with strides (1, N1)
    gx = ops.flat_matern_backward(x1, x2, g, 0.9, 0.5, wrt=wrt)
    assert host.lib.only("gabo_flat_matern_backward") == _backward_expected(host, "flat_matern", wrt, x1.data_ptr(), x2.data_ptr(), g, gx, 1,
                                                                             N1 * DV, N2 * DV, (0, 1, N1))[:13] + (0.9, 1, 1.0 if wrt == 1 else -1.0, 0)
    # the other two take a contiguous copy
    for name in ("spd_ai", "frobenius"):
        host.lib.calls.clear()
        gx = BACKWARD[name][0](x1, x2, g, wrt)
        args = host.lib.only(BACKWARD[name][1])
        assert args[2] != g.data_ptr() and args[10:13] == ((N1 * N2, N2, 1) if wrt == 1 else (N1 * N2, 1, N2))
    with pytest.raises(ValueError, match="wrt must be 1 or 2"):
        ops.flat_matern_backward(x1, x2, g, 0.9, 0.5, wrt=3)


def test_spd_ai_backward2_arguments(host):
    x1, x2, _ = _sets()
    g, u = torch.rand(N1, N2, dtype=torch.float64), torch.rand(N1, DV, dtype=torch.float64)
    hv, dg, mx = ops.spd_ai_backward2(x1, x2, g, u, 0.6, LAPLACE, want_mixed=True)
    assert _cpu64(hv, (N1, DV)) and _cpu64(dg, (N1, N2)) and _cpu64(mx, (N2, DV))
    assert host.lib.only("gabo_spd_ai_backward2") == (x1.data_ptr(), x2.data_ptr(), g.data_ptr(), u.data_ptr(), hv.data_ptr(), dg.data_ptr(),
                                                      mx.data_ptr(), 1, N1, N2, D, N1 * DV, N2 * DV, N1 * N2, N2, 1, 0.6, LAPLACE, SOME, WSB,
                                                      host.status(), 0)
    assert host.lib.sizes == [("gabo_spd_ai_backward2_workspace_bytes", (1, N1, N2, D))]
    # defaults: dg, no mixed block; x2 one expand()ed set
    host.lib.calls.clear()
    x1, x2, base = _sets((2,), expand2=True)
    g, u = torch.rand(2, N1, N2, dtype=torch.float64), torch.rand(2, N1, DV, dtype=torch.float64)
    hv, dg, mx = ops.spd_ai_backward2(x1, x2, g, u)
    assert _cpu64(hv, (2, N1, DV)) and _cpu64(dg, (2, N1, N2)) and mx is None
    assert host.lib.only("gabo_spd_ai_backward2") == (x1.data_ptr(), base.data_ptr(), g.data_ptr(), u.data_ptr(), hv.data_ptr(), dg.data_ptr(),
                                                      None, 2, N1, N2, D, N1 * DV, 0, N1 * N2, N2, 1, 1.0, GAUSS, SOME, WSB, host.status(), 0)
    # x1 one expand()ed set with a direction per batch entry: every entry gets its own copy of the set
    host.lib.calls.clear()
    x2, x1, base = _sets((2,), n1=N2, n2=N1, expand2=True)
    hv, dg, mx = ops.spd_ai_backward2(x1, x2, g, u, want_dgrad_out=False, want_mixed=True)
    assert _cpu64(hv, (2, N1, DV)) and dg is None and _cpu64(mx, (2, N2, DV))
    args = host.lib.only("gabo_spd_ai_backward2")
    assert args[0] not in (base.data_ptr(), x1.data_ptr()) and args[1:7] == (x2.data_ptr(), g.data_ptr(), u.data_ptr(), hv.data_ptr(), None,
                                                                              mx.data_ptr())
    assert args[7:16] == (2, N1, N2, D, N1 * DV, N2 * DV, N1 * N2, N2, 1)
    with pytest.raises(RuntimeError, match="is not shaped like x1"):
        ops.spd_ai_backward2(x1, x2, g, u[0])
    # empty second set: zeros, no launch
    host.lib.calls.clear()
    x1, x2, _ = _sets(n2=0)
    hv, dg, mx = ops.spd_ai_backward2(x1, x2, torch.zeros(N1, 0, dtype=torch.float64), torch.ones(N1, DV, dtype=torch.float64), want_mixed=True)
    assert _cpu64(hv, (N1, DV)) and not hv.any() and _cpu64(dg, (N1, 0)) and _cpu64(mx, (0, DV)) and host.lib.calls == []


# ------------------------------------------------------------------------------------------------------------ nested Gram entries
NESTED = {
    "gaussian": (lambda a, b, w: ops.nested_spd_gram(a, b, w, 0.6, _lib.GABO_METRIC_LOG_EUCLIDEAN, LAPLACE), "gabo_nested_spd_gram",
                 (_lib.GABO_METRIC_LOG_EUCLIDEAN, 0.6, LAPLACE)),
    "matern": (lambda a, b, w: ops.nested_spd_matern_gram(a, b, w, 0.9, 1.5), "gabo_nested_spd_matern_gram", (0.9, 3)),
}


@pytest.mark.parametrize("name", sorted(NESTED))
def test_nested_gram_arguments(host, name):
    call, entry, scalars = NESTED[name]
    w = torch.rand(D, 2, dtype=torch.float64)

    def expected(p1, p2, out, nb, n1=N1, n2=N2):
        return (p1, p2, w.data_ptr(), out.data_ptr(), nb, n1, n2, D, 2) + scalars + (SOME, WSB, host.status(), 0)
    x1, x2, _ = _sets()
    out = call(x1, x2, w)
    assert _cpu64(out, (N1, N2))
    assert host.lib.only(entry) == expected(x1.data_ptr(), x2.data_ptr(), out, 1)
    assert host.lib.sizes == [("gabo_nested_spd_gram_workspace_bytes", (1, N1, N2, 2))]
    # a dense batch; an expand()ed x2 is laid out in full (the entry takes no batch strides)
    host.lib.calls.clear()
    x1, x2, _ = _sets((2,))
    out = call(x1, x2, w)
    assert _cpu64(out, (2, N1, N2)) and host.lib.only(entry) == expected(x1.data_ptr(), x2.data_ptr(), out, 2)
    host.lib.calls.clear()
    x1, x2, base = _sets((2,), expand2=True)
    out = call(x1, x2, w)
    args = host.lib.only(entry)
    assert args[1] != base.data_ptr() and args == expected(x1.data_ptr(), args[1], out, 2)
    # one point set: projected once, the same pointer twice - also when it had to be converted
    host.lib.calls.clear()
    x32 = _sets(dtype=torch.float32)[0]
    out = call(x32, x32, w.float())
    args = host.lib.only(entry)
    host.converted(args[0], x32), host.converted(args[2], w.float())
    assert args[0] == args[1] and _cpu64(out, (N1, N1)) and args[4:9] == (1, N1, N1, D, 2)
    host.lib.calls.clear()
    out = call(x32, x32.clone(), w)
    args = host.lib.only(entry)
    assert args[0] != args[1]
    # empty: returned without a launch; a projection matrix of the wrong height is refused
    for n1, n2 in ((N1, 0), (0, N2)):
        host.lib.calls.clear()
        del host.lib.sizes[:]
        x1, x2, _ = _sets(n1=n1, n2=n2)
        assert _cpu64(call(x1, x2, w), (n1, n2)) and host.lib.calls == [] and host.lib.sizes == []
    with pytest.raises(RuntimeError, match=r"projection matrix must be \(2, d_latent\), got \(3, 2\)"):
        call(x1, x2, torch.rand(3, 2, dtype=torch.float64))


# ------------------------------------------------------------------------------------------------------------ the scalar kernel parameter
KERNELS = {
    # name -> (entry(x1, x2, parameter), the autograd Function it hands the parameter to, position of the parameter there, the text)
    "spd_ai": (lambda a, b, p: ops.spd_ai_kernel(a, b, p), "_SpdAiKernelFunction", 2,
               "gabotorch_amd SPD kernels take a single beta (batch_shape == ()), as every reference example does"),
    "frobenius": (lambda a, b, p: ops.frobenius_kernel(a, b, p), "_FrobeniusKernelFunction", 2,
                  "gabotorch_amd SPD kernels take a single lengthscale (batch_shape == ())"),
    "flat_matern": (lambda a, b, p: ops.flat_matern_kernel(a, b, p, 1.5), "_FlatMaternKernelFunction", 2,
                    "gabotorch_amd SPD kernels take a single lengthscale (batch_shape == ())"),
    "sphere_matern": (lambda a, b, p: ops.sphere_matern_kernel(a.requires_grad_(), b, p, 1.5, 4), "_SphereMaternFromInner", 1,
                      "gabotorch_amd sphere kernels take a single lengthscale (batch_shape == ())"),
    "sphere": (lambda a, b, p: ops.sphere_kernel(a.requires_grad_(), b, p), "_SphereFromInner", 1,
               "gabotorch_amd sphere kernels take a single beta (batch_shape == ())"),
}


@pytest.mark.parametrize("name", sorted(KERNELS))
def test_the_kernel_parameter_reaches_the_function_as_one_fp64_element(host, monkeypatch, name):
    entry, function, position, text = KERNELS[name]
    seen = []
    monkeypatch.setattr(getattr(ops, function), "apply", staticmethod(lambda *args: seen.append(args[position]) or torch.zeros(N1, N2)))
    for given, shape in ((0.5, ()), (2, ()), (torch.tensor(0.5), ()), (torch.tensor([[0.5]], dtype=torch.float32), (1, 1)),
                         (torch.tensor([0.5], dtype=torch.float64), (1,))):
        x1, x2, _ = _sets()
        entry(x1, x2, given)
        p = seen.pop()
        assert torch.is_tensor(p) and p.dtype == torch.float64 and p.device.type == "cpu" and tuple(p.shape) == shape
        assert float(p) == float(given)
    x1, x2, _ = _sets()
    with pytest.raises(RuntimeError) as err:
        entry(x1, x2, torch.tensor([0.5, 0.5]))
    assert str(err.value) == text and seen == []


@pytest.mark.parametrize("shape", [(), (1,), (1, 1)])
@pytest.mark.parametrize("name", sorted(KERNELS))
def test_the_parameter_gradient_comes_back_in_the_shape_it_came_in(host, name, shape):
    """through the real Functions, forward and backward, on the recording library (the numbers are whatever the allocations held)"""
    entry = KERNELS[name][0]
    p = torch.full(shape, 0.5, dtype=torch.float32, requires_grad=True)
    x1, x2, _ = _sets()
    x1 = torch.nn.functional.normalize(x1, dim=-1)
    out = entry(x1, torch.nn.functional.normalize(x2, dim=-1), p)
    assert tuple(out.shape) == (N1, N2) and out.dtype == torch.float64
    out.backward(torch.ones_like(out))
    assert p.grad is not None and tuple(p.grad.shape) == shape and p.grad.dtype == torch.float32 and p.grad.device == p.device
