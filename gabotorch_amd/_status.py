"""Device status words: how a data error a kernel detects (a non-SPD input, a failed GP Cholesky, an exhausted MVN jitter ladder) becomes a
RuntimeError.  A launch is handed a word (two int32: error code, index of the offender) that only a failing kernel writes; the host keeps ONE
record per launch that somebody still has to look at, and one routine (_raise_if_failed) that turns a non-zero word into the exception."""
import contextlib

import torch

from . import _lib

_mode = "deferred"


def set_error_checking(flag):
    """How device-side data errors (a non-SPD input matrix, a NaN entry) reach the caller.  The reference raises from torch.cholesky at the call
    (spd_utils_torch.py:87); a launch is asynchronous, so raising AT the call costs a stream synchronisation per call.
      "deferred" (default): every launch gets a status word of its own; the words are read back - ONE copy for all pending launches of a stream -
                 at the next synchronisation point: check_deferred(), which the acquisition sweep, the GP posterior and the solvers call where
                 they wait for the device anyway, or when 62 launches are pending on one stream.  The RuntimeError names the launch that failed.
      True / "sync": read back after every call (one stream synchronisation per call): the reference's behaviour to the statement.
      False:     launches share one word per stream that is never read - except those that register with force=True (the GP's Cholesky),
                 which keep a word of their own and are reported by check_deferred() in every mode.
    Switching modes forgets nothing: a launch that was registered - before checking was switched off, or forced while it was off - stays pending
    until a check has looked at it.  Coming back from False only zeroes the shared words the unchecked launches may have written.
    Returns the previous setting."""
    global _mode
    prev = _mode
    if flag == "sync":
        flag = True
    if flag not in (True, False, "deferred"):
        raise ValueError("set_error_checking: True / 'sync', 'deferred' or False")
    if prev is False and flag is not False:
        for ring in _status_rings.values():
            ring.clear(0)
    _mode = flag
    return prev


def error_checking():
    """the current setting of set_error_checking: True, "deferred" or False"""
    return _mode


def _not_spd_message(what):
    return lambda st: f"{what}: input matrix #{st[1]} is not positive definite (Cholesky pivot <= 0)"


class _Record:
    """One launch whose status word has not been looked at: the word is slot `slot` of `ring`, or (ring None) the caller's own tensor `word`.
    No __init__ (one is made per launch): _StatusRing.take and _raise_if_not_spd fill it in."""
    __slots__ = ("ring", "slot", "word", "forced", "message", "on_fail")


def _raise_if_failed(rec, code, index):
    """THE raise path, for a record and the two ints of its word.  Non-zero: clear the word (the next launch that is handed it starts from
    zero), let the caller drop what the failed launch was meant to fill, raise."""
    if code == 0:
        return
    if rec.ring is not None:
        rec.ring.clear(rec.slot)
    else:
        rec.word.zero_()
    if rec.on_fail is not None:
        rec.on_fail()
    raise RuntimeError(rec.message([int(code), int(index)]) if callable(rec.message) else rec.message)


class _StatusRing:
    """The status words of the launches on ONE stream of one device: a ring of `N` words in device memory, zeroed once - the kernels only ever
    write a word on an error, so no fill launch in front of a call (4 us of GPU time next to a 6 us projection,
    profiles/r03_config5_kernel_stats.csv) - each launch taking the next word.  `pending` holds the records of the launches nobody has checked
    yet, oldest first; check() waits for the stream, reads the whole ring in one copy, forgets the launches that succeeded and raises for the
    first that did not.  stream None: a ring in host memory (the bookkeeping is the same; tests/test_status_cpu.py)."""
    N = 64

    def __init__(self, dev, stream):
        self.buf = torch.zeros(self.N, 2, dtype=torch.int32, device=dev)
        self.stream = stream
        self.next = 0
        self.pending = []
        self.host = None

    def _on_stream(self):
        return contextlib.nullcontext() if self.stream is None else torch.cuda.stream(self.stream)

    def take(self, forced=False):
        k = self.next = self.next % (self.N - 1) + 1          # slots 1 ... N - 1 (slot 0: the word of launches nobody checks)
        w = self.buf[k]
        w._gabo_record = rec = _Record()
        rec.ring, rec.slot, rec.forced = self, k, forced
        return w

    def clear(self, k):
        with self._on_stream():
            self.buf[k].zero_()

    def reset(self):
        """forget everything: all words zero, nothing pending"""
        with self._on_stream():
            self.buf.zero_()
        self.pending.clear()

    def prefetch(self):
        """Enqueue on the CURRENT stream - the ring's own: see prefetch_deferred - a copy of the ring into page-locked host memory; -> the token
        for check_prefetched: the ring and the records the copy covers."""
        if self.host is None:
            host = torch.zeros(self.N, 2, dtype=torch.int32)
            self.host = host.pin_memory() if self.buf.is_cuda else host
        self.host.copy_(self.buf, non_blocking=True)
        return self, list(self.pending)

    def check(self):
        if self.pending:
            with self._on_stream():
                vals = self.buf.cpu()              # (waits for everything enqueued on the ring's stream)
            self.evaluate(vals.tolist())

    def evaluate(self, vals, records=None):
        """`records` (default: all that are pending), in that order, against `vals`: a host copy of the ring taken after they had completed.
        A record that is no longer pending - something else has checked it since - is passed over."""
        for rec in list(self.pending) if records is None else records:
            if rec in self.pending:
                self.pending.remove(rec)
                _raise_if_failed(rec, *vals[rec.slot])


_status_rings = {}          # (device index, raw stream) -> _StatusRing
_deferred = []              # records of the words their callers own (fixed address: captured in a hipGraph, or owned by a solver object)


def _ring_key(dev=None):
    idx = torch.cuda.current_device() if dev is None or dev.index is None else dev.index        # (None: the current device)
    return idx, torch._C._cuda_getCurrentRawStream(idx)


def _status_word(dev, force=False):
    """A status word for the launch about to be enqueued on the current stream of `dev` (a view of that stream's ring: _StatusRing).
    force: a word that is registered and read even while error checking is off (the GP's Cholesky: see gp_factor)."""
    key = _ring_key(dev)
    ring = _status_rings.get(key)
    if ring is None:
        ring = _status_rings[key] = _StatusRing(dev, torch.cuda.current_stream(dev))
    if _mode is False and not force:
        return ring.buf[0]          # (never read while checking is off; set_error_checking zeroes it when checking comes back on)
    if len(ring.pending) >= ring.N - 2:
        ring.check()
    return ring.take(force)


def _raise_if_not_spd(status, what, message=None, on_fail=None, force=False):
    """Called after the launch that was handed `status`: registers the launch for the next check (deferred), or reads the word now (sync).
    message: the RuntimeError's text, or a callable of the two status ints; on_fail: called before raising (e.g. to drop a cache the failed launch
    was meant to fill)."""
    if _mode is False and not force:
        return
    rec = getattr(status, "_gabo_record", None)
    if rec is None:         # a word of the caller's own
        rec = _Record()
        rec.ring, rec.word, rec.forced = None, status, force
    rec.message, rec.on_fail = message or _not_spd_message(what), on_fail
    if rec.ring is not None:
        rec.ring.pending.append(rec)
        if _mode is True:
            rec.ring.check()
    elif _mode is True:
        _raise_if_failed(rec, *status.tolist())
    else:
        _deferred.append(rec)
        if len(_deferred) > 32:
            check_deferred()


def _check_launch(rc, status, what, on_fail=None):
    """return code first, then the device status word.  A launch refused by its return code never ran: its word is not registered."""
    try:
        _lib.check(rc, what)
    except Exception:
        if on_fail is not None:
            on_fail()
        raise
    _raise_if_not_spd(status, what, on_fail=on_fail)


def prefetch_deferred():
    """For a caller that is about to wait for its stream anyway (the acquisition sweep before its scoring call returns): enqueue the read-back of
    the status ring of the current stream of the current device and return a token for check_prefetched - which then needs no device access at
    all.  Launches on other streams stay pending for check_deferred()."""
    ring = _status_rings.get(_ring_key())
    return ring.prefetch() if ring is not None and ring.pending else None


def check_prefetched(token):
    """check_deferred for the launches prefetch_deferred's token names (those of them that nothing has checked since); ONLY after the stream that
    copy was enqueued on has been waited for (the data is read from host memory as it is)."""
    if token is not None:
        ring, records = token
        ring.evaluate(ring.host.numpy(), records)


def check_deferred():
    """Reads the status words of every launch that has not been checked yet - one copy per stream that has any - and raises for the first failure,
    naming the launch.  Called at the natural host synchronisation points of a sweep (after the raw samples' scores have reached the host, after a
    solve, before a posterior); free when nothing is pending.  The launches that were still queued behind a failed one stay queued."""
    for ring in list(_status_rings.values()):
        ring.check()
    while _deferred:
        rec = _deferred.pop(0)
        _raise_if_failed(rec, *rec.word.tolist())
