"""The bookkeeping of the device status words (gabotorch_amd/_status.py) on a stand-in ring: a CPU int32 tensor as the "device" words, no stream.
A kernel that detects an error is played by `_kernel_writes`."""
import pytest
import torch

from gabotorch_amd import _status, ops

KEY = ("host", 0)


@pytest.fixture
def ring(monkeypatch):
    """a host ring as the ring of 'the current stream', in the default mode; forgotten afterwards"""
    r = _status._StatusRing("cpu", None)
    monkeypatch.setattr(_status, "_ring_key", lambda dev=None: KEY)
    monkeypatch.setitem(_status._status_rings, KEY, r)
    prev = _status.set_error_checking("deferred")
    yield r
    _status.set_error_checking(prev)
    _status._deferred.clear()


def _kernel_writes(word, code, index):
    word.copy_(torch.tensor([code, index], dtype=torch.int32))


def _launch(what, fail_at=None, force=False, on_fail=None, message=None):
    """what a wrapper in ops.py does around its launch -> the word it used"""
    word = _status._status_word(torch.device("cpu"), force=force)
    if fail_at is not None:
        _kernel_writes(word, 1, fail_at)
    _status._raise_if_not_spd(word, what, message=message, on_fail=on_fail, force=force)
    return word


@pytest.mark.parametrize("message, text", [(lambda st: f"launch failed with {st[0]} at #{st[1]}", "launch failed with 3 at #7"),
                                           ("a fixed text", "a fixed text")])
def test_the_raise_path_clears_the_word_and_calls_on_fail_before_raising(ring, message, text):
    seen = []
    own = torch.tensor([3, 7], dtype=torch.int32)
    owned, slot = _status._Record(), _status._Record()
    owned.ring, owned.word = None, own
    slot.ring, slot.slot = ring, 5
    for rec, word in ((owned, own), (slot, ring.buf[5])):
        _kernel_writes(word, 3, 7)
        rec.message, rec.on_fail = message, lambda word=word: seen.append(word.tolist())
        _status._raise_if_failed(rec, 0, 0)                                # a word that is zero: nothing happens
        assert word.tolist() == [3, 7] and seen == []
        with pytest.raises(RuntimeError) as err:
            _status._raise_if_failed(rec, 3, 7)
        assert str(err.value) == text
        assert word.tolist() == [0, 0]
        assert seen.pop() == [0, 0]                                        # on_fail ran (once), after the word was cleared and before the raise
    rec.on_fail = None
    with pytest.raises(RuntimeError):
        _status._raise_if_failed(rec, 1, 0)


def test_ring_arithmetic(ring):
    """64 words; slot 0 is the unchecked one, 1 ... 63 are taken round-robin; a check is forced at 62 pending"""
    assert ring.N == 64 and tuple(ring.buf.shape) == (64, 2)
    slots = []
    for _ in range(62):
        slots.append(_launch("k")._gabo_record.slot)
    assert slots == list(range(1, 63)) and len(ring.pending) == 62
    assert _launch("k")._gabo_record.slot == 63 and len(ring.pending) == 1           # (the 62 were checked first: all fine)
    assert _launch("k")._gabo_record.slot == 1
    _status.set_error_checking(False)
    word = _launch("k", fail_at=2)
    assert word.data_ptr() == ring.buf.data_ptr() and len(ring.pending) == 2         # slot 0, not registered


def test_two_failures_are_reported_in_registration_order(ring):
    _launch("first", fail_at=4)
    _launch("fine")
    own = torch.zeros(2, dtype=torch.int32)                                           # a word of the caller's own
    _kernel_writes(own, 1, 9)
    _status._raise_if_not_spd(own, "owned")
    _launch("second", fail_at=6)
    assert len(ring.pending) == 3 and len(ops._deferred) == 1
    for want in ("first: input matrix #4 is not positive definite", "second: input matrix #6", "owned: input matrix #9"):
        with pytest.raises(RuntimeError, match=want):
            ops.check_deferred()
    ops.check_deferred()                                                              # all reported: silent
    assert ring.pending == [] and ops._deferred == [] and not ring.buf.any() and not own.any()


def test_sync_mode_raises_at_the_call(ring):
    _status.set_error_checking("sync")
    assert _status.error_checking() is True
    _launch("fine")
    with pytest.raises(RuntimeError, match="bad: input matrix #2"):
        _launch("bad", fail_at=2)
    own = torch.tensor([1, 3], dtype=torch.int32)
    with pytest.raises(RuntimeError, match="owned: input matrix #3"):
        _status._raise_if_not_spd(own, "owned")
    assert ring.pending == [] and ops._deferred == [] and not own.any()


def test_switching_checking_off_and_on_loses_nothing(ring):
    dropped = []
    _launch("before", fail_at=1)
    own = torch.zeros(2, dtype=torch.int32)
    _status._raise_if_not_spd(own, "owned before")
    assert ops.set_error_checking(False) == "deferred"
    assert _launch("unchecked", fail_at=8).data_ptr() == ring.buf.data_ptr()           # the shared word, dirtied; nobody is told
    forced = _launch("forced", fail_at=0, force=True, message="the factor failed", on_fail=lambda: dropped.append(1))
    assert forced._gabo_record.forced and forced._gabo_record.slot != 0
    assert ring.buf[0].tolist() == [1, 8]
    assert ops.set_error_checking("deferred") is False
    assert ring.buf[0].tolist() == [0, 0]                                               # only slot 0 was zeroed ...
    assert ring.pending[1].message == "the factor failed"
    assert len(ring.pending) == 2 and len(ops._deferred) == 1                           # ... and every record is still there
    with pytest.raises(RuntimeError, match="before: input matrix #1"):
        ops.check_deferred()
    assert dropped == []
    with pytest.raises(RuntimeError, match="the factor failed"):
        ops.check_deferred()
    assert dropped == [1]
    ops.check_deferred()
    assert ring.pending == [] and ops._deferred == []


def test_a_forced_record_is_checked_while_checking_is_off(ring):
    ops.set_error_checking(False)
    _launch("forced", fail_at=3, force=True)
    with pytest.raises(RuntimeError, match="forced: input matrix #3"):
        ops.check_deferred()


def test_a_token_overtaken_by_a_check_is_harmless(ring):
    """token over [A]; A is checked by somebody else and a failing B registered before check_prefetched(token): B is none of the token's business"""
    _launch("A")
    token = ops.prefetch_deferred()
    assert token[1] == ring.pending and token[1] is not ring.pending
    ops.check_deferred()
    _launch("B", fail_at=5)
    ops.check_prefetched(token)                                                          # silent, and B is still pending
    assert len(ring.pending) == 1
    with pytest.raises(RuntimeError, match="B: input matrix #5"):
        ops.check_deferred()
    ops.check_deferred()


def test_a_token_checks_exactly_its_own_records(ring):
    _launch("A")
    _launch("B", fail_at=2)
    token = ops.prefetch_deferred()
    _launch("C", fail_at=4)                                                              # behind the copy: not covered by the token
    with pytest.raises(RuntimeError, match="B: input matrix #2"):
        ops.check_prefetched(token)
    assert [r.slot for r in ring.pending] == [3]
    ops.check_prefetched(token)                                                          # nothing of it is left
    assert len(ring.pending) == 1
    with pytest.raises(RuntimeError, match="C: input matrix #4"):
        ops.check_deferred()
    assert ops.prefetch_deferred() is None                                               # nothing pending: nothing to copy
    ops.check_prefetched(None)


def test_prefetch_leaves_the_rings_of_other_streams_alone(ring):
    other = _status._StatusRing("cpu", None)
    _status._status_rings[("host", 1)] = other
    try:
        word = other.take()
        _kernel_writes(word, 1, 6)
        _status._raise_if_not_spd(word, "elsewhere")
        _launch("here")
        token = ops.prefetch_deferred()
        assert token[0] is ring and other.host is None
        ops.check_prefetched(token)
        assert ring.pending == [] and len(other.pending) == 1
        with pytest.raises(RuntimeError, match="elsewhere: input matrix #6"):
            ops.check_deferred()
    finally:
        del _status._status_rings[("host", 1)]


def test_ops_keeps_the_names_the_test_fixtures_use(ring):
    """tests/conftest.py: set_error_checking("deferred"), every ring of ops._status_rings reset, ops._deferred cleared"""
    assert ops._status_rings is _status._status_rings and isinstance(ops._status_rings, dict) and ops._deferred is _status._deferred
    for name in ("set_error_checking", "check_deferred", "prefetch_deferred", "check_prefetched", "_status_word", "_raise_if_not_spd",
                 "_check_launch", "_not_spd_message"):
        assert getattr(ops, name) is getattr(_status, name)
    assert not hasattr(ops, "_StatusRing") and callable(ops._stream_ptr)
    ops.set_error_checking(True)
    assert ops.set_error_checking(False) is True and ops.set_error_checking("sync") is False and ops.set_error_checking("deferred") is True
    with pytest.raises(ValueError, match="True / 'sync', 'deferred' or False"):
        ops.set_error_checking("later")
    assert _status.error_checking() == "deferred"
    _launch("bad", fail_at=1)
    _status._raise_if_not_spd(torch.ones(2, dtype=torch.int32), "owned")
    ops.set_error_checking("deferred")
    for r in ops._status_rings.values():
        r.reset()
    ops._deferred.clear()
    assert ring.pending == [] and not ring.buf.any() and _status._deferred == []
    ops.check_deferred()


def test_check_launch_reports_the_return_code_first(ring):
    dropped = []
    word = _status._status_word(torch.device("cpu"))
    with pytest.raises(RuntimeError, match="refused: libgabo_hip error"):
        _status._check_launch(-1, word, "refused", on_fail=lambda: dropped.append(1))
    assert dropped == [1] and ring.pending == []                                         # a launch that never ran is not registered
    _status._check_launch(0, _status._status_word(torch.device("cpu")), "ran")
    assert len(ring.pending) == 1
