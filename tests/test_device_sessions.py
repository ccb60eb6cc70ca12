"""The life cycle that every native session object shares (runtime._DeviceSession): closed once, closed by its
context before the handle goes, never touched again afterwards.  No GPU: a stub subclass records its destroy calls."""
import ctypes as C
import gc
import weakref

import pytest

from alphadia_amd import runtime


class FakeContext:
    """What a session needs of a Context: a handle and the set of live sessions."""

    def __init__(self):
        self._h = C.c_void_p(0x1000)
        self._sessions = weakref.WeakSet()

    def close(self):
        if self._h:
            runtime.Context._close_sessions(self)
            self._h = C.c_void_p()


class StubSession(runtime._DeviceSession):
    def __init__(self, ctx, log, fail=False):
        super().__init__(ctx)
        self._s = C.c_void_p(0x2000 + len(log["created"]))
        log["created"].append(self._s.value)
        self._log, self._fail = log, fail

    def _native_destroy(self, s):
        # (handle destroyed, was the context's handle alive?)
        self._log["destroyed"].append((s.value, bool(self._ctx._h)))
        if self._fail:
            raise RuntimeError("destroy failed")


@pytest.fixture
def log():
    return {"created": [], "destroyed": []}


def test_close_destroys_once(log):
    s = StubSession(FakeContext(), log)
    s.close()
    s.close()
    del s
    gc.collect()
    assert log["destroyed"] == [(0x2000, True)]


def test_del_swallows_a_failing_destroy(log):
    s = StubSession(FakeContext(), log, fail=True)
    with pytest.raises(RuntimeError):
        s.close()
    assert not s._s  # the handle is given up before the call: no second destroy
    t = StubSession(s._ctx, log, fail=True)
    t.__del__()  # must not raise
    assert [d[0] for d in log["destroyed"]] == [0x2000, 0x2001]


def test_context_closes_its_live_sessions_first(log):
    ctx = FakeContext()
    a, b = StubSession(ctx, log), StubSession(ctx, log)
    ctx.close()
    assert sorted(log["destroyed"]) == [(0x2000, True), (0x2001, True)]  # each saw a live context handle
    assert not ctx._h and not a._s and not b._s
    a.close()
    b.__del__()
    del a, b
    gc.collect()
    assert len(log["destroyed"]) == 2  # no native call after the context went


def test_context_skips_collected_sessions(log):
    ctx = FakeContext()
    a, b = StubSession(ctx, log), StubSession(ctx, log)
    del a
    gc.collect()
    assert log["destroyed"] == [(0x2000, True)] and len(ctx._sessions) == 1
    ctx.close()
    assert log["destroyed"] == [(0x2000, True), (0x2001, True)]
    assert not b._s


class FakeLib:
    """Stands in for the loaded library: records adh_destroy among the sessions' destroys."""

    def __init__(self, order):
        self._order = order

    def adh_destroy(self, h):
        self._order.append(("adh_destroy", h.value))


class FakePinned:
    def close(self):
        pass


def test_real_context_closes_sessions_before_the_handle(log, monkeypatch):
    ctx = runtime.Context.__new__(runtime.Context)  # no adh_create: the real close() on a made-up handle
    ctx._h, ctx._sessions, ctx.pinned = C.c_void_p(0x1000), weakref.WeakSet(), FakePinned()
    order = log["destroyed"]
    monkeypatch.setattr(runtime, "lib", FakeLib(order))
    a, b = StubSession(ctx, log), StubSession(ctx, log)
    ctx.close()
    assert sorted(order[:2]) == [(0x2000, True), (0x2001, True)] and order[2:] == [("adh_destroy", 0x1000)]
    assert not ctx._h and not a._s and not b._s
    ctx.close()
    del a, b
    gc.collect()
    assert len(order) == 3


SESSION_CLASSES = ["DeviceMlp", "DeviceQuant", "DeviceProteinGroups", "DeviceProteinFdr", "DeviceTransferLibrary",
                   "DeviceMbr"]


@pytest.mark.parametrize("name", SESSION_CLASSES)
def test_real_sessions_share_the_life_cycle(name, monkeypatch):
    cls = getattr(runtime, name)
    assert issubclass(cls, runtime._DeviceSession)
    assert "close" not in vars(cls) and "__del__" not in vars(cls)
    # its own part is the call of one destroy export, with the handle it is given

    class Recorder:
        def __init__(self):
            self.calls = []

        def __getattr__(self, export):
            return lambda *args: self.calls.append((export, args))

    rec = Recorder()
    monkeypatch.setattr(runtime, "lib", rec)
    s = cls.__new__(cls)
    s._ctx, s._s = FakeContext(), C.c_void_p(0x3000)
    s.close()
    s.close()
    assert len(rec.calls) == 1 and rec.calls[0][0].endswith("_destroy") and rec.calls[0][0] in runtime.EXPORTED_SYMBOLS
    assert rec.calls[0][1][0].value == 0x3000
