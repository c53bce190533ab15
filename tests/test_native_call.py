"""CPU: ``runtime.call``, the one place the library's calling convention is written down — a forward ends in ``(..., stream)``, or
in ``(..., ws, ws_bytes, stream)`` when it takes scratch — and the frame-layout helpers beside it.  The library is a stub that records
what it is called with (the technique of test_graph_cache.py): no GPU, no libsfnative."""
import ctypes

import pytest
import torch

from streamingflow_amd import runtime

STREAM = 0x5EED


class _StubLib:
    def __init__(self):
        self.calls, self.queries, self.status = [], [], 0

    def sf_foo_fwd(self, *args):
        self.calls.append(("sf_foo_fwd", args))
        return self.status

    def sf_foo_ws_bytes(self, *dims):
        self.queries.append(("sf_foo_ws_bytes", dims))
        return 4000

    def sf_lift_index_rig_fwd(self, *args):
        self.calls.append(("sf_lift_index_rig_fwd", args))
        return 0

    def sf_lift_index_ws_bytes(self, *dims):
        self.queries.append(("sf_lift_index_ws_bytes", dims))
        return 512

    def sf_status_string(self, status):
        return b"workspace too small" if status == 7 else b"?"


@pytest.fixture
def stub(monkeypatch):
    s = _StubLib()
    monkeypatch.setattr(runtime._lib, "lib", lambda: s)
    monkeypatch.setattr(runtime, "stream_ptr", lambda device=None: ctypes.c_void_p(STREAM))
    return s


class _Workspace:
    """Stands in for runtime.workspace: records its arguments and hands out a CPU buffer of `numel` floats."""

    def __init__(self, numel):
        self.asked, self.buf = [], torch.zeros(numel)

    def __call__(self, nbytes, device):
        self.asked.append((nbytes, device))
        return self.buf


def _tail(args, n):
    return [a.value if isinstance(a, ctypes.c_void_p) else a for a in args[len(args) - n:]]


def test_query_form_asks_once_and_appends_pointer_bytes_stream(stub, monkeypatch):
    ws = _Workspace(1500)
    monkeypatch.setattr(runtime, "workspace", ws)
    a, b = object(), ctypes.c_void_p(77)
    got = runtime.call("foo", a, b, 3, 2.5, device="dev0", scratch=("foo", 64, 2, 8, 16))
    assert stub.queries == [("sf_foo_ws_bytes", (64, 2, 8, 16))]
    assert ws.asked == [(4000, "dev0")]
    (name, args), = stub.calls
    assert name == "sf_foo_fwd" and len(args) == 7
    assert args[0] is a and args[1] is b and args[2:4] == (3, 2.5)
    assert _tail(args, 3) == [ws.buf.data_ptr(), 1500 * 4, STREAM]       # the size of the buffer handed out, not of the query
    assert got is ws.buf


def test_a_monkeypatched_workspace_is_the_one_used(stub, monkeypatch):
    """tests/test_gpu_workspace_exact.py replaces runtime.workspace after the package is imported: the lookup is at call time."""
    first, second = _Workspace(1024), _Workspace(1000)
    monkeypatch.setattr(runtime, "workspace", first)
    runtime.call("foo", 1, device=None, scratch=("foo", 1))
    monkeypatch.setattr(runtime, "workspace", second)
    runtime.call("foo", 2, device=None, scratch=("foo", 1))
    assert len(first.asked) == 1 and len(second.asked) == 1
    assert _tail(stub.calls[0][1], 3) == [first.buf.data_ptr(), 4096, STREAM]
    assert _tail(stub.calls[1][1], 3) == [second.buf.data_ptr(), 4000, STREAM]


def test_tensor_form_makes_no_query(stub, monkeypatch):
    ws = _Workspace(1)
    monkeypatch.setattr(runtime, "workspace", ws)
    own = torch.zeros(300)
    got = runtime.call(stub.sf_foo_fwd, 9, device=None, scratch=own)
    assert stub.queries == [] and ws.asked == []
    (_, args), = stub.calls
    assert args[0] == 9 and _tail(args, 3) == [own.data_ptr(), 1200, STREAM] and len(args) == 4
    assert got is own


def test_without_scratch_only_the_stream_is_appended(stub, monkeypatch):
    ws = _Workspace(1)
    monkeypatch.setattr(runtime, "workspace", ws)
    assert runtime.call("foo", 5, 6, device=None) is None
    (_, args), = stub.calls
    assert args[:2] == (5, 6) and len(args) == 3 and args[2].value == STREAM
    assert stub.queries == [] and ws.asked == []


def test_the_query_may_carry_another_name_than_the_forward(stub, monkeypatch):
    ws = _Workspace(256)
    monkeypatch.setattr(runtime, "workspace", ws)
    runtime.call("lift_index_rig", 1, 2, device="d", scratch=("lift_index", 1000, 40))
    assert stub.queries == [("sf_lift_index_ws_bytes", (1000, 40))] and ws.asked == [(512, "d")]
    (name, args), = stub.calls
    assert name == "sf_lift_index_rig_fwd" and _tail(args, 3) == [ws.buf.data_ptr(), 1024, STREAM]


@pytest.mark.parametrize("by_name", [True, False])
def test_a_non_zero_status_raises_with_the_entry_point_and_the_status_text(stub, by_name):
    stub.status = 7
    with pytest.raises(RuntimeError) as e:
        runtime.call("foo" if by_name else stub.sf_foo_fwd, 1, device=None)
    assert "sf_foo_fwd" in str(e.value) and "workspace too small" in str(e.value) and "(7)" in str(e.value)


def _nhwc(x):       # what runtime.to_nhwc computes, on the CPU
    return x.permute(0, 2, 3, 1).contiguous()


def _frames():
    b, T, C, h, w = 2, 3, 4, 2, 5
    return torch.arange(b * T * C * h * w, dtype=torch.float32).view(b, T, C, h, w)


def test_frames_first_and_last_are_inverse_views_of_the_documented_layouts():
    x = _frames()
    b, T, C, h, w = x.shape
    flat = _nhwc(x.reshape(b * T, C, h, w))                     # [b * T, h, w, C], sample-major
    y = runtime.frames_first(flat, b)
    assert tuple(y.shape) == (T, b, h, w, C) and y.is_contiguous()
    for t, bi, yy, xx, c in [(0, 0, 0, 0, 0), (2, 1, 1, 4, 3), (1, 0, 1, 2, 3), (2, 0, 0, 4, 1), (0, 1, 1, 0, 2)]:
        assert y[t, bi, yy, xx, c] == x[bi, t, c, yy, xx]
    assert torch.equal(y, x.permute(1, 0, 3, 4, 2))
    back = runtime.frames_last(y)
    assert tuple(back.shape) == (b * T, h, w, C) and torch.equal(back, flat)


def test_frames_to_nhwc_and_back_round_trip_with_one_transpose_each(monkeypatch):
    calls = []
    monkeypatch.setattr(runtime, "to_nhwc", lambda t: calls.append(("nhwc", tuple(t.shape))) or _nhwc(t))
    monkeypatch.setattr(runtime, "to_nchw", lambda t: calls.append(("nchw", tuple(t.shape))) or t.permute(0, 3, 1, 2).contiguous())
    x = _frames()
    b, T, C, h, w = x.shape
    y = runtime.frames_to_nhwc(x)
    assert tuple(y.shape) == (T, b, h, w, C) and y.is_contiguous() and torch.equal(y, x.permute(1, 0, 3, 4, 2))
    z = runtime.frames_to_nchw(y)
    assert tuple(z.shape) == (b, T, C, h, w) and torch.equal(z, x)
    assert calls == [("nhwc", (b * T, C, h, w)), ("nchw", (b * T, h, w, C))]
