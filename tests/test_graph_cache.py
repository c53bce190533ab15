"""CPU: ``runtime.GraphCache``, the bounded cache of captured hipGraphs that the one-shot rollout and the streaming session share.
The library is replaced by a stub that records what is destroyed and launched; entries are inserted directly (no capture, no GPU)."""
import ctypes
import gc

import pytest

from streamingflow_amd import runtime


class _StubLib:
    def __init__(self):
        self.destroyed, self.launched = [], []

    def sf_graph_destroy(self, ex):
        self.destroyed.append(ex.value)
        return 0

    def sf_graph_launch(self, ex, stream):
        self.launched.append(ex.value)
        return 0


@pytest.fixture
def stub(monkeypatch):
    s = _StubLib()
    monkeypatch.setattr(runtime._lib, "lib", lambda: s)
    monkeypatch.setattr(runtime, "stream_ptr", lambda device=None: ctypes.c_void_p(0))
    return s


def _entry(handle):
    return {"exec": ctypes.c_void_p(handle), "out": object()}


def test_limit_holds_at_the_insertion_that_exceeds_it_and_least_recently_used_leaves(stub):
    cache = runtime.GraphCache()
    entries = {k: _entry(10 + k) for k in range(5)}
    for k in range(3):
        cache.insert(k, entries[k], 3)
        assert len(cache) == k + 1 and stub.destroyed == []
    cache.replay(entries[0], None)                 # 0 becomes the most recently used: 1 is now the oldest
    assert stub.launched == [10] and list(cache) == [1, 2, 0]
    cache.insert(3, entries[3], 3)
    assert list(cache) == [2, 0, 3] and stub.destroyed == [11]
    cache.replay(entries[2], None)
    cache.insert(4, entries[4], 3)
    assert list(cache) == [3, 2, 4] and stub.destroyed == [11, 10]
    assert 2 in cache and 0 not in cache and cache[4] is entries[4]


def test_a_limit_lowered_between_insertions_is_honoured(stub):
    cache = runtime.GraphCache()
    for k in range(4):
        cache.insert(k, _entry(20 + k), 4)
    assert len(cache) == 4 and stub.destroyed == []
    cache.insert(4, _entry(24), 2)                 # the owner's limit is read at every insertion
    assert list(cache) == [3, 4] and stub.destroyed == [20, 21, 22]


def test_drop_destroys_the_rest_once_each_and_skips_entries_without_a_graph(stub):
    cache = runtime.GraphCache()
    cache.insert("a", _entry(31), 2)
    cache["stand-in"] = {"out": object()}          # plain mapping use, no "exec": never handed to the library
    cache.insert("b", _entry(32), 2)               # 3 entries > 2: "a" leaves
    assert stub.destroyed == [31] and list(cache) == ["stand-in", "b"]
    cache.insert("c", _entry(33), 2)               # the entry without a graph leaves: nothing to destroy
    assert stub.destroyed == [31] and list(cache) == ["b", "c"]
    cache["none"] = {"exec": None}
    cache.drop()
    assert len(cache) == 0 and "b" not in cache and stub.destroyed == [31, 32, 33]
    cache.drop()
    assert stub.destroyed == [31, 32, 33]


def test_deleting_the_cache_calls_nothing(stub):
    cache = runtime.GraphCache()
    cache.insert("a", _entry(41), 4)
    cache["k"] = {"exec": ctypes.c_void_p(1)}
    del cache
    gc.collect()
    assert stub.destroyed == [] and stub.launched == []
