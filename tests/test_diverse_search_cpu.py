"""Host side of the diverse search without a device: the exported symbols, the depth plan's invariants, the argument checks
that come before the device is touched, and the numpy restatement of the definition on a hand-written example."""
from ctypes import POINTER, byref, c_float, c_int, c_int32, c_int64

import numpy as np
import pytest

from index_host_fakes import bare_index
from test_diverse_search import _greedy_fast, greedy_diverse


def _plan(n, nq, k, min_dist, mode):
    from video_quierer_amd import _lib
    depth, producer, pair_bytes, slices, launches = c_int64(), c_int(), c_int64(), c_int(), c_int()
    _lib.check(_lib.load().vq_debug_diverse_plan(n, nq, k, c_float(min_dist), mode, byref(depth), byref(producer), byref(pair_bytes),
                                                 byref(slices), byref(launches)))
    return depth.value, producer.value, pair_bytes.value, slices.value, launches.value


def _distinct_producer(n, mode):
    from video_quierer_amd import _lib
    depth, producer, slices = c_int64(), c_int(), c_int()
    _lib.check(_lib.load().vq_debug_distinct_plan(n, 1, 10, 3, mode, byref(depth), byref(producer), byref(slices)))
    return producer.value


def test_new_symbols_are_exported():
    from video_quierer_amd import _lib
    lib = _lib.load()
    for name in ("vq_index_search_diverse", "vq_index_search_diverse_device", "vq_debug_diverse_plan"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    import video_quierer_amd
    video_quierer_amd.install_dropin()
    from indexes.hnsw import HNSWIndex, OptimizedHNSWIndex
    from video_quierer_amd.overhaul_index import SimpleVideoIndex
    assert callable(HNSWIndex.search_diverse) and callable(HNSWIndex.search_diverse_batch)
    assert callable(OptimizedHNSWIndex.search_diverse) and callable(SimpleVideoIndex.search_diverse)


def test_plan_invariants(monkeypatch):
    monkeypatch.delenv("VQ_AMD_DIVERSE_DEPTH", raising=False)
    for mode in (0, 1, 2):
        for n in (1, 5, 63, 1_500, 16_383, 16_384, 1_000_000):
            last = 0
            for k in (1, 2, 10, 16, 17, 64, 100, 101, 256):
                for min_dist in (0.0, 1e-6, 0.05, 3.0):
                    for nq in (1, 33):
                        depth, producer, pair_bytes, slices, launches = _plan(n, nq, k, min_dist, mode)
                        assert 1 <= depth <= n
                        assert producer == _distinct_producer(n, mode) == (1 if mode == 2 or (mode == 0 and n >= 16_384) else 0)
                        assert depth <= (100 if producer else 1024)
                        if (min_dist == 0 or k == 1) and k <= (100 if producer else 1024):
                            assert depth == min(k, n) and slices == 0 and pair_bytes == 0      # the plain search
                        if depth == n:
                            assert slices == 0                                  # the prefix is the whole list
                        if min_dist > 0 and depth > 1:
                            assert pair_bytes == nq * depth * ((depth + 63) // 64) * 8
                        assert launches >= 1 and (slices > 0) == (launches > 2)
                        if slices:                                              # the redo's distances stay within 512 MiB
                            per_slice = -(-nq // slices)
                            assert per_slice * ((n + 63) // 64 * 64) * 4 <= 512 << 20 or per_slice == 1
                depth = _plan(n, 33, k, 0.05, mode)[0]
                assert depth >= last                                            # monotone in k
                last = depth
    assert _plan(16_383, 1, 10, 0.05, 0)[1] == 0 and _plan(16_384, 1, 10, 0.05, 0)[1] == 1
    assert _plan(1_000_000, 1, 10, 0.05, 0)[3] == 1 and _plan(1_000_000, 300, 10, 0.05, 0)[3] == 3
    assert _plan(1_000_000, 300, 10, 0.0, 0)[3] == 0
    nan = float("nan")
    for bad in ((0, 1, 1, 0.0, 0), (10, 1, 0, 0.0, 0), (10, 1, 257, 0.0, 0), (10, 1, 1, -1e-3, 0), (10, 1, 1, nan, 0), (10, 1, 1, 0.0, 3),
                (10, 0, 1, 0.0, 0), (2 ** 31, 1, 1, 0.0, 0)):
        with pytest.raises(ValueError):
            _plan(*bad)


def test_plan_honours_the_depth_override(monkeypatch):
    rule = _plan(20_000, 5, 10, 0.05, 1)[0]
    monkeypatch.setenv("VQ_AMD_DIVERSE_DEPTH", "16")
    assert _plan(20_000, 5, 10, 0.05, 2)[:4] == (16, 1, 5 * 16 * 8, 1)
    assert _plan(20_000, 5, 100, 0.0, 1)[:4] == (16, 0, 0, 1)     # a prefix shorter than k leaves queries to the redo
    assert _plan(20_000, 5, 10, 0.0, 1)[:4] == (16, 0, 0, 0)      # ... one that holds k rows does not
    assert _plan(20_000, 5, 1, 0.05, 1)[3] == 0                   # k = 1: the first row is always kept
    assert _plan(10, 5, 10, 0.05, 1)[:4] == (10, 0, 5 * 10 * 8, 0)               # still capped by the size
    monkeypatch.setenv("VQ_AMD_DIVERSE_DEPTH", "65")
    assert _plan(20_000, 3, 10, 0.05, 1)[:3] == (65, 0, 3 * 65 * 2 * 8)
    monkeypatch.setenv("VQ_AMD_DIVERSE_DEPTH", "5000")
    assert _plan(20_000, 5, 10, 0.05, 2)[0] == 100 and _plan(20_000, 5, 10, 0.05, 1)[0] == 1024
    monkeypatch.setenv("VQ_AMD_DIVERSE_DEPTH", "0")
    assert _plan(20_000, 5, 10, 0.05, 1)[0] == rule


def test_arguments_are_refused_before_the_device_is_touched():
    from video_quierer_amd import _lib
    lib = _lib.load()
    q = np.zeros(4, np.float32); ids = np.zeros(4, np.int32); dist = np.zeros(4, np.float32)
    qp = q.ctypes.data_as(POINTER(c_float))
    out = (ids.ctypes.data_as(POINTER(c_int32)), dist.ctypes.data_as(POINTER(c_float)))
    nan = float("nan")
    for nq, k, md, word in ((1, 1, -1.0, b"min_dist"), (1, 1, nan, b"min_dist"), (1, 0, 0.05, b"k 0"), (1, -2, 0.05, b"k -2"),
                            (1, 257, 0.05, b"k 257"), (0, 1, 0.05, b"nq 0"), (-1, 1, 0.05, b"nq -1")):
        assert lib.vq_index_search_diverse(None, qp, nq, k, 1, c_float(md), *out) == -1
        assert word in lib.vq_last_error()
        assert lib.vq_index_search_diverse_device(None, None, nq, k, 1, c_float(md), None, None) == -1
        assert word in lib.vq_last_error()
    # the wrappers: a negative or NaN threshold raises, k <= 0 answers [] as the other searches do, neither reaches the library
    idx = bare_index(["a_0", "a_1"], tie_order="device")
    for bad in (-1e-3, nan):
        with pytest.raises(ValueError):
            idx.search_diverse(np.ones(4, np.float32), 2, bad)
        with pytest.raises(ValueError):
            idx.search_diverse_batch([np.ones(4, np.float32)], 2, bad)
    assert idx.search_diverse(np.ones(4, np.float32), 0, 0.05) == []
    assert idx.search_diverse_batch([np.ones(4, np.float32)] * 2, -1, 0.05) == [[], []]
    assert idx.search_diverse_batch([], 3, 0.05) == []
    assert bare_index().search_diverse(np.ones(4, np.float32), 3) == []
    from video_quierer_amd.overhaul_index import SimpleVideoIndex
    sv = SimpleVideoIndex()
    for bad in (1.0001, nan):
        with pytest.raises(ValueError):
            sv.search_diverse(np.ones(4, np.float32), 3, bad)
    assert sv.search_diverse(np.ones(4, np.float32), 3) == []


def test_the_restatement_on_a_hand_written_example():
    # eight rows on a line of "looks": 0 and 1 are one shot, 2 is a bit-exact copy of 0 (its distance to 0 is the -1.2e-7 an exact
    # copy of a unit row may give), 3 and 4 are a second shot, 5, 6, 7 stand alone
    look = np.array([0.00, 0.01, 0.00, 0.50, 0.53, 1.00, 1.50, 2.00], dtype=np.float32)
    D = np.abs(look[:, None] - look[None, :]).astype(np.float32)
    D[0, 2] = D[2, 0] = np.float32(-1.2e-7)
    assert np.array_equal(D, D.T)
    order = [2, 0, 1, 4, 3, 5, 7, 6]                               # the plain search's exhaustive list

    def pair(s):
        return D[s]
    for greedy in (greedy_diverse, _greedy_fast):
        assert greedy(order, pair, 8, 0.0) == order               # min_dist 0: nothing is suppressed, not even the copy at d < 0
        assert greedy(order, pair, 3, 0.0) == [2, 0, 1]
        assert greedy(order, pair, 8, 1e-6) == [2, 1, 4, 3, 5, 7, 6]              # the copy goes
        assert greedy(order, pair, 8, 0.01) == [2, 1, 4, 3, 5, 7, 6]              # strict: row 1 at exactly 0.01 stays
        assert greedy(order, pair, 8, 0.02) == [2, 4, 3, 5, 7, 6]                 # row 3 is 0.03 from row 4
        assert greedy(order, pair, 2, 0.02) == [2, 4]                             # the answer for k is a prefix
        assert greedy(order, pair, 8, 0.05) == [2, 4, 5, 7, 6]
        assert greedy(order, pair, 8, 0.51) == [2, 4, 7]                          # row 5 is 0.47 from row 4, row 6 is 0.5 from row 7
        assert greedy(order, pair, 8, 0.6) == [2, 5, 7]                           # a dropped row (4) suppresses nothing
        assert greedy(order, pair, 8, 3.0) == [2]                                 # above every pair distance: one row
        assert greedy(order, pair, 8, 0.02, depth=3) == [2]                       # a prefix keeps the kept rows among it
        assert greedy(order, pair, 8, 0.02, depth=5) == [2, 4, 3]
        assert greedy(order, pair, 8, 0.0, depth=5) == order[:5]
