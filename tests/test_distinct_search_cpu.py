"""Host side of the distinct-moment search without a device: the exported symbols, the depth plan, `frame_of`, the argument
checks that come before the device is touched, and the numpy restatement of the definition on a hand-written example."""
import ctypes
from ctypes import POINTER, byref, c_float, c_int, c_int32, c_int64

import numpy as np
import pytest

from index_host_fakes import bare_index
from test_distinct_search import greedy_distinct


def _plan(n, nq, k, gap, mode):
    from video_quierer_amd import _lib
    depth, producer, slices = c_int64(), c_int(), c_int()
    _lib.check(_lib.load().vq_debug_distinct_plan(n, nq, k, gap, mode, byref(depth), byref(producer), byref(slices)))
    return depth.value, producer.value, slices.value


def test_new_symbols_are_exported():
    from video_quierer_amd import _lib
    lib = _lib.load()
    for name in ("vq_index_set_positions", "vq_index_search_distinct", "vq_index_search_distinct_device", "vq_debug_distinct_plan"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    import video_quierer_amd
    video_quierer_amd.install_dropin()
    from indexes.hnsw import HNSWIndex, frame_of                                # noqa: F401
    from video_quierer_amd.overhaul_index import SimpleVideoIndex
    assert callable(HNSWIndex.search_distinct) and callable(HNSWIndex.search_distinct_batch)
    assert callable(SimpleVideoIndex.search_moments)


def test_plan_depth_respects_the_size_and_the_producers_k_limit(monkeypatch):
    monkeypatch.delenv("VQ_AMD_DISTINCT_DEPTH", raising=False)
    for mode in (0, 1, 2):
        for n in (1, 5, 63, 1_500, 16_383, 16_384, 1_000_000):
            last = 0
            for k in (1, 2, 10, 16, 17, 25, 26, 100, 101, 256, 1024):
                for gap in (0, 1, 3, 2 ** 40):
                    depth, producer, slices = _plan(n, 33, k, gap, mode)
                    assert 1 <= depth <= n
                    assert producer == (1 if mode == 2 or (mode == 0 and n >= 16_384) else 0)
                    assert depth <= (100 if producer else 1024)
                    if gap == 0 and k <= (100 if producer else 1024):
                        assert depth == min(k, n) and slices == 0              # nothing is suppressed: the plain search
                    if depth == n:
                        assert slices == 0                                      # the prefix is the whole list
                depth = _plan(n, 33, k, 3, mode)[0]
                assert depth >= last                                            # monotone in k
                last = depth
    assert _plan(16_383, 1, 10, 3, 0)[1] == 0 and _plan(16_384, 1, 10, 3, 0)[1] == 1
    assert _plan(20_000, 1, 10, 3, 2) == (64, 1, 1) and _plan(20_000, 1, 10, 3, 1) == (64, 0, 1)
    assert _plan(20_000, 1, 100, 3, 1)[0] == 400 and _plan(20_000, 1, 100, 3, 2)[0] == 100
    # the redo's distances stay within 512 MiB: 2^27 floats / 1M rows = 128 queries per slice
    assert _plan(1_000_000, 1, 10, 3, 0)[2] == 1 and _plan(1_000_000, 300, 10, 3, 0)[2] == 3
    for bad in ((0, 1, 1, 0, 0), (10, 1, 0, 0, 0), (10, 1, 1025, 0, 0), (10, 1, 1, -1, 0), (10, 1, 1, 0, 3), (10, 0, 1, 0, 0)):
        with pytest.raises(ValueError):
            _plan(*bad)


def test_plan_honours_the_depth_override(monkeypatch):
    monkeypatch.setenv("VQ_AMD_DISTINCT_DEPTH", "16")
    assert _plan(20_000, 5, 10, 3, 2) == (16, 1, 1)
    assert _plan(20_000, 5, 100, 0, 1) == (16, 0, 1)              # a prefix shorter than k leaves queries to the redo
    assert _plan(10, 5, 10, 3, 1) == (10, 0, 0)                   # still capped by the size
    monkeypatch.setenv("VQ_AMD_DISTINCT_DEPTH", "5000")
    assert _plan(20_000, 5, 10, 3, 2)[0] == 100 and _plan(20_000, 5, 10, 3, 1)[0] == 1024
    monkeypatch.setenv("VQ_AMD_DISTINCT_DEPTH", "0")
    assert _plan(20_000, 5, 10, 3, 2)[0] == 64


def test_frame_of():
    from video_quierer_amd.indexes.hnsw import frame_of
    assert frame_of("a_b_12") == 12 and frame_of(7) == 7 and frame_of(np.int64(9)) == 9 and frame_of("v_-3") == -3
    for bad in ("a_b_x", "nounderscore", "12", ("v", 1), 1.5, None, "v_"):
        with pytest.raises(ValueError) as e:
            frame_of(bad)
        assert repr(bad) in str(e.value)


def test_arguments_are_refused_before_the_device_is_touched():
    from video_quierer_amd import _lib
    lib = _lib.load()
    q = np.zeros(4, np.float32); ids = np.zeros(4, np.int32); dist = np.zeros(4, np.float32)
    args = (q.ctypes.data_as(POINTER(c_float)), 1)
    out = (ids.ctypes.data_as(POINTER(c_int32)), dist.ctypes.data_as(POINTER(c_float)))
    for k, gap, word in ((1, -1, b"min_gap"), (0, 3, b"k 0"), (-2, 3, b"k -2"), (1025, 3, b"k 1025")):
        assert lib.vq_index_search_distinct(None, *args, k, 1, gap, *out) == -1
        assert word in lib.vq_last_error()
        assert lib.vq_index_search_distinct_device(None, None, 1, k, 1, gap, None, None) == -1
        assert word in lib.vq_last_error()
    # the wrapper: a negative gap raises, k <= 0 answers [] as the other searches do, neither reaches the library
    idx = bare_index(["a_0", "a_1"], tie_order="device")
    with pytest.raises(ValueError):
        idx.search_distinct(np.ones(4, np.float32), 2, -1)
    with pytest.raises(ValueError):
        idx.search_distinct_batch([np.ones(4, np.float32)], 2, -5)
    assert idx.search_distinct(np.ones(4, np.float32), 0, 3) == []
    assert idx.search_distinct_batch([np.ones(4, np.float32)] * 2, -1, 3) == [[], []]


def test_the_restatement_on_a_hand_written_example():
    #        row:  0    1    2    3    4    5    6    7
    groups = ["a", "a", "a", "b", "b", "a", "c", "a"]
    positions = [10, 11, 14, 10, 10, 2 ** 31 - 1, 0, -2 ** 31]
    order = [1, 0, 3, 2, 4, 7, 5, 6]                               # the plain search's exhaustive list
    assert greedy_distinct(order, groups, positions, 8, 0) == order
    assert greedy_distinct(order, groups, positions, 3, 0) == [1, 0, 3]
    assert greedy_distinct(order, groups, positions, 8, 1) == [1, 0, 3, 2, 7, 5, 6]       # row 4 shares b / 10 with row 3
    assert greedy_distinct(order, groups, positions, 8, 2) == [1, 3, 2, 7, 5, 6]          # row 0 is 1 from row 1
    assert greedy_distinct(order, groups, positions, 8, 4) == [1, 3, 7, 5, 6]             # row 2 is 3 from row 1
    assert greedy_distinct(order, groups, positions, 2, 4) == [1, 3]
    assert greedy_distinct(order, groups, positions, 8, 2 ** 31 - 12) == [1, 3, 7, 5, 6]  # rows 7 and 5 are 2^32 - 1 apart, row 5
    assert greedy_distinct(order, groups, positions, 8, 2 ** 31 - 11) == [1, 3, 7, 6]     # ... is 2^31 - 12 from row 1,
    assert greedy_distinct(order, groups, positions, 8, 2 ** 31 + 11) == [1, 3, 7, 6]     # ... row 7 is 2^31 + 11 from row 1
    assert greedy_distinct(order, groups, positions, 8, 2 ** 31 + 12) == [1, 3, 6]
    assert greedy_distinct(order, groups, positions, 8, 2 ** 40) == [1, 3, 6]             # one row per group
    assert greedy_distinct(order, groups, positions, 8, 4, depth=3) == [1, 3]             # a prefix keeps the kept rows among it
    assert greedy_distinct(order, groups, positions, 8, 4, depth=6) == [1, 3, 7]
