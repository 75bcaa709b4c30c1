"""Host side of the clip search (HNSWIndex.search_set / similar_groups, SimpleVideoIndex.similar_videos) without a device:
which labels and flags reach vq_index_search_set, `within` and the self-exclusion folded into one include list, the error
cases, the short cuts that make no device call, and the shape of the result dicts."""
import numpy as np
import pytest

from index_host_fakes import bare_index as _index, fake_lib, fill


def _fake(monkeypatch, stored=None):
    def read_rows(calls, h, rn, n, out):
        calls.append(("read_rows", [rn[i] for i in range(n)]))
        fill(out, stored[[rn[i] for i in range(n)]].reshape(-1).tolist())

    def search_set(calls, h, q, m, k, mode, sel, n_sel, exclude, groups, dist, rows):
        calls.append(("search_set", m, k, mode, [sel[i] for i in range(n_sel)], exclude, bool(rows), [q[i] for i in range(m * 4)]))
        fill(groups, [1] + [-1] * (k - 1)), fill(dist, [np.float32(0.25)] + [np.inf] * (k - 1))      # group 1 first, then nothing
        if rows:
            fill(rows, [(2 if i % 2 == 0 else 5) if i < m else -1 for i in range(k * m)])

    return fake_lib(monkeypatch, vq_index_read_rows=read_rows, vq_index_search_set=search_set)


IDS = ["a_0", "a_1", "b_0", "c_0", "c_1", "b_1"]        # videos a, b, c -> labels 0, 1, 2
Q = np.ones(4, dtype=np.float32)


def test_labels_flags_and_normalised_queries_reach_the_library(monkeypatch):
    calls = _fake(monkeypatch)
    idx = _index(IDS)
    res = idx.search_set([Q, 2 * Q, Q], 2)
    assert calls[0] == ("set_id_ranks", 6) and calls[1] == ("set_groups", [0, 0, 1, 2, 2, 1], 3)
    name, m, k, mode, sel, excl, want_rows, q = calls[2]
    assert (name, m, k, mode, sel, excl, want_rows) == ("search_set", 3, 2, 0, [], 1, False)      # no filter: nothing excluded
    assert q == [0.5] * 12                                        # every frame normalised, as search() does
    assert res == [{"group": "b", "distance": np.float32(0.25), "score": np.float32(0.75)}]
    assert type(res[0]["distance"]) is np.float32 and type(res[0]["score"]) is np.float32
    idx.search_mode = 2
    res = idx.search_set([Q, Q], 9, within=["c", "b", "nope", "c"], matches=True)
    assert calls[3][:7] == ("search_set", 2, 3, 2, [1, 2], 0, True) and len(calls) == 4          # k capped at the groups; labels current
    assert res == [{"group": "b", "distance": np.float32(0.25), "score": np.float32(0.75), "matches": ["b_0", "b_1"]}]
    idx.search_set([Q], 1, exclude=iter(["a", "zzz"]))
    assert calls[4][:7] == ("search_set", 1, 1, 2, [0], 1, False)
    meta = {nid: "V" + nid[0] for nid in IDS}
    idx.search_set([Q], 1, within=["Vc"], group_of=meta.__getitem__)
    assert calls[-1][:7] == ("search_set", 1, 1, 2, [2], 0, False)


def test_errors_and_short_cuts_make_no_device_call(monkeypatch):
    calls = _fake(monkeypatch)
    idx = _index(IDS)
    with pytest.raises(ValueError):
        idx.search_set([], 3)                                     # an empty clip
    with pytest.raises(ValueError):
        idx.search_set([Q], 3, within=["a"], exclude=["b"])
    with pytest.raises(ValueError):
        idx.search_set([Q], 3, within="a")
    with pytest.raises(ValueError):
        idx.search_set([np.ones(5, dtype=np.float32)], 3)         # the dimension is checked
    with pytest.raises(ValueError, match="4096"):
        idx.search_set(np.ones((4097, 4), dtype=np.float32), 3)
    assert idx.search_set([Q], 0) == []
    assert idx.search_set([Q], -1) == []
    assert idx.search_set([Q], 3, within=[]) == []
    empty = _index([])
    assert empty.search_set([Q], 3) == []
    with pytest.raises(ValueError):
        empty.search_set([], 3)
    assert calls == []
    assert idx.search_set([Q], 3, within=["unknown"]) == []       # nothing known: labels synced, no search
    assert [c[0] for c in calls] == ["set_id_ranks", "set_groups"]


def test_similar_groups_reads_the_stored_rows_and_folds_the_filters(monkeypatch):
    stored = np.arange(24, dtype=np.float32).reshape(6, 4)
    calls = _fake(monkeypatch, stored)
    idx = _index(IDS)
    res = idx.similar_groups("b", 2, matches=True)
    assert calls[0] == ("read_rows", [2, 5])                      # the rows of b, in row order
    assert [c[0] for c in calls[1:]] == ["set_id_ranks", "set_groups", "search_set"]
    assert calls[3][:7] == ("search_set", 2, 2, 0, [1], 1, True)                                # b itself excluded
    assert calls[3][7] == stored[[2, 5]].reshape(-1).tolist()     # used as stored: not normalised again
    assert res[0]["group"] == "b" and res[0]["matches"] == ["b_0", "b_1"]
    idx.similar_groups("b", 2, within=["c", "b", "a"])
    assert calls[-1][:7] == ("search_set", 2, 2, 0, [0, 2], 0, False)                           # one include list without b
    n = len(calls)
    assert idx.similar_groups("b", 2, within=["b"]) == []         # nothing left: no search
    assert idx.similar_groups("b", 0) == []
    assert len(calls) == n
    with pytest.raises(KeyError):
        idx.similar_groups("nope", 2)
    with pytest.raises(ValueError):
        idx.similar_groups("b", 2, within="a")
    big = _index([f"v_{i}" for i in range(4097)] + ["w_0"])
    with pytest.raises(ValueError, match="4096"):
        big.similar_groups("v", 2)


def test_similar_videos_groups_by_video_name(monkeypatch):
    from video_quierer_amd import overhaul_index
    calls = _fake(monkeypatch, np.ones((5, 4), dtype=np.float32))
    svi = overhaul_index.SimpleVideoIndex()
    with pytest.raises(KeyError):
        svi.similar_videos("x.mp4")
    for name, t in (("x.mp4", 0.0), ("y.mp4", 0.0), ("x.mp4", 1.0), ("z.mp4", 0.0), ("y.mp4", 1.0)):
        svi.add_frame(np.ones(4, dtype=np.float32), name, t)
    dev = _index([-i for i in range(5)])
    dev._tie_order = "device"
    svi._dev, svi._pushed = dev, 5                                # as _sync_device leaves it
    res = svi.similar_videos("y.mp4", 3)
    assert calls[0] == ("read_rows", [1, 4])
    assert calls[1] == ("set_groups", [0, 1, 0, 2, 1], 3)
    assert calls[2][:7] == ("search_set", 2, 3, 0, [1], 1, False)
    assert res == [{"video_name": "y.mp4", "score": 0.75}] and type(res[0]["score"]) is float
    with pytest.raises(KeyError):
        svi.similar_videos("nope.mp4")
