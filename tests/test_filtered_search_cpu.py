"""Host side of the filtered search (HNSWIndex.search_filtered / search_filtered_batch, search_grouped(within=, exclude=)) without
a device: the within / exclude argument checks, which labels reach the library, and the empty-within short cut."""
import numpy as np
import pytest

from index_host_fakes import bare_index as _index, fake_lib, fill, nothing


def _search_filtered(calls, h, q, nq, k, mode, sel, n_sel, exclude, ids, dist):
    calls.append(("search_filtered", k, mode, [sel[i] for i in range(n_sel)], exclude))
    nothing((ids, -1), (dist, np.inf))(nq * k)
    for j in range(nq):                                       # row 2 first, then nothing
        fill(ids, [2], j * k), fill(dist, [np.float32(0.25)], j * k)


def _search_grouped_filtered(calls, h, q, nq, k, mode, sel, n_sel, exclude, groups, rows, dist):
    calls.append(("search_grouped_filtered", k, mode, [sel[i] for i in range(n_sel)], exclude))
    nothing((groups, -1), (rows, -1), (dist, np.inf))(nq * k)
    for j in range(nq):
        fill(groups, [1], j * k), fill(rows, [2], j * k), fill(dist, [np.float32(0.25)], j * k)


def _fake(monkeypatch):
    return fake_lib(monkeypatch, vq_index_search_filtered=_search_filtered, vq_index_search_grouped_filtered=_search_grouped_filtered)


IDS = ["a_0", "a_1", "b_0", "c_0", "c_1", "b_1"]        # videos a, b, c -> labels 0, 1, 2
Q = np.ones(4, dtype=np.float32)


def test_keys_map_to_sorted_unique_labels_and_unknown_keys_are_dropped(monkeypatch):
    calls = _fake(monkeypatch)
    idx = _index(IDS)
    res = idx.search_filtered(Q, 3, within=["c", "b", "nope", "c"])
    assert calls[0] == ("set_id_ranks", 6) and calls[1] == ("set_groups", [0, 0, 1, 2, 2, 1], 3)
    assert calls[2] == ("search_filtered", 3, 0, [1, 2], 0)
    assert res == [{"id": "b_0", "distance": np.float32(0.25), "score": np.float32(0.75)}]
    assert type(res[0]["distance"]) is np.float32 and type(res[0]["score"]) is np.float32
    idx.search_filtered_batch([Q, Q], 2, exclude=iter(["a", "zzz"]))          # any iterable; one call for the batch
    assert calls[3] == ("search_filtered", 2, 0, [0], 1) and len(calls) == 4   # labels are current: no re-upload
    idx.search_filtered(Q, 2, exclude=["zzz"])                                # excluding nothing known: still one call
    assert calls[4] == ("search_filtered", 2, 0, [], 1)
    idx.search_mode = 1
    idx.search_filtered(Q, 9, within={"a"})                                   # k above the rows: capped as search() caps it
    assert calls[5] == ("search_filtered", 6, 1, [0], 0)


def test_group_of_maps_keys_like_search_grouped(monkeypatch):
    calls = _fake(monkeypatch)
    idx = _index(IDS)
    meta = {nid: "V" + nid[0] for nid in IDS}
    fn = meta.__getitem__
    idx.search_filtered(Q, 2, within=["Vb"], group_of=fn)
    assert calls[-1] == ("search_filtered", 2, 0, [1], 0)


def test_within_and_exclude_are_checked(monkeypatch):
    calls = _fake(monkeypatch)
    idx = _index(IDS)
    for kw in ({}, {"within": ["a"], "exclude": ["b"]}, {"within": "a"}, {"exclude": b"a"}, {"within": 3}):
        with pytest.raises(ValueError):
            idx.search_filtered(Q, 2, **kw)
        with pytest.raises(ValueError):
            idx.search_filtered_batch([Q], 2, **kw)
    with pytest.raises(ValueError):
        idx.search_grouped(Q, 2, within=["a"], exclude=["b"])
    with pytest.raises(ValueError):
        idx.search_grouped_batch([Q], 2, within="a")
    with pytest.raises(ValueError):                                            # the query's dimension is still checked
        idx.search_filtered(np.ones(5, dtype=np.float32), 2, within=["a"])
    empty = _index([])
    with pytest.raises(ValueError):                                            # checked before the empty-index answer
        empty.search_filtered(Q, 2)
    assert empty.search_filtered(Q, 2, within=["a"]) == []
    assert calls == []


def test_empty_within_answers_without_a_device_call(monkeypatch):
    calls = _fake(monkeypatch)
    idx = _index(IDS)
    assert idx.search_filtered(Q, 3, within=[]) == []
    assert idx.search_filtered_batch([Q, Q], 3, within=()) == [[], []]
    assert idx.search_grouped(Q, 3, within=[]) == []
    assert calls == []
    assert idx.search_filtered_batch([Q], 3, within=["unknown"]) == [[]]      # nothing known: labels synced, no search
    assert [c[0] for c in calls] == ["set_id_ranks", "set_groups"]


def test_grouped_filter_reaches_the_filtered_entry_point(monkeypatch):
    calls = _fake(monkeypatch)
    idx = _index(IDS)
    res = idx.search_grouped(Q, 2, exclude=["a"])
    assert calls[-1] == ("search_grouped_filtered", 2, 0, [0], 1)
    assert res == [{"group": "b", "id": "b_0", "distance": np.float32(0.25), "score": np.float32(0.75)}]
    idx.search_grouped_batch([Q], 5, within=["c", "a"])
    assert calls[-1] == ("search_grouped_filtered", 3, 0, [0, 2], 0)
    idx.search_grouped(Q, 2)                                                   # no filter: today's entry point
    assert calls[-1] == ("search_grouped", 2)
