"""Host-side bookkeeping of row removal (HNSWIndex.remove / remove_batch / remove_group, SimpleVideoIndex.remove_video) without
a device: which row numbers reach vq_index_remove_rows, and that no search afterwards re-uploads ranks or labels."""
import numpy as np
import pytest

from index_host_fakes import bare_index, fake_lib as _fake


def _index(ids, tie_order="device", identity=False):
    return bare_index(ids, tie_order=tie_order, identity=identity)


def _consistent(idx):
    assert idx._row_of == {nid: r for r, nid in enumerate(idx._ids)}
    assert idx.element_count == len(idx._ids)
    assert idx.entry_point == (idx._ids[0] if idx._ids else None)


IDS = ["a_0", "a_1", "b_0", "c_0", "c_1", "b_1", "c_2", "d_0"]


def test_remove_batch_passes_sorted_unique_rows_and_compacts_the_ids(monkeypatch):
    calls = _fake(monkeypatch)
    idx = _index(IDS)
    ids_list = idx._ids
    assert idx.remove_batch(["c_1", "a_1", "c_1"]) == 2          # duplicate tolerated, removed once
    assert calls == [("remove", [1, 4])]
    assert idx._ids is ids_list                                   # compacted in place
    assert idx._ids == ["a_0", "b_0", "c_0", "b_1", "c_2", "d_0"]
    _consistent(idx)
    idx.remove("a_0")
    assert calls[-1] == ("remove", [0]) and idx.entry_point == "b_0"
    _consistent(idx)
    with pytest.raises(KeyError):
        idx.remove("a_0")
    assert idx.remove_batch([]) == 0 and len(calls) == 2


def test_remove_batch_changes_nothing_on_an_unknown_id(monkeypatch):
    calls = _fake(monkeypatch)
    idx = _index(IDS)
    with pytest.raises(KeyError):
        idx.remove_batch(["a_0", "nope", "b_0"])
    assert calls == [] and idx._ids == IDS and idx.element_count == len(IDS)
    _consistent(idx)


def test_remove_everything_leaves_an_empty_index(monkeypatch):
    calls = _fake(monkeypatch)
    idx = _index(IDS)
    assert idx.remove_batch(list(reversed(IDS))) == len(IDS)
    assert calls == [("remove", list(range(len(IDS))))]
    assert idx._ids == [] and idx.entry_point is None and idx.size() == 0
    assert idx.search(np.ones(4, np.float32), 3) == []
    _consistent(idx)


def test_group_labels_are_compacted_like_the_library(monkeypatch):
    calls = _fake(monkeypatch)
    idx = _index(IDS)
    gl = idx._sync_groups(None)
    assert calls[-1] == ("set_groups", [0, 0, 1, 2, 2, 1, 2, 3], 4)
    # group "a" empties, "c" loses one row: a's number goes, the others shift down in their old order
    assert idx.remove_batch(["a_0", "a_1", "c_1"]) == 3
    assert idx._groups is gl and gl.keys == ["b", "c", "d"] and gl.index == {"b": 0, "c": 1, "d": 2}
    assert gl.labels.tolist() == [0, 1, 0, 1, 2] and gl.labels.dtype == np.int32
    n_calls = len(calls)
    idx.search_grouped_batch([np.ones(4, np.float32)], 2)           # labels still current on the device: no upload
    idx.search(np.ones(4, np.float32), 2)                           # ranks still current on the device: no upload
    assert [c[0] for c in calls[n_calls:]] == ["search_grouped", "search"]


def test_remove_group_finds_the_rows_through_the_labels(monkeypatch):
    calls = _fake(monkeypatch)
    idx = _index(IDS)
    idx._sync_groups(None)
    assert idx.remove_group("c") == 3
    assert calls[-1] == ("remove", [3, 4, 6])
    assert idx._ids == ["a_0", "a_1", "b_0", "b_1", "d_0"]
    assert idx._groups.keys == ["a", "b", "d"] and idx._groups.labels.tolist() == [0, 0, 1, 1, 2]
    _consistent(idx)
    assert idx.remove_group("c") == 0 and calls[-1][0] == "remove" and len([c for c in calls if c[0] == "remove"]) == 1
    # labels never uploaded: remove_group labels on the host only, and the next grouped search uploads them once
    calls.clear()
    idx2 = _index(IDS)
    assert idx2.remove_group("b") == 2
    assert calls == [("remove", [2, 5])]
    idx2.search_grouped(np.ones(4, np.float32), 2)
    assert calls[1] == ("set_groups", [0, 0, 1, 1, 1, 2], 3)
    # another mapping: relabelled, device labels stale (uploaded at the next grouped search with that mapping)
    fn = lambda nid: nid[0] in "ab"                                   # noqa: E731
    calls.clear()
    assert idx2.remove_group(True, group_of=fn) == 2
    assert calls == [("remove", [0, 1])] and idx2._groups.uploaded == -1
    idx2.search_grouped(np.ones(4, np.float32), 2, group_of=fn)
    assert calls[1] == ("set_groups", [0, 0, 0, 0], 1)


def test_stale_labels_are_compacted_and_uploaded_later(monkeypatch):
    calls = _fake(monkeypatch)
    idx = _index(IDS)
    idx._sync_groups(None)
    idx._ids.extend(["e_0", "a_2"])                                   # rows added since the upload: device labels stale
    idx._row_of.update({"e_0": 8, "a_2": 9})
    idx.element_count += 2
    idx.remove_batch(["d_0"])
    assert idx._groups.keys == ["a", "b", "c", "e"] and idx._groups.uploaded == -1
    idx.search_grouped(np.ones(4, np.float32), 2)
    assert calls[-2] == ("set_groups", [0, 0, 1, 2, 2, 1, 2, 3, 0], 4)


def test_identity_index_after_a_remove(monkeypatch):
    calls = _fake(monkeypatch)
    idx = _index(range(6), identity=True)
    idx.remove_batch([4, 5])                                          # only the tail: still 0..n-1
    assert idx._identity and idx._ids == [0, 1, 2, 3]
    idx.remove(1)
    assert not idx._identity and idx._ids == [0, 2, 3] and idx._tie_order == "device"
    _consistent(idx)
    idx.search(np.ones(4, np.float32), 2)                             # ids still increase with the row: no ranks needed
    assert [c[0] for c in calls] == ["remove", "remove", "search"]


def test_stale_ranks_stay_stale(monkeypatch):
    calls = _fake(monkeypatch)
    idx = _index(IDS, tie_order="stale")
    idx.remove("b_0")
    assert idx._tie_order == "stale"
    idx.search(np.ones(4, np.float32), 2)
    assert calls[1] == ("set_id_ranks", len(IDS) - 1)


def test_simple_video_index_remove_video_bookkeeping(monkeypatch):
    from video_quierer_amd.overhaul_index import SimpleVideoIndex
    calls = _fake(monkeypatch)
    svi = SimpleVideoIndex()
    names = ["v1", "v2", "v1", "v3", "v2", "v1"]
    for i, v in enumerate(names):
        svi.add_frame(np.full(4, i, np.float32), v, float(i))
    svi.video_hashes = {"v1": "h1", "v2": "h2", "v3": "h3"}
    dev = _index([-i for i in range(4)])                              # frames 0..3 pushed, 4..5 not yet
    svi._dev, svi._pushed = dev, 4
    assert svi.remove_video("v1") == 3
    assert calls == [("remove", [0, 2])]
    assert [m["video_name"] for m in svi.metadata] == ["v2", "v3", "v2"]
    assert [m["frame_id"] for m in svi.metadata] == [1, 3, 4]         # kept as stored
    assert [float(e[0]) for e in svi.embeddings] == [1.0, 3.0, 4.0]
    assert svi.video_hashes == {"v2": "h2", "v3": "h3"}
    assert svi._pushed == 2 and dev._ids == [0, -1] and dev._row_of == {0: 0, -1: 1} and dev.element_count == 2
    assert svi.remove_video("nope") == 0 and len(calls) == 1


def test_remove_video_labels_rows_added_since_the_last_grouped_search_by_their_old_positions(monkeypatch):
    """Frames pushed after the labels were last uploaded are labelled inside the removal, through ids that are still the old
    positions: the metadata must not have shrunk yet (it did once: an IndexError, or the neighbour's video name)."""
    from index_host_fakes import fake_device, fill
    from video_quierer_amd.overhaul_index import SimpleVideoIndex

    def no_moment(calls, h, q, nq, k, mode, min_gap, rows, dist):
        fill(rows, [-1] * (nq * k))

    calls = fake_device(monkeypatch, vq_index_search_distinct=no_moment)
    svi = SimpleVideoIndex()
    for i in range(6):
        svi.add_frame(np.ones(4, np.float32), "ab"[i % 2], float(i))
    assert svi.search_moments(np.ones(4, np.float32), 2) == []            # ranks, labels and positions of six rows
    svi.add_frame(np.ones(4, np.float32), "c", 0.0)
    svi.add_frame(np.ones(4, np.float32), "a", 9.0)
    svi.search(np.ones(4, np.float32), 1)                                 # pushes the two frames; their labels are not made yet
    assert svi.remove_video("b") == 3 and calls[-1] == ("remove", [1, 3, 5])
    dev = svi._dev
    assert dev._groups.keys == ["a", "c"] and dev._groups.labels.tolist() == [0, 0, 0, 1, 0]
    assert dev._positions.values.tolist() == [0, 2000, 4000, 0, 9000]
    assert dev._ids == [0, -1, -2, -3, -4] and [m["video_name"] for m in svi.metadata] == ["a", "a", "a", "c", "a"]
    _consistent(dev)
