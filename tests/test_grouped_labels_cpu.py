"""Host-side bookkeeping of the grouped search (hnsw.py _sync_groups) without a device: which labels reach
vq_index_set_groups, and when."""
import numpy as np

from index_host_fakes import bare_index as _index, fake_lib


def _fake(monkeypatch):
    return fake_lib(monkeypatch, vq_index_set_groups=lambda calls, h, ptr, n, n_groups: calls.append(([ptr[i] for i in range(n)], n_groups)))


def test_default_group_is_the_callers_video_id():
    from video_quierer_amd.indexes.hnsw import video_of
    assert video_of("video0_10") == "video0"
    assert video_of("my_clip_2024_7") == "my_clip_2024"          # video ids may contain "_": split at the LAST one
    assert video_of("nounderscore") == "nounderscore"
    assert video_of(17) == 17 and video_of((1, 2)) == (1, 2)      # non-string ids are their own group


def test_labels_are_dense_incremental_and_uploaded_once_per_add(monkeypatch):
    calls = _fake(monkeypatch)
    idx = _index(["b_0", "b_1", "a_0", "b_2"])
    gl = idx._sync_groups(None)
    assert calls == [([0, 0, 1, 0], 2)] and gl.keys == ["b", "a"]
    idx._sync_groups(None)                                        # nothing new: no upload
    assert len(calls) == 1
    idx._ids.extend(["c_0", "a_1"])                               # add_batch appends to the same list
    gl2 = idx._sync_groups(None)
    assert gl2 is gl and calls[-1] == ([0, 0, 1, 0, 2, 1], 3)
    meta = {nid: {"video_id": "V" + nid[0]} for nid in idx._ids}
    fn = lambda nid: meta[nid]["video_id"]                        # noqa: E731
    gl3 = idx._sync_groups(fn)                                    # another mapping: everything relabelled
    assert gl3 is not gl and gl3.keys == ["Vb", "Va", "Vc"] and calls[-1] == ([0, 0, 1, 0, 2, 1], 3)
    idx._sync_groups(fn)
    assert len(calls) == 3
    idx._ids = ["x_0", "y_0"]                                     # load() replaces the id list: relabel
    meta.update({"x_0": {"video_id": "X"}, "y_0": {"video_id": "Y"}})     # same mapping
    idx._sync_groups(fn)
    assert calls[-1] == ([0, 1], 2)
    labels = np.asarray(calls[-1][0])
    assert labels.min() == 0 and set(labels) == set(range(calls[-1][1]))
