"""Host side of zero-shot labelling without a device: the exported symbols, the plan (chunking kept within its scratch bounds,
the path at the mode-0 edges, the exported error bound), the argument checks that come before the device is touched, the numpy
restatement of the definition (tests/label_ref.py) on hand-made cases, and the Python layer over a recording library."""
import math
from ctypes import POINTER, byref, c_float, c_int, c_int32, c_int64

import numpy as np
import pytest

import label_ref
from index_host_fakes import bare_index, fake_device, fake_lib, fill

MIB = 1 << 20


def _plan(n, dim, P, mode, largest_group=0, groups=False):
    from video_quierer_amd import _lib
    fp16, chunk, chunks, tiles, ranges, split, piece = c_int(), c_int(), c_int(), c_int(), c_int(), c_int(), c_int()
    exact_bytes, row_tiles, part_bytes, eps, pieces = c_int64(), c_int64(), c_int64(), c_float(), c_int64()
    _lib.check(_lib.load().vq_debug_label_plan(n, dim, P, mode, largest_group, byref(fp16), byref(chunk), byref(chunks), byref(exact_bytes),
                                               byref(tiles), byref(ranges), byref(row_tiles), byref(part_bytes), byref(eps), byref(split),
                                               byref(piece), byref(pieces)))
    if groups:
        return dict(split=split.value, piece=piece.value, pieces=pieces.value)
    return dict(fp16=fp16.value, chunk=chunk.value, chunks=chunks.value, exact_bytes=exact_bytes.value, tiles=tiles.value,
                ranges=ranges.value, row_tiles=row_tiles.value, part_bytes=part_bytes.value, eps=eps.value)


def plan_restated(n, dim, P, mode):
    """The chunking rules of csrc/knn_label.h plan_label, near-unit rows."""
    ok = dim in (256, 512, 768)
    ld = -(-n // 64) * 64
    chunk = max(1, min(P, (128 * MIB) // ld))
    if chunk >= 32:
        chunk = chunk // 32 * 32
    tiles = -(-P // 256)
    ranges = -(-tiles // 8)
    row_tiles = -(-n // 256)
    return dict(fp16=int((mode == 2 and ok) or (mode == 0 and ok and n >= 16384 and n * P >= 2 ** 22)), chunk=chunk, chunks=-(-P // chunk), exact_bytes=chunk * ld * 4,
                tiles=tiles, ranges=ranges, row_tiles=row_tiles, part_bytes=ranges * 5 * row_tiles * 256 * 4)


def test_new_symbols_are_exported():
    from video_quierer_amd import _lib
    lib = _lib.load()
    for name in ("vq_index_label_rows", "vq_index_label_rows_device", "vq_debug_label_plan"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    import video_quierer_amd
    video_quierer_amd.install_dropin()
    from indexes.hnsw import HNSWIndex
    from video_quierer_amd.overhaul_index import SimpleVideoIndex
    assert callable(HNSWIndex.label_rows) and callable(HNSWIndex.label_groups) and callable(SimpleVideoIndex.tag_videos)


def test_plan_matches_the_restated_chunking_and_stays_within_its_scratch():
    for n in (1, 63, 64, 65, 300, 16383, 16384, 16389, 1_000_000, 40_000_000, 2 ** 31 - 1):
        for dim in (64, 512, 768):
            for P in (1, 31, 32, 33, 255, 256, 257, 600, 2048, 2049, 4096):
                for mode in (0, 1) + ((2,) if dim != 64 else ()):
                    got = _plan(n, dim, P, mode)
                    eps = got.pop("eps")
                    assert got == plan_restated(n, dim, P, mode), (n, dim, P, mode)
                    assert got["chunk"] * got["chunks"] >= P > got["chunk"] * (got["chunks"] - 1)
                    assert got["exact_bytes"] <= 512 * MIB or got["chunk"] == 1
                    assert got["tiles"] * 256 >= P > (got["tiles"] - 1) * 256 and got["ranges"] in (1, 2)
                    assert got["part_bytes"] <= 40 * (n + 255)          # 20 B per row and range, never a [P][n] table
                    assert (eps == 0.0) == (dim == 64)


def test_plan_path_at_the_mode0_edges():
    assert _plan(16383, 512, 4096, 0)["fp16"] == 0 and _plan(16384, 512, 256, 0)["fp16"] == 1      # 16,384 rows and n x P >= 2^22
    assert _plan(16384, 512, 255, 0)["fp16"] == 0 and _plan(65536, 768, 63, 0)["fp16"] == 0 and _plan(65536, 768, 64, 0)["fp16"] == 1
    assert _plan(10 ** 6, 512, 4, 0)["fp16"] == 0 and _plan(10 ** 6, 512, 5, 0)["fp16"] == 1
    assert _plan(16384, 64, 100, 0)["fp16"] == 0 and _plan(10 ** 6, 1024, 100, 0)["fp16"] == 0     # no fp16 path at these dims
    assert _plan(1, 768, 1, 2)["fp16"] == 1 and _plan(10 ** 6, 768, 4096, 1)["fp16"] == 0
    for bad in ((0, 512, 5, 0), (2 ** 31, 512, 5, 0), (10, 0, 5, 0), (10, 514, 5, 0), (10, 512, 0, 0), (10, 512, 4097, 0), (10, 512, 5, 3),
                (10, 64, 5, 2), (10, 1024, 5, 2)):
        with pytest.raises(ValueError):
            _plan(*bad)


def test_plan_splits_groups_above_4096_rows_into_pieces():
    for largest, pieces in ((0, 0), (1, 0), (4096, 0), (4097, 2), (5000, 2), (8192, 2), (8193, 3), (20_000, 5), (1_000_000, 245)):
        assert _plan(1_000_000, 512, 24, 0, largest, groups=True) == dict(split=4096, piece=4096, pieces=pieces), largest
    assert 4096 * 4 <= 64 << 10                               # a piece's histogram (P <= 4,096 counters) fits the static LDS limit
    with pytest.raises(ValueError):
        _plan(100, 512, 24, 0, 101)                           # a group longer than the index


def test_plan_exports_the_bound_of_the_proof():
    """eps = scan_eps_unit(dim) x 1.0001^2 + 2^-20: the scan's bound for norms up to 1.0001 plus half the proof's slack."""
    for dim in (256, 512, 768):
        unit = (2.0 / 2048 + 1.0 / 4194304 + dim / 8388608.0 + 1.0 / 65536 + 2.0 * math.sqrt(dim) / 33554432.0) * 1.02
        assert _plan(4096, dim, 257, 2)["eps"] == pytest.approx(unit * 1.0001 ** 2 + 2.0 ** -20, rel=1e-5)
    assert 1.0e-3 < _plan(4096, 512, 600, 2)["eps"] < _plan(4096, 768, 600, 2)["eps"] < 1.5e-3


def test_c_abi_refuses_bad_arguments_before_the_device():
    from video_quierer_amd import _lib
    lib = _lib.load()
    p = np.zeros((4, 8), np.float32)
    out = np.full(64, -7, np.int32)
    pp, op = p.ctypes.data_as(POINTER(c_float)), out.ctypes.data_as(POINTER(c_int32))
    for P, m, md, groups in ((0, 3, 1.0, False), (4097, 3, 1.0, False), (-1, 3, 1.0, False), (4, 0, 1.0, True), (4, 17, 1.0, True),
                             (4, 3, math.nan, False)):
        g = (op, op, op, op) if groups else (None, None, None, None)
        assert lib.vq_index_label_rows(None, pp, P, 1, c_float(md), op, None, m, *g) == -1, (P, m, md)
        assert "vq_index_label_rows" in lib.vq_last_error().decode()
        assert lib.vq_index_label_rows_device(None, pp, P, 1, c_float(md), None, None, m, *g) == -1
    assert (out == -7).all()


# ---- the restatement on hand-made cases ----
def test_row_labels_by_hand():
    D = np.array([[0.5, 0.2, 0.9, 0.30],
                  [0.1, 0.2, 0.9, 0.25],
                  [0.1, 0.7, 0.8, 0.25]], dtype=np.float32)           # [P = 3][n = 4]
    L, best = label_ref.row_labels(D)
    assert L.tolist() == [1, 0, 2, 1] and L.dtype == np.int32        # equal distances: the smaller prompt index
    assert best.tolist() == [np.float32(0.1), np.float32(0.2), np.float32(0.8), np.float32(0.25)] and best.dtype == np.float32
    L, b2 = label_ref.row_labels(D, np.float32(0.25))                 # inclusive on the labelled side
    assert L.tolist() == [1, 0, -1, 1] and b2.tobytes() == best.tobytes()
    L, _ = label_ref.row_labels(D, np.nextafter(np.float32(0.25), np.float32(0), dtype=np.float32))
    assert L.tolist() == [1, 0, -1, -1]


def test_group_tags_by_hand():
    #          row: 0    1    2    3    4    5    6
    L = np.array([2,   0,   2,   0,  -1,   1,   1])
    best = np.array([.3, .1, .3, .4, .9, .2, .2], dtype=np.float32)
    groups = [0, 0, 0, 0, 0, 1, 1]
    tie = [6, 5, 4, 3, 2, 1, 0]                                       # the id order reverses the rows
    tags, votes, show, unl = label_ref.group_tags(L, best, groups, tie, 2, 3)
    assert tags.tolist() == [[0, 2, -1], [1, -1, -1]]                 # two votes each in group 0: the smaller label first
    assert votes.tolist() == [[2, 2, 0], [2, 0, 0]]
    assert show.tolist() == [[1, 2, -1], [6, -1, -1]]                 # label 2: rows 0 and 2 tie at 0.3 -> the smaller tie (row 2)
    assert unl.tolist() == [1, 0]
    tags, votes, show, _ = label_ref.group_tags(L, best, groups, tie, 2, 1)
    assert tags.tolist() == [[0], [1]] and votes.tolist() == [[2], [2]] and show.tolist() == [[1], [6]]
    _, _, _, unl = label_ref.group_tags(np.full(7, -1), best, groups, tie, 2, 2)
    assert unl.tolist() == [5, 2]


# ---- the Python layer over a recording library ----
IDS = ["a_0", "a_10", "a_2", "b_0", "b_1", "c_0"]                      # string ids: the tie order is uploaded first


def label_entry(labels, dists, tags=None):
    """vq_index_label_rows answering with the given rows' labels / distances and per-group (label, votes, show row) lists."""
    def entry(calls, h, prompts, P, mode, max_dist, row_label, row_dist, m, g_tags, g_votes, g_show, g_unl):
        dim = 4
        calls.append(("label", [[prompts[j * dim + i] for i in range(dim)] for j in range(P)], mode, max_dist, m, g_tags is not None))
        fill(row_label, labels)
        fill(row_dist, dists)
        if g_tags is not None:
            for g, found in enumerate(tags):
                ans = (found + [(-1, 0, -1)] * m)[:m]
                fill(g_tags, [a[0] for a in ans], g * m)
                fill(g_votes, [a[1] for a in ans], g * m)
                fill(g_show, [a[2] for a in ans], g * m)
                g_unl[g] = 0
    return entry


def test_label_rows_normalises_and_returns_row_order(monkeypatch):
    calls = fake_lib(monkeypatch, vq_index_label_rows=label_entry([1, 0, 1, -1, 0, 1], [.1, .2, .3, .9, .5, .6]))
    idx = bare_index(IDS)
    lab, dist = idx.label_rows([np.array([3.0, 0, 0, 4.0]), np.array([0, 2.0, 0, 0])], max_distance=0.75, mode=1)
    assert [c[0] for c in calls] == ["label"]                          # row labels need neither the tie order nor the group labels
    assert calls[0] == ("label", [[np.float32(0.6), 0.0, 0.0, np.float32(0.8)], [0.0, 1.0, 0.0, 0.0]], 1, 0.75, 0, False)
    assert lab.tolist() == [1, 0, 1, -1, 0, 1] and lab.dtype == np.int32 and dist.dtype == np.float32
    assert dist.tolist() == [np.float32(x) for x in (.1, .2, .3, .9, .5, .6)]
    idx.label_rows([np.array([0, 1.0, 0, 0])])
    assert calls[-1][2:] == (0, math.inf, 0, False)                   # mode 0, no threshold
    with pytest.raises(ValueError):
        idx.label_rows([])
    with pytest.raises(ValueError):
        idx.label_rows([np.ones(4)] * 4097)
    with pytest.raises(ValueError):
        idx.label_rows([np.ones(5)])                                  # the dimension
    with pytest.raises(ValueError):
        idx.label_rows([np.ones(4)], max_distance=math.nan)


def test_label_groups_shapes_share_and_show(monkeypatch):
    tags = [[(1, 2, 2), (0, 1, 1)], [(0, 2, 4)], [(1, 1, 5)]]
    calls = fake_lib(monkeypatch, vq_index_label_rows=label_entry([1, 0, 1, 0, 0, 1], [.1, .2, .3, .4, .5, .6], tags))
    idx = bare_index(IDS)
    idx.search_mode = 2
    res = idx.label_groups([np.array([1.0, 0, 0, 0]), np.array([0, 1.0, 0, 0])], top=2)
    assert [c[0] for c in calls] == ["set_id_ranks", "set_groups", "label"]          # _prepare's order
    assert calls[-1][2:] == (2, math.inf, 2, True)                    # the index's search mode
    assert res == {"a": [{"label": 1, "votes": 2, "share": 2 / 3, "id": "a_2", "distance": np.float32(.3)},
                         {"label": 0, "votes": 1, "share": 1 / 3, "id": "a_10", "distance": np.float32(.2)}],
                   "b": [{"label": 0, "votes": 2, "share": 1.0, "id": "b_1", "distance": np.float32(.5)}],
                   "c": [{"label": 1, "votes": 1, "share": 1.0, "id": "c_0", "distance": np.float32(.6)}]}
    calls = fake_lib(monkeypatch, vq_index_label_rows=label_entry([0] * 6, [.1] * 6, [[(0, 6, 0)]]))
    res = idx.label_groups([np.array([1.0, 0, 0, 0])], top=40, group_of=lambda nid: "all")      # at most 16 tags; another grouping
    assert calls[-1][4] == 16 and calls[-2] == ("set_groups", [0] * 6, 1) and list(res) == ["all"]
    with pytest.raises(ValueError):
        idx.label_groups([np.ones(4)], top=0)


def test_empty_index_and_stale_labels(monkeypatch):
    calls = fake_lib(monkeypatch)
    idx = bare_index([])
    lab, dist = idx.label_rows([np.ones(4)])
    assert len(lab) == 0 and lab.dtype == np.int32 and len(dist) == 0 and idx.label_groups([np.ones(4)]) == {} and calls == []
    # rows added since the last call: the labels are mapped and uploaded again before the C call
    idx = bare_index(IDS[:5])
    calls = fake_lib(monkeypatch, vq_index_label_rows=label_entry([0] * 5, [.1] * 5, [[(0, 3, 0)], [(0, 2, 3)]]))
    assert list(idx.label_groups([np.ones(4)], top=1)) == ["a", "b"] and ("set_groups", [0, 0, 0, 1, 1], 2) in calls
    idx._ids.append("c_0"); idx._row_of["c_0"] = 5; idx.element_count = 6; idx._tie_order = "stale"
    calls = fake_lib(monkeypatch, vq_index_label_rows=label_entry([0] * 6, [.1] * 6, [[(0, 3, 0)], [(0, 2, 3)], [(0, 1, 5)]]))
    res = idx.label_groups([np.ones(4)], top=1)
    assert ("set_groups", [0, 0, 0, 1, 1, 2], 3) in calls and list(res) == ["a", "b", "c"]
    assert res["c"] == [{"label": 0, "votes": 1, "share": 1.0, "id": "c_0", "distance": np.float32(.1)}]
    # a group key the caller's mapping no longer produces holds no rows: it simply does not appear
    assert "zzz" not in res


def test_tag_videos_names_tags_and_reads_the_metadata(monkeypatch):
    from video_quierer_amd.overhaul_index import SimpleVideoIndex
    tags = [[(1, 2, 1), (0, 1, 0)], [(0, 1, 3)]]
    calls = fake_device(monkeypatch, vq_index_label_rows=label_entry([0, 1, 1, 0], [.5, .25, .3, .75], tags))
    sv = SimpleVideoIndex()
    assert sv.tag_videos([np.ones(4)]) == {}
    for i, (name, ts) in enumerate((("x", 0.0), ("x", 1.5), ("x", 3.0), ("y", 0.0))):
        sv.add_frame(np.eye(4, dtype=np.float32)[i], name, ts)
    res = sv.tag_videos([np.array([2.0, 0, 0, 0]), np.array([0, 0, 3.0, 0])], tags=["cat", "dog"], top=2)
    label = [c for c in calls if c[0] == "label"][-1]
    assert label[1] == [[1.0, 0.0, 0.0, 0.0], [0.0, 0.0, 1.0, 0.0]] and label[4:] == (2, True)
    assert res == {"x": [{"tag": "dog", "frames": 2, "share": 2 / 3, "timestamp": 1.5, "frame_id": 1, "score": 0.75},
                         {"tag": "cat", "frames": 1, "share": 1 / 3, "timestamp": 0.0, "frame_id": 0, "score": 0.5}],
                   "y": [{"tag": "cat", "frames": 1, "share": 1.0, "timestamp": 0.0, "frame_id": 3, "score": 0.25}]}
    assert [t["tag"] for t in sv.tag_videos([np.ones(4), np.ones(4)], top=1)["x"]] == [1]      # default names: the indices
    with pytest.raises(ValueError):
        sv.tag_videos([])
    with pytest.raises(ValueError):
        sv.tag_videos([np.ones(4)], tags=["a", "b"])
