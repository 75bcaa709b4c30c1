"""Host side of library neighbours without a device: the exported symbols, the plan (vq_debug_neighbors_plan: chunks at the key
budget and the distance budget, ragged m, the re-score kind, the refusals), the numpy restatement of the definition
(tests/neighbors_ref.py) against a brute-force double loop, the main GPU fixture's preconditions, and the Python layer over a
recording library."""
from ctypes import byref, c_float, c_int, c_int64

import numpy as np
import pytest

import neighbors_ref as ref
from index_host_fakes import bare_index, fake_device, fake_lib, fill, tie_ranks
from oracle import knn_oracle

MIB = 1 << 20


def _plan(n, dim, m, k, exclude=1, mode=2):
    from video_quierer_amd import _lib
    fp16, kind, eps = c_int(), c_int(), c_float()
    chunk, chunks, key_bytes = c_int64(), c_int64(), c_int64()
    _lib.check(_lib.load().vq_debug_neighbors_plan(n, dim, m, k, exclude, mode, byref(fp16), byref(chunk), byref(chunks), byref(key_bytes),
                                                   byref(kind), byref(eps)))
    return dict(fp16=fp16.value, chunk=chunk.value, chunks=chunks.value, key_bytes=key_bytes.value, kind=kind.value, eps=eps.value)


def test_new_symbols_are_exported():
    from video_quierer_amd import _lib
    lib = _lib.load()
    for name in ("vq_index_neighbors", "vq_index_neighbors_device", "vq_debug_neighbors_plan"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    from video_quierer_amd.indexes.hnsw import HNSWIndex
    from video_quierer_amd.overhaul_index import SimpleVideoIndex
    assert callable(HNSWIndex.neighbors) and callable(HNSWIndex.neighbors_of)
    assert callable(SimpleVideoIndex.related_videos) and callable(SimpleVideoIndex.duplicate_frames)


def test_plan_chunks_at_the_key_budget():
    """Tile path: whole 256-row tiles, streams x chunk <= 2^27 key pairs (1 GiB), exactly plan_scan's q_chunk."""
    p = _plan(1 << 20, 512, 1 << 20, 10)
    assert p["fp16"] == 1 and p["chunk"] == 16384 and p["chunks"] == 64 and p["key_bytes"] == 1024 * MIB
    p = _plan(1_000_000, 512, 1_000_000, 10)             # 489 ranges -> 7,824 streams: 2^27 / 7,824 = 17,154 -> 67 tiles
    assert p["chunk"] == 17152 and p["chunks"] == 59 and p["key_bytes"] == 7824 * 17152 * 8 <= 1024 * MIB
    p = _plan(40_000_000, 256, 40_000_000, 10)           # the budget holds less than two tiles: one tile per chunk
    assert p["chunk"] == 256 and p["chunks"] == 156250
    for n, m in ((2341, 2341), (2341, 300), (2341, 1), (100_000, 257), (100_000, 256)):
        p = _plan(n, 256, m, 10)
        assert p["chunk"] == -(-m // 256) * 256 and p["chunks"] == 1, (n, m)       # ragged m: rounded up to whole tiles, one chunk
        assert p["key_bytes"] == -(-n // 2048) * 16 * p["chunk"] * 8


def test_plan_exact_path_chunks_within_the_distance_budget():
    p = _plan(2341, 256, 2341, 10, mode=1)
    assert p["fp16"] == 0 and p["chunk"] == 2560 and p["chunks"] == 1 and p["key_bytes"] == 0
    p = _plan(100_000, 320, 100_000, 1024, mode=1)       # ld = 100,032: 134,217,728 / 100,032 = 1,341 -> 5 tiles
    assert p["chunk"] == 1280 and p["chunks"] == 79 and p["chunk"] * 100_032 * 4 <= 512 * MIB
    p = _plan(1_000_000, 512, 1_000_000, 10, mode=1)     # fewer than 256 rows of distances fit: one tile all the same
    assert p["chunk"] == 256 and p["chunks"] == 3907


def test_plan_rescore_kind_and_error_bound():
    assert [_plan(5000, 512, 5000, k)["kind"] for k in (1, 20, 21, 64, 65, 100)] == [0, 0, 1, 1, 2, 2]
    for dim in (256, 512, 768):
        e = 2.0 / 2048 + 1.0 / 4194304 + dim / 8388608.0 + 1.0 / 65536 + 2.0 * np.sqrt(dim) / 33554432.0
        assert _plan(5000, dim, 5000, 10)["eps"] == pytest.approx(e * 1.02 * 1.0001 ** 2, rel=1e-5)
    assert _plan(5000, 320, 5000, 10, mode=1)["eps"] == 0.0


def test_plan_paths_and_refusals():
    assert _plan(16384, 512, 64, 10, mode=0)["fp16"] == 1              # mode 0: 16,384 stored rows and 64 asked rows
    assert _plan(16383, 512, 16383, 10, mode=0)["fp16"] == 0 and _plan(16384, 512, 63, 10, mode=0)["fp16"] == 0
    assert _plan(100_000, 512, 100_000, 101, mode=0)["fp16"] == 0        # k beyond the re-score kernels: the exact path
    assert _plan(100_000, 320, 100_000, 10, mode=0)["fp16"] == 0
    assert _plan(1, 768, 1, 1, mode=2)["fp16"] == 1 and _plan(1, 768, 1, 1, exclude=0, mode=2)["fp16"] == 1
    for bad in (dict(n=5000, dim=320, m=10, k=10, mode=2),               # mode 2 needs dim 256, 512 or 768
                dict(n=5000, dim=512, m=10, k=101, mode=2), dict(n=5000, dim=512, m=10, k=0, mode=1),
                dict(n=5000, dim=512, m=10, k=1025, mode=1), dict(n=0, dim=512, m=10, k=5), dict(n=5000, dim=512, m=0, k=5),
                dict(n=5000, dim=512, m=10, k=5, exclude=2), dict(n=5000, dim=512, m=10, k=5, mode=3), dict(n=5000, dim=510, m=10, k=5, mode=1)):
        with pytest.raises(ValueError):
            _plan(**bad)


def test_chunk_override_is_read_per_call_and_rounded_up(monkeypatch):
    monkeypatch.setenv("VQ_AMD_NEIGHBORS_CHUNK", "300")
    assert _plan(2341, 256, 2341, 10)["chunk"] == 512 and _plan(2341, 256, 2341, 10)["chunks"] == 5
    monkeypatch.setenv("VQ_AMD_NEIGHBORS_CHUNK", "256")
    assert _plan(2341, 256, 2341, 10, mode=1)["chunk"] == 256 and _plan(2341, 256, 2341, 10)["chunks"] == 10
    monkeypatch.delenv("VQ_AMD_NEIGHBORS_CHUNK")
    assert _plan(2341, 256, 2341, 10)["chunk"] == 2560


# ---- the reference ----
def _small(seed=5, n=60, dim=16):
    rng = np.random.default_rng(seed)
    v = rng.standard_normal((n, dim)).astype(np.float32)
    v[7] = v[3]; v[40] = v[3]; v[41] = v[3]; v[22] = v[21]          # noqa: E702  bit-equal rows: ties
    groups = np.array([0] * 1 + [1] * 20 + [2, 3] * 12 + [4] * 15)
    ids = [f"video{g}_{i}" for i, g in enumerate(groups)]
    return knn_oracle.normalize_rows(v), groups, ids


def test_reference_equals_the_brute_force_double_loop():
    stored, groups, ids = _small()
    rank = tie_ranks(ids)
    assert not np.array_equal(rank, np.arange(60))                       # "video1_10" before "video1_2"
    rows = list(range(60))
    for g in (None, groups):
        for tie in (None, rank):
            for k in (1, 5, 45, 70):
                got = ref.neighbors(stored, k, groups=g, tie=tie)
                want = ref.brute_force(stored, k, rows, groups=g, tie=tie)
                assert np.array_equal(got[0], want[0]) and np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32)), (g is None, k)
    picked = [59, 3, 3, 0, 21]
    got = ref.neighbors(stored, 4, rows=picked, groups=groups, tie=rank)
    want = ref.brute_force(stored, 4, picked, groups=groups, tie=rank)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert np.array_equal(got[0][1], got[0][2])                           # a repeated row gets its line twice


def test_reference_ties_and_padding():
    stored, groups, ids = _small()
    rank = tie_ranks(ids)
    i0, d0 = ref.neighbors(stored, 3, rows=[3], groups=None)              # its three bit-equal copies, by row number
    assert i0[0].tolist() == [7, 40, 41] and len(set(d0[0].tolist())) == 1
    ir, _ = ref.neighbors(stored, 3, rows=[3], groups=None, tie=rank)
    assert ir[0].tolist() == sorted([7, 40, 41], key=lambda r: ids[r])
    i1, _ = ref.neighbors(stored, 3, rows=[3], groups=groups)             # row 7 is of row 3's own group
    assert 7 not in i1[0].tolist() and i1[0][0] in (40, 41)
    one = np.zeros(60, dtype=np.int64)
    i2, d2 = ref.neighbors(stored, 4, groups=one)                         # one group only: nothing is eligible
    assert np.all(i2 == -1) and np.all(np.isinf(d2))
    i3, d3 = ref.neighbors(stored, 70, groups=None)                       # 59 eligible rows, 11 empty slots
    assert np.all(i3[:, :59] >= 0) and np.all(i3[:, 59:] == -1) and np.all(np.isinf(d3[:, 59:])) and np.all(np.isfinite(d3[:, :59]))
    assert all(r not in i3[r].tolist() for r in range(60))
    single = stored[:1]
    i4, d4 = ref.neighbors(single, 2, groups=None)
    assert i4.tolist() == [[-1, -1]] and np.all(np.isinf(d4))


def test_main_fixture_layout_and_preconditions():
    """The layout tests/test_neighbors.py relies on, and how many rows the tile path can NOT prove on this fixture by the scores
    alone (the stats condition there — at most half of the rows outside the cluster redone — must be within reach)."""
    v, g, ids, plants = ref.main_fixture()
    n = ref.MAIN_N
    assert v.shape == (n, ref.MAIN_DIM) and n == 2048 + 293 and n == 9 * 256 + 37
    counts = np.bincount(g)
    assert counts[0] == 1 and counts[1] == 300 and np.all(g[256:512] == 1) and g[2047] == g[2048] and g[n - 1] == g[2304] == 63
    assert np.all(g[1:250:2] == 3) and np.all(g[2:250:2] == 2)
    assert all(g[a] != g[b] for a, b in plants["cross"]) and all(g[a] == g[b] for a, b in plants["within"])
    assert len({g[r] for r in plants["triple"]}) == 3 and len({g[r] for r in plants["cluster"]}) == ref.CLUSTER
    assert all(np.array_equal(v[a], v[b]) for a, b in plants["cross"] + plants["within"])
    assert ids[260] == "video1_10" and ids[252] == "video1_2" and ids[260] < ids[252]
    stored = knn_oracle.normalize_rows(v)
    table = ref.distance_table(stored)
    cl = plants["cluster"]
    s = 1.0 - table[np.ix_(cl, cl)].astype(np.float64)
    assert s.max() - s.min() < 1e-5                                       # pairwise within 1e-5 in score
    eps = _plan(n, ref.MAIN_DIM, n, 10)["eps"]
    assert s.max() - s.min() < eps
    outside = np.setdiff1d(np.arange(n), cl)
    for groups in (g, None):
        ok = ref.eligible(n, np.arange(n), groups)
        # rank 10 against rank 11: unit Gaussian rows in 256 dimensions leave this gap under 4 eps for most rows whatever the seed ...
        assert ref.close_gap_rows(table[outside], ok[outside], 10, 4 * eps) > n // 2
        # ... but the proof compares rank 10 with the best key outside the 32 candidates: that gap is wide for every row
        assert ref.close_gap_rows(table[outside], ok[outside], 10, 4 * eps, below=33) < n // 4


# ---- the Python layer ----
def _neighbors_entry(table_rows, table_dist):
    """vq_index_neighbors over a canned table [n][>= k]: line r of the answer is the table's first k of asked row r."""
    def entry(calls, h, rows, m, k, exclude, mode, ids, dist):
        asked = None if not rows else [rows[i] for i in range(m)]
        calls.append(("neighbors", asked, m, k, exclude, mode))
        for i in range(m):
            r = i if asked is None else asked[i]
            fill(ids, (list(table_rows[r]) + [-1] * k)[:k], i * k)
            fill(dist, (list(table_dist[r]) + [np.inf] * k)[:k], i * k)
    return entry


def test_neighbors_maps_ids_to_rows_and_returns_row_numbers(monkeypatch):
    ids = ["a_0", "a_1", "b_0", "b_1"]
    rows = [[2, 3], [3, 2], [0, 1], [1, 0]]
    dist = [[0.1, 0.2], [0.3, 0.4], [0.1, 0.5], [0.6, 0.7]]
    calls = fake_lib(monkeypatch, vq_index_neighbors=_neighbors_entry(rows, dist))
    idx = bare_index(ids)
    r, d = idx.neighbors(2, other_groups=True, mode=1)
    assert r.dtype == np.int32 and d.dtype == np.float32 and r.tolist() == rows and np.allclose(d, dist)
    assert ("neighbors", None, 4, 2, 1, 1) in calls
    assert any(c[0] == "set_groups" and c[1] == [0, 0, 1, 1] for c in calls)         # labels under video_of, uploaded first
    calls.clear()
    r, d = idx.neighbors(1, ids=["b_1", "a_0", "b_1"])
    assert calls[-1] == ("neighbors", [3, 0, 3], 3, 1, 0, 0) and r.tolist() == [[1], [2], [1]]
    assert not any(c[0] == "set_groups" for c in calls)                               # exclude = 0 reads no labels
    hits = idx.neighbors_of("a_1", 2, other_groups=True)
    assert [h["id"] for h in hits] == ["b_1", "b_0"] and hits[0]["distance"] == np.float32(0.3)
    assert hits[0]["score"] == np.float32(1.0) - np.float32(0.3) and calls[-1][1] == [1]
    r, d = idx.neighbors(3, ids=[])
    assert r.shape == (0, 3) and d.shape == (0, 3)


def test_neighbors_argument_errors_and_empty_index(monkeypatch):
    calls = fake_lib(monkeypatch, vq_index_neighbors=_neighbors_entry([[1], [0]], [[0.5], [0.5]]))
    idx = bare_index(["a_0", "b_0"])
    for bad in (0, -1, 1025):
        with pytest.raises(ValueError):
            idx.neighbors(bad)
    with pytest.raises(ValueError):
        idx.neighbors(1, mode=3)
    with pytest.raises(KeyError):
        idx.neighbors(1, ids=["a_0", "nope"])
    with pytest.raises(KeyError):
        idx.neighbors_of("nope")
    assert idx.neighbors_of("a_0", 0) == [] and not calls
    empty = bare_index([])
    r, d = empty.neighbors(4, other_groups=True)
    assert r.shape == (0, 4) and d.shape == (0, 4) and not calls
    hits = idx.neighbors_of("b_0", 3)                                     # fewer rows than k: the empty slots are dropped
    assert [h["id"] for h in hits] == ["a_0"]


def _library(monkeypatch, table_rows, table_dist, frames):
    from video_quierer_amd.overhaul_index import SimpleVideoIndex
    calls = fake_device(monkeypatch, vq_index_neighbors=_neighbors_entry(table_rows, table_dist))
    lib = SimpleVideoIndex()
    for name, ts in frames:
        lib.add_frame(np.ones(4, dtype=np.float32), name, ts)
    return lib, calls


FRAMES = [("a", 0.0), ("a", 1.0), ("a", 2.0), ("b", 0.0), ("b", 1.0), ("c", 0.0)]
#          row 0       row 1       row 2       row 3       row 4       row 5
TABLE_ROWS = [[3, 5], [3, 4], [5, 4], [0, 1], [1, 5], [2, 0]]
TABLE_DIST = [[0.01, 0.30], [0.02, 0.10], [0.20, 0.40], [0.01, 0.02], [0.10, 0.50], [0.20, 0.30]]


def test_related_videos_from_a_hand_written_table(monkeypatch):
    lib, calls = _library(monkeypatch, TABLE_ROWS, TABLE_DIST, FRAMES)
    rel = lib.related_videos(k=5, per_frame=2)
    assert [c for c in calls if c[0] == "neighbors"] == [("neighbors", None, 6, 2, 1, 0)]     # one call over the whole library
    a = rel["a"]                                          # a's six slots: four land in b (rows 3, 3, 4, 4), two in c
    assert [x["video_name"] for x in a] == ["b", "c"]
    assert a[0]["votes"] == 4 and a[1]["votes"] == 2 and a[0]["share"] == pytest.approx(4 / 6) and a[1]["share"] == pytest.approx(2 / 6)
    assert a[0]["score"] == pytest.approx(1 - (0.01 + 0.02 + 0.10 + 0.40) / 4) and a[1]["score"] == pytest.approx(1 - (0.30 + 0.20) / 2)
    b = rel["b"]                                          # a: rows 0, 1, 1 -> 3 votes; c: row 5 -> 1 vote
    assert [(x["video_name"], x["votes"]) for x in b] == [("a", 3), ("c", 1)] and b[0]["share"] == pytest.approx(0.75)
    assert [(x["video_name"], x["votes"]) for x in rel["c"]] == [("a", 2)] and rel["c"][0]["score"] == pytest.approx(0.75)
    assert [x["video_name"] for x in lib.related_videos(k=1, per_frame=2)["a"]] == ["b"]
    with pytest.raises(ValueError):
        lib.related_videos(k=0)
    with pytest.raises(ValueError):
        lib.related_videos(per_frame=0)


def test_related_videos_orders_equal_votes_by_mean_distance_then_name(monkeypatch):
    frames = [("q", 0.0), ("q", 1.0), ("z", 0.0), ("y", 0.0), ("x", 0.0)]
    rows = [[2, 3], [4, -1], [0, 1], [0, 1], [0, 1]]      # q: z 1 vote at 0.3, y 1 vote at 0.2, x 1 vote at 0.2; one empty slot
    dist = [[0.3, 0.2], [0.2, np.inf], [0.1, 0.1], [0.1, 0.1], [0.1, 0.1]]
    lib, _ = _library(monkeypatch, rows, dist, frames)
    q = lib.related_videos(k=3, per_frame=2)["q"]
    assert [x["video_name"] for x in q] == ["x", "y", "z"] and all(x["share"] == pytest.approx(1 / 3) for x in q)


def test_duplicate_frames_from_a_hand_written_table(monkeypatch):
    lib, calls = _library(monkeypatch, TABLE_ROWS, TABLE_DIST, FRAMES)
    dup = lib.duplicate_frames(min_similarity=0.98)
    assert [c for c in calls if c[0] == "neighbors"] == [("neighbors", None, 6, 1, 1, 0)]
    assert [(d["video_name"], d["timestamp"], d["other_video"], d["other_timestamp"]) for d in dup] == \
        [("a", 0.0, "b", 0.0), ("a", 1.0, "b", 0.0), ("b", 0.0, "a", 0.0)]
    assert dup[0]["score"] == pytest.approx(0.99) and dup[1]["score"] == pytest.approx(0.98)     # a frame exactly at the bound is kept
    assert lib.duplicate_frames(min_similarity=1.0) == []
    with pytest.raises(ValueError):
        lib.duplicate_frames(min_similarity=1.5)
    from video_quierer_amd.overhaul_index import SimpleVideoIndex
    assert SimpleVideoIndex().duplicate_frames() == [] and SimpleVideoIndex().related_videos() == {}
