"""Shared-footage search without a device: the numpy restatement (tests/match_ref.py) on layouts whose runs are known by
construction, plan_match's arithmetic through vq_debug_match_plan (the 512 MiB refusal included), the argument refusals that are
judged before the device is asked for, and the Python layer over a recording library."""
import ctypes
from ctypes import POINTER, byref, c_float, c_int, c_int32, c_int64

import numpy as np
import pytest

import match_ref
from index_host_fakes import bare_index, fake_device, fake_lib, fill

CAP_ENV = "VQ_AMD_MATCH_FILED_CAP"


def one_hot_table(clip, videos):
    """Distances of one-hot frames: clip[i] and every video frame name a symbol; d = 0 where they agree, 1 elsewhere (-1 in a video
    matches nothing).  -> (dist [m][n], labels, pos, tie): rows stored video after video, position = frame, tie = row."""
    flat = np.concatenate([np.asarray(v) for v in videos])
    labels = np.concatenate([np.full(len(v), g) for g, v in enumerate(videos)])
    pos = np.concatenate([np.arange(len(v)) for v in videos])
    dist = np.where((np.asarray(clip)[:, None] == flat[None, :]) & (flat[None, :] >= 0), 0.0, 1.0).astype(np.float32)
    return dist, labels, pos, np.arange(len(flat))


def runs_of(slots):
    return [(s["group"], s["hits"], s["span"], s["q_first"], s["row_first"], s["row_last"]) for s in slots if s["group"] >= 0]


# ---- the restatement ----
def test_diagonal_runs_cut_trim_and_count():
    c = np.array([0, 1, 1, 0, 1, 0, 0, 1, 1, 1, 0], dtype=bool)
    assert match_ref.diagonal_runs(c, 0) == [(1, 2, 2), (4, 4, 1), (7, 9, 3)]
    assert match_ref.diagonal_runs(c, 1) == [(1, 4, 3), (7, 9, 3)]             # one miss is bridged, two are a cut
    assert match_ref.diagonal_runs(c, 2) == [(1, 9, 6)]                        # trimmed to the first and last hit
    assert match_ref.diagonal_runs(np.zeros(5, dtype=bool), 3) == []


def test_planted_copies_are_told_apart():
    clip = list(range(100, 120))                                               # 20 distinct frames
    videos = [
        [-1, -1, -1] + clip[4:14] + [-1, -1],          # 0: an exact partial copy at an offset: delta 3 - 4 = -1
        clip[4:14][::-1],                              # 1: the same copy reversed: no run of 2
        clip[0:20:2],                                  # 2: every second frame: the diagonal breaks at once
        clip[2:7] + [-1] + clip[8:14],                 # 3: one replaced frame
        clip[2:7] + [-1, -1] + clip[9:14],             # 4: two replaced frames
        clip[5:9],                                     # 5, 6: two identical copies: the label decides
        clip[5:9],
    ]
    dist, labels, pos, tie = one_hot_table(clip, videos)
    base = np.cumsum([0] + [len(v) for v in videos])
    strict, n = match_ref.answer(dist, labels, pos, tie, 0.5, 2, 0, 10)
    assert n == 5 and runs_of(strict) == [
        (0, 10, 10, 4, base[0] + 3, base[0] + 12),
        (3, 6, 6, 8, base[3] + 6, base[3] + 11),       # max_miss 0: the longer piece behind the replaced frame
        (4, 5, 5, 2, base[4] + 0, base[4] + 4),        # two pieces of 5: the smaller delta is the same, the earlier start wins
        (5, 4, 4, 5, base[5], base[5] + 3),
        (6, 4, 4, 5, base[6], base[6] + 3)]
    assert all(s["mean_dist"] == 0 for s in strict[:5]) and strict[5] == match_ref.EMPTY
    one, _ = match_ref.answer(dist, labels, pos, tie, 0.5, 2, 1, 10)
    assert runs_of(one)[:3] == [(3, 11, 12, 2, base[3], base[3] + 11), (0, 10, 10, 4, base[0] + 3, base[0] + 12),
                                (4, 5, 5, 2, base[4], base[4] + 4)]            # one miss bridged; two in a row still cut
    two, _ = match_ref.answer(dist, labels, pos, tie, 0.5, 2, 2, 10)
    assert runs_of(two)[0] == (3, 11, 12, 2, base[3], base[3] + 11) and runs_of(two)[2] == (4, 10, 12, 2, base[4], base[4] + 11)
    # min_len 1: the reversed and the strided copy appear, with single hits
    loose, n = match_ref.answer(dist, labels, pos, tie, 0.5, 1, 0, 10)
    assert n == 7 and {(g, h) for g, h, *_ in runs_of(loose)} >= {(1, 1), (2, 1)}
    # the filter
    only, n = match_ref.answer(dist, labels, pos, tie, 0.5, 2, 0, 3, allowed={4, 6})
    assert n == 2 and [s["group"] for s in only] == [4, 6, -1]


def test_the_tie_orders_rows_at_one_position():
    clip = [7, 8, 9]
    dist = np.where(np.array(clip)[:, None] == np.array([8, 7, 9])[None, :], 0.0, 1.0).astype(np.float32)
    labels, pos = np.zeros(3, dtype=int), np.array([0, 0, 1])                  # rows 0 and 1 share a position
    by_row, _ = match_ref.answer(dist, labels, pos, np.array([0, 1, 2]), 0.5, 1, 0, 1)
    by_rank, _ = match_ref.answer(dist, labels, pos, np.array([1, 0, 2]), 0.5, 1, 0, 1)
    assert runs_of(by_row) == [(0, 1, 1, 1, 0, 0)]                              # order 8 7 9: single hits only; delta -1 (clip frame 1 on row 0) is the smallest
    assert runs_of(by_rank) == [(0, 3, 3, 0, 1, 2)]                             # order 7 8 9: the whole clip


def test_infinite_thresholds_and_the_inclusive_edge():
    rng = np.random.default_rng(3)
    lengths = [1, 2, 5, 9]
    labels = np.concatenate([np.full(L, g) for g, L in enumerate(lengths)])
    pos = np.concatenate([np.arange(L) for L in lengths])
    tie = np.arange(len(labels))
    base = np.cumsum([0] + lengths)
    for m in (1, 4, 5, 12):
        dist = rng.uniform(0.1, 1.9, (m, len(labels))).astype(np.float32)
        every, n = match_ref.answer(dist, labels, pos, tie, np.inf, 1, 0, 8)
        assert n == 4
        for s in every[:4]:
            L = lengths[s["group"]]
            delta = min(0, L - m)                      # the smallest diagonal of full length
            assert (s["hits"], s["span"], s["q_first"], s["row_first"]) == (min(m, L), min(m, L), -delta, base[s["group"]])
        assert [s["group"] for s in every[:4]] == sorted(range(4), key=lambda g: (-min(m, lengths[g]), g))
        assert match_ref.answer(dist, labels, pos, tie, -np.inf, 1, 0, 8) == ([match_ref.EMPTY] * 8, 0)
        d0 = dist[0, 3]
        at = match_ref.hit_table(dist, d0)
        below = match_ref.hit_table(dist, np.nextafter(d0, np.float32(-np.inf), dtype=np.float32))
        assert at[0, 3] and not below[0, 3]                                     # inclusive
    nan = np.full((2, len(labels)), np.nan, dtype=np.float32)
    assert match_ref.answer(nan, labels, pos, tie, np.inf, 1, 0, 2)[1] == 0     # a NaN distance never hits
    # mean_dist: the fp64 chain over the hit cells, divided once, rounded once
    dist = np.array([[0.1, 9], [9, 0.2], [9, 9]], dtype=np.float32)[:, [0, 1]]
    s = match_ref.answer(np.array([[0.1, 9.0], [9.0, 0.7]], dtype=np.float32), np.zeros(2, int), np.arange(2), np.arange(2), 1.0, 1, 0, 1)[0][0]
    assert s["mean_dist"] == np.float32((float(np.float32(0.1)) + float(np.float32(0.7))) / 2.0) and s["hits"] == 2


# ---- plan_match through vq_debug_match_plan ----
def plan(n, G, dim, m, mode):
    from video_quierer_amd import _lib
    lib = _lib.load()
    i = [c_int() for _ in range(8)]
    l = [c_int64() for _ in range(4)]
    rc = lib.vq_debug_match_plan(n, G, dim, m, mode, byref(i[0]), byref(l[0]), byref(i[1]), byref(i[2]), byref(i[3]), byref(i[4]), byref(l[1]),
                                 byref(l[2]), byref(i[5]), byref(l[3]), byref(i[6]))
    return rc, dict(fp16=i[0].value, bits_bytes=l[0].value, exact_chunk=i[1].value, exact_chunks=i[2].value, q_tiles=i[3].value,
                    ranges=i[4].value, tile_grid=l[1].value, filed_cap=l[2].value, key_bits=i[5].value, run_blocks=l[3].value,
                    launches=i[6].value)


def test_match_plan_arithmetic(monkeypatch):
    from video_quierer_amd import _lib
    monkeypatch.delenv(CAP_ENV, raising=False)
    rc, p = plan(1_000_000, 2000, 512, 4096, 2)
    assert rc == 0
    assert p["fp16"] == 1 and p["bits_bytes"] == 4096 * 31250 * 4 == 512_000_000 and p["q_tiles"] == 16 and p["ranges"] == 489
    assert p["tile_grid"] == 123 * 2 * 32                   # 4 ranges x 8 query tiles per block of 32 workgroups
    assert p["filed_cap"] == 16 << 20 and p["launches"] == 11
    assert p["key_bits"] == 3 * 12 + 20 and p["run_blocks"] == -(-(1_000_000 + 2000 * 4095) // 256)
    assert p["exact_chunk"] == 128 and p["exact_chunks"] == 32          # 512 MiB of distances: 134 rows' worth -> whole 32-query tiles
    rc, p = plan(1_000_000, 2000, 512, 4096, 1)
    assert rc == 0 and p["fp16"] == 0 and p["launches"] == 2 * 32 + 6
    # mode 0: the tile path from 16,384 rows and 32 frames, where it exists
    assert [plan(n, 10, dim, m, 0)[1]["fp16"] for n, dim, m in ((16384, 512, 32), (16383, 512, 32), (16384, 512, 31), (16384, 96, 32),
                                                                 (16384, 768, 4096), (16384, 256, 300))] == [1, 0, 0, 0, 1, 1]
    # the bit table's bound: m x ceil(n / 32) x 4 B <= 512 MiB
    assert plan(1_048_576, 1, 512, 4096, 1)[0] == 0 and plan(1_048_576, 1, 512, 4096, 1)[1]["bits_bytes"] == 512 << 20
    rc, _ = plan(1_048_577, 1, 512, 4096, 1)
    assert rc == -1 and b"bit table" in _lib.load().vq_last_error()
    assert plan(2 ** 31 - 1, 1, 512, 1, 1)[0] == 0 and plan(2 ** 31 - 1, 1, 512, 2, 1)[0] == 0 and plan(2 ** 31 - 1, 1, 512, 3, 1)[0] == -1
    # the run key fits 63 bits wherever the table is allowed
    for n, m in ((2 ** 31 - 1, 1), (2 ** 31 - 1, 2), (2 ** 30, 4), (2 ** 20, 4096), (2 ** 24, 256), (1, 4096), (1, 1)):
        rc, p = plan(n, 1, 512, m, 1)
        assert rc == 0 and 1 <= p["key_bits"] <= 63, (n, m, p)
    # refusals of the plan's own arguments; mode 2 where the tile path does not exist
    assert plan(100, 10, 96, 8, 2)[0] == -1 and plan(100, 10, 96, 8, 0) == plan(100, 10, 96, 8, 1)
    for bad in ((0, 1, 512, 1, 1), (10, 11, 512, 1, 1), (10, 1, 512, 0, 1), (10, 1, 512, 4097, 1), (10, 1, 512, 1, 3), (10, 1, 510, 1, 1)):
        assert plan(*bad)[0] == -1, bad
    # the filed list's capacity: lowered by the environment, never raised
    monkeypatch.setenv(CAP_ENV, "5")
    assert plan(100_000, 10, 512, 64, 2)[1]["filed_cap"] == 5
    monkeypatch.setenv(CAP_ENV, str(1 << 40))
    assert plan(100_000, 10, 512, 64, 2)[1]["filed_cap"] == 16 << 20


def test_arguments_are_judged_before_the_device(monkeypatch):
    """Every refusal below happens before the library is asked for its device: this runs on a box without one, with a null handle."""
    from video_quierer_amd import _lib
    lib = _lib.load()
    q = np.zeros((2, 8), dtype=np.float32)
    out = [np.empty(4, np.int32) for _ in range(6)] + [np.empty(4, np.float32)]
    sel = np.zeros(1, dtype=np.int32)

    def call(m=2, k=4, max_dist=0.1, min_len=1, max_miss=0, mode=1, n_sel=0, exclude=1, device=False):
        fn = lib.vq_index_match_runs_device if device else lib.vq_index_match_runs
        first = None if device else q.ctypes.data_as(POINTER(c_float))
        outs = [None] * 7 if device else [a.ctypes.data_as(POINTER(c_int32)) for a in out[:6]] + [out[6].ctypes.data_as(POINTER(c_float))]
        rc = fn(None, first, m, k, c_float(max_dist), min_len, max_miss, mode, sel.ctypes.data_as(POINTER(c_int32)) if n_sel else None, n_sel,
                exclude, *outs)
        return rc, lib.vq_last_error().decode()

    for device in (False, True):
        for bad, word in ((dict(m=0), "m 0"), (dict(m=4097), "m 4097"), (dict(k=0), "k 0"), (dict(k=1025), "k 1025"),
                          (dict(max_dist=float("nan")), "max_dist"), (dict(min_len=0), "min_len"), (dict(max_miss=-1), "max_miss"),
                          (dict(mode=3), "mode 3"), (dict(n_sel=-1), "filter"), (dict(exclude=2), "filter")):
            rc, msg = call(device=device, **bad)
            assert rc == -1 and word in msg, (bad, rc, msg)


# ---- the Python layer over a recording library ----
IDS = ["a_0", "a_1", "a_2", "b_0", "b_2", "b_1", "c_0"]


def match_entry(answer):
    """vq_index_match_runs answering with answer = [(group, hits, span, q_first, row_first, row_last, mean)]; recorded."""
    def entry(calls, h, q, m, k, max_dist, min_len, max_miss, mode, groups, n_sel, exclude, g, hits, span, qf, rf, rl, mean):
        calls.append(("match", m, k, float(np.float32(max_dist)), min_len, max_miss, [groups[i] for i in range(n_sel)], exclude))
        ans = (answer + [(-1, 0, 0, -1, -1, -1, np.inf)] * k)[:k]
        for j, ptr in enumerate((g, hits, span, qf, rf, rl, mean)):
            fill(ptr, [a[j] for a in ans])
    return entry


def test_shared_runs_prepares_in_order_and_shapes_the_result(monkeypatch):
    calls = fake_lib(monkeypatch, vq_index_match_runs=match_entry([(1, 3, 3, 0, 3, 4, 0.25), (0, 2, 3, 1, 0, 2, 0.5)]))
    idx = bare_index(IDS)
    frames = [np.array([1, 0, 0, 0], np.float32)] * 3
    res = idx.shared_runs(frames, k=5, max_distance=0.125, min_len=2, max_miss=1)
    assert [c[0] for c in calls] == ["set_id_ranks", "set_groups", "set_positions", "match"]
    assert calls[2] == ("set_positions", [0, 1, 2, 0, 2, 1, 0])
    assert calls[3] == ("match", 3, 3, 0.125, 2, 1, [], 1)                       # k capped at the number of groups
    assert res == [{"group": "b", "hits": 3, "span": 3, "query_first": 0, "first": "b_0", "last": "b_2", "positions": (0, 2),
                    "distance": np.float32(0.25), "score": np.float32(0.75)},
                   {"group": "a", "hits": 2, "span": 3, "query_first": 1, "first": "a_0", "last": "a_2", "positions": (0, 2),
                    "distance": np.float32(0.5), "score": np.float32(0.5)}]
    assert type(res[0]["distance"]) is np.float32
    del calls[:]
    idx.shared_runs(frames, k=1, max_distance=0.5, within=["c", "a", "zzz"])
    assert calls == [("match", 3, 1, 0.5, 3, 0, [0, 2], 0)]                       # nothing is uploaded twice; the defaults; unknown keys hold no rows
    del calls[:]
    assert idx.shared_runs(frames, k=2, max_distance=0.5, within=["zzz"]) == [] and idx.shared_runs(frames, k=0, max_distance=0.5) == []
    assert calls == []
    for bad in (dict(max_distance=float("nan")), dict(max_distance=0.1, min_len=0), dict(max_distance=0.1, max_miss=-1),
                dict(max_distance=0.1, within=["a"], exclude=["b"])):
        with pytest.raises(ValueError):
            idx.shared_runs(frames, **bad)
    with pytest.raises(ValueError):
        idx.shared_runs([], max_distance=0.1)
    with pytest.raises(ValueError):
        idx.shared_runs(frames * 1366, max_distance=0.1)                          # 4,098 frames
    assert bare_index([]).shared_runs(frames, max_distance=0.1) == []


def test_shared_runs_of_reads_the_group_in_position_order(monkeypatch):
    read = []

    def read_rows(calls, h, rows, n, out):
        read.append([rows[i] for i in range(n)])
        fill(out, [0.5] * (n * 4))

    calls = fake_lib(monkeypatch, vq_index_match_runs=match_entry([(0, 3, 3, 0, 0, 2, 0.0)]), vq_index_read_rows=read_rows)
    idx = bare_index(IDS)
    res = idx.shared_runs_of("b", k=4, max_distance=0.25)
    assert read == [[3, 5, 4]]                                                   # b_0, b_1, b_2: by position, not by row
    assert calls[-1] == ("match", 3, 3, 0.25, 3, 0, [1], 1)                       # the group itself excluded
    assert [r["group"] for r in res] == ["a"]
    del calls[:]
    idx.shared_runs_of("b", k=4, max_distance=0.25, within=["a", "b"])
    assert calls == [("match", 3, 3, 0.25, 3, 0, [0], 0)]
    assert idx.shared_runs_of("b", max_distance=0.25, within=["b"]) == [] and idx.shared_runs_of("b", k=0, max_distance=0.25) == []
    with pytest.raises(KeyError):
        idx.shared_runs_of("nope", max_distance=0.25)
    big = bare_index([f"v_{i}" for i in range(4097)])
    with pytest.raises(ValueError):
        big.shared_runs_of("v", max_distance=0.25)


def test_find_reuse_shapes_its_result(monkeypatch):
    from video_quierer_amd.overhaul_index import SimpleVideoIndex

    def read_rows(calls, h, rows, n, out):
        calls.append(("read", [rows[i] for i in range(n)]))
        fill(out, [0.5] * (n * 4))

    calls = fake_device(monkeypatch, vq_index_match_runs=match_entry([(1, 2, 2, 1, 3, 5, 0.125)]), vq_index_read_rows=read_rows)
    sv = SimpleVideoIndex()
    for i, (name, ts) in enumerate([("x.mp4", 0.0), ("x.mp4", 1.0), ("x.mp4", 0.5), ("y.mp4", 0.0), ("y.mp4", 0.75), ("y.mp4", 1.5)]):
        sv.add_frame(np.full(4, i + 1.0, np.float32), name, ts)
    got = sv.find_reuse("x.mp4", k=3, min_similarity=0.75, min_seconds=1.0, max_miss=2)
    assert ("read", [0, 2, 1]) in calls                                          # x.mp4 in timestamp order
    assert calls[-1] == ("match", 3, 2, 0.25, 2, 2, [0], 1)                       # 1.0 s over a 0.5 s frame interval: two frames
    assert got == [{"video_name": "y.mp4", "frames": 2, "score": 0.875, "start": 0.0, "end": 1.5, "query_start": 0.5, "query_end": 1.0}]
    with pytest.raises(KeyError):
        sv.find_reuse("z.mp4")
    for bad in (dict(min_similarity=1.5), dict(min_similarity=float("nan")), dict(min_seconds=-1.0), dict(max_miss=-1)):
        with pytest.raises(ValueError):
            sv.find_reuse("x.mp4", **bad)
