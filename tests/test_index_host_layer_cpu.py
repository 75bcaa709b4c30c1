"""The Python layer of the index (indexes/hnsw.py, overhaul_index.py) on a recording stand-in for the library: the exact result
dicts (keys, key order, scalar types) of the families no other CPU test reaches, the three tie regimes of the plain search,
``SimpleVideoIndex`` over a five-frame index, and the table of errors and short cuts of every public search method, in the
order in which they are taken.  Written against the code as it stood before that layer was consolidated; it pins what the
consolidation may not change."""
import numpy as np
import pytest

from index_host_fakes import bare_index, fake_device, fake_lib, fill, ranked_search

F = np.float32
Q = np.ones(4, dtype=np.float32)
Q5 = np.ones(5, dtype=np.float32)                       # the wrong dimension
IDS = ["a_0", "a_1", "b_0", "c_0", "c_1", "b_1"]        # videos a, b, c -> labels 0, 1, 2


def _same(res, want):
    """Equal, with the same key order and the same scalar types."""
    assert res == want
    for r, w in zip(res, want):
        assert list(r) == list(w) and [type(v) for v in r.values()] == [type(v) for v in w.values()], (r, w)
        for v, x in zip(r.values(), w.values()):
            if isinstance(x, list):
                assert [type(e) for e in v] == [type(e) for e in x], (r, w)


# -- the plain search: three tie regimes ------------------------------------------------------------------------------------
def test_search_identity_ids_maps_rows_to_ints(monkeypatch):
    calls = fake_lib(monkeypatch, vq_index_search=ranked_search([3, 1, 4, 0, 5, 2], [.125, .25, .25, .5, .75, 1.]))
    idx = bare_index(range(6), identity=True, tie_order="device")
    res = idx.search(2 * Q, 3)
    _same(res, [{"id": 3, "distance": F(.125), "score": F(.875)}, {"id": 1, "distance": F(.25), "score": F(.75)},
                {"id": 4, "distance": F(.25), "score": F(.75)}])
    assert calls == [("search", 1, 3, 0)] and len(idx.search_times) == 1
    idx.search_mode = 2
    res = idx.search_batch([Q, Q], 9)                                # k capped at the rows; one call for the batch
    assert calls[1:] == [("search", 2, 6, 2)] and len(idx.search_times) == 3
    assert [[r["id"] for r in rr] for rr in res] == [[3, 1, 4, 0, 5, 2]] * 2
    _same(res[1][:1], [{"id": 3, "distance": F(.125), "score": F(.875)}])
    assert idx.search_times[1] == idx.search_times[2]                # the batch's time, split evenly


def test_search_device_ranks_upload_once_and_map_rows_to_names(monkeypatch):
    calls = fake_lib(monkeypatch, vq_index_search=ranked_search([2, 5, 0], [.25, .25, .5]))
    idx = bare_index(IDS)
    res = idx.search(Q, 2)
    _same(res, [{"id": "b_0", "distance": F(.25), "score": F(.75)}, {"id": "b_1", "distance": F(.25), "score": F(.75)}])
    assert calls == [("set_id_ranks", 6), ("search", 1, 2, 0)] and idx._tie_order == "device"
    res = idx.search_batch([Q], 5)                                   # fewer rows than k come back as they are
    assert calls[2:] == [("search", 1, 5, 0)] and [r["id"] for r in res[0]] == ["b_0", "b_1", "a_0"]
    assert len(idx.search_times) == 2


def test_search_ids_without_a_common_order_overfetches_and_sorts_on_the_host(monkeypatch):
    # 24 rows; the exhaustive list is row 23, then rows 22 .. 12 at one distance (a tie group that the first fetch of
    # k + 8 = 10 cuts at rank 2), then the rest: exactly one doubling, then the group is whole and is put in id order
    rows = list(range(23, -1, -1))
    dists = [.125] + [.25] * 11 + [.5] * 12
    calls = fake_lib(monkeypatch, vq_index_search=ranked_search(rows, dists))
    ids = [100 - r for r in range(24)]
    ids[23] = "s"                                                    # a str beside ints: no total order (row 23 is in no tie)
    idx = bare_index(ids)
    res = idx.search(Q, 2)
    assert calls == [("set_id_ranks", 0), ("search", 1, 10, 0), ("search", 1, 20, 0)] and idx._tie_order == "host"
    _same(res, [{"id": "s", "distance": F(.125), "score": F(.875)}, {"id": 78, "distance": F(.25), "score": F(.75)}])
    res = idx.search_batch([Q, Q], 2)                                # the ranks stay cleared; the loop runs again for the batch
    assert calls[3:] == [("search", 2, 10, 0), ("search", 2, 20, 0)]
    assert [[r["id"] for r in rr] for rr in res] == [["s", 78]] * 2
    res = idx.search(Q, 12)                                          # fetch 20 < 24 and rank 12 is not in a cut group
    assert calls[5:] == [("search", 1, 20, 0)]
    assert [r["id"] for r in res] == ["s"] + list(range(78, 89))
    res = idx.search(Q, 20)                                          # 24 rows cover min(24, 28): nothing can be cut
    assert calls[6:] == [("search", 1, 24, 0)] and len(res) == 20


# -- distinct and sequence search: the result dicts ---------------------------------------------------------------------------
def distinct_answer(rows, dists):
    def entry(calls, h, q, nq, k, mode, min_gap, out_rows, out_dist):
        calls.append(("search_distinct", nq, k, mode, min_gap))
        for j in range(nq):
            fill(out_rows, (list(rows) + [-1] * k)[:k], j * k)
            fill(out_dist, (list(dists) + [np.inf] * k)[:k], j * k)
    return entry


def sequence_answer(groups, dists, chains):
    def entry(calls, h, q, m, k, lo, hi, sel, n_sel, exclude, out_groups, out_dist, out_rows):
        calls.append(("search_sequence", m, k, lo, hi, [sel[i] for i in range(n_sel)], exclude))
        fill(out_groups, (list(groups) + [-1] * k)[:k])
        fill(out_dist, (list(dists) + [np.inf] * k)[:k])
        fill(out_rows, ([r for chain in chains for r in (chain * m)[:m]] + [-1] * (k * m))[: k * m])
    return entry


_distinct = distinct_answer([4, 2], [F(.125), F(.5)])
_sequence = sequence_answer([2, 0], [F(.25), F(.375)], [[3, 4], [0, 1]])


def test_search_distinct_result_dicts(monkeypatch):
    calls = fake_lib(monkeypatch, vq_index_search_distinct=_distinct)
    idx = bare_index(IDS)
    res = idx.search_distinct(Q, 3, 2)
    assert calls == [("set_id_ranks", 6), ("set_groups", [0, 0, 1, 2, 2, 1], 3), ("set_positions", [0, 1, 0, 0, 1, 1]),
                     ("search_distinct", 1, 3, 0, 2)]
    _same(res, [{"id": "c_1", "group": "c", "position": 1, "distance": F(.125), "score": F(.875)},
                {"id": "b_0", "group": "b", "position": 0, "distance": F(.5), "score": F(.5)}])
    res = idx.search_distinct_batch([Q, Q], 9)                       # k capped at the rows, the default gap, nothing uploaded again
    assert calls[4:] == [("search_distinct", 2, 6, 0, 1)] and res[0] == res[1] and len(res[0]) == 2
    assert idx.search_times == []                                    # only the plain search keeps times
    ident = bare_index(range(6), identity=True, tie_order="device")  # ints: each its own group, the id its position
    calls.clear()
    res = ident.search_distinct(Q, 1, 0, position_of=lambda nid: 10 * nid)
    assert calls == [("set_groups", [0, 1, 2, 3, 4, 5], 6), ("set_positions", [0, 10, 20, 30, 40, 50]), ("search_distinct", 1, 1, 0, 0)]
    _same(res, [{"id": 4, "group": 4, "position": 40, "distance": F(.125), "score": F(.875)}])


def test_search_sequence_result_dicts(monkeypatch):
    calls = fake_lib(monkeypatch, vq_index_search_sequence=_sequence)
    idx = bare_index(IDS)
    res = idx.search_sequence([Q, 3 * Q], 5, max_gap=4)
    assert calls == [("set_id_ranks", 6), ("set_groups", [0, 0, 1, 2, 2, 1], 3), ("set_positions", [0, 1, 0, 0, 1, 1]),
                     ("search_sequence", 2, 3, 1, 4, [], 1)]            # k capped at the groups; no filter: nothing excluded
    _same(res, [{"group": "c", "distance": F(.25), "score": F(.75), "chain": ["c_0", "c_1"], "positions": [0, 1]},
                {"group": "a", "distance": F(.375), "score": F(.625), "chain": ["a_0", "a_1"], "positions": [0, 1]}])
    idx.search_sequence([Q], 1, max_gap=2 ** 70, min_gap=2, within=["c", "nope", "a"])
    assert calls[4:] == [("search_sequence", 1, 1, 2, 2 ** 62, [0, 2], 0)]      # the gap clamped, the labels sorted, nothing uploaded again
    ident = bare_index(range(6), identity=True, tie_order="device")
    calls.clear()
    res = ident.search_sequence([Q, Q], 1, max_gap=3, group_of=lambda nid: nid // 2)
    assert [c[0] for c in calls] == ["set_groups", "set_positions", "search_sequence"] and calls[-1] == ("search_sequence", 2, 1, 1, 3, [], 1)
    _same(res, [{"group": 2, "distance": F(.25), "score": F(.75), "chain": [3, 4], "positions": [3, 4]}])


# -- SimpleVideoIndex over five frames ------------------------------------------------------------------------------------------
FRAMES = (("x", 0.0), ("y", 0.0), ("x", 1.5), ("z", 0.0), ("y", 2.0))


def _svi(n=5):
    from video_quierer_amd.overhaul_index import SimpleVideoIndex
    svi = SimpleVideoIndex()
    for i, (name, t) in enumerate(FRAMES[:n]):
        svi.add_frame(np.full(4, i + 1, dtype=np.float64), name, t)
    return svi


def test_simple_video_index_search_moments_storyboard(monkeypatch):
    calls = fake_device(monkeypatch, vq_index_search=ranked_search([1, 4, 0, 3, 2, 5], [.25, .25, .5, .5, .75, 1.]),
                        vq_index_search_distinct=_distinct, vq_index_search_sequence=_sequence)
    svi = _svi()
    assert svi.embeddings[0].dtype == np.float32
    res = svi.search(3 * Q, 2)                                       # equal scores: the larger frame first
    assert calls == [("add", 5, 0), ("search", 1, 5, 0)]             # pushed at the first search; k + 8 covers the index
    _same(res, [{"video_name": "y", "timestamp": 2.0, "frame_id": 4, "score": 0.75},
                {"video_name": "y", "timestamp": 0.0, "frame_id": 1, "score": 0.75}])
    assert res[0] is not svi.metadata[4] and "score" not in svi.metadata[4]
    res = svi.search_moments(Q, 2, min_gap_s=0.9995)
    assert calls[2:] == [("set_id_ranks", 5), ("set_groups", [0, 1, 0, 2, 1], 3), ("set_positions", [0, 0, 1500, 0, 2000]),
                         ("search_distinct", 1, 2, 0, 1000)]           # the gap in whole ms, rounded up
    _same(res, [{"video_name": "y", "timestamp": 2.0, "frame_id": 4, "score": 0.875},
                {"video_name": "x", "timestamp": 1.5, "frame_id": 2, "score": 0.5}])
    n = len(calls)
    svi.search_moments(Q, 9)
    assert calls[n:] == [("search_distinct", 1, 5, 0, 2000)]         # nothing uploaded again; k capped at the frames
    # an add clears the ranks (the plain search orders ties on the host) and the next moment search uploads everything again
    svi.add_frame(np.ones(4), "w", 0.5)
    n = len(calls)
    assert [r["frame_id"] for r in svi.search(Q, 3)] == [4, 1, 3]
    assert calls[n:] == [("add", 1, 0), ("set_id_ranks", 0), ("search", 1, 6, 0)]
    n = len(calls)
    svi.search_moments(Q, 2, 1.0)
    assert calls[n:] == [("set_id_ranks", 6), ("set_groups", [0, 1, 0, 2, 1, 3], 4), ("set_positions", [0, 0, 1500, 0, 2000, 500]),
                         ("search_distinct", 1, 2, 0, 1000)]
    n = len(calls)
    res = svi.search_storyboard([Q, 2 * Q], 5, max_gap_s=10.0)
    assert calls[n:] == [("search_sequence", 2, 4, 1, 10000, [], 1)]     # ranks, labels and positions are current
    _same(res, [{"video_name": "z", "score": 0.75, "timestamps": [0.0, 2.0], "frame_ids": [3, 4]},
                {"video_name": "x", "score": 0.625, "timestamps": [0.0, 0.0], "frame_ids": [0, 1]}])
    assert svi._pushed == 6 and svi._dev._ids == [0, -1, -2, -3, -4, -5] and svi._dev.element_count == 6


def test_simple_video_index_errors_and_short_cuts(monkeypatch):
    from video_quierer_amd.overhaul_index import SimpleVideoIndex
    calls = fake_device(monkeypatch, vq_index_search=ranked_search([4, 3, 2, 1, 0], [.25, .25, .5, .5, .75]),
                        vq_index_search_distinct=_distinct)
    empty = SimpleVideoIndex()
    assert empty.search(Q, 3) == [] and empty.search_moments(Q, 3) == [] and empty.search_storyboard([Q]) == []
    with pytest.raises(ValueError, match="min_gap_s"):
        empty.search_moments(Q, 3, -1.0)                             # checked before the empty-index answer
    with pytest.raises(KeyError):
        empty.similar_videos("x")
    assert calls == []
    svi = _svi()
    assert svi.search_storyboard([Q], 0) == [] and calls == []       # k <= 0: answered before anything is pushed
    assert svi.search(Q, 0) == []
    assert calls == [("add", 5, 0), ("search", 1, 5, 0)]             # ... the plain search asks the device all the same
    del calls[:]
    assert svi.search_moments(Q, 0) == []
    assert calls == [("set_id_ranks", 5)]                            # ranks first, then the k <= 0 answer: no labels, no search
    del calls[:]
    with pytest.raises(ValueError, match="dimension"):
        svi.search_moments(Q5, 3)
    assert calls == []


# -- the table: errors and short cuts of every public search method, in the order in which they are taken -------------------
def _none2(name):
    def entry(calls, h, q, nq, k, mode, *rest):
        calls.append((name, k))
        for ptr in rest[-3:] if "grouped" in name else rest[-2:]:
            fill(ptr, [-1] * (nq * k))                                # (-1 where a distance is expected: never read, no row precedes it)
    return entry


def _none_set(calls, h, q, m, k, mode, sel, n_sel, exclude, groups, dist, rows):
    calls.append(("search_set", k))
    fill(groups, [-1] * k)


def _none_sequence(calls, h, q, m, k, lo, hi, sel, n_sel, exclude, groups, dist, rows):
    calls.append(("search_sequence", k))
    fill(groups, [-1] * k)


def _read_rows(calls, h, rn, n, out):
    calls.append(("read_rows", n))
    fill(out, [0.5] * (4 * n))


QUIET = dict(vq_index_search=_none2("search"), vq_index_search_grouped=_none2("search_grouped"),
             vq_index_search_filtered=_none2("search_filtered"), vq_index_search_grouped_filtered=_none2("search_grouped_filtered"),
             vq_index_search_distinct=lambda calls, h, q, nq, k, mode, gap, rows, dist: (calls.append(("search_distinct", k)),
                                                                                          fill(rows, [-1] * (nq * k)))[0],
             vq_index_search_set=_none_set, vq_index_search_sequence=_none_sequence, vq_index_read_rows=_read_rows)
UP = ["set_id_ranks", "set_groups"]                     # what a first grouped / filtered search uploads on IDS
UPP = UP + ["set_positions"]
BOTH = dict(within=["a"], exclude=["b"])
MANY = np.ones((4097, 4), dtype=np.float32)
V = ValueError

# (case, call on (the index over IDS, an empty index), the answer or (exception, a word of its message), the library calls made)
TABLE = [
    ("search: empty index", lambda i, e: e.search(Q, 3), [], []),
    ("search: empty index before the dimension", lambda i, e: e.search(Q5, 3), [], []),
    ("search: k = 0", lambda i, e: i.search(Q, 0), [], []),
    ("search: the dimension before k <= 0", lambda i, e: i.search(Q5, 0), (V, "dimension"), []),
    ("search: wrong dimension", lambda i, e: i.search(Q5, 3), (V, "dimension"), []),
    ("search: k above the rows", lambda i, e: i.search(Q, 9), [], ["set_id_ranks", "search"]),
    ("search_batch: zero queries", lambda i, e: (i.search_batch([], 3), e.search_batch([], 3)), ([], []), []),
    ("search_batch: empty index before the dimension", lambda i, e: e.search_batch([Q5, Q5], 3), [[], []], []),
    ("search_batch: k < 0", lambda i, e: i.search_batch([Q, Q], -1), [[], []], []),
    ("search_batch: wrong dimension", lambda i, e: i.search_batch([Q5], 3), (V, "dimension"), []),

    ("search_grouped: within and exclude before the empty index", lambda i, e: e.search_grouped(Q, 3, **BOTH), (V, "exactly one"), []),
    ("search_grouped: one key instead of a list", lambda i, e: e.search_grouped(Q, 3, within="a"), (V, "iterable"), []),
    ("search_grouped: empty index before the dimension", lambda i, e: e.search_grouped(Q5, 3), [], []),
    ("search_grouped: k = 0", lambda i, e: i.search_grouped(Q, 0), [], []),
    ("search_grouped: the dimension before k <= 0", lambda i, e: i.search_grouped(Q5, 0), (V, "dimension"), []),
    ("search_grouped: wrong dimension", lambda i, e: i.search_grouped(Q5, 3), (V, "dimension"), []),
    ("search_grouped: empty within", lambda i, e: i.search_grouped(Q, 3, within=[]), [], []),
    ("search_grouped: the dimension before an empty within", lambda i, e: i.search_grouped(Q5, 3, within=[]), (V, "dimension"), []),
    ("search_grouped: unknown keys within", lambda i, e: i.search_grouped(Q, 3, within=["nope"]), [], UP),
    ("search_grouped: unknown keys excluded", lambda i, e: i.search_grouped(Q, 3, exclude=["nope"]), [], UP + ["search_grouped_filtered"]),
    ("search_grouped: no filter", lambda i, e: i.search_grouped(Q, 3), [], UP + ["search_grouped"]),
    ("search_grouped_batch: the filter before zero queries", lambda i, e: i.search_grouped_batch([], 3, **BOTH), (V, "exactly one"), []),
    ("search_grouped_batch: zero queries", lambda i, e: (i.search_grouped_batch([], 3), e.search_grouped_batch([], 3)), ([], []), []),
    ("search_grouped_batch: empty index", lambda i, e: e.search_grouped_batch([Q5, Q5], 3, within=["a"]), [[], []], []),

    ("search_filtered: neither within nor exclude, before the empty index", lambda i, e: e.search_filtered(Q, 3), (V, "exactly one"), []),
    ("search_filtered: within and exclude", lambda i, e: i.search_filtered(Q, 3, **BOTH), (V, "exactly one"), []),
    ("search_filtered: empty index before the dimension", lambda i, e: e.search_filtered(Q5, 3, within=["a"]), [], []),
    ("search_filtered: k = 0", lambda i, e: i.search_filtered(Q, 0, within=["a"]), [], []),
    ("search_filtered: the dimension before k <= 0", lambda i, e: i.search_filtered(Q5, 0, within=["a"]), (V, "dimension"), []),
    ("search_filtered: empty within", lambda i, e: i.search_filtered(Q, 3, within=[]), [], []),
    ("search_filtered: the dimension before an empty within", lambda i, e: i.search_filtered(Q5, 3, within=[]), (V, "dimension"), []),
    ("search_filtered: unknown keys within", lambda i, e: i.search_filtered(Q, 3, within=["nope"]), [], UP),
    ("search_filtered: unknown keys excluded", lambda i, e: i.search_filtered(Q, 3, exclude=["nope"]), [], UP + ["search_filtered"]),
    ("search_filtered_batch: the filter before zero queries", lambda i, e: i.search_filtered_batch([], 3), (V, "exactly one"), []),
    ("search_filtered_batch: zero queries", lambda i, e: i.search_filtered_batch([], 3, within=["a"]), [], []),
    ("search_filtered_batch: empty index", lambda i, e: e.search_filtered_batch([Q, Q], 3, exclude=["a"]), [[], []], []),

    ("search_distinct: a negative gap before the empty index", lambda i, e: e.search_distinct(Q, 3, -1), (V, "min_gap"), []),
    ("search_distinct: empty index before the dimension", lambda i, e: e.search_distinct(Q5, 3), [], []),
    ("search_distinct: a negative gap before the dimension", lambda i, e: i.search_distinct(Q5, 3, -1), (V, "min_gap"), []),
    ("search_distinct: k = 0", lambda i, e: i.search_distinct(Q, 0), [], []),
    ("search_distinct: the dimension before k <= 0", lambda i, e: i.search_distinct(Q5, 0), (V, "dimension"), []),
    ("search_distinct: wrong dimension", lambda i, e: i.search_distinct(Q5, 3), (V, "dimension"), []),
    ("search_distinct: every row", lambda i, e: i.search_distinct(Q, 9), [], UPP + ["search_distinct"]),
    ("search_distinct: an id without a frame number, after ranks and labels",
     lambda i, e: (i._ids.append("d"), i.search_distinct(Q, 3)), (V, "frame_of"), UP),
    ("search_distinct_batch: a negative gap before zero queries", lambda i, e: i.search_distinct_batch([], 3, -2), (V, "min_gap"), []),
    ("search_distinct_batch: zero queries", lambda i, e: (i.search_distinct_batch([], 3), e.search_distinct_batch([], 3)), ([], []), []),
    ("search_distinct_batch: empty index", lambda i, e: e.search_distinct_batch([Q5, Q5], 3), [[], []], []),

    ("search_set: the filter before zero frames", lambda i, e: i.search_set([], 3, **BOTH), (V, "exactly one"), []),
    ("search_set: zero frames before the empty index", lambda i, e: e.search_set([], 3), (V, "at least one"), []),
    ("search_set: empty index before the frame limit", lambda i, e: e.search_set(MANY, 3), [], []),
    ("search_set: k = 0 before the frame limit and the dimension", lambda i, e: (i.search_set(MANY, 0), i.search_set([Q5], 0)), ([], []), []),
    ("search_set: the frame limit before the dimension", lambda i, e: i.search_set(np.ones((4097, 5), np.float32), 3), (V, "4096"), []),
    ("search_set: wrong dimension", lambda i, e: i.search_set([Q5], 3), (V, "dimension"), []),
    ("search_set: empty within", lambda i, e: i.search_set([Q], 3, within=[]), [], []),
    ("search_set: the dimension before an empty within", lambda i, e: i.search_set([Q5], 3, within=[]), (V, "dimension"), []),
    ("search_set: unknown keys within", lambda i, e: i.search_set([Q], 3, within=["nope"]), [], UP),
    ("search_set: no filter", lambda i, e: i.search_set([Q, Q], 3), [], UP + ["search_set"]),

    ("similar_groups: empty index", lambda i, e: e.similar_groups("a"), (KeyError, "a"), []),
    ("similar_groups: one key instead of a list, before the group", lambda i, e: i.similar_groups("nope", within="a"), (V, "iterable"), []),
    ("similar_groups: the group before k <= 0", lambda i, e: i.similar_groups("nope", 0), (KeyError, "nope"), []),
    ("similar_groups: k = 0", lambda i, e: i.similar_groups("a", 0), [], []),
    ("similar_groups: within holds the group alone", lambda i, e: i.similar_groups("a", 3, within=["a"]), [], []),
    ("similar_groups: the rows are read before anything is uploaded", lambda i, e: i.similar_groups("a", 3), [], ["read_rows"] + UP + ["search_set"]),

    ("search_sequence: the filter before zero steps", lambda i, e: e.search_sequence([], 3, max_gap=0, **BOTH), (V, "exactly one"), []),
    ("search_sequence: zero steps before the gaps", lambda i, e: e.search_sequence([], 3, max_gap=0), (V, "at least one"), []),
    ("search_sequence: too many steps before the gaps", lambda i, e: e.search_sequence([Q] * 65, 3, max_gap=0), (V, "at most 64"), []),
    ("search_sequence: the gaps before the empty index", lambda i, e: e.search_sequence([Q], 3, max_gap=2, min_gap=3), (V, "gaps"), []),
    ("search_sequence: empty index before the dimension", lambda i, e: e.search_sequence([Q5], 3, max_gap=2), [], []),
    ("search_sequence: k = 0 before the dimension", lambda i, e: i.search_sequence([Q5], 0, max_gap=2), [], []),
    ("search_sequence: wrong dimension", lambda i, e: i.search_sequence([Q5], 3, max_gap=2), (V, "dimension"), []),
    ("search_sequence: empty within", lambda i, e: i.search_sequence([Q], 3, max_gap=2, within=[]), [], []),
    ("search_sequence: the dimension before an empty within", lambda i, e: i.search_sequence([Q5], 3, max_gap=2, within=[]), (V, "dimension"), []),
    ("search_sequence: unknown keys within, after the positions", lambda i, e: i.search_sequence([Q], 3, max_gap=2, within=["nope"]), [], UPP),
    ("search_sequence: no filter", lambda i, e: i.search_sequence([Q, Q], 3, max_gap=2), [], UPP + ["search_sequence"]),
]


@pytest.mark.parametrize("case, call, answer, library_calls", TABLE, ids=[row[0] for row in TABLE])
def test_errors_and_short_cuts_in_order(monkeypatch, case, call, answer, library_calls):
    calls = fake_lib(monkeypatch, **QUIET)
    idx, empty = bare_index(IDS), bare_index([])
    if isinstance(answer, tuple) and isinstance(answer[0], type):
        with pytest.raises(answer[0], match=answer[1]):
            call(idx, empty)
    else:
        assert call(idx, empty) == answer
    assert [c[0] for c in calls] == library_calls
    assert idx.search_times == [] or case.startswith("search:") or case.startswith("search_batch:")
