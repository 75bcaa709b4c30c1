"""Filtered exact top-k (vq_index_search_filtered / vq_index_search_grouped_filtered, HNSWIndex.search_filtered and
search_grouped(within=, exclude=)): the plain or grouped search restricted to the rows of some groups (videos).  The expected
answer is the C oracle's exact distances walked in (distance, id) order with every row outside the filter dropped; ids, groups,
distances and order must match bit for bit in every mode that exists."""
import zlib
from ctypes import POINTER, byref, c_int32, c_int64, c_void_p

import numpy as np
import pytest

from conftest import knn_big_ids, knn_big_inputs
from oracle import knn_oracle
from index_host_fakes import tie_ranks as _tie_ranks, unit as _unit

pytestmark = pytest.mark.gpu


def _mk(vecs, ids):
    from video_quierer_amd.indexes.hnsw import OptimizedHNSWIndex
    idx = OptimizedHNSWIndex(dimension=vecs.shape[1])
    idx.add_batch(vecs, ids)
    return idx


class _Truth:
    """The oracle's distances of one index and query batch, and the (distance, tie) order of every query's rows."""

    def __init__(self, stored, uq, ids, keys):
        self.d = [knn_oracle.distances(stored, q) for q in uq]
        tie = _tie_ranks(ids)
        self.order = [np.lexsort((tie, d)) for d in self.d]
        dense = {}
        self.labels = np.array([dense.setdefault(g, len(dense)) for g in keys], dtype=np.int64)
        self.dense = dense

    def allowed(self, within, exclude):
        sel = np.zeros(len(self.dense), dtype=bool)
        for key in (within if within is not None else exclude):
            if key in self.dense:
                sel[self.dense[key]] = True
        return sel[self.labels] if within is not None else ~sel[self.labels]

    def plain(self, ok, k):
        return [[(int(r), d[r]) for r in o[ok[o]][:k]] for d, o in zip(self.d, self.order)]

    def grouped(self, ok, k):
        out = []
        for d, o in zip(self.d, self.order):
            o = o[ok[o]]
            _, first = np.unique(self.labels[o], return_index=True)
            out.append([(int(r), d[r]) for r in o[np.sort(first)[:k]]])
        return out


def _check(idx, ids, qs, truth, k, mode, within=None, exclude=None, group_of=None, grouped=False):
    from video_quierer_amd.indexes.hnsw import video_of
    fn = video_of if group_of is None else group_of
    idx.search_mode = mode
    if grouped:
        res = (idx.search_grouped_batch(list(qs), k, group_of, within=within, exclude=exclude) if len(qs) != 1
               else [idx.search_grouped(qs[0], k, group_of, within=within, exclude=exclude)])
    else:
        res = (idx.search_filtered_batch(list(qs), k, within=within, exclude=exclude, group_of=group_of) if len(qs) != 1
               else [idx.search_filtered(qs[0], k, within=within, exclude=exclude, group_of=group_of)])
    ok = truth.allowed(within, exclude)
    want = truth.grouped(ok, k) if grouped else truth.plain(ok, k)
    what = f"mode {mode}, k {k}, within {within is not None}, grouped {grouped}"
    for j, (rr, ww) in enumerate(zip(res, want)):
        assert [r["id"] for r in rr] == [ids[r] for r, _ in ww], f"query {j}: ids differ ({what})"
        assert [r["distance"] for r in rr] == [d for _, d in ww], f"query {j}: distances differ ({what})"
        assert all(type(r["distance"]) is np.float32 and r["score"] == np.float32(1.0) - r["distance"] for r in rr)
        if grouped:
            assert [r["group"] for r in rr] == [fn(ids[r]) for r, _ in ww], f"query {j}: groups differ ({what})"
    return res


def _contiguous(n, lengths):
    out, i = [], 0
    while sum(out) < n:
        out.append(min(lengths[i % len(lengths)], n - sum(out)))
        i += 1
    return out


def _filters(videos, rng):
    """(within, exclude) pairs: one video, 10 % and 60 % of the videos, excluding one and all but one, unknown and duplicate
    keys."""
    v = list(videos)
    pick = lambda frac: [v[i] for i in rng.choice(len(v), max(1, int(len(v) * frac)), replace=False)]   # noqa: E731
    one = v[len(v) // 2]
    return [([one], None), (pick(0.1), None), (pick(0.6), None), (None, [one]), (None, v[1:]),
            ([one, "no_such_video", one], None), (None, [v[0], v[0], "no_such_video"])]


MODES = (0, 1, 2)


def _has_fp16(dim, nq, k):
    """The masked fp16 path exists (mode 2 is refused elsewhere): dim 256 / 512 / 768, nq <= SCAN3_MAX_Q, k <= 100."""
    return dim in (256, 512, 768) and nq <= 96 and k <= 100


def _modes(dim, nq, k):
    return [m for m in MODES if m != 2 or _has_fp16(dim, nq, k)]


def _check_stats(idx, mode, nq):
    st = idx.last_search_stats()
    if mode == 1:
        assert st["exact_fallback"] == nq and st["verified"] == 0, st
    else:
        assert st["verified"] + st["exact_fallback"] == nq, st
    return st

# (name, rows, dim, nq, ks)
LAYOUTS = [
    ("contiguous", 20_000, 512, 4, (1, 10, 100)),
    ("contiguous_one_query", 20_000, 512, 1, (20, 40)),
    ("shuffled", 12_000, 256, 33, (10,)),
    ("contiguous_768", 8_000, 768, 97, (20,)),
    ("contiguous_batch", 20_000, 256, 300, (10,)),
]


@pytest.mark.timeout(900)
@pytest.mark.parametrize("name,n,dim,nq,ks", LAYOUTS, ids=[x[0] for x in LAYOUTS])
def test_filtered_matches_oracle(gpu_lib, name, n, dim, nq, ks):
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    vecs = rng.standard_normal((n, dim)).astype(np.float32)
    qs = rng.standard_normal((nq, dim)).astype(np.float32)
    qs[: (nq + 1) // 2] = vecs[rng.integers(0, n, (nq + 1) // 2)] + np.float32(0.3) * rng.standard_normal(((nq + 1) // 2, dim)).astype(np.float32)
    if name == "shuffled":                         # every stream mixed: labels drawn per row
        lab = rng.integers(0, 300, n)
        ids = [f"s{lab[r]}_{r}" for r in range(n)]
    else:                                          # contiguous videos of 1 / 7 / 500 / 3,000 frames
        ids = [f"v{v}_{i}" for v, ln in enumerate(_contiguous(n, [1, 7, 500, 3000])) for i in range(ln)]
    idx = _mk(vecs, ids)
    from video_quierer_amd.indexes.hnsw import video_of
    keys = [video_of(i) for i in ids]
    truth = _Truth(idx._export(), _unit(qs), ids, keys)
    videos = list(truth.dense)
    for within, exclude in _filters(videos, rng):
        for k in ks:
            for mode in _modes(dim, nq, k):
                _check(idx, ids, qs, truth, k, mode, within, exclude)
                _check_stats(idx, mode, nq)
                _check(idx, ids, qs, truth, k, mode, within, exclude, grouped=True)
    if not _has_fp16(dim, nq, 10):
        # mode 2 where the masked fp16 path does not exist: refused, never silently exact
        idx.search_mode = 2
        with pytest.raises(ValueError, match="masked fp16"):
            idx.search_filtered_batch(list(qs), 5, within=[videos[0]])
        with pytest.raises(ValueError, match="masked fp16"):
            idx.search_grouped_batch(list(qs), 5, exclude=[videos[0]])
    idx.close()


def test_filtered_k_beyond_the_allowed_rows_and_k_1024(gpu_lib):
    rng = np.random.default_rng(3)
    n, dim = 20_000, 256
    vecs = rng.standard_normal((n, dim)).astype(np.float32)
    qs = rng.standard_normal((4, dim)).astype(np.float32)
    ids = [f"v{v}_{i}" for v, ln in enumerate(_contiguous(n, [1, 7, 500, 3000])) for i in range(ln)]
    idx = _mk(vecs, ids)
    from video_quierer_amd.indexes.hnsw import video_of
    truth = _Truth(idx._export(), _unit(qs), ids, [video_of(i) for i in ids])
    for mode in MODES:
        res = _check(idx, ids, qs, truth, 20, mode, within=["v1"])            # a 7-frame video: 7 results
        assert all(len(r) == 7 for r in res)
        res = _check(idx, ids, qs, truth, 20, mode, within=["v0", "v1"], grouped=True)
        assert all(len(r) == 2 for r in res)
        _check(idx, ids, qs, truth, 100, mode, exclude=["v3"])                # the fp16 path's largest k
        if mode == 2:
            continue
        _check(idx, ids, qs, truth, 1024, mode, within=["v3", "v2", "v7"])    # 3,500 rows, k = 1024: exact only
        _check(idx, ids, qs, truth, 1024, mode, exclude=["v3"])
        _check(idx, ids, qs, truth, 1024, mode, exclude=["v3"], grouped=True)
    idx.close()


def test_empty_filters(gpu_lib):
    rng = np.random.default_rng(4)
    n, dim = 20_000, 512
    vecs = rng.standard_normal((n, dim)).astype(np.float32)
    qs = rng.standard_normal((6, dim)).astype(np.float32)
    ids = [f"v{r // 500}_{r % 500}" for r in range(n)]
    idx = _mk(vecs, ids)
    for mode in (0, 1, 2):
        idx.search_mode = mode
        assert idx.search_filtered_batch(list(qs), 10, within=[]) == [[]] * 6
        assert idx.search_filtered_batch(list(qs), 10, within=["unknown"]) == [[]] * 6
        plain = idx.search_batch(list(qs), 10)
        assert idx.search_filtered_batch(list(qs), 10, exclude=[]) == plain            # bit for bit, every mode
        assert idx.search_filtered_batch(list(qs), 10, exclude=["unknown"]) == plain
        assert idx.search_grouped_batch(list(qs), 10, exclude=[]) == idx.search_grouped_batch(list(qs), 10)
    idx.close()


@pytest.mark.parametrize("grouped", [False, True])
def test_filtered_ties_follow_the_callers_string_ids(gpu_lib, grouped):
    """Rows 777 ("video0_777") and 5000 ("video1_0") are exact duplicates (conftest.KNN_BIG_DUPES); query 2 sits next to them.
    Unfiltered, video0_777 sorts first; excluding video0 (or within video1) its copy video1_0 takes its place, same distance."""
    n = 20_000
    rows, qs = knn_big_inputs(n, nq=8)
    ids = knn_big_ids(n)
    idx = _mk(rows, ids)
    from video_quierer_amd.indexes.hnsw import video_of
    truth = _Truth(idx._export(), _unit(qs), ids, [video_of(i) for i in ids])
    for mode in MODES:
        full = idx.search_batch(list(qs), 10) if not grouped else idx.search_grouped_batch(list(qs), 10)
        assert full[2][0]["id"] == "video0_777"
        for within, exclude in ((None, ["video0"]), (["video1"], None), (["video1", "video2"], None)):
            res = _check(idx, ids, qs, truth, 10, mode, within, exclude, grouped=grouped)
            assert res[2][0]["id"] == "video1_0" and res[2][0]["distance"] == full[2][0]["distance"]
        res = _check(idx, ids, qs, truth, 10, mode, within=["video0"], grouped=grouped)
        if not grouped:                                                        # duplicates inside video0: 2 / 10 and 3 / 20 / 100
            assert [r["id"] for r in res[0][:2]] == ["video0_10", "video0_2"]
    idx.close()


def test_filtered_labels_follow_adds_and_removals(gpu_lib):
    rng = np.random.default_rng(5)
    dim = 256
    vecs = rng.standard_normal((3000, dim)).astype(np.float32)
    ids = [f"clip{v}_{i}" for v in range(6) for i in range(500)]
    qs = rng.standard_normal((4, dim)).astype(np.float32)
    idx = _mk(vecs, ids)
    idx.search_filtered(qs[0], 5, within=["clip1"])
    more = rng.standard_normal((700, dim)).astype(np.float32)
    more[0] = qs[0]
    more_ids = [f"new_clip_{i}" for i in range(400)] + [f"clip2_{500 + i}" for i in range(300)]
    idx.add_batch(more, more_ids)                                              # labels stale: Python uploads them again
    all_ids = ids + more_ids
    from video_quierer_amd.indexes.hnsw import video_of
    truth = _Truth(idx._export(), _unit(qs), all_ids, [video_of(i) for i in all_ids])
    for mode in MODES:
        res = _check(idx, all_ids, qs, truth, 8, mode, within=["new_clip"])
        assert res[0][0]["id"] == "new_clip_0"
        _check(idx, all_ids, qs, truth, 8, mode, within=["clip2"])
        _check(idx, all_ids, qs, truth, 8, mode, exclude=["new_clip", "clip0"], grouped=True)
    assert idx.remove_group("clip2") == 800
    assert idx._groups.uploaded == len(idx._ids)                              # the device kept the labels: nothing to upload
    left = [i for i in all_ids if video_of(i) != "clip2"]
    truth = _Truth(idx._export(), _unit(qs), left, [video_of(i) for i in left])
    for mode in MODES:
        _check(idx, left, qs, truth, 8, mode, within=["clip3", "clip2"])
        _check(idx, left, qs, truth, 8, mode, exclude=["clip1"])
        _check(idx, left, qs, truth, 8, mode, exclude=["clip1"], grouped=True)
    assert idx._groups.uploaded == len(idx._ids)
    idx.close()


def test_filtered_c_abi_contract(gpu_lib):
    lib = gpu_lib.load()
    rng = np.random.default_rng(9)
    rows = rng.standard_normal((300, 256)).astype(np.float32)
    rows /= np.linalg.norm(rows, axis=1, keepdims=True)
    h = c_void_p()
    gpu_lib.check(lib.vq_index_create(256, byref(h)))
    gpu_lib.check(lib.vq_index_add(h, gpu_lib.fptr(rows), 300, 0))
    i32 = lambda a: a.ctypes.data_as(POINTER(c_int32))             # noqa: E731
    ids = np.empty((1, 5), np.int32); d = np.empty((1, 5), np.float32)
    g = np.empty((1, 5), np.int32); r = np.empty((1, 5), np.int32)

    def search(sel, exclude=0, mode=1, grouped=False):
        sel = np.asarray(sel, dtype=np.int32)
        q = gpu_lib.fptr(rows[7:8].copy())
        if grouped:
            return lib.vq_index_search_grouped_filtered(h, q, 1, 5, mode, i32(sel), len(sel), exclude, i32(g), i32(r), gpu_lib.fptr(d))
        return lib.vq_index_search_filtered(h, q, 1, 5, mode, i32(sel), len(sel), exclude, i32(ids), gpu_lib.fptr(d))
    assert search([0]) < 0 and b"group labels" in lib.vq_last_error()            # never set
    lab = (np.arange(300) // 10).astype(np.int32)
    gpu_lib.check(lib.vq_index_set_groups(h, i32(lab), 300, 30))
    assert search([30]) < 0 and b"outside" in lib.vq_last_error()
    assert search([-1], 1) < 0
    assert search([0], 2) < 0                                                   # exclude is 0 or 1
    assert search([0], 0, 3) < 0                                                # no mode 3
    gpu_lib.check(search([0]))                                                  # row 7 is in group 0
    assert ids[0, 0] == 7 and set(ids[0]) <= set(range(10))
    want1 = ids.copy(), d.copy()
    gpu_lib.check(search([0], 0, 2))                                            # the masked fp16 path: the same answer
    assert np.array_equal(ids, want1[0]) and np.array_equal(d, want1[1])
    gpu_lib.check(search([0], 1))
    assert ids[0, 0] != 7 and (ids[0] >= 10).all()
    want1 = ids.copy(), d.copy()
    gpu_lib.check(search([0], 1, 2))
    assert np.array_equal(ids, want1[0]) and np.array_equal(d, want1[1])
    gpu_lib.check(search([0, 0, 0], 0, 0, grouped=True))                        # duplicates; one allowed group
    assert g[0].tolist() == [0, -1, -1, -1, -1] and r[0, 0] == 7 and np.isinf(d[0, 1:]).all()
    gpu_lib.check(search([], 0))                                                # nothing allowed
    assert (ids == -1).all() and np.isinf(d).all()
    gpu_lib.check(search([], 1, 2))                                             # nothing excluded: the plain search, any mode
    want = np.empty((1, 5), np.int32); wd = np.empty((1, 5), np.float32)
    gpu_lib.check(lib.vq_index_search(h, gpu_lib.fptr(rows[7:8].copy()), 1, 5, 2, i32(want), gpu_lib.fptr(wd)))
    assert np.array_equal(ids, want) and np.array_equal(d, wd)
    gpu_lib.check(lib.vq_index_add(h, gpu_lib.fptr(rows[:2].copy()), 2, 0))
    assert search([0]) < 0 and b"group labels" in lib.vq_last_error()           # stale after an add: refused
    assert search([0], grouped=True) < 0 and b"group labels" in lib.vq_last_error()
    lab2 = np.concatenate([lab, [0, 29]]).astype(np.int32)
    gpu_lib.check(lib.vq_index_set_groups(h, i32(lab2), 302, 30))
    gpu_lib.check(search([29]))
    assert set(ids[0]) <= set(range(290, 300)) | {301}
    rm = (c_int64 * 10)(*range(10))
    gpu_lib.check(lib.vq_index_remove_rows(h, rm, 10))                          # group 0 loses its rows 0..9, keeps row 300 -> 290
    gpu_lib.check(search([0]))
    assert ids[0, 0] == 290 and (ids[0, 1:] == -1).all()
    gpu_lib.check(lib.vq_index_clear(h))
    gpu_lib.check(lib.vq_index_add(h, gpu_lib.fptr(rows), 300, 0))
    assert search([0]) < 0
    gpu_lib.check(lib.vq_index_destroy(h))


def test_filtered_unnormalised_queries_stay_exact(gpu_lib):
    rng = np.random.default_rng(17)
    dim, n = 512, 30_000
    vecs = rng.standard_normal((n, dim)).astype(np.float32)
    ids = [f"v{r // 300}_{r % 300}" for r in range(n)]
    idx = _mk(vecs, ids)
    stored = idx._export()
    uq = _unit(rng.standard_normal((8, dim)).astype(np.float32))
    lib = gpu_lib.load()
    sel = np.array([3, 40, 41], dtype=np.int32)
    ok = np.isin(np.arange(n) // 300, sel)
    tie = _tie_ranks(ids)
    idx._sync_tie_order(); idx._sync_groups(None)
    for scale in (1e-2, 1e1):                                      # |q|^2 = 1e-4, 1e2
        sq = np.ascontiguousarray(uq * np.float32(scale))
        for exclude, mode in ((0, 0), (0, 2), (1, 0), (1, 2)):
            out = np.empty((8, 10), np.int32); d = np.empty((8, 10), np.float32)
            gpu_lib.check(lib.vq_index_search_filtered(idx._h, gpu_lib.fptr(sq), 8, 10, mode, sel.ctypes.data_as(POINTER(c_int32)), 3, exclude,
                                                       out.ctypes.data_as(POINTER(c_int32)), gpu_lib.fptr(d)))
            st = idx.last_search_stats()
            assert st["exact_fallback"] == 8 and st["verified"] == 0
            allow = ok if not exclude else ~ok
            for j, q in enumerate(sq):
                dd = knn_oracle.distances(stored, q)
                o = np.lexsort((tie, dd))
                o = o[allow[o]][:10]
                assert out[j].tolist() == o.tolist(), f"scale {scale}, exclude {exclude}"
                assert np.array_equal(d[j], dd[o])
    idx.close()


def test_filtered_device_entry_points_match_the_host_ones(gpu_lib):
    import ctypes
    rng = np.random.default_rng(21)
    rows = rng.standard_normal((20_000, 512)).astype(np.float32)
    rows /= np.linalg.norm(rows, axis=1, keepdims=True)
    qs = _unit(rng.standard_normal((24, 512)).astype(np.float32))
    lib = gpu_lib.load()
    h = c_void_p()
    gpu_lib.check(lib.vq_index_create(512, byref(h)))
    gpu_lib.check(lib.vq_index_add(h, gpu_lib.fptr(rows), len(rows), 0))
    lab = (np.arange(len(rows)) // 37).astype(np.int32)
    gpu_lib.check(lib.vq_index_set_groups(h, lab.ctypes.data_as(POINTER(c_int32)), len(rows), int(lab[-1]) + 1))
    i32 = lambda a: a.ctypes.data_as(POINTER(c_int32))             # noqa: E731
    hip = ctypes.CDLL("libamdhip64.so")
    ptrs = []

    def dev(nbytes):
        p = c_void_p()
        assert hip.hipMalloc(byref(p), ctypes.c_size_t(nbytes)) == 0
        ptrs.append(p)
        return p

    def back(host_like, p):
        out = np.empty_like(host_like)
        assert hip.hipMemcpy(out.ctypes.data_as(c_void_p), p, ctypes.c_size_t(out.nbytes), 2) == 0
        return out
    k = 12
    dq = dev(qs.nbytes)
    assert hip.hipMemcpy(dq, qs.ctypes.data_as(c_void_p), ctypes.c_size_t(qs.nbytes), 1) == 0
    di, dd, dg = dev(24 * k * 4), dev(24 * k * 4), dev(24 * k * 4)
    for sel, exclude in ((np.array([5, 300, 5], np.int32), 0), (np.array([0, 17], np.int32), 1)):
        ids = np.empty((24, k), np.int32); d = np.empty((24, k), np.float32)
        gpu_lib.check(lib.vq_index_search_filtered(h, gpu_lib.fptr(qs), 24, k, 1, i32(sel), len(sel), exclude, i32(ids), gpu_lib.fptr(d)))
        gpu_lib.check(lib.vq_index_search_filtered_device(h, dq, 24, k, 0, i32(sel), len(sel), exclude, di, dd))
        gpu_lib.check(lib.vq_index_synchronize(h))
        assert np.array_equal(back(ids, di), ids) and np.array_equal(back(d, dd), d)
        g = np.empty((24, k), np.int32); r = np.empty((24, k), np.int32)
        gpu_lib.check(lib.vq_index_search_grouped_filtered(h, gpu_lib.fptr(qs), 24, k, 1, i32(sel), len(sel), exclude, i32(g), i32(r),
                                                           gpu_lib.fptr(d)))
        gpu_lib.check(lib.vq_index_search_grouped_filtered_device(h, dq, 24, k, 0, i32(sel), len(sel), exclude, dg, di, dd))
        gpu_lib.check(lib.vq_index_synchronize(h))
        assert np.array_equal(back(g, dg), g) and np.array_equal(back(r, di), r) and np.array_equal(back(d, dd), d)
        allowed = np.isin(lab, sel) != bool(exclude)
        assert np.isin(g[g >= 0], np.unique(lab[allowed])).all()
    for p in ptrs:
        hip.hipFree(p)
    gpu_lib.check(lib.vq_index_destroy(h))


@pytest.mark.timeout(900)
def test_filtered_one_million_rows_against_the_oracle(gpu_lib):
    """1M x 512 (knn_big_inputs), the caller's string ids, groups of 500 frames; within one group and excluding one, plain and
    grouped, the default mode."""
    n = 1_000_000
    rows, qs = knn_big_inputs(n, nq=4)
    ids = knn_big_ids(n)
    idx = _mk(rows, ids)
    del rows
    shot = lambda nid: (nid.rsplit("_", 1)[0], int(nid.rsplit("_", 1)[1]) // 500)   # noqa: E731
    truth = _Truth(idx._export(), _unit(qs), ids, [shot(i) for i in ids])
    for grouped in (False, True):
        _check(idx, ids, qs, truth, 10, 0, within=[("video1", 3)], group_of=shot, grouped=grouped)
        assert idx.last_search_stats()["exact_fallback"] == 4                 # one video: the gather path
        _check(idx, ids, qs, truth, 10, 0, exclude=[("video0", 1)], group_of=shot, grouped=grouped)
        assert idx.last_search_stats()["verified"] == 4                       # all but one video: proven on the masked fp16 path
        _check(idx, ids, qs, truth, 10, 2, within=[("video1", 3)], group_of=shot, grouped=grouped)
    idx.close()
