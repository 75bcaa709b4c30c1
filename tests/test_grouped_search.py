"""Grouped exact top-k (vq_index_search_grouped / HNSWIndex.search_grouped): the k best groups (videos), one best row
(frame) each, against the C oracle's exact distances walked in (distance, id) order with every row dropped whose group came
earlier.  Ids, groups and distances must match bit for bit on both the exact (mode 1) and the fp16 (mode 2) path."""
import zlib
from ctypes import POINTER, byref, c_int32, c_int64, c_void_p

import numpy as np
import pytest

from conftest import knn_big_ids, knn_big_inputs
from oracle import knn_oracle
from index_host_fakes import tie_ranks as _tie_ranks, unit as _unit

pytestmark = pytest.mark.gpu


def _expected(stored, uq, group_keys, tie, k):
    """Per query: rows in (distance, tie) order, the first row of every group not seen yet, k of them."""
    if isinstance(group_keys, np.ndarray):
        labels = group_keys
    else:
        dense = {}
        labels = np.array([dense.setdefault(g, len(dense)) for g in group_keys], dtype=np.int64)
    out = []
    for q in uq:
        d = knn_oracle.distances(stored, q)
        order = np.lexsort((tie, d))
        _, first = np.unique(labels[order], return_index=True)
        pick = order[np.sort(first)[:k]]
        out.append([(int(r), d[r]) for r in pick])
    return out


def _check(idx, vecs, ids, qs, k, mode, group_of):
    from video_quierer_amd.indexes.hnsw import video_of
    fn = video_of if group_of is None else group_of
    idx.search_mode = mode
    res = idx.search_grouped_batch(list(qs), k, group_of=group_of) if len(qs) != 1 else [idx.search_grouped(qs[0], k, group_of=group_of)]
    st = idx.last_search_stats()
    stored = idx._export()
    keys = [fn(i) for i in ids]
    want = _expected(stored, _unit(qs), keys, _tie_ranks(ids), k)
    for j, (rr, ww) in enumerate(zip(res, want)):
        assert [r["id"] for r in rr] == [ids[r] for r, _ in ww], f"query {j}: ids differ (mode {mode}, stats {st})"
        assert [r["group"] for r in rr] == [keys[r] for r, _ in ww], f"query {j}: groups differ (mode {mode})"
        assert [r["distance"] for r in rr] == [d for _, d in ww], f"query {j}: distances differ (mode {mode})"
        assert all(type(r["distance"]) is np.float32 and r["score"] == np.float32(1.0) - r["distance"] for r in rr)
    assert st["verified"] + st["exact_fallback"] == len(qs)
    return res, st


def _mk(vecs, ids):
    from video_quierer_amd.indexes.hnsw import OptimizedHNSWIndex
    idx = OptimizedHNSWIndex(dimension=vecs.shape[1])
    idx.add_batch(vecs, ids)
    return idx


def _contiguous_lengths(n, lengths):
    out, i = [], 0
    while sum(out) < n:
        out.append(min(lengths[i % len(lengths)], n - sum(out)))
        i += 1
    return out


# (name, rows, dim, nq, k): layouts x sizes x dims covering the single-query, multi-pass (> 16 queries) and chunked paths
LAYOUTS = [
    ("contiguous_varied", 20_000, 512, 33, 10),
    ("shuffled", 12_000, 256, 4, 10),
    ("one_group", 5_000, 768, 1, 5),
    ("singletons", 4_096, 512, 97, 20),
    ("k_above_groups", 6_000, 256, 4, 20),
    ("contiguous_chunked", 100_000, 512, 300, 10),
]


def _layout(name, n, rng):
    if name.startswith("contiguous"):
        lens = _contiguous_lengths(n, [1, 7, 500, 3000] if name == "contiguous_varied" else [50])
        return [f"v{v}_{i}" for v, ln in enumerate(lens) for i in range(ln)], None
    if name == "shuffled":
        lab = rng.integers(0, 300, n)
        return [f"s{lab[r]}_{r}" for r in range(n)], None
    if name == "one_group":
        return [f"only_{r}" for r in range(n)], None
    if name == "singletons":
        return list(range(n)), None
    if name == "k_above_groups":
        return list(range(n)), (lambda nid: nid % 12)
    raise AssertionError(name)


@pytest.mark.timeout(600)
@pytest.mark.parametrize("name,n,dim,nq,k", LAYOUTS, ids=[x[0] for x in LAYOUTS])
def test_grouped_matches_oracle_on_every_layout(gpu_lib, name, n, dim, nq, k):
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    vecs = rng.standard_normal((n, dim)).astype(np.float32)
    qs = rng.standard_normal((nq, dim)).astype(np.float32)
    qs[: nq // 2] = vecs[rng.integers(0, n, nq // 2)] + np.float32(0.3) * rng.standard_normal((nq // 2, dim)).astype(np.float32)
    ids, group_of = _layout(name, n, rng)
    idx = _mk(vecs, ids)
    for mode in (1, 2):
        res, st = _check(idx, vecs, ids, qs, k, mode, group_of)
        if name == "one_group":
            assert len(res[0]) == 1
        if name == "k_above_groups":
            assert all(len(r) == 12 for r in res)
        if name == "singletons":                                   # every row its own group: the plain search's list
            idx.search_mode = mode
            plain = idx.search_batch(list(qs), k)
            assert [[r["id"] for r in rr] for rr in res] == [[r["id"] for r in rr] for rr in plain]
    idx.close()


@pytest.mark.parametrize("mode", [1, 2])
def test_grouped_ties_follow_the_callers_string_ids(gpu_lib, mode):
    """Planted exact duplicates (conftest.KNN_BIG_DUPES) inside one group and across groups, the caller's string ids
    ("video0_10" sorts before "video0_2"): a group's best row and the order of tied groups follow the id order."""
    n = 20_000
    rows, qs = knn_big_inputs(n, nq=8)
    ids = knn_big_ids(n)
    idx = _mk(rows, ids)
    _check(idx, rows, ids, qs, 10, mode, None)                    # the caller's videos (4 of them)
    frames16 = lambda nid: (nid.rsplit("_", 1)[0], int(nid.rsplit("_", 1)[1]) // 16)   # noqa: E731
    res, _ = _check(idx, rows, ids, qs, 10, mode, frames16)       # 16-frame shots: rows 2 and 10 share one, 3 / 20 / 100 do not
    assert res[0][0]["id"] == "video0_10"                         # duplicate of row 2 whose id sorts first
    idx.close()


def _caller_loop(idx, q, k):
    """video_search_system.py:296-342 restated: over-fetch k * 2 frames, keep each video's first (= best) frame."""
    from video_quierer_amd.indexes.hnsw import video_of
    seen, final = set(), []
    for r in idx.search(q, k * 2):
        vid = video_of(r["id"])
        if vid in seen:
            continue
        seen.add(vid)
        final.append(r)
        if len(final) >= k:
            break
    return final


def test_grouped_returns_k_videos_where_the_callers_overfetch_falls_short(gpu_lib):
    rng = np.random.default_rng(11)
    dim, k = 512, 5
    vecs = rng.standard_normal((40 * 50, dim)).astype(np.float32)
    q = rng.standard_normal(dim).astype(np.float32)
    q /= np.linalg.norm(q)
    hot = q[None, :] + np.float32(0.02) * rng.standard_normal((100, dim)).astype(np.float32)   # 100 near-duplicate frames of one shot
    ids = [f"video{v}_{i}" for v in range(40) for i in range(50)] + [f"hot_video_{i}" for i in range(100)]
    idx = _mk(np.concatenate([vecs, hot]), ids)
    for mode in (1, 2):
        idx.search_mode = mode
        loop = _caller_loop(idx, q, k)
        assert len(loop) < k                                      # the caller's bug: the top 2k frames are all one video
        got = idx.search_grouped(q, k)
        assert len(got) == k and len({r["group"] for r in got}) == k
        assert got[0]["group"] == "hot_video"
        assert [(r["id"], r["distance"]) for r in got[: len(loop)]] == [(r["id"], r["distance"]) for r in loop]
        _check(idx, None, ids, q[None, :], k, mode, None)
    idx.close()


def test_grouped_labels_follow_adds(gpu_lib):
    rng = np.random.default_rng(5)
    dim = 256
    vecs = rng.standard_normal((3000, dim)).astype(np.float32)
    ids = [f"clip{v}_{i}" for v in range(6) for i in range(500)]
    qs = rng.standard_normal((4, dim)).astype(np.float32)
    idx = _mk(vecs, ids)
    _check(idx, vecs, ids, qs, 8, 2, None)
    more = rng.standard_normal((700, dim)).astype(np.float32)
    more[0] = qs[0]                                                # the new video holds the best frame for query 0
    more_ids = [f"new_clip_{i}" for i in range(400)] + [f"clip2_{500 + i}" for i in range(300)]
    idx.add_batch(more, more_ids)
    all_ids = ids + more_ids
    for mode in (1, 2):
        res, _ = _check(idx, None, all_ids, qs, 8, mode, None)
        assert res[0][0]["group"] == "new_clip" and res[0][0]["id"] == "new_clip_0"
    idx.close()


def test_grouped_c_abi_contract(gpu_lib):
    lib = gpu_lib.load()
    rng = np.random.default_rng(9)
    rows = rng.standard_normal((300, 256)).astype(np.float32)
    rows /= np.linalg.norm(rows, axis=1, keepdims=True)
    h = c_void_p()
    gpu_lib.check(lib.vq_index_create(256, byref(h)))
    gpu_lib.check(lib.vq_index_add(h, gpu_lib.fptr(rows), 300, 0))
    g = np.empty((1, 3), np.int32); r = np.empty((1, 3), np.int32); d = np.empty((1, 3), np.float32)
    i32 = lambda a: a.ctypes.data_as(POINTER(c_int32))             # noqa: E731

    def search(mode=1):
        return lib.vq_index_search_grouped(h, gpu_lib.fptr(rows[7:8].copy()), 1, 3, mode, i32(g), i32(r), gpu_lib.fptr(d))
    assert search() < 0 and b"group labels" in lib.vq_last_error()     # never set
    lab = (np.arange(300) // 10).astype(np.int32)
    assert lib.vq_index_set_groups(h, i32(lab), 299, 30) < 0           # wrong n
    bad = lab.copy(); bad[5] = 30
    assert lib.vq_index_set_groups(h, i32(bad), 300, 30) < 0           # label out of range
    bad = lab.copy(); bad[5] = -1
    assert lib.vq_index_set_groups(h, i32(bad), 300, 30) < 0
    assert lib.vq_index_set_groups(h, i32(lab), 300, 31) < 0           # group 30 empty: not dense
    gpu_lib.check(lib.vq_index_set_groups(h, i32(lab), 300, 30))
    for mode in (1, 2):
        gpu_lib.check(search(mode))
        assert g[0, 0] == 0 and r[0, 0] == 7 and len(set(g[0])) == 3
    rn = (c_int64 * 1)(12)
    gpu_lib.check(lib.vq_index_update_rows(h, gpu_lib.fptr(rows[5:6].copy()), rn, 1, 0))   # same rows: labels kept
    gpu_lib.check(search())
    gpu_lib.check(lib.vq_index_add(h, gpu_lib.fptr(rows[:2].copy()), 2, 0))
    assert search() < 0 and b"group labels" in lib.vq_last_error()     # stale after an add: refused
    lab2 = np.concatenate([lab, [0, 29]]).astype(np.int32)
    gpu_lib.check(lib.vq_index_set_groups(h, i32(lab2), 302, 30))
    gpu_lib.check(search())
    gpu_lib.check(lib.vq_index_set_groups(h, None, 0, 0))              # cleared
    assert search() < 0
    gpu_lib.check(lib.vq_index_set_groups(h, i32(lab2), 302, 30))
    gpu_lib.check(lib.vq_index_clear(h))                                # clear drops them
    gpu_lib.check(lib.vq_index_add(h, gpu_lib.fptr(rows), 300, 0))
    assert search() < 0
    gpu_lib.check(lib.vq_index_destroy(h))


def test_grouped_device_entry_point_matches_the_host_one(gpu_lib):
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
    k = 12
    g = np.empty((24, k), np.int32); r = np.empty((24, k), np.int32); d = np.empty((24, k), np.float32)
    gpu_lib.check(lib.vq_index_search_grouped(h, gpu_lib.fptr(qs), 24, k, 2, g.ctypes.data_as(POINTER(c_int32)),
                                              r.ctypes.data_as(POINTER(c_int32)), gpu_lib.fptr(d)))
    hip = ctypes.CDLL("libamdhip64.so")                            # device buffers straight from the runtime the library uses
    ptrs = []

    def dev(nbytes):
        p = c_void_p()
        assert hip.hipMalloc(byref(p), ctypes.c_size_t(nbytes)) == 0
        ptrs.append(p)
        return p
    dq, dg, dr, dd = dev(qs.nbytes), dev(g.nbytes), dev(r.nbytes), dev(d.nbytes)
    assert hip.hipMemcpy(dq, qs.ctypes.data_as(c_void_p), ctypes.c_size_t(qs.nbytes), 1) == 0          # hipMemcpyHostToDevice
    gpu_lib.check(lib.vq_index_search_grouped_device(h, dq, 24, k, 2, dg, dr, dd))
    gpu_lib.check(lib.vq_index_synchronize(h))
    for host, p in ((np.empty_like(g), dg), (np.empty_like(r), dr), (np.empty_like(d), dd)):
        assert hip.hipMemcpy(host.ctypes.data_as(c_void_p), p, ctypes.c_size_t(host.nbytes), 2) == 0  # hipMemcpyDeviceToHost
        assert np.array_equal(host, {id(dg): g, id(dr): r, id(dd): d}[id(p)])
    for p in ptrs:
        hip.hipFree(p)
    want = _expected(rows, qs, lab, np.arange(len(rows)), k)
    assert [[int(x) for x in rr] for rr in r] == [[x for x, _ in ww] for ww in want]
    assert np.array_equal(d, np.array([[y for _, y in ww] for ww in want], dtype=np.float32))
    gpu_lib.check(lib.vq_index_destroy(h))


def test_grouped_proof_paths(gpu_lib):
    """fp16 path taken on normal queries; queries at |q|^2 = 1e-4 and 1e2 (C ABI, not normalised) go to the exact path and
    stay exact; one huge group of near-identical rows next to the query stays exact."""
    from video_quierer_amd.indexes.hnsw import MODE_FP16
    rng = np.random.default_rng(17)
    dim, n = 512, 30_000
    vecs = rng.standard_normal((n, dim)).astype(np.float32)
    base = rng.standard_normal(dim).astype(np.float32)
    vecs[10_000:13_000] = base + np.float32(1e-3) * rng.standard_normal((3000, dim)).astype(np.float32)   # one huge near-tied group
    ids = list(range(n))
    group_of = lambda nid: 10_000 if 10_000 <= nid < 13_000 else nid // 100   # noqa: E731
    qs = rng.standard_normal((8, dim)).astype(np.float32)
    qs[0] = base + np.float32(1e-3) * rng.standard_normal(dim).astype(np.float32)
    idx = _mk(vecs, ids)
    _, st = _check(idx, vecs, ids, qs, 10, MODE_FP16, group_of)
    assert st["verified"] == len(qs) and st["exact_fallback"] == 0 and st["rescanned"] > 0
    stored = idx._export()
    lib = gpu_lib.load()
    labels = np.array([group_of(i) for i in ids])
    dense = np.unique(labels, return_inverse=True)[1]
    uq = _unit(qs)
    for scale in (1e-2, 1e1):                                      # |q|^2 = 1e-4, 1e2
        sq = np.ascontiguousarray(uq * np.float32(scale))
        g = np.empty((8, 10), np.int32); r = np.empty((8, 10), np.int32); d = np.empty((8, 10), np.float32)
        gpu_lib.check(lib.vq_index_search_grouped(idx._h, gpu_lib.fptr(sq), 8, 10, 2, g.ctypes.data_as(POINTER(c_int32)),
                                                  r.ctypes.data_as(POINTER(c_int32)), gpu_lib.fptr(d)))
        st = idx.last_search_stats()
        assert st["exact_fallback"] == 8 and st["verified"] == 0
        want = _expected(stored, sq, dense, np.arange(n), 10)
        assert [[int(x) for x in rr] for rr in r] == [[x for x, _ in ww] for ww in want], f"scale {scale}"
        assert np.array_equal(d, np.array([[y for _, y in ww] for ww in want], dtype=np.float32)), f"scale {scale}"
    idx.close()


@pytest.mark.timeout(900)
def test_grouped_one_million_rows_against_the_oracle(gpu_lib):
    """1M x 512 unit rows in 2,000 contiguous videos of 500 frames, nq = 8, k = 10, the default mode."""
    rng = np.random.default_rng(1_000_000)
    n, dim = 1_000_000, 512
    vecs = rng.standard_normal((n, dim), dtype=np.float32)
    qs = rng.standard_normal((8, dim), dtype=np.float32)
    qs[:4] = vecs[rng.integers(0, n, 4)] + np.float32(0.5) * rng.standard_normal((4, dim), dtype=np.float32)
    ids = range(n)
    idx = _mk(vecs, ids)
    del vecs
    res = idx.search_grouped_batch(list(qs), 10, group_of=lambda nid: nid // 500)
    st = idx.last_search_stats()
    assert st["verified"] == 8
    stored = idx._export()
    want = _expected(stored, _unit(qs), np.arange(n) // 500, np.arange(n), 10)
    for rr, ww in zip(res, want):
        assert [x["id"] for x in rr] == [x for x, _ in ww]
        assert [x["group"] for x in rr] == [x // 500 for x, _ in ww]
        assert [x["distance"] for x in rr] == [y for _, y in ww]
    idx.close()
