"""Clip search (vq_index_search_set / HNSWIndex.search_set / similar_groups): the k groups most similar to a SET of query
frames.  The expectation comes from the C oracle alone: its exact distances per query frame, numpy for the group minimum by
(distance, tie rank), an fp64 loop in query order for the mean, np.lexsort((label, D)).  Labels, distances (bit for bit) and
matches must be identical on the exact (mode 1) and the fp16 (mode 2) path."""
import ctypes
import zlib
from ctypes import POINTER, byref, c_int32, c_int64, c_void_p

import numpy as np
import pytest

from conftest import knn_big_ids, knn_big_inputs
from oracle import knn_oracle
from index_host_fakes import tie_ranks as _tie_ranks, unit as _unit

pytestmark = pytest.mark.gpu

SET_KEY_BUDGET = 16 << 20          # csrc/knn_set.h: candidate (group, query) keys the fp16 path holds before it redoes the call exactly


def _dense(keys):
    seen = {}
    return np.array([seen.setdefault(g, len(seen)) for g in keys], dtype=np.int64), list(seen)


def _expected(stored, uq, labels, tie, k, allowed=None):
    """[(label, D, [row per query frame])]: the first k allowed groups by (D, label)."""
    m, G = len(uq), int(labels.max()) + 1
    acc = np.zeros(G, dtype=np.float64)
    rows = np.empty((m, G), dtype=np.int64)
    for i, q in enumerate(uq):                                    # fp64, query order
        d = knn_oracle.distances(stored, q)
        order = np.lexsort((tie, d))
        lab, first = np.unique(labels[order], return_index=True)  # a group's first row in (distance, tie) order
        assert len(lab) == G
        rows[i] = order[first]
        acc += d[rows[i]].astype(np.float64)
    D = (acc / np.float64(m)).astype(np.float32)
    order = np.lexsort((np.arange(G), D))
    if allowed is not None:
        ok = np.zeros(G, dtype=bool)
        ok[list(allowed)] = True
        order = order[ok[order]]
    return [(int(g), D[g], rows[:, g].tolist()) for g in order[:k]]


def _mk(vecs, ids):
    from video_quierer_amd.indexes.hnsw import OptimizedHNSWIndex
    idx = OptimizedHNSWIndex(dimension=vecs.shape[1])
    idx.add_batch(vecs, ids)
    return idx


def _check(idx, ids, qs, k, mode, group_of=None, within=None, exclude=None):
    from video_quierer_amd.indexes.hnsw import video_of
    fn = video_of if group_of is None else group_of
    idx.search_mode = mode
    res = idx.search_set(list(qs), k, within=within, exclude=exclude, group_of=group_of, matches=True)
    st = idx.last_search_stats()
    labels, keys = _dense([fn(i) for i in ids])
    allowed = None
    if within is not None:
        allowed = {keys.index(g) for g in within if g in keys}
    if exclude is not None:
        allowed = set(range(len(keys))) - {keys.index(g) for g in exclude if g in keys}
    want = _expected(idx._export(), _unit(qs), labels, _tie_ranks(ids), k, allowed)
    tag = f"(mode {mode}, stats {st})"
    assert [r["group"] for r in res] == [keys[g] for g, _, _ in want], f"groups differ {tag}"
    assert [r["distance"] for r in res] == [d for _, d, _ in want], f"distances differ {tag}"
    assert [r["matches"] for r in res] == [[ids[r] for r in rr] for _, _, rr in want], f"matches differ {tag}"
    assert all(type(r["distance"]) is np.float32 and r["score"] == np.float32(1.0) - r["distance"] for r in res)
    assert st["verified"] + st["exact_fallback"] == 1, tag
    if mode == 1:
        assert st["exact_fallback"] == 1
    return res, st


def _contiguous_lengths(n, lengths):
    out, i = [], 0
    while sum(out) < n:
        out.append(min(lengths[i % len(lengths)], n - sum(out)))
        i += 1
    return out


# (name, rows, dim, m, k): m = 1 and 16 take the streaming group-max scan, 17 / 130 one partial query tile of the batch scan,
# 300 more than one query tile
LAYOUTS = [
    ("contiguous_varied", 20_000, 512, 130, 10),
    ("contiguous_768", 20_000, 768, 17, 10),
    ("shuffled", 12_000, 256, 17, 10),
    ("shuffled_300", 12_000, 512, 300, 10),
    ("one_group", 5_000, 768, 1, 5),
    ("singletons", 4_096, 512, 300, 20),
    ("k_above_groups", 6_000, 256, 16, 20),
    ("contiguous_chunked", 100_000, 512, 300, 10),
]


def _layout(name, n, rng):
    if name.startswith("contiguous"):
        lens = _contiguous_lengths(n, [50] if name == "contiguous_chunked" else [1, 7, 500, 3000])
        return [f"v{v}_{i}" for v, ln in enumerate(lens) for i in range(ln)], None
    if name.startswith("shuffled"):
        lab = rng.integers(0, 300, n)
        return [f"s{lab[r]}_{r}" for r in range(n)], None
    if name == "one_group":
        return [f"only_{r}" for r in range(n)], None
    if name == "singletons":
        return list(range(n)), None
    if name == "k_above_groups":
        return list(range(n)), (lambda nid: nid % 12)
    raise AssertionError(name)


def _clip(vecs, m, rng, sigma=0.5):
    """m query frames: half of them noisy copies of a run of stored rows (a cut of an indexed video), half random."""
    n, dim = vecs.shape
    qs = rng.standard_normal((m, dim)).astype(np.float32)
    h = (m + 1) // 2
    start = int(rng.integers(0, max(1, n - h)))
    src = vecs[start:start + h]
    qs[:h] = src / np.linalg.norm(src, axis=1, keepdims=True) + np.float32(sigma / np.sqrt(dim)) * rng.standard_normal((h, dim)).astype(np.float32)
    return qs


@pytest.mark.timeout(900)
@pytest.mark.parametrize("name,n,dim,m,k", LAYOUTS, ids=[x[0] for x in LAYOUTS])
def test_set_search_matches_oracle_on_every_layout(gpu_lib, name, n, dim, m, k):
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    vecs = rng.standard_normal((n, dim)).astype(np.float32)
    ids, group_of = _layout(name, n, rng)
    qs = _clip(vecs, m, rng)
    idx = _mk(vecs, ids)
    for mode in (1, 2):
        res, _ = _check(idx, ids, qs, k, mode, group_of)
        if name == "one_group":
            assert len(res) == 1
        if name == "k_above_groups":
            assert len(res) == 12
    idx.close()


@pytest.mark.parametrize("mode", [1, 2])
def test_set_search_matches_follow_the_callers_string_ids(gpu_lib, mode):
    """Planted exact duplicates (conftest.KNN_BIG_DUPES) inside one group, the caller's string ids ("video0_10" sorts before
    "video0_2"): the matching row of a query frame next to them is the duplicate whose id sorts first."""
    n = 20_000
    rows, qs = knn_big_inputs(n, nq=24)
    ids = knn_big_ids(n)
    idx = _mk(rows, ids)
    res, _ = _check(idx, ids, qs, 4, mode)
    assert res[0]["group"] == "video0"                            # the three planted query frames sit next to rows of video0
    assert res[0]["matches"][0] == "video0_10" and res[0]["matches"][1] == "video0_100"
    frames16 = lambda nid: (nid.rsplit("_", 1)[0], int(nid.rsplit("_", 1)[1]) // 16)   # noqa: E731
    _check(idx, ids, qs, 10, mode, frames16)
    idx.close()


def _planted(n_videos, per, dim, m, seed, planted):
    rng = np.random.default_rng(seed)
    vecs = rng.standard_normal((n_videos * per, dim)).astype(np.float32)
    vecs /= np.linalg.norm(vecs, axis=1, keepdims=True)
    clip = rng.standard_normal((m, dim)).astype(np.float32)
    clip /= np.linalg.norm(clip, axis=1, keepdims=True)
    where = rng.permutation(n_videos)[:planted]
    for j, v in enumerate(where.tolist()):                        # video v holds every clip frame under noise sigma_j
        sigma = 0.25 + 0.08 * j
        f = clip[np.arange(per) % m] + np.float32(sigma / np.sqrt(dim)) * rng.standard_normal((per, dim)).astype(np.float32)
        vecs[v * per:(v + 1) * per] = f / np.linalg.norm(f, axis=1, keepdims=True)
    return vecs, clip, where.tolist()


def test_fp16_path_proves_planted_videos(gpu_lib):
    """Twelve videos hold the clip's frames under growing noise (exact mean scores 0.970 down to 0.659, every other video
    0.10 .. 0.12): the fp16 path must PROVE the answer, re-scoring few rows."""
    n_videos, per, dim, m, k = 400, 100, 512, 64, 10
    vecs, clip, where = _planted(n_videos, per, dim, m, 20261016, 12)
    ids = list(range(n_videos * per))
    group_of = lambda nid: nid // per                            # noqa: E731
    idx = _mk(vecs, ids)
    res, st = _check(idx, ids, clip, k, 2, group_of)
    assert st["verified"] == 1 and st["exact_fallback"] == 0
    assert 0 < st["rescanned"] < m * len(ids)
    assert [r["group"] for r in res] == where[:k]                 # the planted videos in sigma order
    assert res[0]["score"] > 0.96 and res[k - 1]["score"] > 0.7
    _check(idx, ids, clip, k, 1, group_of)
    idx.close()


def test_fp16_path_stays_exact_on_unstructured_data(gpu_lib):
    """Only random rows: many groups lie within the error bound of the 10th; the answer is still exact on mode 2, whichever of
    proof or redo produced it."""
    vecs, clip, _ = _planted(388, 100, 512, 64, 20261017, 0)
    ids = list(range(len(vecs)))
    idx = _mk(vecs, ids)
    _check(idx, ids, clip, 10, 2, lambda nid: nid // 100)
    idx.close()


def _raw_index(gpu_lib, rows, labels):
    lib = gpu_lib.load()
    h = c_void_p()
    gpu_lib.check(lib.vq_index_create(rows.shape[1], byref(h)))
    gpu_lib.check(lib.vq_index_add(h, gpu_lib.fptr(rows), len(rows), 0))
    lab = np.ascontiguousarray(labels, dtype=np.int32)
    gpu_lib.check(lib.vq_index_set_groups(h, lab.ctypes.data_as(POINTER(c_int32)), len(rows), int(lab.max()) + 1))
    return lib, h


def _i32(a):
    return a.ctypes.data_as(POINTER(c_int32))


def _raw_set(gpu_lib, lib, h, qs, k, mode, sel=(), exclude=1, matches=True):
    m = len(qs)
    g = np.empty(k, np.int32); d = np.empty(k, np.float32); r = np.empty((k, m), np.int32)
    s = np.array(list(sel), dtype=np.int32)
    rc = lib.vq_index_search_set(h, gpu_lib.fptr(np.ascontiguousarray(qs, dtype=np.float32)), m, k, mode, _i32(s) if len(s) else None,
                                 len(s), exclude, _i32(g), gpu_lib.fptr(d), _i32(r) if matches else None)
    st = (c_int64 * 3)()
    if rc == 0:
        gpu_lib.check(lib.vq_index_last_search_stats(h, st))
    return rc, g, d, r, [int(x) for x in st]


def _assert_raw(got, want, k):
    _, g, d, r, _ = got
    assert g.tolist() == [x for x, _, _ in want] + [-1] * (k - len(want))
    assert np.array_equal(d[:len(want)], np.array([y for _, y, _ in want], dtype=np.float32)) and np.all(np.isinf(d[len(want):]))
    assert r[:len(want)].tolist() == [rr for _, _, rr in want] and np.all(r[len(want):] == -1)


def test_redo_on_queries_outside_the_bound_and_on_candidate_overflow(gpu_lib):
    rng = np.random.default_rng(31)
    n, dim, m, k = 30_000, 512, 40, 10
    rows = rng.standard_normal((n, dim)).astype(np.float32)
    rows /= np.linalg.norm(rows, axis=1, keepdims=True)
    labels = np.arange(n) // 100
    lib, h = _raw_index(gpu_lib, rows, labels)
    tie = np.arange(n)
    base = _unit(_clip(rows, m, rng))
    for scale in (1e-2, 1e1):                                      # one frame at |q|^2 = 1e-4, one at 1e2
        qs = base.copy()
        qs[7] *= np.float32(scale)
        want = _expected(rows, qs, labels, tie, k)
        got2 = _raw_set(gpu_lib, lib, h, qs, k, 2)
        assert got2[0] == 0 and got2[4] == [0, 0, 1], f"scale {scale}: {got2[4]}"
        _assert_raw(got2, want, k)
        got1 = _raw_set(gpu_lib, lib, h, qs, k, 1)
        assert got1[0] == 0 and got1[4] == [0, 0, 1]
        _assert_raw(got1, want, k)
    got = _raw_set(gpu_lib, lib, h, base, k, 2)                    # the same clip as given: proven
    assert got[4][0] == 1 and got[4][2] == 0
    _assert_raw(got, _expected(rows, base, labels, tie, k), k)
    gpu_lib.check(lib.vq_index_destroy(h))
    # Candidate overflow: 60,000 singleton groups of near-identical rows; every group's mean fp16 score lies within the error
    # bound of the k-th, so all of them are candidates: 60,000 x 300 = 18,000,000 (group, query) keys > SET_KEY_BUDGET.
    n, dim, m = 60_000, 256, 300
    assert n * m > SET_KEY_BUDGET
    b = rng.standard_normal(dim).astype(np.float32)
    rows = b + np.float32(1e-3) * rng.standard_normal((n, dim)).astype(np.float32)
    rows /= np.linalg.norm(rows, axis=1, keepdims=True)
    rows = rows.astype(np.float32)
    lib, h = _raw_index(gpu_lib, rows, np.arange(n))
    qs = _unit(rng.standard_normal((m, dim)).astype(np.float32))
    want = _expected(rows, qs, np.arange(n), np.arange(n), k)
    got2 = _raw_set(gpu_lib, lib, h, qs, k, 2)
    assert got2[0] == 0 and got2[4] == [0, 0, 1], got2[4]
    _assert_raw(got2, want, k)
    _assert_raw(_raw_set(gpu_lib, lib, h, qs, k, 1), want, k)
    gpu_lib.check(lib.vq_index_destroy(h))


def test_device_form_on_a_caller_owned_stream(gpu_lib):
    rng = np.random.default_rng(41)
    n, dim, m, k = 20_000, 512, 130, 12
    rows = rng.standard_normal((n, dim)).astype(np.float32)
    rows /= np.linalg.norm(rows, axis=1, keepdims=True)
    labels = np.arange(n) // 37
    lib, h = _raw_index(gpu_lib, rows, labels)
    qs = _unit(_clip(rows, m, rng))
    want = _expected(rows, qs, labels, np.arange(n), k)
    hip = ctypes.CDLL("libamdhip64.so")
    stream = c_void_p()
    assert hip.hipStreamCreate(byref(stream)) == 0
    gpu_lib.check(lib.vq_index_set_stream(h, stream))
    ptrs = []

    def dev(nbytes):
        p = c_void_p()
        assert hip.hipMalloc(byref(p), ctypes.c_size_t(nbytes)) == 0
        ptrs.append(p)
        return p
    dq, dg, dd, dr = dev(qs.nbytes), dev(4 * k), dev(4 * k), dev(4 * k * m)
    assert hip.hipMemcpy(dq, qs.ctypes.data_as(c_void_p), ctypes.c_size_t(qs.nbytes), 1) == 0
    for mode in (1, 2):
        gpu_lib.check(lib.vq_index_search_set_device(h, dq, m, k, mode, None, 0, 1, dg, dd, dr))
        assert hip.hipStreamSynchronize(stream) == 0
        g = np.empty(k, np.int32); d = np.empty(k, np.float32); r = np.empty((k, m), np.int32)
        for host, p in ((g, dg), (d, dd), (r, dr)):
            assert hip.hipMemcpy(host.ctypes.data_as(c_void_p), p, ctypes.c_size_t(host.nbytes), 2) == 0
        st = (c_int64 * 3)()
        gpu_lib.check(lib.vq_index_last_search_stats(h, st))
        assert st[0] + st[2] == 1 and (mode == 2 or st[2] == 1)
        _assert_raw((0, g, d, r, None), want, k)
    # the filter list stays on the host in the device form; no match rows asked for
    sel = np.array([want[0][0], want[2][0]], dtype=np.int32)
    gpu_lib.check(lib.vq_index_search_set_device(h, dq, m, k, 2, _i32(sel), 2, 1, dg, dd, None))
    assert hip.hipStreamSynchronize(stream) == 0
    g = np.empty(k, np.int32)
    assert hip.hipMemcpy(g.ctypes.data_as(c_void_p), dg, ctypes.c_size_t(g.nbytes), 2) == 0
    assert g.tolist() == [x for x, _, _ in _expected(rows, qs, labels, np.arange(n), k, set(range(int(labels.max()) + 1)) - set(sel.tolist()))]
    gpu_lib.check(lib.vq_index_set_stream(h, None))
    for p in ptrs:
        hip.hipFree(p)
    assert hip.hipStreamDestroy(stream) == 0
    gpu_lib.check(lib.vq_index_destroy(h))


@pytest.mark.parametrize("mode", [1, 2])
def test_filters_strike_groups_out_of_the_unfiltered_ranking(gpu_lib, mode):
    rng = np.random.default_rng(51)
    n, dim, m = 24_000, 512, 33
    vecs = rng.standard_normal((n, dim)).astype(np.float32)
    ids = [f"v{r // 200}_{r % 200}" for r in range(n)]            # 120 videos
    qs = _clip(vecs, m, rng)
    idx = _mk(vecs, ids)
    full, _ = _check(idx, ids, qs, 120, mode)
    ranking = [r["group"] for r in full]
    assert len(ranking) == 120
    top = ranking[0]
    res, _ = _check(idx, ids, qs, 10, mode, exclude=[top])
    assert [r["group"] for r in res] == ranking[1:11]
    inc = [ranking[5], ranking[40], ranking[2], ranking[40], "unknown"]       # a duplicate and an unknown key
    res, _ = _check(idx, ids, qs, 10, mode, within=inc)
    assert [r["group"] for r in res] == [ranking[2], ranking[5], ranking[40]]
    res, _ = _check(idx, ids, qs, 10, mode, exclude=[])           # nothing excluded: the unfiltered call
    assert [r["group"] for r in res] == ranking[:10]
    assert idx.search_set(list(qs), 10, within=[]) == []
    assert idx.search_set(list(qs), 10, exclude=ranking) == []    # every group excluded
    # n_sel = 0 both ways and every group excluded, through the raw entry point
    lib = gpu_lib.load()
    uq = _unit(qs)
    rc, g, d, r, st = _raw_set(gpu_lib, lib, idx._h, uq, 5, mode, (), 0)
    assert rc == 0 and g.tolist() == [-1] * 5 and np.all(np.isinf(d)) and np.all(r == -1)
    rc, g, d, r, st = _raw_set(gpu_lib, lib, idx._h, uq, 5, mode, range(120), 1)
    assert rc == 0 and g.tolist() == [-1] * 5 and np.all(np.isinf(d)) and np.all(r == -1)
    rc, g, d, r, st = _raw_set(gpu_lib, lib, idx._h, uq, 5, mode, (), 1)
    assert rc == 0 and [f"v{x}" for x in g.tolist()] == ranking[:5]
    # similar_groups(g) never returns g and equals search_set(stored rows of g, exclude=[g])
    sim = idx.similar_groups(top, 7, matches=True)
    assert len(sim) == 7 and top not in [r["group"] for r in sim]
    rows_of_top = idx._export()[[r for r, i in enumerate(ids) if i.rsplit("_", 1)[0] == top]]
    assert sim == idx.search_set(list(rows_of_top), 7, exclude=[top], matches=True)
    sim_in = idx.similar_groups(top, 7, within=[top, ranking[3], ranking[9]])
    assert sorted(r["group"] for r in sim_in) == sorted([ranking[3], ranking[9]])
    idx.close()


def test_lifetime_and_argument_checks(gpu_lib):
    rng = np.random.default_rng(61)
    rows = rng.standard_normal((3000, 256)).astype(np.float32)
    rows /= np.linalg.norm(rows, axis=1, keepdims=True)
    labels = np.arange(3000) // 100
    lib, h = _raw_index(gpu_lib, rows, labels)
    qs = rows[100:108].copy()
    want = _expected(rows, qs, labels, np.arange(3000), 3)
    for mode in (0, 1, 2):
        got = _raw_set(gpu_lib, lib, h, qs, 3, mode)
        assert got[0] == 0 and got[1][0] == 1
        _assert_raw(got, want, 3)
    bad = [dict(qs=qs[:0]), dict(qs=np.zeros((4097, 256), np.float32)), dict(k=0), dict(k=1025), dict(sel=(30,)), dict(sel=(-1,)),
           dict(mode=3), dict(exclude=2)]
    for kw in bad:
        a = dict(qs=qs, k=3, mode=1, sel=(), exclude=1)
        a.update(kw)
        assert _raw_set(gpu_lib, lib, h, a["qs"], a["k"], a["mode"], a["sel"], a["exclude"])[0] == -1, kw
        assert _raw_set(gpu_lib, lib, h, qs, 3, 2)[0] == 0        # the next valid call works
    g3 = np.empty(3, np.int32); d3 = np.empty(3, np.float32)
    assert lib.vq_index_search_set(h, gpu_lib.fptr(qs), 0, 3, 1, None, 0, 1, _i32(g3), gpu_lib.fptr(d3), None) == -1      # m = 0, valid pointers
    rn = (c_int64 * 1)(12)
    gpu_lib.check(lib.vq_index_update_rows(h, gpu_lib.fptr(rows[12:13].copy()), rn, 1, 0))     # same rows: labels kept
    _assert_raw(_raw_set(gpu_lib, lib, h, qs, 3, 2), want, 3)
    gpu_lib.check(lib.vq_index_add(h, gpu_lib.fptr(rows[:2].copy()), 2, 0))
    for mode in (1, 2):                                           # stale labels after an add: refused
        assert _raw_set(gpu_lib, lib, h, qs, 3, mode)[0] == -1 and b"group labels" in lib.vq_last_error()
    lab2 = np.concatenate([labels, [0, 29]]).astype(np.int32)
    gpu_lib.check(lib.vq_index_set_groups(h, _i32(lab2), 3002, 30))
    assert _raw_set(gpu_lib, lib, h, qs, 3, 2)[0] == 0
    gpu_lib.check(lib.vq_index_destroy(h))
    # mode 2 where the fp16 path does not exist (dim 384): refused; mode 0 and 1 answer
    rows = rng.standard_normal((500, 384)).astype(np.float32)
    rows /= np.linalg.norm(rows, axis=1, keepdims=True)
    lib, h = _raw_index(gpu_lib, rows, np.arange(500) // 50)
    assert _raw_set(gpu_lib, lib, h, rows[:5].copy(), 3, 2)[0] == -1
    want = _expected(rows, rows[:5], np.arange(500) // 50, np.arange(500), 3)
    for mode in (0, 1):
        _assert_raw(_raw_set(gpu_lib, lib, h, rows[:5].copy(), 3, mode), want, 3)
    gpu_lib.check(lib.vq_index_destroy(h))


def test_set_search_after_remove_group(gpu_lib):
    rng = np.random.default_rng(71)
    vecs = rng.standard_normal((6000, 256)).astype(np.float32)
    ids = [f"clip{r // 500}_{r % 500}" for r in range(6000)]
    qs = _clip(vecs, 20, rng)
    idx = _mk(vecs, ids)
    res, _ = _check(idx, ids, qs, 5, 2)
    gone = res[0]["group"]
    assert idx.remove_group(gone) == 500
    left = [i for i in ids if i.rsplit("_", 1)[0] != gone]
    for mode in (1, 2):
        res2, _ = _check(idx, left, qs, 5, mode)
        assert gone not in [r["group"] for r in res2]
    idx.close()


def test_similar_videos_on_a_toy_index(gpu_lib):
    from video_quierer_amd.overhaul_index import SimpleVideoIndex
    rng = np.random.default_rng(81)
    dim = 512
    a = rng.standard_normal((6, dim)).astype(np.float32)
    frames = [("a.mp4", a[i]) for i in range(6)]
    frames += [("b.mp4", a[i] + np.float32(0.3) * rng.standard_normal(dim).astype(np.float32)) for i in (1, 3, 4)]     # a cut of a
    frames += [("c.mp4", rng.standard_normal(dim).astype(np.float32)) for _ in range(5)]
    order = rng.permutation(len(frames))
    svi = SimpleVideoIndex()
    names = []
    for t, j in enumerate(order.tolist()):
        v = frames[j][1] / np.linalg.norm(frames[j][1])
        svi.add_frame(v.astype(np.float32), frames[j][0], float(t))
        names.append(frames[j][0])
    got = svi.similar_videos("b.mp4", 5)
    stored = np.stack(svi.embeddings)
    labels, keys = _dense(names)
    b = keys.index("b.mp4")
    want = _expected(stored, stored[labels == b], labels, np.arange(len(names)), 5, set(range(3)) - {b})
    assert [r["video_name"] for r in got] == [keys[g] for g, _, _ in want] and got[0]["video_name"] == "a.mp4"
    assert [r["score"] for r in got] == [float(np.float32(1.0) - d) for _, d, _ in want]
    assert [r["video_name"] for r in svi.similar_videos("a.mp4", 1)] == ["b.mp4"]
    with pytest.raises(KeyError):
        svi.similar_videos("nope.mp4")


@pytest.mark.timeout(900)
def test_set_search_one_million_rows_against_the_oracle(gpu_lib):
    """1M x 512 unit rows in 2,000 contiguous videos of 500 frames, a clip of 64 frames, k = 10, both modes."""
    rng = np.random.default_rng(1_000_064)
    n, dim, m, k = 1_000_000, 512, 64, 10
    vecs = rng.standard_normal((n, dim), dtype=np.float32)
    qs = rng.standard_normal((m, dim), dtype=np.float32)
    src = vecs[777 * 500 + 100:777 * 500 + 100 + 48]
    qs[:48] = src / np.linalg.norm(src, axis=1, keepdims=True) + np.float32(0.6 / np.sqrt(dim)) * rng.standard_normal((48, dim), dtype=np.float32)
    idx = _mk(vecs, range(n))
    del vecs
    group_of = lambda nid: nid // 500                             # noqa: E731
    want = _expected(idx._export(), _unit(qs), np.arange(n) // 500, np.arange(n), k)
    assert want[0][0] == 777
    for mode in (1, 2):
        idx.search_mode = mode
        res = idx.search_set(list(qs), k, group_of=group_of, matches=True)
        st = idx.last_search_stats()
        assert [r["group"] for r in res] == [g for g, _, _ in want], f"mode {mode} {st}"
        assert [r["distance"] for r in res] == [d for _, d, _ in want], f"mode {mode} {st}"
        assert [r["matches"] for r in res] == [rr for _, _, rr in want], f"mode {mode} {st}"
        assert st["verified"] + st["exact_fallback"] == 1 and (mode == 2 or st["exact_fallback"] == 1)
    idx.close()
