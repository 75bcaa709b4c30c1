"""Distinct-moment search (vq_index_search_distinct / HNSWIndex.search_distinct / SimpleVideoIndex.search_moments): the k best
rows such that two results of one group lie at least min_gap positions apart.  The expected answer is the definition restated in
numpy (`greedy_distinct` below) over the C oracle's exact distances in (distance, tie) order; ids, positions and float32
distances must match bit for bit in every mode, on the prefix path and on the exact redo.

The rows are video-like (consecutive frames of a video are near-duplicates), so that the plain top-k holds neighbours and the
gap bites: every case asserts on the oracle's own lists that its answer differs from the plain top-k."""
import ctypes
import math
from ctypes import POINTER, byref, c_int32, c_int64, c_void_p

import numpy as np
import pytest

from oracle import knn_oracle
from index_host_fakes import tie_ranks as _tie_ranks, unit as _unit

GPU = pytest.mark.gpu
LENGTHS = [1, 7, 63, 64, 65, 300, 3000]          # singletons, both sides of a wave, multi-pass groups
BIG_GAP = 2 ** 40
GAPS = [0, 1, 3, 50, BIG_GAP]
# k = 6 is there for the forced depth of 16: at gap 3 a prefix of 16 near-consecutive frames keeps 5 to 7 rows, so only k = 6
# leaves some queries of a batch to the redo and proves the others (k = 10 files all of them, k = 1 none)
KS = [1, 6, 10, 100]
NQS = (1, 5, 33)


# ---- the definition, restated ----
def greedy_distinct(order, groups, positions, k, min_gap, depth=None):
    """Walk `order` (rows in the plain search's order; at most `depth` of them); keep a row unless a kept row of the same
    group lies at |position difference| < min_gap; the first k kept rows."""
    kept, by_group = [], {}
    for r in (order if depth is None else order[:depth]):
        p = positions[r]
        seen = by_group.setdefault(groups[r], [])
        if any(abs(p - o) < min_gap for o in seen):
            continue
        seen.append(p)
        kept.append(r)
        if len(kept) == k:
            break
    return kept


# ---- video-like rows ----
def video_lengths(n, lengths=LENGTHS):
    out, i = [], 0
    while sum(out) < n:
        out.append(min(lengths[i % len(lengths)], n - sum(out)))
        i += 1
    return out


def video_rows(n, dim, seed, lengths=LENGTHS):
    """Per video a random unit v0, v[i+1] = normalize(v[i] + 0.2 g / sqrt(dim)).  -> rows [n][dim], video [n], frame [n]"""
    rng = np.random.default_rng(seed)
    rows = np.empty((n, dim), dtype=np.float32)
    video, frame = [], []
    r = 0
    for v, ln in enumerate(video_lengths(n, lengths)):
        x = rng.standard_normal(dim)
        x /= np.linalg.norm(x)
        steps = rng.standard_normal((ln, dim)) * (0.2 / math.sqrt(dim))
        for i in range(ln):
            rows[r] = x
            video.append(v)
            frame.append(i)
            r += 1
            x = x + steps[i]
            x /= np.linalg.norm(x)
    return rows, video, frame


def video_queries(rows, nq, seed):
    """A stored row plus Gaussian noise of norm ~ 1.2, normalised."""
    rng = np.random.default_rng([seed, 1])
    src = rng.integers(0, len(rows), nq)
    noise = rng.standard_normal((nq, rows.shape[1])) * (1.2 / math.sqrt(rows.shape[1]))
    q = rows[src] + noise
    return (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)


def _i32(a):
    return a.ctypes.data_as(POINTER(c_int32))


class Data:
    """One index and everything the oracle needs about it, computed once: exported rows, per-query distances and the
    exhaustive (distance, tie) order.  Never modified by a test."""

    def __init__(self, vecs, ids, groups, positions, qs, group_of=None, position_of=None):
        from video_quierer_amd.indexes.hnsw import OptimizedHNSWIndex
        self.ids, self.groups, self.positions, self.qs = ids, list(groups), [int(p) for p in positions], qs
        self.group_of, self.position_of = group_of, position_of
        self.idx = OptimizedHNSWIndex(dimension=vecs.shape[1])
        self.idx.add_batch(vecs, ids)
        self.n = len(ids)
        self.refresh()

    def refresh(self):
        stored = self.idx._export()
        tie = _tie_ranks(self.ids)
        self.dist = [knn_oracle.distances(stored, q) for q in _unit(self.qs)]
        self.order = [np.lexsort((tie, d)).tolist() for d in self.dist]
        self._want = {}

    def want(self, k, gap, depth=None):
        key = (k, gap, depth)
        if key not in self._want:
            self._want[key] = [greedy_distinct(o, self.groups, self.positions, k, gap, depth) for o in self.order]
        return self._want[key]

    def run(self, nq, k, gap, mode):
        self.idx.search_mode = mode
        kw = dict(group_of=self.group_of, position_of=self.position_of)
        if nq == 1:
            return [self.idx.search_distinct(self.qs[0], k, gap, **kw)]
        return self.idx.search_distinct_batch(list(self.qs[:nq]), k, gap, **kw)

    def check(self, nq, k, gap, mode, depth=None):
        res = self.run(nq, k, gap, mode)
        st = self.idx.last_search_stats()
        want = self.want(k, gap)
        for j in range(nq):
            rr, ww = res[j], want[j]
            tag = f"query {j} (nq {nq}, k {k}, gap {gap}, mode {mode}, depth {depth}, stats {st})"
            assert [r["id"] for r in rr] == [self.ids[r] for r in ww], f"{tag}: ids differ"
            assert [r["position"] for r in rr] == [self.positions[r] for r in ww], f"{tag}: positions differ"
            assert [r["group"] for r in rr] == [self.groups[r] for r in ww], f"{tag}: groups differ"
            got = np.array([r["distance"] for r in rr], dtype=np.float32)
            assert np.array_equal(got.view(np.uint32), self.dist[j][ww].view(np.uint32)), f"{tag}: distances differ"
            assert all(type(r["distance"]) is np.float32 and r["score"] == np.float32(1.0) - r["distance"] for r in rr)
        return st

    def assert_gap_bites(self, k, gap):
        """On the oracle's lists: the answer differs from the plain top-k for at least half of the queries."""
        want = self.want(k, gap)
        differ = sum(ww != o[:k] for ww, o in zip(want, self.order))
        assert 2 * differ >= len(self.order), f"the gap bites for {differ} of {len(self.order)} queries only (k {k}, gap {gap})"


SHAPES = {"m2_20000x512": (20_000, 512, 2), "m1_1500x256": (1_500, 256, 1), "m1_5000x768": (5_000, 768, 1)}
_CACHE = {}


def dataset(name, kind):
    key = (name, kind)
    if key not in _CACHE:
        n, dim, _ = SHAPES[name]
        vecs, video, frame = video_rows(n, dim, seed=n + dim)
        qs = video_queries(vecs, 33, seed=n + dim)
        if kind == "str":                       # "v0_10" sorts before "v0_2": tie rank != row
            ids = [f"v{v}_{i}" for v, i in zip(video, frame)]
            _CACHE[key] = Data(vecs, ids, [f"v{v}" for v in video], frame, qs)
        else:
            ids = list(range(n))
            _CACHE[key] = Data(vecs, ids, video, frame, qs, group_of=video.__getitem__, position_of=frame.__getitem__)
    return _CACHE[key]


@pytest.fixture(scope="module", autouse=True)
def _close_indexes():
    yield
    for d in _CACHE.values():
        d.idx.close()
    _CACHE.clear()


# ---- 1. the matrix ----
@GPU
@pytest.mark.parametrize("gap", GAPS)
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("kind", ["int", "str"])
@pytest.mark.parametrize("name", list(SHAPES))
def test_distinct_matches_the_definition(gpu_lib, name, kind, k, gap):
    d = dataset(name, kind)
    mode = SHAPES[name][2]
    if k > 1 and gap > 1:
        d.assert_gap_bites(k, gap)
    for nq in NQS:
        st = d.check(nq, k, gap, mode)
        assert st["verified"] + st["exact_fallback"] == nq
        if gap == 3 and k == 10:                                  # the depth rule covers the usual call: no redo
            assert st["exact_fallback"] == 0, st


# ---- 2. the prefix / redo split under a forced depth ----
def _filed(d, nq, k, gap, depth):
    return sum(len(kept) < k for kept in d.want(k, gap, depth)[:nq])


@GPU
@pytest.mark.parametrize("gap", GAPS)
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("kind", ["int", "str"])
@pytest.mark.parametrize("name", list(SHAPES))
def test_forced_depth_splits_the_queries_between_prefix_and_redo(gpu_lib, monkeypatch, name, kind, k, gap):
    d = dataset(name, kind)
    monkeypatch.setenv("VQ_AMD_DISTINCT_DEPTH", "16")
    for nq in NQS:
        st = d.check(nq, k, gap, SHAPES[name][2], depth=16)
        assert st["exact_fallback"] == _filed(d, nq, k, gap, 16), st
        assert st["verified"] == nq - st["exact_fallback"]


@GPU
@pytest.mark.parametrize("name", list(SHAPES))
def test_both_paths_answer_within_one_call(gpu_lib, monkeypatch, name):
    """Some (k, gap) leaves the forced prefix short for some of the 33 queries and long enough for others."""
    d = dataset(name, "str")
    mixed = [(k, gap) for k in KS for gap in GAPS if 0 < _filed(d, 33, k, gap, 16) < 33]
    assert mixed, "no case splits the batch"
    monkeypatch.setenv("VQ_AMD_DISTINCT_DEPTH", "16")
    k, gap = mixed[0]
    st = d.check(33, k, gap, SHAPES[name][2], depth=16)
    assert 0 < st["exact_fallback"] == _filed(d, 33, k, gap, 16) < 33


# ---- 3. degenerate equalities through the C ABI ----
def _c_distinct(gpu_lib, h, uq, k, mode, gap):
    nq = len(uq)
    ids = np.empty((nq, k), np.int32); dist = np.empty((nq, k), np.float32)
    rc = gpu_lib.load().vq_index_search_distinct(h, gpu_lib.fptr(uq), nq, k, mode, gap, _i32(ids), gpu_lib.fptr(dist))
    return rc, ids, dist


@GPU
@pytest.mark.parametrize("name,kind", [("m2_20000x512", "str"), ("m1_1500x256", "int"), ("m1_5000x768", "str")])
def test_gap_zero_is_the_plain_search_and_a_huge_gap_the_grouped_search(gpu_lib, name, kind):
    d = dataset(name, kind)
    mode = SHAPES[name][2]
    d.check(5, 10, 3, mode)                                       # ranks, labels and positions are on the device
    lib, h, uq = gpu_lib.load(), d.idx._h, _unit(d.qs)
    for k in (10, 100):
        rc, ids, dist = _c_distinct(gpu_lib, h, uq, k, mode, 0)
        gpu_lib.check(rc)
        pi = np.empty_like(ids); pd = np.empty_like(dist)
        gpu_lib.check(lib.vq_index_search(h, gpu_lib.fptr(uq), len(uq), k, mode, _i32(pi), gpu_lib.fptr(pd)))
        assert np.array_equal(ids, pi) and np.array_equal(dist.view(np.uint32), pd.view(np.uint32))
        rc, ids, dist = _c_distinct(gpu_lib, h, uq, k, mode, BIG_GAP)
        gpu_lib.check(rc)
        kg = min(k, len(set(d.groups)))                           # (the wrapper never asks the grouped search for more)
        gg = np.empty((len(uq), kg), np.int32); gr = np.empty_like(gg); gd = np.empty((len(uq), kg), np.float32)
        gpu_lib.check(lib.vq_index_search_grouped(h, gpu_lib.fptr(uq), len(uq), kg, mode, _i32(gg), _i32(gr), gpu_lib.fptr(gd)))
        assert np.array_equal(ids[:, :kg], gr) and np.array_equal(dist[:, :kg].view(np.uint32), gd.view(np.uint32))
        assert (ids[:, :kg] >= 0).all() and (ids[:, kg:] == -1).all() and np.isposinf(dist[:, kg:]).all()


# ---- 4. planted ties ----
@GPU
@pytest.mark.parametrize("mode", [1, 2])
def test_planted_ties_follow_the_tie_ranks(gpu_lib, mode):
    """40 copies of one row: 20 consecutive frames of one video (they conflict at gap 3) and every fifth frame of another
    (they conflict at gap 50 only).  Their distances are equal, so order and suppression follow the string ids' ranks."""
    vecs, video, frame = video_rows(3_000, 256, seed=44, lengths=[300])
    ids = [f"v{v}_{i}" for v, i in zip(video, frame)]
    planted = [300 * 3 + i for i in range(10, 30)] + [300 * 6 + 5 * i for i in range(20)]
    vecs[planted] = vecs[planted[0]]
    rng = np.random.default_rng(45)
    qs = np.stack([vecs[planted[0]] + np.float32(0.02) * rng.standard_normal(256).astype(np.float32) for _ in range(3)])
    d = Data(vecs, ids, [f"v{v}" for v in video], frame, qs)
    try:
        assert len({d.dist[0][r].tobytes() for r in planted}) == 1
        for gap in (1, 3, 50):
            d.check(3, 30, gap, mode)
            first = d.want(30, gap)[0]
            assert first[0] == min(planted, key=ids.__getitem__)      # "v3_10" is the smallest id among the copies
        assert d.want(30, 3)[0] != d.want(30, 50)[0] != d.want(30, 1)[0]
    finally:
        d.idx.close()


# ---- 5. positions of the caller's choosing ----
@GPU
@pytest.mark.parametrize("mode", [1, 2])
def test_positions_shuffled_repeated_negative_and_near_the_int32_ends(gpu_lib, mode):
    n, dim = 1_500, 256
    vecs, video, frame = video_rows(n, dim, seed=51)
    qs = video_queries(vecs, 9, seed=51)
    rng = np.random.default_rng(52)
    shuffled = list(frame)                                         # not monotone in row order: frames permuted in blocks of 8
    for v in set(video):
        rows = [r for r in range(n) if video[r] == v]
        for b0 in range(0, len(rows), 8):
            blk = rows[b0:b0 + 8]
            for r, p in zip(blk, rng.permutation([frame[r] for r in blk]).tolist()):
                shuffled[r] = p
    assert shuffled != frame
    ends = [(-2 ** 31 + f) if f % 2 else (2 ** 31 - 1 - f) for f in frame]
    d = Data(vecs, list(range(n)), video, frame, qs, group_of=video.__getitem__)
    try:
        for positions, gaps in ((shuffled, (3, 50)), ([f // 4 for f in frame], (1, 2)), ([f - 1000 for f in frame], (3,)),
                                (ends, (50, 2 ** 31, 2 ** 32 + 5))):
            d.positions, d.position_of, d._want = positions, positions.__getitem__, {}
            for gap in gaps:
                d.check(9, 10, gap, mode)
                d.assert_gap_bites(10, gap)
        # without 64-bit differences, rows at opposite ends of the int32 range would look adjacent
        assert d.want(10, 2 ** 31) != d.want(10, 2 ** 32 + 5)
    finally:
        d.idx.close()


# ---- 6. one group holding every row ----
@GPU
@pytest.mark.parametrize("mode", [1, 2])
def test_one_group_of_5000_rows_is_walked_to_k_100(gpu_lib, mode):
    vecs, video, frame = video_rows(5_000, 256, seed=61, lengths=[5_000])
    qs = video_queries(vecs, 3, seed=61)
    d = Data(vecs, [f"only_{i}" for i in frame], ["only"] * 5_000, frame, qs)
    try:
        st = d.check(3, 100, 50, mode)
        d.assert_gap_bites(100, 50)
        assert st["exact_fallback"] == 3                          # 100 rows 50 apart do not fit any prefix
        assert all(50 <= len(w) <= 100 for w in d.want(100, 50))      # (greedy packs 5,000 positions less tightly than every 50th)
        st = d.check(3, 100, 20, mode)
        assert st["exact_fallback"] == 3 and all(len(w) == 100 for w in d.want(100, 20))
        # 8. k above the rows that can be kept: one row, then -1 / +inf
        rc, ids, dist = _c_distinct(gpu_lib, d.idx._h, _unit(qs), 5, mode, BIG_GAP)
        gpu_lib.check(rc)
        assert [int(r) for r in ids[:, 0]] == [w[0] for w in d.want(5, BIG_GAP)]
        assert (ids[:, 1:] == -1).all() and np.isposinf(dist[:, 1:]).all() and np.isfinite(dist[:, 0]).all()
    finally:
        d.idx.close()


# ---- 7. singletons ----
@GPU
@pytest.mark.parametrize("mode", [1, 2])
def test_singleton_groups_give_the_plain_search(gpu_lib, mode):
    vecs, _, _ = video_rows(1_500, 256, seed=71)
    qs = video_queries(vecs, 5, seed=71)
    n = len(vecs)
    d = Data(vecs, list(range(n)), list(range(n)), list(range(n)), qs)       # int ids: their own group, their own position
    try:
        d.idx.search_mode = mode
        plain = d.idx.search_batch(list(qs), 10)
        for gap in (3, BIG_GAP):
            d.check(5, 10, gap, mode)
            res = d.run(5, 10, gap, mode)
            assert [[r["id"] for r in rr] for rr in res] == [[r["id"] for r in rr] for rr in plain]
            assert [[r["distance"] for r in rr] for rr in res] == [[r["distance"] for r in rr] for rr in plain]
    finally:
        d.idx.close()


# ---- 9. lifetime of the positions ----
@GPU
def test_positions_lifetime(gpu_lib):
    lib = gpu_lib.load()
    n, dim = 1_500, 256
    vecs, video, frame = video_rows(n + 200, dim, seed=91)
    video, frame = list(video), list(frame)
    qs = video_queries(vecs, 5, seed=91)
    ids = list(range(n + 200))
    d = Data(vecs[:n], ids[:n], video[:n], frame[:n], qs, group_of=video.__getitem__, position_of=frame.__getitem__)
    try:
        h, uq = d.idx._h, _unit(qs)
        d.check(5, 10, 3, 1)
        d.idx.add_batch(vecs[n:], ids[n:])                        # stale after an add: refused
        rc, _, _ = _c_distinct(gpu_lib, h, uq, 10, 1, 3)
        assert rc < 0
        dense = {}
        lab = np.array([dense.setdefault(v, len(dense)) for v in video], dtype=np.int32)
        gpu_lib.check(lib.vq_index_set_groups(h, _i32(lab), n + 200, len(dense)))
        rc, _, _ = _c_distinct(gpu_lib, h, uq, 10, 1, 3)
        assert rc < 0 and b"positions" in lib.vq_last_error()
        pos = np.array(frame, dtype=np.int32)
        gpu_lib.check(lib.vq_index_set_positions(h, _i32(pos), n + 200))
        rc, rows, _ = _c_distinct(gpu_lib, h, uq, 10, 1, 3)
        gpu_lib.check(rc)
        # the wrapper uploads by itself after the add
        d.ids, d.groups, d.positions, d.n = ids, video, frame, n + 200
        d.refresh()
        assert [[int(r) for r in rr] for rr in rows] == d.want(10, 3)
        d.check(5, 10, 3, 1)
        # update_rows (re-adding an id) keeps them
        d.idx.add_batch(vecs[5:6] * np.float32(-1.0), [700])
        rc, _, _ = _c_distinct(gpu_lib, h, uq, 10, 1, 3)
        gpu_lib.check(rc)
        d.refresh()
        d.check(5, 10, 3, 1)
        # remove_rows drops them; the wrapper uploads again and answers on the compacted index
        gone = list(range(40, 90)) + [300, 301, 1400]
        d.idx.remove_batch(gone)
        rc, _, _ = _c_distinct(gpu_lib, h, uq, 10, 1, 3)
        assert rc < 0 and b"positions" in lib.vq_last_error()
        keep = [r for r in range(n + 200) if r not in set(gone)]
        d.ids = [ids[r] for r in keep]; d.groups = [video[r] for r in keep]; d.positions = [frame[r] for r in keep]
        d.refresh()
        for mode in (1, 2):
            d.check(5, 10, 3, mode)
        gpu_lib.check(lib.vq_index_clear(h))                      # clear drops them
        gpu_lib.check(lib.vq_index_add(h, gpu_lib.fptr(np.ascontiguousarray(vecs[:n])), n, 0))
        gpu_lib.check(lib.vq_index_set_groups(h, _i32(np.ascontiguousarray(lab[:n])), n, int(lab[:n].max()) + 1))
        rc, _, _ = _c_distinct(gpu_lib, h, uq, 10, 1, 3)
        assert rc < 0 and b"positions" in lib.vq_last_error()
    finally:
        d.idx.close()


# ---- 10. the device form ----
@GPU
def test_device_form_matches_the_host_form_twice_without_a_wait(gpu_lib):
    d = dataset("m2_20000x512", "str")
    d.check(5, 10, 3, 2)
    lib, h, uq = gpu_lib.load(), d.idx._h, _unit(d.qs)
    nq = len(uq)
    calls = [(10, 3, 2), (100, 50, 2)]                            # (k, gap, mode): the second one needs the redo
    want = []
    for k, gap, mode in calls:
        rc, ids, dist = _c_distinct(gpu_lib, h, uq, k, mode, gap)
        gpu_lib.check(rc)
        want.append((ids, dist))
    hip = ctypes.CDLL("libamdhip64.so")
    ptrs = []

    def dev(nbytes):
        p = c_void_p()
        assert hip.hipMalloc(byref(p), ctypes.c_size_t(nbytes)) == 0
        ptrs.append(p)
        return p
    dq = dev(uq.nbytes)
    assert hip.hipMemcpy(dq, uq.ctypes.data_as(c_void_p), ctypes.c_size_t(uq.nbytes), 1) == 0
    outs = [(dev(nq * k * 4), dev(nq * k * 4)) for k, _, _ in calls]
    for (k, gap, mode), (di, dd) in zip(calls, outs):             # back to back on the index's stream
        gpu_lib.check(lib.vq_index_search_distinct_device(h, dq, nq, k, mode, c_int64(gap), di, dd))
    gpu_lib.check(lib.vq_index_synchronize(h))
    for (k, gap, mode), (di, dd), (ids, dist) in zip(calls, outs, want):
        gi = np.empty_like(ids); gd = np.empty_like(dist)
        assert hip.hipMemcpy(gi.ctypes.data_as(c_void_p), di, ctypes.c_size_t(gi.nbytes), 2) == 0
        assert hip.hipMemcpy(gd.ctypes.data_as(c_void_p), dd, ctypes.c_size_t(gd.nbytes), 2) == 0
        assert np.array_equal(gi, ids) and np.array_equal(gd.view(np.uint32), dist.view(np.uint32)), (k, gap)
        assert [[int(r) for r in rr if r >= 0] for rr in gi] == d.want(k, gap)
    for p in ptrs:
        hip.hipFree(p)


# ---- 11. SimpleVideoIndex.search_moments ----
@GPU
def test_search_moments_on_fractional_timestamps(gpu_lib):
    from video_quierer_amd.overhaul_index import SimpleVideoIndex
    vecs, video, frame = video_rows(600, 512, seed=111, lengths=[150])
    rng = np.random.default_rng(112)
    names = [f"clip{v}.mp4" for v in video]
    stamps = [round(f * 0.4 + float(rng.uniform(0, 0.3)), 3) for f in frame]      # ~2.5 fps, jittered
    sv = SimpleVideoIndex()
    for e, nm, ts in zip(vecs, names, stamps):
        sv.add_frame(e, nm, ts)
    qs = video_queries(vecs, 6, seed=111) * np.float32(3.0)       # search_moments normalises the query itself
    positions = [int(round(ts * 1000)) for ts in stamps]
    tie = -np.arange(600)                                         # search's tie rule: the larger frame id first
    for q in qs:
        qn = (q / (np.linalg.norm(q) + 1e-10)).astype(np.float32)
        dist = knn_oracle.distances(np.stack(sv.embeddings), qn)
        order = np.lexsort((tie, dist)).tolist()
        assert [r["frame_id"] for r in sv.search(q, 5)] == order[:5]
        for gap_s in (0.0, 0.75, 2.0, 1000.0):
            want = greedy_distinct(order, names, positions, 5, math.ceil(gap_s * 1000))
            got = sv.search_moments(q, 5, gap_s)
            assert [r["frame_id"] for r in got] == want, gap_s
            assert [r["video_name"] for r in got] == [names[r] for r in want]
            assert [r["timestamp"] for r in got] == [stamps[r] for r in want]
            assert [r["score"] for r in got] == [float(np.float32(1.0) - dist[r]) for r in want]
        assert greedy_distinct(order, names, positions, 5, 2000) != order[:5]
        assert len(sv.search_moments(q, 5, 1000.0)) == 4          # one moment per video
    sv.add_frame(vecs[0], "late.mp4", 1.0)                        # `search` keeps working once the index has grown
    assert len(sv.search(qs[0], 5)) == 5 and len(sv.search_moments(qs[0], 5, 2.0)) == 5
