"""Diverse search (vq_index_search_diverse / HNSWIndex.search_diverse / SimpleVideoIndex.search_diverse): the k best rows no two
of which lie closer than min_dist to each other.  The expected answer is the definition restated in numpy (`greedy_diverse`
below) over the C oracle's distances: the queries' exhaustive (distance, tie) lists, and the row-to-row distances
`distances(stored, stored[s])` of every kept row s (cached).  Ids and float32 distances must match bit for bit in every mode, on
the prefix path and on the redo.

The rows are video-like (consecutive frames are near-duplicates) with a planted intro (20 frames of one long video copied, with
a little noise, over the first rows of 12 other videos) and one bit-exact copy of a row; the first 8 queries aim at the intro.
Conditions that keep a case from passing vacuously are asserted on the oracle's own lists."""
import ctypes
import math
from ctypes import POINTER, byref, c_float, c_int32, c_void_p

import numpy as np
import pytest

from oracle import knn_oracle
from index_host_fakes import tie_ranks as _tie_ranks, unit as _unit
from test_distinct_search import video_queries, video_rows

GPU = pytest.mark.gpu
MIN_DISTS = [0.0, 1e-6, 0.02, 0.05, 0.3, 3.0]
KS = [1, 6, 10]
NQS = (1, 5, 33)
LENGTHS = [100, 150, 300]                        # every video outlasts a forced prefix of 64 entries
INTRO_FRAMES, INTRO_COPIES, INTRO_QUERIES = 20, 12, 8


# ---- the definition, restated ----
def greedy_diverse(order, pair_dist, k, min_dist, depth=None):
    """Walk `order` (rows in the plain search's order; at most `depth` of them); keep a row r unless min_dist > 0 and an
    already kept row s has d(r, s) < min_dist (float32, strict); the first k kept rows.  pair_dist(s) -> float32 [n], the
    distances of every row to row s."""
    min_dist = np.float32(min_dist)
    kept = []
    for r in (order if depth is None else order[:depth]):
        if min_dist > 0 and any(pair_dist(s)[r] < min_dist for s in kept):
            continue
        kept.append(r)
        if len(kept) == k:
            break
    return kept


def _greedy_fast(order, pair_dist, k, min_dist, depth=None):
    """greedy_diverse with the test "is r suppressed by a kept row" done for all rows at once when a row is kept (the same
    answer: d is symmetric bit for bit, and a row is only ever asked about after the rows kept before it)."""
    min_dist = np.float32(min_dist)
    order = np.asarray(order if depth is None else order[:depth])
    dead = np.zeros(int(order.max()) + 1 if len(order) else 0, dtype=bool)
    kept, pos = [], 0
    while len(kept) < k and pos < len(order):
        alive = np.flatnonzero(~dead[order[pos:]])
        if len(alive) == 0:
            break
        pos += int(alive[0])
        s = int(order[pos])
        kept.append(s)
        pos += 1
        if min_dist > 0 and len(kept) < k:
            dead[: len(dead)] |= pair_dist(s)[: len(dead)] < min_dist
    return kept


def plant(vecs, video, frame, seed):
    """The intro and the bit-exact copy, in place.  -> the intro's source rows"""
    rng = np.random.default_rng([seed, 2])
    n, dim = vecs.shape
    video = np.asarray(video); frame = np.asarray(frame)
    lengths = np.bincount(video)
    src_video = int(np.argmax(lengths >= 300))                    # the first long video
    src = np.flatnonzero(video == src_video)[40:40 + INTRO_FRAMES]
    others = [v for v in range(len(lengths)) if v != src_video and lengths[v] >= INTRO_FRAMES][:INTRO_COPIES]
    assert len(others) == INTRO_COPIES
    for v in others:
        first = np.flatnonzero(video == v)[:INTRO_FRAMES]
        vecs[first] = vecs[src] + (rng.standard_normal((INTRO_FRAMES, dim)) * (0.02 / math.sqrt(dim))).astype(np.float32)
    vecs[n - 5] = vecs[n // 2]                                    # one bit-exact copy
    return src


def _i32(a):
    return a.ctypes.data_as(POINTER(c_int32))


class Data:
    """One index and everything the oracle needs about it, computed once: exported rows, per-query distances, the exhaustive
    (distance, tie) order, and the kept rows' row-to-row distances.  Never modified by a test (but `refresh`ed by the one
    that changes the index, which owns its Data)."""

    def __init__(self, n, dim, seed, kind="int", nq=33):
        from video_quierer_amd.indexes.hnsw import OptimizedHNSWIndex
        vecs, video, frame = video_rows(n, dim, seed=seed, lengths=LENGTHS)
        src = plant(vecs, video, frame, seed)
        qs = video_queries(vecs, nq, seed=seed)
        rng = np.random.default_rng([seed, 3])
        for j in range(min(INTRO_QUERIES, nq)):                   # aimed at the intro
            q = vecs[src[(2 * j) % INTRO_FRAMES]] + rng.standard_normal(dim) * (0.3 / math.sqrt(dim))
            qs[j] = (q / np.linalg.norm(q)).astype(np.float32)
        self.ids = [f"v{v}_{i}" for v, i in zip(video, frame)] if kind == "str" else list(range(n))   # "v0_10" < "v0_2": rank != row
        self.vecs, self.qs, self.n = vecs, qs, n
        self.idx = OptimizedHNSWIndex(dimension=dim)
        self.idx.add_batch(vecs, self.ids)
        self.refresh()

    def refresh(self):
        self.stored = self.idx._export()
        self.n = len(self.ids)
        tie = _tie_ranks(self.ids)
        self.dist = [knn_oracle.distances(self.stored, q) for q in _unit(self.qs)]
        self.order = [np.lexsort((tie, d)) for d in self.dist]
        self._pair, self._want = {}, {}

    def pair_dist(self, s):
        if s not in self._pair:
            self._pair[s] = knn_oracle.distances(self.stored, self.stored[s])
        return self._pair[s]

    def want(self, j, k, min_dist, depth=None):
        """Query j's answer as rows.  (Computed at the largest k asked so far: the answer for k is a prefix of it.)"""
        key = (j, float(np.float32(min_dist)), depth)
        have = self._want.get(key)
        if have is None or (have[0] < k and len(have[1]) == have[0]):    # (a list shorter than its k is the whole answer)
            have = (k, _greedy_fast(self.order[j], self.pair_dist, k, min_dist, depth))
            self._want[key] = have
        return have[1][:k]

    def run(self, nq, k, min_dist, mode):
        self.idx.search_mode = mode
        if nq == 1:
            return [self.idx.search_diverse(self.qs[0], k, min_dist)]
        return self.idx.search_diverse_batch(list(self.qs[:nq]), k, min_dist)

    def check(self, nq, k, min_dist, mode, depth=None):
        res = self.run(nq, k, min_dist, mode)
        st = self.idx.last_search_stats()
        for j in range(nq):
            rr, ww = res[j], self.want(j, k, min_dist)
            tag = f"query {j} (n {self.n}, nq {nq}, k {k}, min_dist {min_dist}, mode {mode}, depth {depth}, stats {st})"
            assert [r["id"] for r in rr] == [self.ids[r] for r in ww], f"{tag}: ids differ"
            got = np.array([r["distance"] for r in rr], dtype=np.float32)
            assert np.array_equal(got.view(np.uint32), self.dist[j][ww].view(np.uint32)), f"{tag}: distances differ"
            assert all(type(r["distance"]) is np.float32 and r["score"] == np.float32(1.0) - r["distance"] for r in rr)
            assert all(set(r) == {"id", "distance", "score"} for r in rr)
        assert st["verified"] + st["exact_fallback"] == nq, st
        return st

    def filed(self, nq, k, min_dist, depth):
        """On the oracle's lists: the queries whose prefix of `depth` entries keeps fewer than k rows."""
        return sum(len(self.want(j, k, min_dist, depth)) < k for j in range(nq))

    def assert_suppression_bites(self, nq, k, min_dist):
        differ = sum(self.want(j, k, min_dist) != self.order[j][:k].tolist() for j in range(nq))
        assert 2 * differ >= nq, f"the answer differs from the plain top-k for {differ} of {nq} queries only (k {k}, min_dist {min_dist})"


# name -> (n, dim, id kind, modes)
SHAPES = {"3000x64": (3_000, 64, "int", (1, 2)), "3000x512": (3_000, 512, "str", (1, 2)), "20000x512": (20_000, 512, "int", (0, 2))}
_CACHE = {}


def dataset(name):
    if name not in _CACHE:
        n, dim, kind, _ = SHAPES[name]
        _CACHE[name] = Data(n, dim, seed=n + dim, kind=kind)
    return _CACHE[name]


@pytest.fixture(scope="module", autouse=True)
def _close_indexes():
    yield
    for d in _CACHE.values():
        d.idx.close()
    _CACHE.clear()


def _plan_depth(gpu_lib, n, nq, k, min_dist, mode):
    depth, producer, pair_bytes = ctypes.c_int64(), ctypes.c_int(), ctypes.c_int64()
    slices, launches = ctypes.c_int(), ctypes.c_int()
    gpu_lib.check(gpu_lib.load().vq_debug_diverse_plan(n, nq, k, c_float(min_dist), mode, byref(depth), byref(producer), byref(pair_bytes),
                                                       byref(slices), byref(launches)))
    return depth.value


# ---- 1. the matrix, at the rule's depth ----
@GPU
@pytest.mark.parametrize("min_dist", MIN_DISTS)
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("name", ["3000x64", "3000x512"])
def test_diverse_matches_the_definition(gpu_lib, monkeypatch, name, k, min_dist):
    monkeypatch.delenv("VQ_AMD_DIVERSE_DEPTH", raising=False)
    d = dataset(name)
    if min_dist >= 0.02 and k >= 6:
        d.assert_suppression_bites(33, k, min_dist)
    for mode in SHAPES[name][3]:
        for nq in NQS:
            st = d.check(nq, k, min_dist, mode)
            depth = _plan_depth(gpu_lib, d.n, nq, k, min_dist, mode)
            assert st["exact_fallback"] == d.filed(nq, k, min_dist, depth), (st, depth)


@GPU
@pytest.mark.parametrize("mode", [0, 2])
def test_diverse_matches_the_definition_at_20000_rows(gpu_lib, monkeypatch, mode):
    monkeypatch.delenv("VQ_AMD_DIVERSE_DEPTH", raising=False)
    d = dataset("20000x512")
    d.assert_suppression_bites(33, 10, 0.05)
    d.check(33, 10, 0.05, mode)
    d.check(1, 6, 0.05, mode)
    for min_dist in MIN_DISTS:                                    # (oracle cost: five queries for the other thresholds)
        for k in KS:
            d.check(5, k, min_dist, mode)


@GPU
def test_k_100(gpu_lib, monkeypatch):
    monkeypatch.delenv("VQ_AMD_DIVERSE_DEPTH", raising=False)
    d = dataset("3000x512")
    for mode in (1, 2):
        d.check(5, 100, 0.05, mode)
    assert all(len(d.want(j, 100, 0.05)) == 100 for j in range(5))


# ---- 2. forced depths: bit-matrix word boundaries, a kept set that crosses 64 prefix entries, both paths in one call ----
@GPU
@pytest.mark.parametrize("depth", [16, 64, 65, 128, 1024])
@pytest.mark.parametrize("name", ["3000x64", "3000x512"])
def test_forced_depths(gpu_lib, monkeypatch, name, depth):
    d = dataset(name)
    monkeypatch.setenv("VQ_AMD_DIVERSE_DEPTH", str(depth))
    for mode in SHAPES[name][3]:
        eff = min(depth, 100) if mode == 2 else depth             # the fp16 producer's k limit caps the override
        for k, min_dist in ((6, 0.02), (10, 0.05), (10, 0.3), (10, 0.0), (10, 3.0)):
            st = d.check(33, k, min_dist, mode, depth=eff)
            assert st["exact_fallback"] == d.filed(33, k, min_dist, eff), (st, eff)
    if depth >= 128:                                              # some query keeps a row beyond prefix entry 64, past suppressed ones
        beyond = 0
        for j in range(33):
            pos = {r: i for i, r in enumerate(d.order[j][:depth].tolist())}
            w = [pos[r] for r in d.want(j, 10, 0.05, depth)]
            beyond += any(p >= 64 for p in w) and len(w) < w[-1] + 1
        assert beyond >= 1


@GPU
def test_both_paths_answer_within_one_call(gpu_lib, monkeypatch):
    d = dataset("3000x512")
    for depth, k, min_dist in ((16, 6, 0.02), (64, 10, 0.05)):
        filed = d.filed(33, k, min_dist, depth)
        assert 0 < filed < 33, (depth, k, min_dist, filed)
        monkeypatch.setenv("VQ_AMD_DIVERSE_DEPTH", str(depth))
        for mode in (1, 2):
            st = d.check(33, k, min_dist, mode, depth=depth)
            assert st["verified"] == 33 - filed >= 1 and st["exact_fallback"] == filed >= 1, st
    assert d.filed(33, 10, 0.3, 64) == 33
    monkeypatch.setenv("VQ_AMD_DIVERSE_DEPTH", "64")
    for mode in (1, 2):
        st = d.check(33, 10, 0.3, mode, depth=64)
        assert st["exact_fallback"] == 33 and st["verified"] == 0, st


@GPU
@pytest.mark.parametrize("name", ["3000x64", "3000x512"])
def test_redo_on_both_sides_of_the_row_form_threshold(gpu_lib, monkeypatch, name):
    """The redo suppresses row by row while at most 4 slots of a slice are filed and by tiles from 5 on: batches of 1, 3, 4, 5 and
    8 queries aimed at the intro, every one of them filed (min_dist 0 under a prefix shorter than k: only the picked row dies)."""
    d = dataset(name)
    monkeypatch.setenv("VQ_AMD_DIVERSE_DEPTH", "16")
    for mode in SHAPES[name][3]:
        for nq in (1, 3, 4, 5, 8):
            for k, min_dist in ((10, 0.3), (6, 0.05), (20, 0.0)):
                assert d.filed(nq, k, min_dist, 16) == nq
                st = d.check(nq, k, min_dist, mode, depth=16)
                assert st["exact_fallback"] == nq and st["verified"] == 0, st


# ---- 3. consequences of the definition, through the C ABI ----
def _c_diverse(gpu_lib, h, uq, k, mode, min_dist):
    nq = len(uq)
    ids = np.empty((nq, k), np.int32); dist = np.empty((nq, k), np.float32)
    rc = gpu_lib.load().vq_index_search_diverse(h, gpu_lib.fptr(uq), nq, k, mode, c_float(min_dist), _i32(ids), gpu_lib.fptr(dist))
    return rc, ids, dist


@GPU
@pytest.mark.parametrize("name", list(SHAPES))
def test_consequences(gpu_lib, monkeypatch, name):
    monkeypatch.delenv("VQ_AMD_DIVERSE_DEPTH", raising=False)
    d = dataset(name)
    lib, h, uq = gpu_lib.load(), d.idx._h, _unit(d.qs)
    d.check(5, 6, 0.05, SHAPES[name][3][0])                       # the id ranks are on the device
    for mode in SHAPES[name][3]:
        for k in (10, 100):                                       # min_dist 0 is the plain search, bit for bit (a bit-exact copy is in the index)
            rc, ids, dist = _c_diverse(gpu_lib, h, uq, k, mode, 0.0)
            gpu_lib.check(rc)
            pi = np.empty_like(ids); pd = np.empty_like(dist)
            gpu_lib.check(lib.vq_index_search(h, gpu_lib.fptr(uq), len(uq), k, mode, _i32(pi), gpu_lib.fptr(pd)))
            assert np.array_equal(ids, pi) and np.array_equal(dist.view(np.uint32), pd.view(np.uint32))
        rc, ids, dist = _c_diverse(gpu_lib, h, uq, 10, mode, 3.0)  # above every pair distance: one row
        gpu_lib.check(rc)
        assert np.array_equal(ids[:, 0], [o[0] for o in d.order]) and (ids[:, 1:] == -1).all() and np.isposinf(dist[:, 1:]).all()
        assert np.array_equal(dist[:, 0].view(np.uint32), np.array([dd[o[0]] for dd, o in zip(d.dist, d.order)]).view(np.uint32))
        rc, i10, d10 = _c_diverse(gpu_lib, h, uq, 10, mode, 0.05)  # the answer for k is a prefix of the answer for k' > k
        gpu_lib.check(rc)
        for k in (1, 6):
            rc, ik, dk = _c_diverse(gpu_lib, h, uq, k, mode, 0.05)
            gpu_lib.check(rc)
            assert np.array_equal(ik, i10[:, :k]) and np.array_equal(dk.view(np.uint32), d10[:, :k].view(np.uint32))
        rc, again, dagain = _c_diverse(gpu_lib, h, uq, 10, mode, 0.05)      # a second call repeats the first
        gpu_lib.check(rc)
        assert np.array_equal(again, i10) and np.array_equal(dagain.view(np.uint32), d10.view(np.uint32))


@GPU
def test_the_bit_exact_copy_takes_one_slot_only_above_zero(gpu_lib, monkeypatch):
    monkeypatch.delenv("VQ_AMD_DIVERSE_DEPTH", raising=False)
    d = dataset("3000x64")
    a, b = d.n // 2, d.n - 5
    assert np.array_equal(d.stored[a], d.stored[b])
    uq = d.stored[a:a + 1].copy()
    for mode in (1, 2):
        rc, ids, _ = _c_diverse(gpu_lib, d.idx._h, uq, 4, mode, 0.0)
        gpu_lib.check(rc)
        assert ids[0, :2].tolist() == [a, b]
        rc, ids, _ = _c_diverse(gpu_lib, d.idx._h, uq, 4, mode, 1e-6)
        gpu_lib.check(rc)
        assert ids[0, 0] == a and b not in ids[0].tolist()


@GPU
def test_k_above_the_rows_that_can_be_kept_leaves_empty_slots(gpu_lib, monkeypatch):
    """60 rows of one slow video: at min_dist 0.3 a handful can be kept, the other slots are empty (the redo finds no live row).
    dim 48 is no multiple of 32: the row form's other chain."""
    from video_quierer_amd.indexes.hnsw import OptimizedHNSWIndex
    vecs, _, _ = video_rows(60, 48, seed=5, lengths=[60])
    qs = video_queries(vecs, 3, seed=5)
    idx = OptimizedHNSWIndex(dimension=48)
    try:
        idx.add_batch(vecs, list(range(60)))
        stored = idx._export()
        pair = {}
        for depth in (None, 16):
            if depth:
                monkeypatch.setenv("VQ_AMD_DIVERSE_DEPTH", str(depth))
            rc, ids, dist = _c_diverse(gpu_lib, idx._h, _unit(qs), 40, 1, 0.3)
            gpu_lib.check(rc)
            for j, q in enumerate(_unit(qs)):
                dq = knn_oracle.distances(stored, q)
                order = np.lexsort((np.arange(60), dq)).tolist()
                want = greedy_diverse(order, lambda s: pair.setdefault(s, knn_oracle.distances(stored, stored[s])), 40, 0.3)
                assert 1 <= len(want) < 40
                assert ids[j, :len(want)].tolist() == want and (ids[j, len(want):] == -1).all() and np.isposinf(dist[j, len(want):]).all()
                assert np.array_equal(dist[j, :len(want)].view(np.uint32), dq[want].view(np.uint32))
        assert idx.search_diverse(qs[0], 100, 0.3) == idx.search_diverse(qs[0], 60, 0.3)      # the wrapper caps k at the rows
    finally:
        idx.close()


# ---- 4. the index changes under the search ----
@GPU
def test_same_answers_after_remove_and_add(gpu_lib, monkeypatch):
    monkeypatch.delenv("VQ_AMD_DIVERSE_DEPTH", raising=False)
    d = Data(3_000, 64, seed=77, kind="str", nq=5)
    try:
        d.check(5, 10, 0.05, 1)
        gone = list(range(40, 90)) + [300, 301, 1400, int(d.order[0][0])]
        d.idx.remove_batch([d.ids[r] for r in gone])
        keep = [r for r in range(d.n) if r not in set(gone)]
        d.ids = [d.ids[r] for r in keep]
        d.refresh()
        for mode in (1, 2):
            d.check(5, 10, 0.05, mode)
        extra, _, _ = video_rows(200, 64, seed=78, lengths=[100])
        new_ids = [f"w{i // 100}_{i % 100}" for i in range(200)]
        d.idx.add_batch(extra, new_ids)
        h, uq = d.idx._h, _unit(d.qs[:5])
        rc, _, _ = _c_diverse(gpu_lib, h, uq, 10, 1, 0.05)        # stale id ranks: refused
        assert rc < 0 and b"id ranks" in gpu_lib.load().vq_last_error()
        d.ids = d.ids + new_ids
        d.refresh()
        for mode in (1, 2):
            d.check(5, 10, 0.05, mode)                            # the wrapper uploads the ranks again
        monkeypatch.setenv("VQ_AMD_DIVERSE_DEPTH", "16")
        d.check(5, 10, 0.05, 1, depth=16)
    finally:
        d.idx.close()


@GPU
def test_empty_index_returns_every_slot_empty(gpu_lib):
    lib = gpu_lib.load()
    h = c_void_p()
    gpu_lib.check(lib.vq_index_create(64, byref(h)))
    try:
        uq = _unit(np.ones((2, 64), np.float32))
        rc, ids, dist = _c_diverse(gpu_lib, h, uq, 5, 1, 0.05)
        gpu_lib.check(rc)
        assert (ids == -1).all() and np.isposinf(dist).all()
    finally:
        lib.vq_index_destroy(h)


# ---- 5. the device form ----
@GPU
def test_device_form_writes_the_same_bits_without_a_wait(gpu_lib, monkeypatch):
    d = dataset("3000x512")
    lib, h, uq = gpu_lib.load(), d.idx._h, _unit(d.qs)
    d.check(5, 6, 0.05, 1)
    monkeypatch.setenv("VQ_AMD_DIVERSE_DEPTH", "64")
    nq = len(uq)
    calls = [(10, 0.05, 1), (10, 0.3, 2), (6, 0.0, 1)]            # (k, min_dist, mode): proven and redone; all redone; the plain search
    want = []
    for k, md, mode in calls:
        rc, ids, dist = _c_diverse(gpu_lib, h, uq, k, mode, md)
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
    for (k, md, mode), (di, dd) in zip(calls, outs):              # back to back on the index's stream
        gpu_lib.check(lib.vq_index_search_diverse_device(h, dq, nq, k, mode, c_float(md), di, dd))
    gpu_lib.check(lib.vq_index_synchronize(h))
    for (k, md, mode), (di, dd), (ids, dist) in zip(calls, outs, want):
        gi = np.empty_like(ids); gd = np.empty_like(dist)
        assert hip.hipMemcpy(gi.ctypes.data_as(c_void_p), di, ctypes.c_size_t(gi.nbytes), 2) == 0
        assert hip.hipMemcpy(gd.ctypes.data_as(c_void_p), dd, ctypes.c_size_t(gd.nbytes), 2) == 0
        assert np.array_equal(gi, ids) and np.array_equal(gd.view(np.uint32), dist.view(np.uint32)), (k, md)
        assert [[int(r) for r in rr if r >= 0] for rr in gi] == [d.want(j, k, md) for j in range(nq)]
    for p in ptrs:
        hip.hipFree(p)


# ---- 6. SimpleVideoIndex.search_diverse ----
@GPU
def test_simple_video_index_search_diverse(gpu_lib, monkeypatch):
    monkeypatch.delenv("VQ_AMD_DIVERSE_DEPTH", raising=False)
    from video_quierer_amd.overhaul_index import SimpleVideoIndex
    vecs, video, frame = video_rows(600, 512, seed=111, lengths=[150])
    vecs[450:470] = vecs[20:40]                                   # a re-upload: bit-exact copies in another video
    sv = SimpleVideoIndex()
    for e, v, f in zip(vecs, video, frame):
        sv.add_frame(e, f"clip{v}.mp4", f * 0.5)
    qs = video_queries(vecs, 4, seed=111) * np.float32(3.0)       # search_diverse normalises the query itself
    qs[0] = vecs[25] * np.float32(2.0)
    stored = np.stack(sv.embeddings)
    tie = -np.arange(600)                                         # search's tie rule: the larger frame id first
    pair = {}
    for q in qs:
        qn = (q / (np.linalg.norm(q) + 1e-10)).astype(np.float32)
        dist = knn_oracle.distances(stored, qn)
        order = np.lexsort((tie, dist)).tolist()
        for sim in (1.0, 0.98, 0.95, 0.7):
            md = np.float32(1) - np.float32(sim)
            want = greedy_diverse(order, lambda s: pair.setdefault(s, knn_oracle.distances(stored, stored[s])), 5, md)
            got = sv.search_diverse(q, 5, sim)
            assert [r["frame_id"] for r in got] == want, sim
            assert [r["score"] for r in got] == [float(np.float32(1.0) - dist[r]) for r in want]
            assert all(set(r) == set(sv.search(q, 1)[0]) for r in got)
        assert [r["frame_id"] for r in sv.search_diverse(q, 5, 1.0)] == [r["frame_id"] for r in sv.search(q, 5)]
    top = [r["frame_id"] for r in sv.search_diverse(qs[0], 5, 0.95)]
    assert top[0] == 455 and 25 not in top                        # the copy with the larger frame id comes first and absorbs the other
    with pytest.raises(ValueError):
        sv.search_diverse(qs[0], 5, 1.5)
    with pytest.raises(ValueError):
        sv.search_diverse(qs[0], 5, float("nan"))
