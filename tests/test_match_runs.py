"""Shared-footage search on the device (vq_index_match_runs / HNSWIndex.shared_runs / SimpleVideoIndex.find_reuse) against the
numpy restatement of the definition (tests/match_ref.py) over the C oracle's distances on vq_index_export's rows: every output
bit for bit, integers as integers, mean_dist as fp32 bits.

One index per dimension of 2,300 rows (past one 2,048-row range of the tile kernel, no multiple of 128 or 256) in twelve
groups; the groups' rows are interleaved by a permutation, two frames share each position, the labels are shuffled, and the id
ranks order a group's rows by frame — where the row numbers do not — so the tie decides the (position, tie) order.  The clip is
300 random directions; the planted videos hold noisy copies of stretches of it (distances 2e-4 .. 0.012), the rest is random
(distances around 1)."""
import ctypes
from ctypes import POINTER, byref, c_float, c_int, c_int32, c_int64, c_void_p

import numpy as np
import pytest

import match_ref
from oracle import knn_oracle

GPU = pytest.mark.gpu
FP16_DIMS = (256, 512, 768)
ODD_DIM = 96                                  # the tile path does not exist: mode 2 is refused, modes 0 / 1 answer
CLIP = 300
CLIP_LENGTHS = (1, 2, 33, 255, 256, 257, 300)
CAP_ENV = "VQ_AMD_MATCH_FILED_CAP"
NAMES = ("group", "hits", "span", "q_first", "row_first", "row_last", "mean_dist")
SLACK = 2.0 ** -19                            # MATCH_SLACK (csrc/knn_match.h)

# name: (length, [(first frame of the video, first clip frame, frames copied)], frames replaced by noise inside the copy)
VIDEOS = {
    "partial":   (300, [(40, 10, 90)], []),           # an exact partial copy at an offset: diagonal 30, s = 10, 90 hits
    "reversed":  (65, "reversed", []),                # clip[10 .. 75) backwards: every diagonal holds one hit, no run of 2
    "strided":   (64, "strided", []),                 # clip[10], clip[12], ..: every second frame, again one hit per diagonal
    "one_gap":   (63, [(0, 20, 63)], [30]),           # one replaced frame: max_miss 0 -> 32 hits, 1 -> 62 over a span of 63
    "two_gaps":  (64, [(0, 20, 64)], [30, 31]),       # two replaced frames: max_miss 0 / 1 -> 32 hits, 2 -> 62 over a span of 64
    "twin_a":    (40, [(0, 100, 40)], []),            # two identical copies in two videos: the label decides
    "twin_b":    (40, [(0, 100, 40)], []),
    "single":    (1, [(0, 5, 1)], []),
    "pair":      (2, [(0, 5, 2)], []),
    "noise_a":   (700, [], []),
    "noise_b":   (900, [], []),
    "noise_c":   (61, [], []),
}
assert sum(v[0] for v in VIDEOS.values()) == 2300


def _i32(a):
    return a.ctypes.data_as(POINTER(c_int32))


def _f32(a):
    return a.ctypes.data_as(POINTER(c_float))


def unit(a):
    a = np.asarray(a, dtype=np.float64)
    return (a / np.linalg.norm(a, axis=-1, keepdims=True)).astype(np.float32)


def eps_unit(dim):
    """scan_eps_unit(dim) (csrc/knn_scan_f16.h), restated."""
    return np.float32((2.0 / 2048 + 1.0 / 4194304 + dim / 8388608.0 + 1.0 / 65536 + 2.0 * np.sqrt(float(dim)) / 33554432.0) * 1.02)


class DeviceArrays:
    """Device buffers for the _device form: the clip and the seven result arrays of up to k slots."""

    def __init__(self, m, dim, k):
        self.hip = ctypes.CDLL("libamdhip64.so")
        self.k = k
        self.q = self._alloc(m * dim)
        self.out = [self._alloc(k) for _ in NAMES]

    def _alloc(self, words):
        p = c_void_p()
        assert self.hip.hipMalloc(byref(p), ctypes.c_size_t(words * 4)) == 0
        return p

    def upload(self, q):
        q = np.ascontiguousarray(q, dtype=np.float32)
        assert self.hip.hipMemcpy(self.q, q.ctypes.data_as(c_void_p), ctypes.c_size_t(q.nbytes), 1) == 0

    def read(self, k):
        out = {}
        for name, p in zip(NAMES, self.out):
            a = np.empty(k, dtype=np.float32 if name == "mean_dist" else np.int32)
            assert self.hip.hipMemcpy(a.ctypes.data_as(c_void_p), p, ctypes.c_size_t(a.nbytes), 2) == 0
            out[name] = a
        return out

    def free(self):
        for p in [self.q] + self.out:
            self.hip.hipFree(p)


class Library:
    """A C-level index with the planted videos, the clip, the oracle's distances [300][n] and cached restatement answers."""

    def __init__(self, lib_mod, dim, ranked=True):
        self.m, self.lib, self.dim = lib_mod, lib_mod.load(), dim
        rng = np.random.default_rng(4_100 + dim)
        self.clip = unit(rng.standard_normal((CLIP, dim)))

        def noisy(frames):
            sigma = rng.uniform(0.02, 0.15, len(frames))[:, None]
            return self.clip[frames] + sigma * rng.standard_normal((len(frames), dim)) / np.sqrt(dim)

        rows, labels, frame, twin = [], [], [], None
        for g, (name, (L, copies, gaps)) in enumerate(VIDEOS.items()):
            v = rng.standard_normal((L, dim))
            if isinstance(copies, str):
                src = np.arange(74, 9, -1) if copies == "reversed" else 10 + 2 * np.arange(L)
                v = noisy(src)
            else:
                for at, c0, count in copies:
                    v[at:at + count] = noisy(np.arange(c0, c0 + count))
            for f in gaps:
                v[f] = rng.standard_normal(dim)
            if name == "twin_a":
                twin = v
            if name == "twin_b":
                v = twin
            rows.append(v)
            labels.append(np.full(L, g))
            frame.append(np.arange(L))
        rows, labels, frame = np.concatenate(rows).astype(np.float32), np.concatenate(labels), np.concatenate(frame)
        relabel = rng.permutation(len(VIDEOS))                                 # shuffled labels
        self.label_of = {name: int(relabel[g]) for g, name in enumerate(VIDEOS)}
        labels = relabel[labels]
        perm = rng.permutation(len(rows))                                      # interleaved rows
        rows, labels, frame = rows[perm], labels[perm], frame[perm]
        self.n = len(rows)
        self.labels = np.ascontiguousarray(labels, dtype=np.int32)
        self.pos = np.ascontiguousarray(3 * (frame // 2), dtype=np.int32)         # two frames share each position: the tie decides
        # ranks: ids sorted by (a shuffled video order, frame) — within a video the frame order, which the row numbers do not follow
        self.ranks = None
        if ranked:
            video_key = rng.permutation(len(VIDEOS))[labels]
            self.ranks = np.empty(self.n, dtype=np.int32)
            self.ranks[np.lexsort((frame, video_key))] = np.arange(self.n, dtype=np.int32)
        self.h = c_void_p()
        self.m.check(self.lib.vq_index_create(dim, byref(self.h)))
        self.m.check(self.lib.vq_index_add(self.h, _f32(rows), self.n, 1))
        if ranked:
            self.m.check(self.lib.vq_index_set_id_ranks(self.h, _i32(self.ranks), self.n))
        self.m.check(self.lib.vq_index_set_groups(self.h, _i32(self.labels), self.n, len(VIDEOS)))
        self.m.check(self.lib.vq_index_set_positions(self.h, _i32(self.pos), self.n))
        self.stored = np.empty((self.n, dim), dtype=np.float32)
        self.m.check(self.lib.vq_index_export(self.h, _f32(self.stored)))
        self.tie = np.arange(self.n) if self.ranks is None else self.ranks
        self.dist = np.stack([knn_oracle.distances(self.stored, q) for q in self.clip])      # computed once, never changed
        self.dist.setflags(write=False)
        self._want = {}

    def want(self, m, max_dist, min_len, max_miss, k, allowed=None, dist=None):
        at = (m, np.float32(max_dist).tobytes(), min_len, max_miss, k, None if allowed is None else tuple(sorted(allowed)), dist is None)
        if dist is not None or at not in self._want:
            res = match_ref.answer((self.dist if dist is None else dist)[:m], self.labels, self.pos, self.tie, max_dist, min_len, max_miss, k,
                                   allowed)
            if dist is not None:
                return res
            self._want[at] = res
        return self._want[at]

    def call(self, q, k, max_dist, min_len, max_miss, mode, groups=(), exclude=1):
        """vq_index_match_runs -> (rc, dict of arrays)"""
        q = np.ascontiguousarray(q, dtype=np.float32)
        g = np.ascontiguousarray(groups, dtype=np.int32)
        out = {name: np.full(k, -7, dtype=np.float32 if name == "mean_dist" else np.int32) for name in NAMES}
        rc = self.lib.vq_index_match_runs(self.h, _f32(q), len(q), k, c_float(max_dist), min_len, max_miss, mode, _i32(g), len(g), exclude,
                                          *(_i32(out[name]) for name in NAMES[:6]), _f32(out["mean_dist"]))
        return rc, out

    def call_device(self, dev, m, k, max_dist, min_len, max_miss, mode, groups=(), exclude=1):
        g = np.ascontiguousarray(groups, dtype=np.int32)
        self.m.check(self.lib.vq_index_match_runs_device(self.h, dev.q, m, k, c_float(max_dist), min_len, max_miss, mode, _i32(g), len(g), exclude,
                                                         *dev.out))
        self.m.check(self.lib.vq_index_synchronize(self.h))
        return dev.read(k)

    def stats(self):
        st = (c_int64 * 3)()
        self.m.check(self.lib.vq_index_last_search_stats(self.h, st))
        return list(st)

    def modes(self):
        return (1, 2, 0) if self.dim in FP16_DIMS else (1, 0)

    def close(self):
        if self.h:
            self.lib.vq_index_destroy(self.h)
            self.h = c_void_p()


def same(got, slots, what):
    want = match_ref.as_arrays(slots)
    for name in NAMES[:6]:
        assert np.array_equal(got[name], want[name]), f"{what}: {name} differ\n got {got[name]}\nwant {want[name]}"
    assert got["mean_dist"].tobytes() == want["mean_dist"].tobytes(), f"{what}: mean_dist bits differ\n got {got['mean_dist']}\nwant {want['mean_dist']}"


_CACHE = {}


def library(gpu_lib, dim, ranked=True):
    if (dim, ranked) not in _CACHE:
        _CACHE[dim, ranked] = Library(gpu_lib, dim, ranked)
    return _CACHE[dim, ranked]


@pytest.fixture(scope="module", autouse=True)
def _close_indexes():
    yield
    for d in _CACHE.values():
        d.close()
    _CACHE.clear()


def median_copy_distance(d):
    """A threshold inside the copies' distances: about half of the planted cells hit, the runs break up."""
    copies = d.dist[d.dist < np.float32(0.05)]
    return float(np.sort(copies)[len(copies) // 2])


# ---- 1. every clip length, every mode, host and device form ----
@GPU
@pytest.mark.parametrize("dim,ranked", [(256, True), (512, True), (768, True), (ODD_DIM, True), (512, False)])
def test_planted_videos_in_every_mode(gpu_lib, monkeypatch, dim, ranked):
    monkeypatch.delenv(CAP_ENV, raising=False)
    d = library(gpu_lib, dim, ranked)
    k = 16                                                  # above the twelve groups: empty slots behind the answer
    mid = median_copy_distance(d)
    dev = DeviceArrays(CLIP, dim, k)
    try:
        for m in CLIP_LENGTHS:
            dev.upload(d.clip[:m])
            for max_dist, min_len, max_miss in ((0.05, 3, 0), (0.05, 1, 1), (0.05, 2, 2), (mid, 2, 1)):
                slots, holding = d.want(m, max_dist, min_len, max_miss, k)
                for mode in d.modes():
                    what = f"dim {dim} ranked {ranked} m {m} max_dist {max_dist:.6g} min_len {min_len} max_miss {max_miss} mode {mode}"
                    rc, got = d.call(d.clip[:m], k, max_dist, min_len, max_miss, mode)
                    gpu_lib.check(rc)
                    st = d.stats()
                    print(what, "stats", st)
                    same(got, slots, what)
                    assert st[0] == holding and st[2] == 0, (what, st, holding)
                    if mode == 1:
                        assert st[1] == 0, (what, st)
                    if mode != 0 and (min_len, max_miss) == (2, 1):
                        same(d.call_device(dev, m, k, max_dist, min_len, max_miss, mode), slots, what + " (device form)")
                        assert d.stats() == st, what
                if dim == ODD_DIM:
                    rc, _ = d.call(d.clip[:m], k, max_dist, min_len, max_miss, 2)
                    assert rc == -1, "mode 2 must be refused where the tile path does not exist"
    finally:
        dev.free()
    if not ranked:
        return
    # what the planted videos promise, on the restatement's own answer for the whole clip
    by = {s["group"]: s for s in d.want(CLIP, 0.05, 3, 0, k)[0] if s["group"] >= 0}
    lab = d.label_of
    order = {name: match_ref.order_of(np.flatnonzero(d.labels == lab[name]), d.pos, d.tie) for name in VIDEOS}
    p = by[lab["partial"]]
    assert (p["hits"], p["span"], p["q_first"]) == (90, 90, 10)
    assert (p["row_first"], p["row_last"]) == (order["partial"][40], order["partial"][129])
    assert lab["reversed"] not in by and lab["strided"] not in by and lab["single"] not in by and lab["pair"] not in by
    assert by[lab["one_gap"]]["hits"] == 32 and by[lab["two_gaps"]]["hits"] == 32
    loose = {s["group"]: s for s in d.want(CLIP, 0.05, 1, 1, k)[0] if s["group"] >= 0}
    assert (loose[lab["one_gap"]]["hits"], loose[lab["one_gap"]]["span"]) == (62, 63)
    assert loose[lab["two_gaps"]]["hits"] == 32                                          # two misses in a row still cut at max_miss 1
    assert loose[lab["reversed"]]["hits"] == 1 and loose[lab["strided"]]["hits"] == 1    # a reversed or strided copy never makes a run of 2
    assert loose[lab["pair"]]["hits"] == 2 and loose[lab["single"]]["hits"] == 1
    wide = {s["group"]: s for s in d.want(CLIP, 0.05, 2, 2, k)[0] if s["group"] >= 0}
    assert (wide[lab["two_gaps"]]["hits"], wide[lab["two_gaps"]]["span"]) == (62, 64)
    ranking = [s["group"] for s in d.want(CLIP, 0.05, 3, 0, k)[0] if s["group"] >= 0]
    ta, tb = ranking.index(lab["twin_a"]), ranking.index(lab["twin_b"])
    assert abs(ta - tb) == 1 and (ta < tb) == (lab["twin_a"] < lab["twin_b"])           # equal runs: the label decides
    assert by[lab["twin_a"]]["mean_dist"] == by[lab["twin_b"]]["mean_dist"]


# ---- 2. the edge of the threshold ----
@GPU
@pytest.mark.parametrize("dim", FP16_DIMS)
def test_threshold_edge_goes_through_the_filed_list(gpu_lib, monkeypatch, dim):
    """max_dist = the oracle's fp32 distance of a planted cell, then the float below it: the cell's hit flips and with it the run.
    The tile path must decide that cell through the filed list.  Pairs filed <= the pairs whose exact score lies within
    E + slack + 2^-22 of T = 1 - max_dist, E = scan_eps_unit(dim) x max|row| x |q| with the norms 1.0001 the index assumes for
    normalised rows (the proof itself bounds the band by 2 E + slack + 2^-22; the fp16 scores of unit vectors are within a small
    fraction of E of the exact ones, so the tighter count holds too)."""
    monkeypatch.delenv(CAP_ENV, raising=False)
    d = library(gpu_lib, dim)
    order = match_ref.order_of(np.flatnonzero(d.labels == d.label_of["partial"]), d.pos, d.tie)
    along = np.array([d.dist[10 + j, order[40 + j]] for j in range(90)])       # the planted run's cells (10 + j, 40 + j)
    j = int(np.argmax(along[1:-1])) + 1                     # its farthest inner cell: at that threshold the run is whole, below it cut
    i, r = 10 + j, order[40 + j]
    at = d.dist[i, r]
    below = np.nextafter(at, np.float32(-np.inf), dtype=np.float32)
    k, answers = 16, []
    for max_dist in (at, below):
        slots, holding = d.want(CLIP, max_dist, 3, 0, k)
        answers.append(next(s for s in slots if s["group"] == d.label_of["partial"]))
        T = 1.0 - float(max_dist)
        band = float(eps_unit(dim)) * 1.0001 * 1.0001 + SLACK + 2.0 ** -22
        near = int((np.abs((1.0 - d.dist.astype(np.float64)) - T) <= band).sum())
        assert 1 <= near < 1 << 20, near                    # the inputs keep the band far below the list's capacity
        for mode in (1, 2):
            what = f"dim {dim} max_dist {max_dist!r} mode {mode}"
            rc, got = d.call(d.clip, k, float(max_dist), 3, 0, mode)
            gpu_lib.check(rc)
            st = d.stats()
            print(what, "stats", st, "pairs in the band", near)
            same(got, slots, what)
            assert st[0] == holding
            if mode == 2:
                assert st[2] == 0 and 1 <= st[1] <= near, (what, st, near)
    assert answers[0] != answers[1], "the flipped cell must change the planted video's run"
    hit = match_ref.hit_table(d.dist, at)
    assert hit[i, r] and not match_ref.hit_table(d.dist, below)[i, r]


# ---- 3. the exact redo behind the flag ----
@GPU
@pytest.mark.parametrize("dim", FP16_DIMS)
def test_overflow_and_unprovable_queries_are_redone_exactly(gpu_lib, monkeypatch, dim):
    d = library(gpu_lib, dim)
    k, m = 16, 257
    mid = median_copy_distance(d)
    slots, holding = d.want(m, mid, 2, 1, k)
    monkeypatch.delenv(CAP_ENV, raising=False)
    rc, got = d.call(d.clip[:m], k, mid, 2, 1, 2)
    gpu_lib.check(rc)
    st = d.stats()
    assert st[2] == 0 and st[1] >= 2, st                    # the threshold sits among the copies' scores: the list is in use
    same(got, slots, "default capacity")
    dev = DeviceArrays(m, dim, k)
    try:
        monkeypatch.setenv(CAP_ENV, "1")                    # the list holds one pair: it overflows
        rc, got = d.call(d.clip[:m], k, mid, 2, 1, 2)
        gpu_lib.check(rc)
        assert d.stats() == [holding, 0, 2]
        same(got, slots, "capacity 1")
        dev.upload(d.clip[:m])
        same(d.call_device(dev, m, k, mid, 2, 1, 2), slots, "capacity 1 (device form)")
        assert d.stats() == [holding, 0, 2]
        monkeypatch.delenv(CAP_ENV)
        # |q|^2 = 9 for one frame: outside what the fp16 bound covers.  d = 1 - 3 s for that frame, as given.
        q = d.clip[:m].copy()
        q[7] *= np.float32(3.0)
        dist = d.dist[:m].copy()
        dist[7] = knn_oracle.distances(d.stored, q[7])
        slots3, holding3 = d.want(m, 0.05, 2, 1, k, dist=dist)
        rc, got = d.call(q, k, 0.05, 2, 1, 2)               # the host form sees the norm and takes the chunked exact path
        gpu_lib.check(rc)
        assert d.stats() == [holding3, 0, 2]
        same(got, slots3, "|q|^2 = 9")
        dev.upload(q)                                       # the device form finds it on the device: the redo kernel answers
        same(d.call_device(dev, m, k, 0.05, 2, 1, 2), slots3, "|q|^2 = 9 (device form)")
        assert d.stats() == [holding3, 0, 2]
    finally:
        dev.free()


# ---- 4. filters and empty slots ----
@GPU
@pytest.mark.parametrize("dim", (512, ODD_DIM))
def test_filters_both_empty_lists_and_empty_slots(gpu_lib, monkeypatch, dim):
    monkeypatch.delenv(CAP_ENV, raising=False)
    d = library(gpu_lib, dim)
    lab, k, m = d.label_of, 20, CLIP
    some = [lab["partial"], lab["twin_b"], lab["noise_a"], lab["one_gap"], lab["one_gap"]]      # a label named twice counts once
    everyone = set(range(len(VIDEOS)))
    for mode in d.modes():
        for groups, exclude, allowed in ((some, 0, set(some)), (some, 1, everyone - set(some)), ([], 1, None), ([lab["noise_b"]], 0, {lab["noise_b"]})):
            slots, holding = d.want(m, 0.05, 2, 1, k, allowed)
            rc, got = d.call(d.clip, k, 0.05, 2, 1, mode, groups, exclude)
            gpu_lib.check(rc)
            what = f"dim {dim} mode {mode} groups {groups} exclude {exclude}"
            same(got, slots, what)
            assert d.stats()[0] == holding, what
            assert holding < k and got["group"][holding] == -1 and np.isinf(got["mean_dist"][holding])
        rc, got = d.call(d.clip, k, 0.05, 2, 1, mode, [], 0)          # an empty include list: nothing is allowed
        gpu_lib.check(rc)
        same(got, [dict(match_ref.EMPTY)] * k, f"dim {dim} mode {mode} empty include list")
        assert d.stats() == [0, 0, 0]
    rc, _ = d.call(d.clip, k, 0.05, 2, 1, 1, [len(VIDEOS)], 0)
    assert rc == -1, "a label outside [0, n_groups) is refused"


# ---- 5. the consequences the definition states ----
@GPU
@pytest.mark.parametrize("dim", (512, ODD_DIM))
def test_consequences(gpu_lib, monkeypatch, dim):
    monkeypatch.delenv(CAP_ENV, raising=False)
    d = library(gpu_lib, dim)
    k, G = 16, len(VIDEOS)
    sizes = np.bincount(d.labels, minlength=G)
    for mode in d.modes():
        for m in (1, 64, 257):
            # +inf: every cell hits; hits = span = min(m, L) on the smallest diagonal of that length
            rc, got = d.call(d.clip[:m], k, np.inf, 1, 0, mode)
            gpu_lib.check(rc)
            same(got, d.want(m, np.inf, 1, 0, k)[0], f"dim {dim} mode {mode} m {m} +inf")
            for j in range(G):
                g = int(got["group"][j])
                L = int(sizes[g])
                order = match_ref.order_of(np.flatnonzero(d.labels == g), d.pos, d.tie)
                delta = min(0, L - m)
                assert got["hits"][j] == got["span"][j] == min(m, L)
                assert got["q_first"][j] == -delta and got["row_first"][j] == order[0]
            # -inf: nothing
            rc, got = d.call(d.clip[:m], k, -np.inf, 1, 0, mode)
            gpu_lib.check(rc)
            same(got, [dict(match_ref.EMPTY)] * k, f"dim {dim} mode {mode} m {m} -inf")
            assert d.stats()[0] == 0
        # m = 1, min_len = 1: exactly the groups whose grouped-search best distance is within max_dist, in label order
        q = np.ascontiguousarray(d.clip[105:106])
        groups, rows, dist = np.empty(G, np.int32), np.empty(G, np.int32), np.empty(G, np.float32)
        gpu_lib.check(d.lib.vq_index_search_grouped(d.h, _f32(q), 1, G, 1, _i32(groups), _i32(rows), _f32(dist)))
        for max_dist in (0.05, 0.9, 1.0, 1.2):
            rc, got = d.call(q, k, max_dist, 1, 0, mode)
            gpu_lib.check(rc)
            want = sorted(int(g) for g, dd in zip(groups, dist) if dd <= np.float32(max_dist))
            assert [int(g) for g in got["group"] if g >= 0] == want, (dim, mode, max_dist)
            assert all(h == 1 for h in got["hits"][:len(want)])
            if max_dist == 0.05:
                assert want == sorted([d.label_of["twin_a"], d.label_of["twin_b"]])      # clip frame 105 is planted in the twins only


# ---- 6. lifetime: stale labels, positions and ranks are refused as the sequence search refuses them ----
@GPU
def test_lifetime_refusals(gpu_lib):
    lib = gpu_lib.load()
    rng = np.random.default_rng(77)
    rows = rng.standard_normal((40, 64)).astype(np.float32)
    labels = np.ascontiguousarray(np.arange(40) // 10, dtype=np.int32)
    pos = np.ascontiguousarray(np.arange(40) % 10, dtype=np.int32)
    ranks = np.ascontiguousarray(rng.permutation(40), dtype=np.int32)
    h = c_void_p()
    gpu_lib.check(lib.vq_index_create(64, byref(h)))
    out = [np.empty(4, np.int32) for _ in range(6)] + [np.empty(4, np.float32)]

    def call():
        q = np.ascontiguousarray(unit(rows[:5]))
        return lib.vq_index_match_runs(h, _f32(q), 5, 4, c_float(0.01), 2, 0, 1, None, 0, 1, *(_i32(a) for a in out[:6]), _f32(out[6]))

    try:
        assert call() == 0 and list(out[0]) == [-1] * 4 and np.isinf(out[6]).all()        # an empty index: empty slots
        gpu_lib.check(lib.vq_index_add(h, _f32(rows), 40, 1))
        assert call() == -1                                                              # no labels yet
        gpu_lib.check(lib.vq_index_set_groups(h, _i32(labels), 40, 4))
        assert call() == -1                                                              # no positions yet
        gpu_lib.check(lib.vq_index_set_positions(h, _i32(pos), 40))
        assert call() == 0 and out[0][0] == 0 and out[1][0] == 5                         # the clip is the head of video 0
        gpu_lib.check(lib.vq_index_set_id_ranks(h, _i32(ranks), 40))
        assert call() == 0 and out[1][0] == 5                                            # ranks only order ties: positions are distinct here
        gpu_lib.check(lib.vq_index_add(h, _f32(rows[:3]), 3, 1))
        assert call() == -1                                                              # ranks, labels and positions cover 40 of 43 rows
        gone = np.array([40, 41, 42], dtype=np.int64)
        gpu_lib.check(lib.vq_index_remove_rows(h, gone.ctypes.data_as(POINTER(c_int64)), 3))
        assert call() == -1                 # ranks and labels that did not cover the index are dropped by a removal, positions always
        gpu_lib.check(lib.vq_index_set_positions(h, _i32(pos), 40))
        assert call() == -1 and b"labels" in lib.vq_last_error()
        gpu_lib.check(lib.vq_index_set_groups(h, _i32(labels), 40, 4))
        assert call() == 0 and out[0][0] == 0 and out[1][0] == 5
        gone = np.array([38, 39], dtype=np.int64)                                        # labels that cover the index survive a removal
        gpu_lib.check(lib.vq_index_remove_rows(h, gone.ctypes.data_as(POINTER(c_int64)), 2))
        assert call() == -1 and b"positions" in lib.vq_last_error()
        gpu_lib.check(lib.vq_index_set_positions(h, _i32(pos), 38))
        assert call() == 0 and out[0][0] == 0 and out[1][0] == 5
    finally:
        lib.vq_index_destroy(h)


# ---- 7. the Python layer on string ids ----
@GPU
def test_python_layer_on_string_ids(gpu_lib):
    from video_quierer_amd.indexes.hnsw import OptimizedHNSWIndex
    from video_quierer_amd.overhaul_index import SimpleVideoIndex
    rng = np.random.default_rng(5)
    dim = 64
    film = unit(rng.standard_normal((60, dim)))
    trailer = film[20:32] + 0.01 * rng.standard_normal((12, dim)).astype(np.float32)       # twelve frames of the film, re-encoded
    other = unit(rng.standard_normal((30, dim)))
    idx = OptimizedHNSWIndex(dimension=dim)
    try:
        vecs = list(film) + list(trailer) + list(other)
        ids = [f"film_{i}" for i in range(60)] + [f"trailer_{i}" for i in range(12)] + [f"other_{i}" for i in range(30)]
        idx.add_batch(vecs, ids)
        res = idx.shared_runs(list(trailer), k=5, max_distance=0.05, min_len=3)
        assert [r["group"] for r in res] == ["film", "trailer"]                             # equal runs: the order of first appearance
        f = res[0]
        assert (f["hits"], f["span"], f["query_first"], f["first"], f["last"], f["positions"]) == (12, 12, 0, "film_20", "film_31", (20, 31))
        assert type(f["distance"]) is np.float32 and f["score"] == np.float32(1.0) - f["distance"]
        assert idx.last_search_stats()["verified"] == 2
        of = idx.shared_runs_of("trailer", k=5, max_distance=0.05, min_len=3)
        assert [r["group"] for r in of] == ["film"] and (of[0]["first"], of[0]["last"], of[0]["hits"]) == ("film_20", "film_31", 12)
        assert idx.shared_runs_of("trailer", k=5, max_distance=0.05, within=["other"]) == []
        assert idx.shared_runs(list(trailer), k=5, max_distance=0.05, exclude=["trailer", "film"]) == []
        assert idx.shared_runs(list(trailer), k=5, max_distance=0.05, min_len=13) == []
        with pytest.raises(KeyError):
            idx.shared_runs_of("nobody", max_distance=0.05)
        with pytest.raises(ValueError):
            idx.shared_runs(list(trailer), max_distance=float("nan"))
        with pytest.raises(ValueError):
            idx.shared_runs(list(trailer), max_distance=0.05, min_len=0)
        with pytest.raises(ValueError):
            idx.shared_runs([], max_distance=0.05)
    finally:
        idx.close()
    svi = SimpleVideoIndex()
    for i, v in enumerate(film):
        svi.add_frame(v, "film.mp4", i * 0.5)
    for i, v in enumerate(trailer):
        svi.add_frame(unit(v), "trailer.mp4", i * 0.5)
    for i, v in enumerate(other):
        svi.add_frame(v, "other.mp4", i * 0.5)
    found = svi.find_reuse("trailer.mp4", k=5, min_similarity=0.95, min_seconds=2.0)
    assert len(found) == 1
    r = found[0]
    assert (r["video_name"], r["frames"], r["start"], r["end"], r["query_start"], r["query_end"]) == ("film.mp4", 12, 10.0, 15.5, 0.0, 5.5)
    assert 0.95 <= r["score"] <= 1.0
    assert svi.find_reuse("other.mp4") == []
    with pytest.raises(KeyError):
        svi.find_reuse("nobody.mp4")
