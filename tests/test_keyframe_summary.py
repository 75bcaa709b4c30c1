"""Keyframe summary (vq_index_summarize_groups / HNSWIndex.summarize_groups / SimpleVideoIndex.video_summary): the k most
representative frames of a video.  The expected answer is the definition restated in numpy (`mean_direction` / `summarize`
below) over the C oracle's exact distances on the exported rows, with row ties by `tie_ranks` of the ids; rows, the float32
radius bits and members must match bit for bit.

The rows are video-like (consecutive frames are near-duplicates), as tests/test_distinct_search.py makes them."""
import ctypes
import math
from ctypes import POINTER, byref, c_float, c_int32, c_void_p

import numpy as np
import pytest

from index_host_fakes import tie_ranks
from oracle import knn_oracle
from test_distinct_search import video_rows

GPU = pytest.mark.gpu
LENGTHS = [1, 2, 3, 63, 64, 65, 300, 700]           # shorter than k, both sides of a wave, more than one 256-row block
KS = [1, 2, 5, 16, 64, 256]
NO_STOP = -math.inf


# ---- the definition, restated ----
def mean_direction(stored, rows):
    """Step 1: per component the fp64 sum of each 256-row block in row order, the blocks added in order, rounded once to fp32."""
    S = np.zeros(stored.shape[1], dtype=np.float64)
    for i0 in range(0, len(rows), 256):
        B = np.zeros(stored.shape[1], dtype=np.float64)
        for r in rows[i0:i0 + 256]:
            B = B + stored[r].astype(np.float64)
        S = S + B
    return S.astype(np.float32)


def summarize(stored, rows, tie, k, max_radius=NO_STOP):
    """One group.  rows: the group's rows (any order; taken ascending), tie: per row of the index.
    -> (keyframe rows int32 [kappa], radius float32 [kappa], members int32 [kappa])"""
    rows = np.sort(np.asarray(rows, dtype=np.int64))
    sub = np.ascontiguousarray(stored[rows])
    T = np.asarray(tie, dtype=np.int64)[rows]
    L = len(rows)
    s = int(np.lexsort((T, knn_oracle.distances(sub, mean_direction(stored, rows))))[0])       # step 2
    near = knn_oracle.distances(sub, sub[s])                                                     # step 3
    owner = np.zeros(L, dtype=np.int64)
    alive = np.ones(L, dtype=bool)
    alive[s] = False
    chosen, radius = [s], []
    while True:
        t = len(chosen) - 1
        rad = near[alive].max() if alive.any() else np.float32(0.0)                             # step 4
        radius.append(rad)
        if t + 1 == k or not alive.any() or rad <= np.float32(max_radius):                      # step 5
            break
        cand = np.flatnonzero(alive & (near == rad))
        nxt = int(cand[np.argmin(T[cand])])
        chosen.append(nxt)
        alive[nxt] = False
        owner[nxt] = t + 1
        d = knn_oracle.distances(sub, sub[nxt])
        upd = alive & (d < near)
        near[upd] = d[upd]
        owner[upd] = t + 1
    return (rows[chosen].astype(np.int32), np.array(radius, dtype=np.float32),
            np.bincount(owner, minlength=len(chosen)).astype(np.int32))


def dense_labels(groups):
    index = {}
    return np.array([index.setdefault(g, len(index)) for g in groups], dtype=np.int32), list(index)


def _i32(a):
    return a.ctypes.data_as(POINTER(c_int32))


def c_summarize(gpu_lib, h, groups, k, max_radius=NO_STOP, members=True):
    """vq_index_summarize_groups -> (rc, rows, radius, members)"""
    g = np.ascontiguousarray(groups, dtype=np.int32)
    rows = np.full((len(g), k), -7, dtype=np.int32)
    radius = np.full((len(g), k), -7.0, dtype=np.float32)
    mem = np.full((len(g), k), -7, dtype=np.int32)
    rc = gpu_lib.load().vq_index_summarize_groups(h, _i32(g), len(g), k, c_float(max_radius), _i32(rows),
                                                  radius.ctypes.data_as(POINTER(c_float)), _i32(mem) if members else None)
    return rc, rows, radius, mem


def padded(want, k):
    """The restatement's answer in the C layout: -1 / +inf / 0 in the unused slots."""
    rows, radius, mem = want
    n = len(rows)
    return (np.concatenate([rows, np.full(k - n, -1, np.int32)]), np.concatenate([radius, np.full(k - n, np.inf, np.float32)]),
            np.concatenate([mem, np.zeros(k - n, np.int32)]))


class Data:
    """One index over string ids f"v{video}_{frame}" (their order differs from the rows': ranks are set) and what the oracle
    needs about it: exported rows, tie ranks, dense labels.  The restatement's answers are cached."""

    def __init__(self, vecs, video, frame):
        from video_quierer_amd.indexes.hnsw import OptimizedHNSWIndex
        self.idx = OptimizedHNSWIndex(dimension=vecs.shape[1])
        self.set(video, frame)
        self.idx.add_batch(vecs, self.ids)
        self.refresh()

    def set(self, video, frame):
        self.ids = [f"v{v}_{f}" for v, f in zip(video, frame)]
        self.groups = [f"v{v}" for v in video]

    def refresh(self):
        self.stored = self.idx._export()
        self.tie = tie_ranks(self.ids)
        self.labels, self.keys = dense_labels(self.groups)
        self.sizes = np.bincount(self.labels)
        self._want = {}

    def want(self, key, k, max_radius=NO_STOP):
        at = (key, k, max_radius)
        if at not in self._want:
            g = self.keys.index(key)
            self._want[at] = summarize(self.stored, np.flatnonzero(self.labels == g), self.tie, k, max_radius)
        return self._want[at]

    def check(self, res, k, max_radius=NO_STOP, tag=""):
        """A `summarize_groups` answer against the restatement, every group it holds."""
        for key, got in res.items():
            rows, radius, mem = self.want(key, k, max_radius)
            what = f"{tag} group {key} ({self.sizes[self.keys.index(key)]} rows) k {k} max_radius {max_radius}"
            got_rad = np.array([r["radius"] for r in got], dtype=np.float32)
            print(f"{what}: ids {[r['id'] for r in got][:4]} radius got {got_rad[:4]} want {radius[:4]}")
            assert [r["id"] for r in got] == [self.ids[r] for r in rows], f"{what}: keyframes differ"
            assert got_rad.tobytes() == radius.tobytes(), f"{what}: radii differ"
            assert [r["members"] for r in got] == mem.tolist(), f"{what}: members differ"
            assert [r["rank"] for r in got] == list(range(len(rows)))
            assert all(type(r["radius"]) is np.float32 for r in got)


_CACHE = {}


def cached(name, build):
    if name not in _CACHE:
        _CACHE[name] = build()
    return _CACHE[name]


@pytest.fixture(scope="module", autouse=True)
def _close_indexes():
    yield
    for d in _CACHE.values():
        d.idx.close()
    _CACHE.clear()


def plant_duplicates(rows, video):
    """Exact duplicate rows inside one video (zero and equal distances: the tie rule decides) and at a video's first row.  One
    3-row video becomes three copies of one row: at k = 2 the third copy is as far (0) from the second keyframe as from the
    first, and must stay with the first (the strict compare of step 5)."""
    video = np.asarray(video)
    for length, pairs in ((300, ((40, 7), (41, 7), (250, 130))), (700, ((0, 350), (699, 350), (300, 20))), (65, ((0, 64),)), (3, ((2, 1), (0, 1)))):
        v = next((v for v in np.unique(video) if (video == v).sum() == length), None)
        if v is None:
            continue
        first = int(np.flatnonzero(video == v)[0])
        for dst, src in pairs:
            rows[first + dst] = rows[first + src]
    return rows


def small(dim=512, n=1_500):
    def build():
        rows, video, frame = video_rows(n, dim, seed=4104 + dim, lengths=LENGTHS)
        return Data(plant_duplicates(rows, video), video, frame)
    return cached(("small", dim, n), build)


def split(d, lds_rows):
    """(LDS-form groups, wide-form groups) of a call over every group."""
    wide = int((d.sizes > lds_rows).sum())
    return len(d.keys) - wide, wide


def run_both_forms(d, monkeypatch, k, max_radius=None):
    """Every group in one call, as built and with the LDS form limited to 64 rows; both against the restatement, the stats
    against the split, and the two runs against each other."""
    rho = NO_STOP if max_radius is None else max_radius
    out = []
    for lds_rows in (None, 64):
        if lds_rows is None:
            monkeypatch.delenv("VQ_AMD_SUM_LDS_ROWS", raising=False)
        else:
            monkeypatch.setenv("VQ_AMD_SUM_LDS_ROWS", str(lds_rows))
        res = d.idx.summarize_groups(k=k, max_radius=max_radius)
        st = d.idx.last_search_stats()
        assert list(res) == d.keys
        d.check(res, k, rho, tag=f"lds_rows {lds_rows}")
        lds, wide = split(d, 4_096 if lds_rows is None else lds_rows)
        assert (st["verified"], st["rescanned"]) == (lds, wide), st
        assert st["exact_fallback"] == sum(len(v) for v in res.values()), st
        out.append(res)
    assert out[0] == out[1]                                        # ids, float32 radii, members: bit for bit
    return out[0]


# ---- 1. the definition on small shapes, LDS form and wide form ----
@GPU
@pytest.mark.parametrize("k", KS)
def test_every_group_against_the_restatement(gpu_lib, monkeypatch, k):
    d = small()
    assert sorted(set(d.sizes.tolist())) == sorted(set(LENGTHS + [104]))        # 1,500 rows: LENGTHS, six of them again, 104 left
    res = run_both_forms(d, monkeypatch, k)
    assert all(len(res[key]) == min(k, n) for key, n in zip(d.keys, d.sizes))   # kappa = min(k, L) without max_radius
    if k == 2:                                                     # the oracle's own numbers on the three copies of one row
        triple = d.keys[int(np.flatnonzero(d.sizes == 3)[0])]
        rows, radius, mem = d.want(triple, 2)
        assert radius[0] == radius[1] and abs(radius[0]) < 1e-6 and mem.tolist() == [2, 1]       # (1 - |x|^2 in fp32: 0 or an ulp)
        assert [d.ids[r] for r in rows] == sorted(d.ids[r] for r in np.flatnonzero(d.labels == d.keys.index(triple)))[:2]


@GPU
@pytest.mark.parametrize("dim", [64, 72])
def test_other_dimensions(gpu_lib, monkeypatch, dim):
    """dim 72 is not a multiple of 32: the chain without the eight-load prefetch."""
    d = small(dim, 700)
    for k in (5, 64):
        run_both_forms(d, monkeypatch, k)


# ---- 2. max_radius ----
@GPU
def test_max_radius_returns_the_shortest_prefix(gpu_lib, monkeypatch):
    d = small()
    key = d.keys[int(np.argmax(d.sizes))]
    _, radius, _ = d.want(key, 16)
    assert radius[3] > radius[4] and radius[5] > radius[6]         # the oracle's own numbers: distinct radii to cut at
    between = np.float32((float(radius[3]) + float(radius[4])) / 2)
    assert radius[4] < between < radius[3]
    for rho, kappa in ((float(between), 5), (float(radius[6]), 7), (math.inf, 1)):
        res = run_both_forms(d, monkeypatch, 16, max_radius=rho)
        assert len(res[key]) == kappa
        full = d.idx.summarize_groups(k=16)
        for g, got in res.items():                                 # the exact prefix: keyframes and radii; the last radius meets rho
            assert [(r["id"], r["radius"]) for r in got] == [(r["id"], r["radius"]) for r in full[g][:len(got)]]
            assert got[-1]["radius"] <= np.float32(rho) or len(got) == min(16, len(full[g]))
            assert all(r["radius"] > np.float32(rho) for r in got[:-1])


# ---- 3. properties ----
@GPU
def test_prefix_radius_members_and_duplicate_labels(gpu_lib, monkeypatch):
    monkeypatch.delenv("VQ_AMD_SUM_LDS_ROWS", raising=False)
    d = small()
    by_k = {k: d.idx.summarize_groups(k=k) for k in KS}
    for key, n in zip(d.keys, d.sizes):
        longest = by_k[256][key]
        for k in KS:
            got = by_k[k][key]
            assert [(r["id"], r["radius"]) for r in got] == [(r["id"], r["radius"]) for r in longest[:k]]      # prefix
            assert sum(r["members"] for r in got) == n
            rad = [r["radius"] for r in got]
            assert all(a >= b for a, b in zip(rad, rad[1:]))       # never increases
        assert longest[-1]["radius"] == 0 or len(longest) == 256   # every row chosen: nothing is left
    # C ABI: duplicate labels are answered one by one, identically; members_out may be NULL
    big, one = int(np.argmax(d.sizes)), int(np.argmin(d.sizes))
    for lds_rows in (None, 64):
        if lds_rows is not None:
            monkeypatch.setenv("VQ_AMD_SUM_LDS_ROWS", str(lds_rows))
        rc, rows, radius, mem = c_summarize(gpu_lib, d.idx._h, [big, one, big, 3, big], 16)
        gpu_lib.check(rc)
        for j, g in enumerate([big, one, big, 3, big]):
            w = padded(d.want(d.keys[g], 16), 16)
            assert (rows[j].tobytes(), radius[j].tobytes(), mem[j].tobytes()) == tuple(a.tobytes() for a in w), (lds_rows, j)
        rc, rows2, radius2, mem2 = c_summarize(gpu_lib, d.idx._h, [big, one, big, 3, big], 16, members=False)
        gpu_lib.check(rc)
        assert rows2.tobytes() == rows.tobytes() and radius2.tobytes() == radius.tobytes() and (mem2 == -7).all()
    rc = c_summarize(gpu_lib, d.idx._h, [0, len(d.keys)], 4)[0]
    assert rc < 0 and b"outside" in gpu_lib.load().vq_last_error()


@GPU
def test_no_label_is_left_without_rows_and_an_empty_index_answers_empty(gpu_lib):
    """The C definition gives empty slots to a label that holds no row.  The index keeps its labels dense (vq_index_set_groups
    refuses a label without rows, vq_index_remove_rows renumbers them away), so no call sequence reaches that case: what can be
    checked is that refusal, and the empty index, whose every slot is empty."""
    from video_quierer_amd.indexes.hnsw import OptimizedHNSWIndex
    lib = gpu_lib.load()
    idx = OptimizedHNSWIndex(dimension=64)
    try:
        rc, rows, radius, mem = c_summarize(gpu_lib, idx._h, [0, 5], 3)
        gpu_lib.check(rc)
        assert (rows == -1).all() and np.isinf(radius).all() and (mem == 0).all()
        assert idx.last_search_stats() == {"verified": 0, "rescanned": 0, "exact_fallback": 0}
        assert idx.summarize_groups() == {}
        with pytest.raises(KeyError):
            idx.summarize_group("v0")
        idx.add_batch(np.eye(64, dtype=np.float32)[:4], list(range(4)))
        lab = np.array([0, 0, 2, 2], dtype=np.int32)
        assert lib.vq_index_set_groups(idx._h, _i32(lab), 4, 3) < 0 and b"no rows" in lib.vq_last_error()
    finally:
        idx.close()


# ---- 4. one longer group: the wide form without an override ----
@GPU
def test_one_group_of_5000_rows_takes_the_wide_form(gpu_lib, monkeypatch):
    monkeypatch.delenv("VQ_AMD_SUM_LDS_ROWS", raising=False)
    rows, video, frame = video_rows(5_300, 128, seed=5005, lengths=[5_000, 300])
    rows[4_999] = rows[17]                                         # the last row of the last (partial) block duplicates an early one
    d = Data(rows, video, frame)
    try:
        res = d.idx.summarize_groups(k=8)
        st = d.idx.last_search_stats()
        assert (st["verified"], st["rescanned"], st["exact_fallback"]) == (1, 1, 16), st
        d.check(res, 8)
        assert sum(r["members"] for r in res["v0"]) == 5_000
    finally:
        d.idx.close()


# ---- 5. the device form ----
@GPU
def test_device_form_twice_without_a_wait(gpu_lib, monkeypatch):
    d = small()
    lib, h = gpu_lib.load(), d.idx._h
    q = [d.stored[5] + d.stored[900], d.stored[1_400]]
    before = d.idx.search_batch(q, 7)
    calls = [(np.arange(len(d.keys), dtype=np.int32), 16, NO_STOP), (np.array([7, 6, 7], dtype=np.int32), 5, 0.05)]
    monkeypatch.setenv("VQ_AMD_SUM_LDS_ROWS", "64")                # both forms in each call
    want = []
    for g, k, rho in calls:
        rc, rows, radius, mem = c_summarize(gpu_lib, h, g, k, rho)
        gpu_lib.check(rc)
        want.append((rows, radius, mem))
    hip = ctypes.CDLL("libamdhip64.so")
    stream = c_void_p()
    assert hip.hipStreamCreate(byref(stream)) == 0
    ptrs = []

    def dev(nbytes):
        p = c_void_p()
        assert hip.hipMalloc(byref(p), ctypes.c_size_t(nbytes)) == 0
        ptrs.append(p)
        return p
    try:
        d.idx.set_stream(stream.value)
        outs = [tuple(dev(len(g) * k * 4) for _ in range(3)) for g, k, _ in calls]
        for (g, k, rho), (dr, df, dm) in zip(calls, outs):         # back to back, nothing read back in between
            gpu_lib.check(lib.vq_index_summarize_groups_device(h, _i32(g), len(g), k, c_float(rho), dr, df, dm))
        assert hip.hipStreamSynchronize(stream) == 0
        for bufs, refs in zip(outs, want):
            for src, ref in zip(bufs, refs):
                got = np.empty_like(ref)
                assert hip.hipMemcpy(got.ctypes.data_as(c_void_p), src, ctypes.c_size_t(got.nbytes), 2) == 0
                assert got.tobytes() == ref.tobytes()
    finally:
        d.idx.set_stream(0)
        for p in ptrs:
            hip.hipFree(p)
        hip.hipStreamDestroy(stream)
    after = d.idx.search_batch(q, 7)
    assert [[(r["id"], r["distance"]) for r in rr] for rr in before] == [[(r["id"], r["distance"]) for r in rr] for rr in after]
    for j, (g, k, rho) in enumerate(calls):                        # and the host form equals the restatement
        for e, label in enumerate(g):
            w = padded(d.want(d.keys[label], k, rho), k)
            assert tuple(a[e].tobytes() for a in want[j]) == tuple(a.tobytes() for a in w)


# ---- 6. lifetime ----
@GPU
def test_lifetime_after_add_and_remove(gpu_lib, monkeypatch):
    monkeypatch.delenv("VQ_AMD_SUM_LDS_ROWS", raising=False)
    lib = gpu_lib.load()
    n, dim = 800, 64
    vecs, video, frame = video_rows(n + 200, dim, seed=6006, lengths=[1, 65, 300])
    d = Data(vecs[:n], video[:n], frame[:n])
    try:
        h = d.idx._h
        d.check(d.idx.summarize_groups(k=5), 5, tag="fresh")
        gpu_lib.check(c_summarize(gpu_lib, h, [0, 1], 5)[0])
        d.idx.add_batch(vecs[n:], [f"v{v}_{f}" for v, f in zip(video[n:], frame[n:])])
        rc = c_summarize(gpu_lib, h, [0, 1], 5)[0]                 # stale after an add: refused until the labels are set again
        assert rc < 0 and (b"labels" in lib.vq_last_error() or b"ranks" in lib.vq_last_error())
        d.set(video, frame)
        d.refresh()
        res = d.idx.summarize_groups(k=5)                          # the wrapper re-syncs by itself
        d.check(res, 5, tag="after add")
        rc, rows, radius, mem = c_summarize(gpu_lib, h, [0, 1], 5)
        gpu_lib.check(rc)
        for j in (0, 1):
            assert rows[j].tobytes() == padded(d.want(d.keys[j], 5), 5)[0].tobytes()
        gone_key = next(key for key, size in zip(d.keys, d.sizes) if size == 300)
        assert d.idx.remove_group(gone_key) == 300
        keep = [r for r in range(n + 200) if d.groups[r] != gone_key]
        d.set([video[r] for r in keep], [frame[r] for r in keep])
        d.refresh()
        other = next(key for key, size in zip(d.keys, d.sizes) if size == 300)
        got = d.idx.summarize_group(other, 8)
        d.check({other: got}, 8, tag="after removal")              # the restatement on the compacted rows
        d.check(d.idx.summarize_groups(k=3), 3, tag="after removal, all")
    finally:
        d.idx.close()


# ---- 7. Python end to end ----
@GPU
def test_video_summary_on_fractional_timestamps(gpu_lib, monkeypatch):
    monkeypatch.delenv("VQ_AMD_SUM_LDS_ROWS", raising=False)
    from video_quierer_amd.overhaul_index import SimpleVideoIndex
    vecs, video, frame = video_rows(600, 512, seed=811, lengths=[150])
    rng = np.random.default_rng(812)
    names = [f"clip{v}.mp4" for v in video]
    stamps = [round(f * 0.4 + float(rng.uniform(0, 0.3)), 3) for f in frame]
    sv = SimpleVideoIndex()
    for e, nm, ts in zip(vecs, names, stamps):
        sv.add_frame(e, nm, ts)
    stored = np.stack(sv.embeddings)
    tie = -np.arange(600)                                          # search's tie rule: the larger frame id first
    rows, radius, mem = summarize(stored, np.arange(150, 300), tie, 6)
    got = sv.video_summary("clip1.mp4", 6)
    assert [md["frame_id"] for md in got] == rows.tolist() and [md["rank"] for md in got] == list(range(6))
    assert [md["radius"] for md in got] == [float(r) for r in radius] and [md["members"] for md in got] == mem.tolist()
    assert all(md["video_name"] == "clip1.mp4" and md["timestamp"] == stamps[md["frame_id"]] for md in got)
    chrono = sv.video_summary("clip1.mp4", 6, chronological=True)
    assert chrono == sorted(got, key=lambda md: md["timestamp"]) and chrono != got
    short = sv.video_summary("clip1.mp4", 6, max_radius=float(radius[2]))
    assert len(short) == 1 + int(np.argmax(radius <= radius[2]))   # the exact prefix (the members are those at the stop)
    assert [(md["frame_id"], md["radius"]) for md in short] == [(md["frame_id"], md["radius"]) for md in got[:len(short)]]
    assert sum(md["members"] for md in short) == 150
    with pytest.raises(KeyError):
        sv.video_summary("nope.mp4")


@GPU
def test_similar_videos_by_keyframes_above_4096_frames(gpu_lib, monkeypatch):
    monkeypatch.delenv("VQ_AMD_SUM_LDS_ROWS", raising=False)
    from video_quierer_amd.overhaul_index import SimpleVideoIndex
    vecs, video, frame = video_rows(4_600, 64, seed=911, lengths=[4_200, 100])
    vecs[4_300:4_400] = vecs[1_000:4_000:30] + np.float32(0.01)    # a later video cut from the long one
    sv = SimpleVideoIndex()
    for e, v, f in zip(vecs, video, frame):
        sv.add_frame(e, f"clip{v}.mp4", f * 0.04)
    with pytest.raises(ValueError):
        sv.similar_videos("clip0.mp4", 3)                          # 4,200 frames: unchanged without keyframes=
    keyframes = sv.video_summary("clip0.mp4", 8)
    assert len(keyframes) == 8
    got = sv.similar_videos("clip0.mp4", 3, keyframes=8)
    dev = sv._device(ranks=True)
    unit = np.stack([sv.embeddings[md["frame_id"]] for md in keyframes])      # the eight stored rows, as stored
    with dev.lock:
        want = dev._search_set(unit, 3, (["clip0.mp4"], True), sv._group_fn, False, given=True)
    print("similar by keyframes:", got)
    assert [(r["video_name"], r["score"]) for r in got] == [(r["group"], float(r["score"])) for r in want]
    assert [r["video_name"] for r in got] == ["clip2.mp4", "clip1.mp4"]         # the cut of the long video comes first
