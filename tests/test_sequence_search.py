"""Sequence search (vq_index_search_sequence / HNSWIndex.search_sequence / SimpleVideoIndex.search_storyboard): the k videos that
show a list of steps in order.  The expected answer is the definition restated in numpy (`group_dp` / `sequence_answer` below)
over the C oracle's exact distances on the exported rows, with row ties by `_tie_ranks` of the ids; groups, float32 distances,
chains and positions must match bit for bit.

The rows are video-like (consecutive frames are near-duplicates), as tests/test_distinct_search.py makes them."""
import ctypes
import math
from ctypes import POINTER, byref, c_int32, c_int64, c_void_p

import numpy as np
import pytest

from oracle import knn_oracle
from test_distinct_search import _tie_ranks, _unit, video_rows

GPU = pytest.mark.gpu
BIG_GAP = 2 ** 40
LENGTHS = [1, 2, 3, 7, 63, 64, 65, 300, 700]        # shorter than m, exactly m, both sides of a wave, several 64-row blocks


# ---- the definition, restated ----
def group_dp(dist, rows, pos, tie, min_gap, max_gap):
    """One group.  dist [m][n] float32 (d(j, r) for every row of the index), rows: the group's rows, pos / tie: per row of the
    index.  -> None when the group holds no chain, else (D float32, chain rows in step order, tie_decided) — tie_decided: some
    p* or the end row had a rival of bit-equal cost, so the tie chose."""
    rows = np.asarray(rows, dtype=np.int64)
    m, L = len(dist), len(rows)
    P = np.asarray(pos, dtype=np.int64)[rows]
    T = np.asarray(tie, dtype=np.int64)[rows]
    diff = P[:, None] - P[None, :]                             # [r][p] = pos(r) - pos(p), 64-bit
    adm = (diff >= min_gap) & (diff <= max_gap)
    C = dist[0][rows].astype(np.float64)                       # C_0
    defined = np.ones(L, dtype=bool)
    back, tie_decided = [], False
    for j in range(1, m):
        rank = np.empty(L, dtype=np.int64)
        rank[np.lexsort((T, C))] = np.arange(L)                # the order (C_{j-1}, tie)
        ok = adm & defined[None, :]
        best = np.where(ok, rank[None, :], L).argmin(axis=1)   # p*: the admissible predecessor of the smallest (C, tie)
        has = ok.any(axis=1)
        rivals = (ok & (C[None, :] == C[best][:, None])).sum(axis=1)
        tie_decided = tie_decided or bool(((rivals > 1) & has).any())
        C = np.where(has, C[best] + dist[j][rows].astype(np.float64), np.inf)      # one fp64 addition
        defined = has
        back.append(best)
    cand = np.flatnonzero(defined)
    if len(cand) == 0:
        return None
    e = cand[np.lexsort((T[cand], C[cand]))[0]]
    tie_decided = tie_decided or int((C[cand] == C[e]).sum()) > 1
    chain = [int(e)]
    for best in reversed(back):
        chain.append(int(best[chain[-1]]))
    return np.float32(C[e] / m), [int(rows[i]) for i in reversed(chain)], tie_decided


def window_dp(dist, rows, tie, min_gap, max_gap):
    """`group_dp` for one LONG group whose positions are 0, 1, 2, .. in the order of `rows` (no L x L tables): the admissible
    predecessors of the i-th row are rows[i - max_gap .. i - min_gap]."""
    rows = np.asarray(rows, dtype=np.int64)
    m, L = len(dist), len(rows)
    T = np.asarray(tie, dtype=np.int64)[rows]
    C = dist[0][rows].astype(np.float64)
    back = []
    for j in range(1, m):
        new = np.full(L, np.inf)
        best = np.full(L, -1, dtype=np.int64)
        dj = dist[j][rows].astype(np.float64)
        for i in range(L):
            a, b = max(0, i - max_gap), i - min_gap + 1
            if b <= a:
                continue
            w = C[a:b]
            cm = w.min()
            if not np.isfinite(cm):
                continue
            cand = a + np.flatnonzero(w == cm)
            p = cand[np.argmin(T[cand])]
            best[i], new[i] = p, C[p] + dj[i]
        C = new
        back.append(best)
    cand = np.flatnonzero(np.isfinite(C))
    if len(cand) == 0:
        return None
    e = cand[np.lexsort((T[cand], C[cand]))[0]]
    chain = [int(e)]
    for best in reversed(back):
        chain.append(int(best[chain[-1]]))
    return np.float32(C[e] / m), [int(rows[i]) for i in reversed(chain)]


def sequence_answer(dist, labels, pos, tie, min_gap, max_gap, k, allowed=None):
    """-> [(label, D, chain)] : the first k allowed groups that hold a chain by (D, label); and {label: tie_decided}."""
    labels = np.asarray(labels)
    out, decided = [], {}
    for g in range(int(labels.max()) + 1):
        if allowed is not None and g not in allowed:
            continue
        res = group_dp(dist, np.flatnonzero(labels == g), pos, tie, min_gap, max_gap)
        if res is not None:
            out.append((g, res[0], res[1]))
            decided[g] = res[2]
    out.sort(key=lambda t: (t[1], t[0]))
    return out[:k], decided, len(out)


def set_distance(dist, rows):
    """The clip search's D of one group: fp32(sum over the steps, in order, of the group's smallest distance / m)."""
    s = 0.0
    for d in dist:
        s += float(d[rows].min())
    return np.float32(s / len(dist))


def dense_labels(groups):
    index = {}
    return np.array([index.setdefault(g, len(index)) for g in groups], dtype=np.int32), list(index)


def _i32(a):
    return a.ctypes.data_as(POINTER(c_int32))


class Data:
    """One index and what the oracle needs about it: exported rows, tie ranks, dense labels.  Distances are cached per step list."""

    def __init__(self, vecs, ids, groups, positions, group_of=None, position_of=None):
        from video_quierer_amd.indexes.hnsw import OptimizedHNSWIndex
        self.ids, self.groups, self.positions = list(ids), list(groups), [int(p) for p in positions]
        self.group_of, self.position_of = group_of, position_of
        self.idx = OptimizedHNSWIndex(dimension=vecs.shape[1])
        self.idx.add_batch(vecs, ids)
        self.refresh()

    def refresh(self):
        self.stored = self.idx._export()
        self.tie = _tie_ranks(self.ids)
        self.labels, self.keys = dense_labels(self.groups)
        self._dist = {}

    def dist(self, unit):
        key = unit.tobytes()
        if key not in self._dist:
            self._dist[key] = [knn_oracle.distances(self.stored, q) for q in unit]
        return self._dist[key]

    def want(self, unit, min_gap, max_gap, k, allowed_keys=None):
        allowed = None if allowed_keys is None else {self.keys.index(a) for a in allowed_keys if a in self.keys}
        return sequence_answer(self.dist(unit), self.labels, self.positions, self.tie, min_gap, max_gap, k, allowed)

    def check(self, steps, min_gap, max_gap, k=10, within=None, exclude=None, tag=""):
        """The wrapper's answer against the restatement.  -> (the oracle's list, {label: tie_decided}, groups with a chain, stats)"""
        unit = _unit(steps)
        res = self.idx.search_sequence(list(steps), k, min_gap=min_gap, max_gap=max_gap, within=within, exclude=exclude,
                                       group_of=self.group_of, position_of=self.position_of)
        st = self.idx.last_search_stats()
        allowed = within if within is not None else (None if exclude is None else [g for g in self.keys if g not in set(exclude)])
        want, decided, holding = self.want(unit, min_gap, max_gap, k, allowed)
        tag = f"{tag} m {len(steps)} gaps ({min_gap}, {max_gap}) k {k} stats {st}"
        assert [r["group"] for r in res] == [self.keys[g] for g, _, _ in want], f"{tag}: groups differ"
        got = np.array([r["distance"] for r in res], dtype=np.float32)
        exp = np.array([d for _, d, _ in want], dtype=np.float32)
        print(f"{tag}: D got {got[:4]} want {exp[:4]}")
        assert np.array_equal(got.view(np.uint32), exp.view(np.uint32)), f"{tag}: distances differ"
        assert [r["chain"] for r in res] == [[self.ids[r] for r in c] for _, _, c in want], f"{tag}: chains differ"
        assert [r["positions"] for r in res] == [[self.positions[r] for r in c] for _, _, c in want], f"{tag}: positions differ"
        assert all(type(r["distance"]) is np.float32 and r["score"] == np.float32(1.0) - r["distance"] for r in res)
        for r in res:                                              # every chain is admissible
            dp = np.diff(np.array(r["positions"], dtype=np.int64))
            assert ((dp >= min_gap) & (dp <= max_gap)).all()
        assert st["verified"] == holding, f"{tag}: stats[0] is the number of groups that hold a chain"
        return want, decided, holding, st


def noisy_steps(rows, frames, seed, noise=0.3):
    """The given stored rows plus Gaussian noise of norm ~ `noise`, not normalised (the wrapper does that)."""
    rng = np.random.default_rng([seed, 7])
    dim = rows.shape[1]
    return [(rows[f] + rng.standard_normal(dim).astype(np.float32) * np.float32(noise / math.sqrt(dim))) * np.float32(2.0) for f in frames]


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


# ---- 1. planted forward, reversed and strided videos ----
def planted_rows(dim=256, seed=1001):
    """~4,000 background rows, then video A (64 frames), B = A reversed, C = every second frame of A.
    -> rows, video, frame, (first row of A, of B, of C)"""
    base, video, frame = video_rows(4_000, dim, seed=seed, lengths=[1, 7, 63, 64, 65, 300])
    a, _, _ = video_rows(64, dim, seed=seed + 1, lengths=[64])
    rows = np.concatenate([base, a, a[::-1], a[::2]])
    v0 = max(video) + 1
    video = list(video) + [v0] * 64 + [v0 + 1] * 64 + [v0 + 2] * 32
    frame = list(frame) + list(range(64)) + list(range(64)) + list(range(32))
    return np.ascontiguousarray(rows), video, frame, (4_000, 4_064, 4_128)


def planted():
    def build():
        rows, video, frame, starts = planted_rows()
        d = Data(rows, list(range(len(rows))), video, frame, group_of=video.__getitem__, position_of=frame.__getitem__)
        d.rows, d.starts = rows, starts
        return d
    return cached("planted", build)


PLANTED_STEPS = [(2, 3), (2, 5), (4, 3), (4, 5), (8, 3), (8, 5), (16, 3)]      # (m, stride): 16 x 5 does not fit 64 frames
PLANTED_GAPS = [(1, 8), (1, 4), (1, BIG_GAP), (3, 8)]


def planted_oracle(d, m, stride, min_gap, max_gap):
    """The oracle's own numbers: the clip-search D of A and B are bit-equal, the sequence D are not, A is ahead."""
    a0, b0, c0 = d.starts
    steps = noisy_steps(d.rows, [a0 + 2 + stride * j for j in range(m)], seed=m * 10 + stride)
    dist = d.dist(_unit(steps))
    va, vb = d.labels[a0], d.labels[b0]
    ra, rb = np.flatnonzero(d.labels == va), np.flatnonzero(d.labels == vb)
    assert set_distance(dist, ra).tobytes() == set_distance(dist, rb).tobytes(), "the clip search cannot tell A from B"
    seq_a = group_dp(dist, ra, d.positions, d.tie, min_gap, max_gap)
    seq_b = group_dp(dist, rb, d.positions, d.tie, min_gap, max_gap)
    assert seq_a is not None and seq_b is not None
    assert seq_a[0] < seq_b[0], f"the sequence search must rank the forward video ahead: {seq_a[0]} vs {seq_b[0]}"
    return steps, va, vb, seq_a[0], seq_b[0]


@GPU
@pytest.mark.parametrize("min_gap,max_gap", PLANTED_GAPS)
@pytest.mark.parametrize("m,stride", PLANTED_STEPS)
def test_planted_forward_reversed_and_strided_videos(gpu_lib, m, stride, min_gap, max_gap):
    d = planted()
    steps, va, vb, da, db = planted_oracle(d, m, stride, min_gap, max_gap)
    want, _, _, _ = d.check(steps, min_gap, max_gap, k=len(d.keys), tag="planted")
    order = [g for g, _, _ in want]
    assert order.index(va) < order.index(vb)
    if min_gap <= stride <= max_gap:                               # the clip's own frames are an admissible chain: A leads
        assert order[0] == va, (order[:3], da, db)


# ---- 2. group lengths on both sides of everything ----
def lengths_data():
    def build():
        rows, video, frame = video_rows(4_820, 256, seed=2002, lengths=LENGTHS)      # four rounds of LENGTHS
        d = Data(rows, list(range(len(rows))), video, frame, group_of=video.__getitem__, position_of=frame.__getitem__)
        d.rows, d.video, d.frame = rows, video, frame
        return d
    return cached("lengths", build)


def lengths_steps(d, m, seed=3):
    """m frames of the first 300-row video at a stride of 2 (m = 64: 128 frames), plus noise."""
    first = next(r for r in range(len(d.video)) if d.video.count(d.video[r]) == 300)
    return noisy_steps(d.rows, [first + 5 + 2 * j for j in range(m)], seed=seed + m)


LENGTH_CASES = [(1, 1, 1), (2, 1, 1), (2, 1, 200), (2, 100, BIG_GAP), (3, 2, 5), (3, 1, 200), (3, 100, BIG_GAP), (8, 1, 1), (8, 1, 3),
                (8, 1, 200), (8, 30, 200), (64, 1, 1), (64, 1, 3), (64, 1, 200), (64, 4, 200)]


@GPU
@pytest.mark.parametrize("m,min_gap,max_gap", LENGTH_CASES)
def test_group_lengths_around_m_a_wave_and_the_blocks(gpu_lib, m, min_gap, max_gap):
    d = lengths_data()
    want, _, holding, st = d.check(lengths_steps(d, m), min_gap, max_gap, k=len(d.keys), tag="lengths")
    if m > 1:                                                      # (one step: every group holds a chain)
        assert 0 < holding < len(d.keys), "some group has no chain and some group has one"
    else:
        assert holding == len(d.keys)
    assert st["rescanned"] == 0 and st["exact_fallback"] == 1      # no global form, one chunk


# ---- 3. positions of the caller's choosing, shuffled labels, string ids, planted ties ----
def ties_rows(seed=3003):
    """3,900 rows of 300-row videos in shuffled row order; string ids "v{video}_{frame}".  In video 3 the row of frame 100 is
    a copy of the row of frame 99: chains through either cost the same and "v3_100" sorts before "v3_99"."""
    rows, video, frame = video_rows(3_900, 256, seed=seed, lengths=[300])
    rows[3 * 300 + 100] = rows[3 * 300 + 99]
    perm = np.random.default_rng(seed + 1).permutation(len(rows))
    return np.ascontiguousarray(rows[perm]), [video[i] for i in perm], [frame[i] for i in perm]


def ties_data():
    def build():
        rows, video, frame = ties_rows()
        ids = [f"v{v}_{f}" for v, f in zip(video, frame)]
        d = Data(rows, ids, [f"v{v}" for v in video], frame)
        d.rows, d.video, d.frame = rows, video, frame
        d.row_of = {i: r for r, i in enumerate(ids)}
        return d
    return cached("ties", build)


def _variant(d, name):
    f = d.frame
    if name == "frames":
        return list(f)
    if name == "repeated":                                         # three rows share every position
        return [x // 3 for x in f]
    if name == "scrambled":                                        # not monotone in frame order either
        return [(x // 8) * 8 + (x * 3) % 8 for x in f]
    if name == "negative":
        return [x - 1000 for x in f]
    assert name == "ends"                                          # odd frames at the bottom, even ones at the top of int32
    return [(-2 ** 31 + x) if x % 2 else (2 ** 31 - 300 + x) for x in f]


@GPU
@pytest.mark.parametrize("variant,gaps", [("frames", [(1, 8), (3, 8)]), ("repeated", [(1, 3), (1, 1)]), ("scrambled", [(1, 8)]),
                                          ("negative", [(1, 8)]), ("ends", [(2, 8), (2 ** 32 - 400, 2 ** 32), (1, BIG_GAP)])])
def test_positions_ties_and_shuffled_labels(gpu_lib, variant, gaps):
    d = ties_data()
    positions = _variant(d, variant)
    d.positions, d.position_of = positions, (lambda nid, p=positions, ro=d.row_of: p[ro[nid]])
    # steps around the planted copy: frames 81, 84, .. of video 3 (the seventh is frame 99), each used twice in `repeated`
    frames = [81 + 3 * j for j in range(10)]
    if variant == "repeated":
        frames = [f for f in frames[:5] for _ in (0, 1)]
    steps = noisy_steps(d.rows, [d.row_of[f"v3_{f}"] for f in frames], seed=33)
    for min_gap, max_gap in gaps:
        use = steps[:2] if min_gap > 2 ** 31 else steps            # (positions increase: only one jump across the range fits)
        want, decided, holding, _ = d.check(use, min_gap, max_gap, k=5, tag=f"ties/{variant}")
        assert holding > 0
        if variant == "frames":
            assert any(decided.values()), "some p* or end row is decided by the tie"
            v3 = d.keys.index("v3")
            assert decided[v3] and want[0][0] == v3
            # both copies are admissible for the step that follows them; the chain takes the one of the smaller id
            if min_gap == 1:                                       # (from 100 to the next step's 102 is a gap of 2)
                assert d.row_of["v3_100"] in want[0][2] and d.row_of["v3_99"] not in want[0][2], [d.ids[r] for r in want[0][2]]
        if variant == "repeated":                                  # two rows at one position never follow each other
            for _, _, chain in want:
                assert len({positions[r] for r in chain}) == len(chain)
        if min_gap > 2 ** 31:                                      # bottom of int32 -> top: a 32-bit difference would be negative
            assert all(positions[c[0]] < 0 < positions[c[1]] for _, _, c in want)


# ---- 4. dims, and un-normalised steps through the C ABI ----
def c_sequence(gpu_lib, h, steps, k, min_gap, max_gap, sel=None, exclude=1, chains=True):
    steps = np.ascontiguousarray(steps, dtype=np.float32)
    m = len(steps)
    g = np.full(k, -7, np.int32); dd = np.full(k, -7, np.float32); ch = np.full((k, m), -7, np.int32)
    sel = np.asarray([] if sel is None else sel, dtype=np.int32)
    rc = gpu_lib.load().vq_index_search_sequence(h, gpu_lib.fptr(steps), m, k, c_int64(min_gap), c_int64(max_gap), _i32(sel), len(sel),
                                                 exclude, _i32(g), gpu_lib.fptr(dd), _i32(ch) if chains else None)
    return rc, g, dd, ch


def assert_c_answer(g, dd, ch, want, k):
    nw = len(want)
    assert g[:nw].tolist() == [w[0] for w in want]
    assert np.array_equal(dd[:nw].view(np.uint32), np.array([w[1] for w in want], np.float32).view(np.uint32)), (dd[:nw], [w[1] for w in want])
    assert ch[:nw].tolist() == [w[2] for w in want]
    assert (g[nw:] == -1).all() and np.isposinf(dd[nw:]).all() and (ch[nw:] == -1).all()


@GPU
@pytest.mark.parametrize("dim", [192, 256, 512, 768])
def test_dims_and_unnormalised_steps(gpu_lib, dim):
    rows, video, frame = video_rows(1_205, dim, seed=4000 + dim, lengths=LENGTHS)
    d = Data(rows, list(range(len(rows))), video, frame, group_of=video.__getitem__, position_of=frame.__getitem__)
    try:
        first = next(r for r in range(len(video)) if video.count(video[r]) == 300)
        steps = noisy_steps(rows, [first + 4 + 3 * j for j in range(8)], seed=dim)
        d.check(steps, 1, 8, k=7, tag=f"dim {dim}")                # labels, positions on the device
        for q2 in (1e-4, 1e2):                                     # |q|^2: costs of 1 -+ 0.01 and of -9 .. 11, sums that round
            raw = np.ascontiguousarray(_unit(steps) * np.float32(math.sqrt(q2)))
            dist = [knn_oracle.distances(d.stored, q) for q in raw]
            if q2 > 1:
                assert min(float(x.min()) for x in dist) < 0, "negative costs occur"
            want, _, holding = sequence_answer(dist, d.labels, d.positions, d.tie, 1, 8, 7)
            rc, g, dd, ch = c_sequence(gpu_lib, d.idx._h, raw, 7, 1, 8)
            gpu_lib.check(rc)
            assert_c_answer(g, dd, ch, want, 7)
            assert d.idx.last_search_stats()["verified"] == holding
    finally:
        d.idx.close()


# ---- 5. forced boundaries: the global form, several step chunks, the sliced chain redo ----
@GPU
@pytest.mark.parametrize("m,min_gap,max_gap", [(8, 1, 3), (8, 1, 200), (3, 100, BIG_GAP), (64, 1, 200)])
def test_forced_boundaries_give_the_same_answers(gpu_lib, monkeypatch, m, min_gap, max_gap):
    d = lengths_data()
    steps = lengths_steps(d, m)
    kw = dict(min_gap=min_gap, max_gap=max_gap, group_of=d.group_of, position_of=d.position_of)
    plain = d.idx.search_sequence(steps, 12, **kw)
    ld = (len(d.ids) + 63) // 64 * 64

    monkeypatch.setenv("VQ_AMD_SEQ_LDS_ROWS", "128")               # the 300- and 700-row groups take the global form
    _, _, _, st = d.check(steps, min_gap, max_gap, k=12, tag="forced global")
    assert st["rescanned"] == 8 and st["exact_fallback"] == 1, st
    assert d.idx.search_sequence(steps, 12, **kw) == plain
    monkeypatch.delenv("VQ_AMD_SEQ_LDS_ROWS")

    monkeypatch.setenv("VQ_AMD_SEQ_DIST_BYTES", str(3 * ld * 4))   # chunks of 3 steps
    _, _, _, st = d.check(steps, min_gap, max_gap, k=12, tag="forced chunks")
    assert st["exact_fallback"] == (m + 2) // 3 and st["rescanned"] == 0, st
    if m == 8:
        assert st["exact_fallback"] == 3
    assert d.idx.search_sequence(steps, 12, **kw) == plain

    monkeypatch.setenv("VQ_AMD_SEQ_LDS_ROWS", "128")               # both at once, and the chains by the sliced redo
    monkeypatch.setenv("VQ_AMD_SEQ_BP_BYTES", str(2 * len(d.ids) * 4))
    _, _, _, st = d.check(steps, min_gap, max_gap, k=12, tag="forced all")
    assert st["rescanned"] == 8 and st["exact_fallback"] == (m + 2) // 3
    assert d.idx.search_sequence(steps, 12, **kw) == plain


# ---- 6. consequences ----
@GPU
def test_one_step_is_the_grouped_search_and_the_clip_search_never_scores_worse(gpu_lib):
    d = lengths_data()
    lib, h = gpu_lib.load(), d.idx._h
    steps = lengths_steps(d, 8)
    d.check(steps, 1, 8, k=5)                                      # labels and positions are on the device
    unit = _unit(steps)
    G = len(d.keys)
    for k in (1, 10, G):
        for sel, excl in ((None, 1), ([3, 7, 8, 20, 30], 0), ([7, 8], 1)):
            rc, g, dd, ch = c_sequence(gpu_lib, h, unit[:1], k, 1, 8, sel, excl)
            gpu_lib.check(rc)
            gg = np.empty((1, k), np.int32); gr = np.empty((1, k), np.int32); gd = np.empty((1, k), np.float32)
            if sel is None:
                gpu_lib.check(lib.vq_index_search_grouped(h, gpu_lib.fptr(unit[:1]), 1, k, 1, _i32(gg), _i32(gr), gpu_lib.fptr(gd)))
            else:
                s = np.asarray(sel, np.int32)
                gpu_lib.check(lib.vq_index_search_grouped_filtered(h, gpu_lib.fptr(unit[:1]), 1, k, 1, _i32(s), len(s), excl, _i32(gg), _i32(gr),
                                                                   gpu_lib.fptr(gd)))
            assert np.array_equal(g, gg[0]) and np.array_equal(ch[:, 0], gr[0]) and np.array_equal(dd.view(np.uint32), gd[0].view(np.uint32))
    # D_seq(g) >= D_set(g), the clip search in its exact mode on the same steps
    for min_gap, max_gap in ((1, 8), (1, BIG_GAP), (2, 2)):
        rc, g, dd, _ = c_sequence(gpu_lib, h, unit, G, min_gap, max_gap)
        gpu_lib.check(rc)
        sg = np.empty(G, np.int32); sd = np.empty(G, np.float32)
        gpu_lib.check(lib.vq_index_search_set(h, gpu_lib.fptr(unit), len(unit), G, 1, None, 0, 1, _i32(sg), gpu_lib.fptr(sd), None))
        d_set = dict(zip(sg.tolist(), sd.tolist()))
        held = [(int(a), float(b)) for a, b in zip(g, dd) if a >= 0]
        assert held and all(b >= d_set[a] for a, b in held)
        assert any(b > d_set[a] for a, b in held)                  # (and the order constraint costs something somewhere)


# ---- 7. filter, lifetime, unused slots, the device form, repeatability ----
@GPU
def test_filter_within_exclude_and_the_empty_lists(gpu_lib):
    d = lengths_data()
    steps = lengths_steps(d, 3)
    keys = d.keys
    long_ones = [g for g in keys if d.groups.count(g) >= 63]
    d.check(steps, 1, 5, k=6, within=long_ones[:5] + [keys[0], keys[1]], tag="within")
    d.check(steps, 1, 5, k=6, exclude=long_ones[:3], tag="exclude")
    d.check(steps, 1, 5, k=6, within=long_ones[:2] + ["no such video"], tag="within unknown")
    assert d.idx.search_sequence(steps, 6, min_gap=1, max_gap=5, within=[], group_of=d.group_of, position_of=d.position_of) == []
    full = d.idx.search_sequence(steps, 6, min_gap=1, max_gap=5, group_of=d.group_of, position_of=d.position_of)
    assert d.idx.search_sequence(steps, 6, min_gap=1, max_gap=5, exclude=[], group_of=d.group_of, position_of=d.position_of) == full
    # the same two cases through the C ABI: nothing allowed -> every slot empty; nothing excluded -> the unfiltered call
    unit = _unit(steps)
    rc, g, dd, ch = c_sequence(gpu_lib, d.idx._h, unit, 6, 1, 5, [], 0)
    gpu_lib.check(rc)
    assert (g == -1).all() and np.isposinf(dd).all() and (ch == -1).all()
    rc, g, dd, ch = c_sequence(gpu_lib, d.idx._h, unit, 6, 1, 5, [], 1)
    gpu_lib.check(rc)
    assert_c_answer(g, dd, ch, d.want(unit, 1, 5, 6)[0], 6)
    rc, _, _, _ = c_sequence(gpu_lib, d.idx._h, unit, 6, 1, 5, [len(keys)], 0)
    assert rc < 0 and b"outside" in gpu_lib.load().vq_last_error()
    # k above the groups that hold a chain: unused slots (m = 64 leaves the groups of at least 64 rows)
    steps64 = lengths_steps(d, 64)
    u64 = _unit(steps64)
    want, _, holding = d.want(u64, 1, 3, len(keys))
    assert 0 < holding < len(keys)
    rc, g, dd, ch = c_sequence(gpu_lib, d.idx._h, u64, len(keys), 1, 3)
    gpu_lib.check(rc)
    assert_c_answer(g, dd, ch, want, len(keys))
    rc, g2, dd2, _ = c_sequence(gpu_lib, d.idx._h, u64, len(keys), 1, 3, chains=False)      # chain_rows = NULL
    gpu_lib.check(rc)
    assert np.array_equal(g, g2) and np.array_equal(dd.view(np.uint32), dd2.view(np.uint32))
    lib, h = gpu_lib.load(), d.idx._h
    q = np.zeros((65, 256), np.float32); og = np.empty(1025, np.int32); od = np.empty(1025, np.float32)
    for m, k, lo, hi in ((0, 5, 1, 8), (65, 5, 1, 8), (3, 0, 1, 8), (3, 1025, 1, 8), (3, 5, 0, 8), (3, 5, 9, 8)):
        rc = lib.vq_index_search_sequence(h, gpu_lib.fptr(q), m, k, c_int64(lo), c_int64(hi), None, 0, 1, _i32(og), gpu_lib.fptr(od), None)
        assert rc < 0, (m, k, lo, hi)


@GPU
def test_a_second_identical_call_gives_identical_bits(gpu_lib):
    d = lengths_data()
    unit = _unit(lengths_steps(d, 8))
    d.check(lengths_steps(d, 8), 1, 8, k=5)
    first = c_sequence(gpu_lib, d.idx._h, unit, 20, 1, 200)
    second = c_sequence(gpu_lib, d.idx._h, unit, 20, 1, 200)
    assert first[0] == 0 and second[0] == 0
    for a, b in zip(first[1:], second[1:]):
        assert a.tobytes() == b.tobytes()


@GPU
def test_device_form_on_a_caller_owned_stream(gpu_lib):
    d = lengths_data()
    lib, h = gpu_lib.load(), d.idx._h
    steps = lengths_steps(d, 8)
    d.check(steps, 1, 8, k=5)
    unit = _unit(steps)
    calls = [(10, 1, 8), (len(d.keys), 1, 200)]
    want = []
    for k, lo, hi in calls:
        rc, g, dd, ch = c_sequence(gpu_lib, h, unit, k, lo, hi)
        gpu_lib.check(rc)
        want.append((g, dd, ch))
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
        dq = dev(unit.nbytes)
        assert hip.hipMemcpy(dq, unit.ctypes.data_as(c_void_p), ctypes.c_size_t(unit.nbytes), 1) == 0
        outs = [(dev(k * 4), dev(k * 4), dev(k * len(unit) * 4)) for k, _, _ in calls]
        for (k, lo, hi), (dg, ddist, dch) in zip(calls, outs):     # back to back, nothing read back in between
            gpu_lib.check(lib.vq_index_search_sequence_device(h, dq, len(unit), k, c_int64(lo), c_int64(hi), None, 0, 1, dg, ddist, dch))
        assert hip.hipStreamSynchronize(stream) == 0
        for (dg, ddist, dch), (g, dd, ch) in zip(outs, want):
            for src, ref in ((dg, g), (ddist, dd), (dch, ch)):
                got = np.empty_like(ref)
                assert hip.hipMemcpy(got.ctypes.data_as(c_void_p), src, ctypes.c_size_t(got.nbytes), 2) == 0
                assert got.tobytes() == ref.tobytes()
    finally:
        d.idx.set_stream(0)
        for p in ptrs:
            hip.hipFree(p)
        hip.hipStreamDestroy(stream)


@GPU
def test_lifetime_of_labels_positions_and_the_order(gpu_lib):
    lib = gpu_lib.load()
    n, dim = 1_205, 256
    vecs, video, frame = video_rows(n + 300, dim, seed=7007, lengths=LENGTHS)
    video, frame = list(video), list(frame)
    ids = list(range(n + 300))
    d = Data(vecs[:n], ids[:n], video[:n], frame[:n], group_of=video.__getitem__, position_of=frame.__getitem__)
    try:
        h = d.idx._h
        first = next(r for r in range(n) if video.count(video[r]) >= 300)
        steps = noisy_steps(vecs, [first + 3 + 2 * j for j in range(4)], seed=70)
        unit = _unit(steps)
        d.check(steps, 1, 6, k=6, tag="fresh")
        d.idx.add_batch(vecs[n:], ids[n:])                         # stale after an add: refused, labels first
        rc, _, _, _ = c_sequence(gpu_lib, h, unit, 6, 1, 6)
        assert rc < 0 and b"labels" in lib.vq_last_error()
        lab, _ = dense_labels(video)
        gpu_lib.check(lib.vq_index_set_groups(h, _i32(lab), n + 300, int(lab.max()) + 1))
        rc, _, _, _ = c_sequence(gpu_lib, h, unit, 6, 1, 6)
        assert rc < 0 and b"positions" in lib.vq_last_error()
        pos = np.array(frame, dtype=np.int32)
        gpu_lib.check(lib.vq_index_set_positions(h, _i32(pos), n + 300))
        d.ids, d.groups, d.positions = ids, video, frame
        d.refresh()
        rc, g, dd, ch = c_sequence(gpu_lib, h, unit, 6, 1, 6)
        gpu_lib.check(rc)
        assert_c_answer(g, dd, ch, d.want(unit, 1, 6, 6)[0], 6)
        d.check(steps, 1, 6, k=6, tag="after add")                 # the wrapper uploads by itself
        d.idx.add_batch(vecs[first + 5:first + 6] * np.float32(-1.0), [first + 5])      # update_rows keeps labels and positions
        rc, _, _, _ = c_sequence(gpu_lib, h, unit, 6, 1, 6)
        gpu_lib.check(rc)
        d.refresh()
        d.check(steps, 1, 6, k=6, tag="after update")
        gone = list(range(first + 7, first + 40)) + [0, 5, n + 10]
        d.idx.remove_batch(gone)                                   # remove_rows drops the positions
        rc, _, _, _ = c_sequence(gpu_lib, h, unit, 6, 1, 6)
        assert rc < 0 and b"positions" in lib.vq_last_error()
        keep = [r for r in range(n + 300) if r not in set(gone)]
        d.ids = [ids[r] for r in keep]; d.groups = [video[r] for r in keep]; d.positions = [frame[r] for r in keep]
        d.refresh()
        d.check(steps, 1, 6, k=6, tag="after removal")
        d.check(steps, 1, 40, k=6, tag="after removal, across the hole")
    finally:
        d.idx.close()


# ---- 8. SimpleVideoIndex.search_storyboard ----
@GPU
def test_search_storyboard_on_fractional_timestamps(gpu_lib):
    from video_quierer_amd.overhaul_index import SimpleVideoIndex
    vecs, video, frame = video_rows(600, 512, seed=811, lengths=[150])
    rng = np.random.default_rng(812)
    names = [f"clip{v}.mp4" for v in video]
    stamps = [round(f * 0.4 + float(rng.uniform(0, 0.3)), 3) for f in frame]      # ~2.5 fps, jittered
    sv = SimpleVideoIndex()
    for e, nm, ts in zip(vecs, names, stamps):
        sv.add_frame(e, nm, ts)
    positions = [int(round(ts * 1000)) for ts in stamps]
    labels, keys = dense_labels(names)
    tie = -np.arange(600)                                          # search's tie rule: the larger frame id first
    stored = np.stack(sv.embeddings)
    steps = noisy_steps(vecs, [150 + 20 + 5 * j for j in range(4)], seed=81)       # clip1.mp4, two seconds apart
    unit = np.stack([(q / (np.linalg.norm(q) + 1e-10)).astype(np.float32) for q in steps])
    dist = [knn_oracle.distances(stored, q) for q in unit]
    for max_gap_s, min_gap_s in ((10.0, 0.0), (2.5, 1.0), (0.5, 0.0), (1000.0, 3.0)):
        lo, hi = max(1, math.ceil(min_gap_s * 1000)), math.floor(max_gap_s * 1000)
        want, _, _ = sequence_answer(dist, labels, positions, tie, lo, hi, 3)
        got = sv.search_storyboard(steps, 3, max_gap_s, min_gap_s)
        assert [r["video_name"] for r in got] == [keys[g] for g, _, _ in want], (max_gap_s, min_gap_s)
        assert [r["frame_ids"] for r in got] == [c for _, _, c in want]
        assert [r["timestamps"] for r in got] == [[stamps[r] for r in c] for _, _, c in want]
        assert [r["score"] for r in got] == [float(np.float32(1.0) - dd) for _, dd, _ in want]
    assert sv.search_storyboard(steps, 3, 10.0)[0]["video_name"] == "clip1.mp4"
    assert sequence_answer(dist, labels, positions, tie, 1, 500, 3)[0] != sequence_answer(dist, labels, positions, tie, 1, 10_000, 3)[0]


# ---- 9. one long group: the global form beyond 64 blocks of 64 rows ----
@GPU
def test_one_group_of_9000_rows_through_the_second_level_of_minima(gpu_lib):
    """9,000 rows above the LDS form's 4,096: ranges of up to 9,000 rows cover more than 64 whole blocks, so whole 4,096-row
    superblocks are read as one minimum.  Expected by `window_dp`, the restatement for positions 0, 1, 2, .. (checked against
    `group_dp` without a device)."""
    vecs, video, frame = video_rows(9_300, 192, seed=9009, lengths=[9_000, 300])
    d = Data(vecs, list(range(len(vecs))), video, frame, group_of=video.__getitem__, position_of=frame.__getitem__)
    try:
        rows0 = np.arange(9_000)
        steps = noisy_steps(vecs, [100, 4_500, 8_900], seed=99, noise=1.0)      # far apart, noisy: the best predecessor is anywhere
        unit = _unit(steps)
        dist = d.dist(unit)
        for min_gap, max_gap in ((1, BIG_GAP), (1, 6_000), (4_200, 4_400), (70, 4_200)):
            res = d.idx.search_sequence(steps, 2, min_gap=min_gap, max_gap=max_gap, group_of=d.group_of, position_of=d.position_of)
            st = d.idx.last_search_stats()
            assert st["rescanned"] == 1, st                        # one group in the global form
            want = window_dp(dist, rows0, d.tie, min_gap, min(max_gap, 10_000))
            small = group_dp(dist, np.arange(9_000, 9_300), d.positions, d.tie, min_gap, max_gap)
            by_group = {r["group"]: r for r in res}
            assert (1 in by_group) == (small is not None)
            got = by_group[0]
            print(f"long group gaps ({min_gap}, {max_gap}): D got {got['distance']} want {want[0]} chain {got['chain']}")
            assert got["distance"].tobytes() == want[0].tobytes() and got["chain"] == want[1]
            if small is not None:
                assert by_group[1]["distance"].tobytes() == small[0].tobytes() and by_group[1]["chain"] == small[1]
    finally:
        d.idx.close()
