"""Span search (vq_index_search_spans / HNSWIndex.search_spans / SimpleVideoIndex.search_spans): per query the k videos with
the best time span.  The expected answer is the definition restated in numpy (tests/span_ref.py, `span_answer` over `span_scan`,
which tests/test_span_search_cpu.py holds against the O(L^2) `span_brute`) over the C oracle's exact distances on the exported
rows, with row ties by `_tie_ranks` of the ids; groups, the bits of D, masses, lengths and the start, end and peak rows must
match exactly.

The rows are video-like (consecutive frames are near-duplicates), as tests/test_distinct_search.py makes them."""
import ctypes
import math
from ctypes import POINTER, byref, c_float, c_int32, c_int64, c_void_p

import numpy as np
import pytest

from oracle import knn_oracle
from span_ref import NO_LIMIT, gains, rank_value, span_answer
from test_distinct_search import _unit, video_rows
from test_sequence_search import Data, dense_labels, noisy_steps

GPU = pytest.mark.gpu
LENGTHS = [1, 2, 3, 7, 63, 64, 65, 300, 700]        # single rows, both sides of a wave and of a 64-row block, several tiles of 256


def _i32(a):
    return a.ctypes.data_as(POINTER(c_int32))


def c_spans(gpu_lib, h, queries, k, tau, max_gap=NO_LIMIT, max_span=NO_LIMIT, sel=None, exclude=1, extras=True):
    """The C call.  -> rc, groups [nq][k], D [nq][k], masses, lengths, rows [nq][k][3] (the last three None without `extras`)"""
    q = np.ascontiguousarray(queries, dtype=np.float32)
    nq = len(q)
    g = np.full((nq, k), -7, np.int32); dd = np.full((nq, k), -7, np.float32)
    m = np.full((nq, k), -7, np.int64); ln = np.full((nq, k), -7, np.int32); rows = np.full((nq, k, 3), -7, np.int32)
    sel = np.asarray([] if sel is None else sel, dtype=np.int32)
    rc = gpu_lib.load().vq_index_search_spans(h, gpu_lib.fptr(q), nq, k, c_float(float(tau)), c_int64(max_gap), c_int64(max_span), _i32(sel),
                                              len(sel), exclude, _i32(g), gpu_lib.fptr(dd),
                                              m.ctypes.data_as(POINTER(c_int64)) if extras else None, _i32(ln) if extras else None,
                                              _i32(rows) if extras else None)
    return (rc, g, dd, m, ln, rows) if extras else (rc, g, dd, None, None, None)


def assert_c_answer(got, want, k, tag=""):
    """got: c_spans' arrays; want: span_answer's per-query tuples"""
    _, g, dd, m, ln, rows = got
    for i, (ans, _, _, _) in enumerate(want):
        nw = len(ans)
        exp_d = np.array([a[1] for a in ans], np.float32)
        print(f"{tag} query {i}: groups got {g[i][:4].tolist()} want {[a[0] for a in ans][:4]}; D got {dd[i][:4]} want {exp_d[:4]}")
        assert g[i][:nw].tolist() == [a[0] for a in ans], f"{tag} query {i}: groups differ"
        assert np.array_equal(dd[i][:nw].view(np.uint32), exp_d.view(np.uint32)), f"{tag} query {i}: D differs"
        assert (g[i][nw:] == -1).all() and np.isposinf(dd[i][nw:]).all()
        if m is not None:
            assert m[i][:nw].tolist() == [a[2] for a in ans], f"{tag} query {i}: masses differ"
            assert ln[i][:nw].tolist() == [a[3] for a in ans], f"{tag} query {i}: lengths differ"
            assert rows[i][:nw].tolist() == [list(a[4]) for a in ans], f"{tag} query {i}: start / end / peak rows differ"
            assert (m[i][nw:] == 0).all() and (ln[i][nw:] == 0).all() and (rows[i][nw:] == -1).all()


def want_for(d, unit, tau, max_gap, max_span, k, allowed=None):
    return span_answer(d.dist(unit), d.labels, d.positions, d.tie, tau, max_gap, max_span, k, allowed)


def upload(d, positions=None):
    """Labels, ranks and positions go to the device through the wrapper (one tiny call); `positions`: per row, replaces d's."""
    if positions is not None:
        positions = [int(p) for p in positions]
        d.positions, d.position_of = positions, (lambda nid, p=positions, ro=d.row_of: p[ro[nid]])
    q = np.ones(d.idx.dimension, np.float32)
    d.idx.search_spans(q, 1, max_distance=-10.0, group_of=d.group_of, position_of=d.position_of)


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


# ---- 1. video-like rows: every group length, every limit, tau across the distances ----
def lengths_data():
    def build():
        rows, video, frame = video_rows(sum(LENGTHS), 512, seed=5005, lengths=LENGTHS)      # one round of LENGTHS: nine groups
        d = Data(rows, list(range(len(rows))), video, frame, group_of=video.__getitem__)
        d.rows, d.video, d.frame = rows, video, frame
        d.row_of = {i: i for i in range(len(rows))}
        first = {ln: video.index(v) for v, ln in enumerate(LENGTHS)}
        # queries near a frame of the 700-, the 300- and the 63-row video, then two more for the chunked call
        d.queries = _unit(noisy_steps(rows, [first[700] + 350, first[300] + 100, first[63] + 30, first[65] + 10, first[700] + 600], seed=55))
        return d
    return cached("lengths", build)


def _positions(d, name):
    f = d.frame
    if name == "frames":
        return list(f)
    if name == "holes":                                            # a hole of 51 positions behind every 40 frames
        return [x + 50 * (x // 40) for x in f]
    assert name == "dups"                                          # three rows share every position
    return [x // 3 for x in f]


def _tau(d, unit, which):
    flat = np.sort(np.concatenate(d.dist(unit)))
    if which == "below":
        return np.float32(np.nextafter(flat[0], np.float32(-np.inf)))
    return np.float32(flat[min(len(flat) - 1, int(which * (len(flat) - 1)))])      # an exact distance of some row: zero gains occur


LIMIT_CASES = [("frames", NO_LIMIT, NO_LIMIT), ("holes", 5, NO_LIMIT), ("holes", 2 ** 32, 2 ** 33), ("frames", NO_LIMIT, 0), ("frames", NO_LIMIT, 5),
               ("frames", NO_LIMIT, 200), ("dups", NO_LIMIT, 5), ("dups", 0, NO_LIMIT), ("holes", 60, 200)]


@GPU
@pytest.mark.parametrize("which", [0.05, 0.30, 1.0, "below"])
@pytest.mark.parametrize("variant,max_gap,max_span", LIMIT_CASES)
def test_video_like_rows_every_limit(gpu_lib, variant, max_gap, max_span, which):
    d = lengths_data()
    upload(d, _positions(d, variant))
    unit = d.queries[:3]
    tau = _tau(d, unit, which)
    G = len(d.keys)
    full = want_for(d, unit, tau, max_gap, max_span, G + 3)
    free = want_for(d, unit, tau, NO_LIMIT, NO_LIMIT, G + 3)
    holding = sum(w[2] for w in full)
    # not vacuous, on the restatement alone
    if which == "below":
        assert holding == 0
    if which == 0.30:
        assert all(w[2] >= 2 for w in full), "at least two groups hold a span for every query"
    if which in (0.30, 1.0) and (max_gap < 2 ** 32 or max_span < 2 ** 32):
        cut = sum(a[1:] != b[1:] for wf, wu in zip(full, free) for a in wf[0] for b in wu[0] if a[0] == b[0])
        assert cut >= 1, "some span is cut by the limit"
    if which == 1.0 and max_gap >= 2 ** 32 and max_span >= 2 ** 32:
        assert all(w[2] >= G - 1 for w in full)                    # every gain >= 0: every group but one whose only row is the farthest
    for k in (1, 4, G + 3):
        got = c_spans(gpu_lib, d.idx._h, unit, k, tau, max_gap, max_span)
        gpu_lib.check(got[0])
        assert_c_answer(got, [(w[0][:k],) + w[1:] for w in full], k, tag=f"{variant} gap {max_gap} span {max_span} tau {tau} k {k}")
        st = d.idx.last_search_stats()
        assert st == {"verified": holding, "rescanned": 0, "exact_fallback": 1}, st       # no global form, one chunk
        short = c_spans(gpu_lib, d.idx._h, unit, k, tau, max_gap, max_span, extras=False)   # the optional outputs NULL
        gpu_lib.check(short[0])
        assert short[1].tobytes() == got[1].tobytes() and short[2].tobytes() == got[2].tobytes()


# ---- 2. the same rows through the global form and in several query chunks ----
@GPU
@pytest.mark.parametrize("variant,max_gap,max_span", LIMIT_CASES)
def test_forced_global_form_and_query_chunks_give_the_same_bits(gpu_lib, monkeypatch, variant, max_gap, max_span):
    d = lengths_data()
    upload(d, _positions(d, variant))
    unit = d.queries
    G = len(d.keys)
    ld = (len(d.ids) + 63) // 64 * 64
    for which in (0.05, 0.30, 1.0):
        tau = _tau(d, unit, which)
        want = want_for(d, unit, tau, max_gap, max_span, G)
        holding = sum(w[2] for w in want)
        plain = c_spans(gpu_lib, d.idx._h, unit, G, tau, max_gap, max_span)
        gpu_lib.check(plain[0])
        assert_c_answer(plain, want, G, tag="plain")

        monkeypatch.setenv("VQ_AMD_SPAN_LDS_ROWS", "64")           # the groups of 65, 300 and 700 rows take the global form
        forced = c_spans(gpu_lib, d.idx._h, unit, G, tau, max_gap, max_span)
        gpu_lib.check(forced[0])
        assert d.idx.last_search_stats() == {"verified": holding, "rescanned": 3, "exact_fallback": 1}
        assert all(a.tobytes() == b.tobytes() for a, b in zip(forced[1:], plain[1:])), "the global form's bits are the LDS form's"

        monkeypatch.setenv("VQ_AMD_SPAN_DIST_BYTES", str(2 * ld * 4))     # five queries: chunks of 2, 2 and 1
        both = c_spans(gpu_lib, d.idx._h, unit, G, tau, max_gap, max_span)
        gpu_lib.check(both[0])
        assert d.idx.last_search_stats() == {"verified": holding, "rescanned": 3, "exact_fallback": 3}
        assert all(a.tobytes() == b.tobytes() for a, b in zip(both[1:], plain[1:]))
        monkeypatch.delenv("VQ_AMD_SPAN_LDS_ROWS")
        chunked = c_spans(gpu_lib, d.idx._h, unit, G, tau, max_gap, max_span)
        gpu_lib.check(chunked[0])
        assert d.idx.last_search_stats() == {"verified": holding, "rescanned": 0, "exact_fallback": 3}
        assert all(a.tobytes() == b.tobytes() for a, b in zip(chunked[1:], plain[1:]))
        monkeypatch.delenv("VQ_AMD_SPAN_DIST_BYTES")


# ---- 3. the boundary between the forms at full size, and ranges above 64 whole blocks ----
def boundary_data():
    def build():
        rows, video, frame = video_rows(4_096 + 4_097 + 9_000, 64, seed=6006, lengths=[4_096, 4_097, 9_000])
        d = Data(rows, list(range(len(rows))), video, frame, group_of=video.__getitem__)
        d.rows, d.video, d.frame = rows, video, frame
        d.row_of = {i: i for i in range(len(rows))}
        d.queries = _unit(noisy_steps(rows, [2_000, 4_096 + 4_000, 8_193 + 5], seed=66, noise=1.0))
        return d
    return cached("boundary", build)


@GPU
@pytest.mark.parametrize("variant,max_gap,max_span", [("frames", NO_LIMIT, NO_LIMIT), ("frames", NO_LIMIT, 100), ("jump", 10, NO_LIMIT),
                                                      ("jump", 10, 6_000)])
def test_groups_of_4096_and_4097_rows_and_ranges_above_64_blocks(gpu_lib, variant, max_gap, max_span):
    """4,096 rows: the LDS form at its limit; 4,097 and 9,000: the global form.  `jump`: a hole behind the fifth frame, so every
    later range starts at 5 and covers up to 63 (LDS form) or 140 (global form: whole 4,096-row superblocks) whole blocks."""
    d = boundary_data()
    upload(d, d.frame if variant == "frames" else [x + (1_000 if x >= 5 else 0) for x in d.frame])
    unit = d.queries
    flat = np.sort(np.concatenate(d.dist(unit)))
    for tau in (np.float32(flat[len(flat) // 2]), np.float32(flat[len(flat) // 20])):
        want = want_for(d, unit, tau, max_gap, max_span, 3)
        assert sum(w[2] for w in want) >= 3
        got = c_spans(gpu_lib, d.idx._h, unit, 3, tau, max_gap, max_span)
        gpu_lib.check(got[0])
        assert_c_answer(got, want, 3, tag=f"boundary {variant} span {max_span} tau {tau}")
        st = d.idx.last_search_stats()
        assert st["rescanned"] == 2 and st["exact_fallback"] == 1 and st["verified"] == sum(w[2] for w in want), st


# ---- 4. plateaus: equal gains, equal masses, equal D ----
def plateau_data():
    """dim 64, q = e_0.  `near` rows lie around q (d ~ 0.05 .. 0.15), `far` rows around -q (d ~ 2).
       groups 0 and 1: the same ten near rows, bit for bit -> equal D, the smaller label first
       group 2: the ten rows, five far rows, the ten rows again -> two spans of equal mass and length, the earlier wins
       group 3: ten other near rows, then z (d ~ 0.3): with tau = d(q, z) the row z has zero gain at the span's edge
       group 4: three far rows: never holds a span below tau = 1"""
    def build():
        rng = np.random.default_rng(7007)
        q = np.zeros(64, np.float32); q[0] = 1

        def around(c, n, noise):
            x = c[None, :] + rng.standard_normal((n, 64)).astype(np.float32) * np.float32(noise / 8)
            return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)
        near, other, far, z = around(q, 10, 0.4), around(q, 10, 0.4), around(-q, 8, 0.4), around(q, 1, 0.9)
        rows = np.concatenate([near, near, near, far[:5], near, other, z, far[5:]])
        video = [0] * 10 + [1] * 10 + [2] * 25 + [3] * 11 + [4] * 3
        frame = list(range(10)) + list(range(10)) + list(range(25)) + list(range(11)) + list(range(3))
        d = Data(np.ascontiguousarray(rows), list(range(len(rows))), video, frame, group_of=video.__getitem__)
        d.row_of = {i: i for i in range(len(rows))}
        d.q, d.z_row = q[None, :], 55
        return d
    return cached("plateau", build)


@GPU
def test_tie_plateaus(gpu_lib):
    d = plateau_data()
    upload(d, d.positions)
    dist = d.dist(d.q)[0]
    assert dist[:10].tobytes() == dist[10:20].tobytes() == dist[20:30].tobytes() == dist[35:45].tobytes()
    # tau = 0.5: groups 0 and 1 tie in D; group 2's two runs tie in mass and length
    (ans, decided, holding, group_tie), = want = want_for(d, d.q, np.float32(0.5), NO_LIMIT, NO_LIMIT, 5)
    assert holding == 4 and group_tie and decided[2] and not decided[0]
    ans = [a for a in ans if a[0] != 3]
    by = {a[0]: a for a in ans}
    assert by[0][1].tobytes() == by[1][1].tobytes() == by[2][1].tobytes() and [a[0] for a in ans[:3]] == [0, 1, 2]
    assert by[2][4][:2] == (20, 29) and by[2][3] == 10            # the first of the two runs
    got = c_spans(gpu_lib, d.idx._h, d.q, 5, np.float32(0.5))
    gpu_lib.check(got[0])
    assert_c_answer(got, want, 5, tag="plateau 0.5")
    # a limit that cuts every run of ten to the same best window: still equal, still the earlier
    want = want_for(d, d.q, np.float32(0.5), NO_LIMIT, 3, 5)
    assert want[0][3] and want[0][1][2]
    got = c_spans(gpu_lib, d.idx._h, d.q, 5, np.float32(0.5), NO_LIMIT, 3)
    gpu_lib.check(got[0])
    assert_c_answer(got, want, 5, tag="plateau span 3")
    # tau = d(q, z) exactly: z has zero gain behind the ten rows of group 3; both ends give the same mass, the shorter span wins
    tau = np.float32(dist[d.z_row])
    assert gains(dist[d.z_row:d.z_row + 1], tau)[0] == 0 and (dist[45:55] < tau).all()
    (ans, decided, _, _), = want = want_for(d, d.q, tau, NO_LIMIT, NO_LIMIT, 5)
    by = {a[0]: a for a in ans}
    assert decided[3] and by[3][4][:2] == (45, 54) and by[3][3] == 10
    got = c_spans(gpu_lib, d.idx._h, d.q, 5, tau)
    gpu_lib.check(got[0])
    assert_c_answer(got, want, 5, tag="plateau zero gain")


# ---- 5. consequences ----
@GPU
def test_max_span_zero_is_the_grouped_search_below_tau(gpu_lib):
    d = lengths_data()
    upload(d, _positions(d, "frames"))                             # distinct positions inside every group
    lib, h = gpu_lib.load(), d.idx._h
    unit = d.queries[:3]
    G = len(d.keys)
    for which in (0.05, 0.30, 1.0):
        tau = _tau(d, unit, which)
        got = c_spans(gpu_lib, h, unit, G, tau, NO_LIMIT, 0)
        gpu_lib.check(got[0])
        gg = np.empty((3, G), np.int32); gr = np.empty((3, G), np.int32); gd = np.empty((3, G), np.float32)
        gpu_lib.check(lib.vq_index_search_grouped(h, gpu_lib.fptr(unit), 3, G, 1, _i32(gg), _i32(gr), gpu_lib.fptr(gd)))
        for i in range(3):
            keep = gd[i] < tau                                     # the grouped search's list, restricted to best distances below tau
            n = int(keep.sum())
            assert n >= 1 and got[1][i][:n].tolist() == gg[i][keep].tolist() and (got[1][i][n:] == -1).all()
            assert got[5][i][:n, 2].tolist() == gr[i][keep].tolist()                       # the peak rows
            assert (got[5][i][:n, 0] == got[5][i][:n, 2]).all() and (got[5][i][:n, 1] == got[5][i][:n, 2]).all() and (got[4][i][:n] == 1).all()
            assert got[3][i][:n].tolist() == gains(gd[i][keep], tau).tolist()              # S = w of that row
            assert got[2][i][:n].tobytes() == np.array([rank_value(s) for s in got[3][i][:n]], np.float32).tobytes()


@GPU
def test_large_tau_takes_every_group_whole_and_small_tau_nothing(gpu_lib):
    d = lengths_data()
    upload(d, _positions(d, "holes"))
    h = d.idx._h
    unit = d.queries[:3]
    G = len(d.keys)
    tau = np.float32(4.0)
    got = c_spans(gpu_lib, h, unit, G, tau, 2 ** 32, 2 ** 62)
    gpu_lib.check(got[0])
    assert_c_answer(got, want_for(d, unit, tau, NO_LIMIT, NO_LIMIT, G), G, tag="tau 4")
    for i in range(3):
        w = gains(d.dist(unit)[i], tau)
        assert (w > 0).all()
        assert sorted(got[1][i].tolist()) == list(range(G))
        for g, s, ln in zip(got[1][i], got[3][i], got[4][i]):
            rows = np.flatnonzero(d.labels == g)
            assert ln == len(rows) and s == int(w[rows].sum())     # all of its rows, the plain sum
    below = _tau(d, unit, "below")
    got = c_spans(gpu_lib, h, unit, G, below)
    gpu_lib.check(got[0])
    assert (got[1] == -1).all() and np.isposinf(got[2]).all() and (got[3] == 0).all() and (got[4] == 0).all() and (got[5] == -1).all()
    assert d.idx.last_search_stats()["verified"] == 0


# ---- 6. filters ----
@GPU
def test_filter_within_exclude_and_the_empty_lists(gpu_lib):
    d = lengths_data()
    upload(d, _positions(d, "frames"))
    h = d.idx._h
    unit = d.queries[:3]
    G = len(d.keys)
    tau = _tau(d, unit, 0.30)
    for sel, excl in (([8, 4, 7][::-1], 0), ([4, 7, 8], 1), ([0, 1, 2, 3, 5, 6], 0), ([8], 1)):
        sel = sorted(sel)
        allowed = set(sel) if not excl else set(range(G)) - set(sel)
        want = want_for(d, unit, tau, NO_LIMIT, 200, G, allowed)
        assert any(w[2] for w in want)
        got = c_spans(gpu_lib, h, unit, G, tau, NO_LIMIT, 200, sel, excl)
        gpu_lib.check(got[0])
        assert_c_answer(got, want, G, tag=f"filter {sel} exclude {excl}")
        assert d.idx.last_search_stats()["verified"] == sum(w[2] for w in want)
    got = c_spans(gpu_lib, h, unit, 4, tau, NO_LIMIT, 200, [], 0)          # nothing allowed: every slot empty
    gpu_lib.check(got[0])
    assert (got[1] == -1).all() and np.isposinf(got[2]).all() and (got[3] == 0).all() and (got[4] == 0).all() and (got[5] == -1).all()
    got = c_spans(gpu_lib, h, unit, 4, tau, NO_LIMIT, 200, [], 1)          # nothing excluded: the unfiltered call
    gpu_lib.check(got[0])
    assert_c_answer(got, [(w[0][:4],) + w[1:] for w in want_for(d, unit, tau, NO_LIMIT, 200, G)], 4, tag="exclude nothing")
    rc = c_spans(gpu_lib, h, unit, 4, tau, NO_LIMIT, 200, [G], 0)[0]
    assert rc < 0 and b"outside" in gpu_lib.load().vq_last_error()
    # the wrapper: keys, an unknown key, an empty `within`
    kw = dict(max_distance=tau, max_span=200, group_of=d.group_of, position_of=d.position_of)
    res = d.idx.search_spans_batch(list(unit), G, within=[d.keys[8], d.keys[4], "no such video"], **kw)
    want = want_for(d, unit, tau, NO_LIMIT, 200, G, {4, 8})
    assert [[r["group"] for r in rq] for rq in res] == [[d.keys[a[0]] for a in w[0]] for w in want]
    assert d.idx.search_spans(unit[0], G, within=[], **kw) == []
    assert d.idx.search_spans(unit[0], G, exclude=[], **kw) == d.idx.search_spans(unit[0], G, **kw)


# ---- 7. lifetime, the device form, repeatability ----
@GPU
def test_stale_labels_positions_and_ranks_are_refused(gpu_lib):
    lib = gpu_lib.load()
    n = sum(LENGTHS)
    vecs, video, frame = video_rows(n + 300, 256, seed=8008, lengths=LENGTHS)
    video, frame = list(video), list(frame)
    d = Data(vecs[:n], list(range(n)), video[:n], frame[:n], group_of=video.__getitem__, position_of=frame.__getitem__)
    try:
        d.row_of = {i: i for i in range(n + 300)}
        h = d.idx._h
        unit = _unit(noisy_steps(vecs, [300, 900], seed=80))
        upload(d)
        tau = np.float32(0.6)
        got = c_spans(gpu_lib, h, unit, 5, tau, 3, 50)
        gpu_lib.check(got[0])
        assert_c_answer(got, want_for(d, unit, tau, 3, 50, 5), 5, tag="fresh")
        d.idx.add_batch(vecs[n:], list(range(n, n + 300)))         # stale after an add: refused, labels first
        assert c_spans(gpu_lib, h, unit, 5, tau, 3, 50)[0] < 0 and b"labels" in lib.vq_last_error()
        lab, _ = dense_labels(video)
        gpu_lib.check(lib.vq_index_set_groups(h, _i32(lab), n + 300, int(lab.max()) + 1))
        assert c_spans(gpu_lib, h, unit, 5, tau, 3, 50)[0] < 0 and b"positions" in lib.vq_last_error()
        pos = np.array(frame, dtype=np.int32)
        gpu_lib.check(lib.vq_index_set_positions(h, _i32(pos), n + 300))
        d.ids, d.groups, d.positions = list(range(n + 300)), video, frame
        d.refresh()
        got = c_spans(gpu_lib, h, unit, 5, tau, 3, 50)
        gpu_lib.check(got[0])
        assert_c_answer(got, want_for(d, unit, tau, 3, 50, 5), 5, tag="after add")
    finally:
        d.idx.close()
    # string ids: the id ranks are on the device; after an add they no longer cover the index
    ids = [f"v{v}_{f}" for v, f in zip(video, frame)]
    s = Data(vecs[:n], ids[:n], [f"v{v}" for v in video[:n]], frame[:n])
    try:
        assert s.idx.search_spans(unit[0], 3, max_distance=0.6) != []
        gpu_lib.check(c_spans(gpu_lib, s.idx._h, unit, 5, tau)[0])
        s.idx.add_batch(vecs[n:], ids[n:])
        assert c_spans(gpu_lib, s.idx._h, unit, 5, tau)[0] < 0 and b"ranks" in lib.vq_last_error()
    finally:
        s.idx.close()


@GPU
def test_a_second_call_and_the_device_form_give_identical_bits(gpu_lib):
    d = lengths_data()
    upload(d, _positions(d, "holes"))
    lib, h = gpu_lib.load(), d.idx._h
    unit = d.queries
    nq, G = len(unit), len(d.keys)
    calls = [(4, _tau(d, unit, 0.30), 5, NO_LIMIT), (G + 3, _tau(d, unit, 0.05), 60, 200)]
    want = []
    for k, tau, gap, span in calls:
        first = c_spans(gpu_lib, h, unit, k, tau, gap, span)
        second = c_spans(gpu_lib, h, unit, k, tau, gap, span)
        assert first[0] == 0 and second[0] == 0 and all(a.tobytes() == b.tobytes() for a, b in zip(first[1:], second[1:]))
        want.append(first[1:])
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
        outs = [tuple(dev(nq * k * b) for b in (4, 4, 8, 4, 12)) for k, _, _, _ in calls]
        for (k, tau, gap, span), o in zip(calls, outs):            # back to back, nothing read back in between
            gpu_lib.check(lib.vq_index_search_spans_device(h, dq, nq, k, c_float(float(tau)), c_int64(gap), c_int64(span), None, 0, 1, *o))
        assert hip.hipStreamSynchronize(stream) == 0
        for o, refs in zip(outs, want):
            for src, ref in zip(o, refs):
                got = np.empty_like(ref)
                assert hip.hipMemcpy(got.ctypes.data_as(c_void_p), src, ctypes.c_size_t(got.nbytes), 2) == 0
                assert got.tobytes() == ref.tobytes()
    finally:
        d.idx.set_stream(0)
        for p in ptrs:
            hip.hipFree(p)
        hip.hipStreamDestroy(stream)


# ---- 8. the wrappers ----
@GPU
def test_search_spans_under_string_ids(gpu_lib):
    """Shuffled rows, ids "v{video}_{frame}" (so "v3_100" sorts before "v3_99": the ranks are not the rows), the default
    `video_of` / `frame_of`; one frame of video 3 is a bit-exact copy of its neighbour, so the peak is decided by the id."""
    rows, video, frame = video_rows(6 * 300, 256, seed=9009, lengths=[300])
    rows[3 * 300 + 100] = rows[3 * 300 + 99]
    perm = np.random.default_rng(9010).permutation(len(rows))
    rows, video, frame = np.ascontiguousarray(rows[perm]), [video[i] for i in perm], [frame[i] for i in perm]
    ids = [f"v{v}_{f}" for v, f in zip(video, frame)]
    d = Data(rows, ids, [f"v{v}" for v in video], frame)
    try:
        row_of = {i: r for r, i in enumerate(ids)}
        queries = [rows[row_of["v3_99"]] * np.float32(3.0)] + noisy_steps(rows, [row_of["v1_20"], row_of["v5_250"]], seed=90)
        unit = _unit(queries)
        for tau, gap, span in ((0.5, None, None), (0.7, 3, 40), (0.9, None, 0)):
            res = d.idx.search_spans_batch(queries, 4, max_distance=tau, max_gap=gap, max_span=span)
            want = want_for(d, unit, np.float32(tau), NO_LIMIT if gap is None else gap, NO_LIMIT if span is None else span, 4)
            assert d.idx.last_search_stats()["verified"] == sum(w[2] for w in want)
            for rq, (ans, _, _, _) in zip(res, want):
                assert [r["group"] for r in rq] == [d.keys[a[0]] for a in ans]
                assert [(r["start_id"], r["end_id"], r["peak_id"]) for r in rq] == [tuple(ids[x] for x in a[4]) for a in ans]
                assert [(r["start"], r["end"], r["frames"]) for r in rq] == [(frame[a[4][0]], frame[a[4][1]], a[3]) for a in ans]
                assert [r["mass"] for r in rq] == [a[2] * 2.0 ** -24 for a in ans]
                assert [r["score"] for r in rq] == [1.0 - (float(np.float32(tau)) - a[2] * 2.0 ** -24 / a[3]) for a in ans]
            assert res[0] == d.idx.search_spans(queries[0], 4, max_distance=tau, max_gap=gap, max_span=span)
            # both copies lie in the span: the peak is the copy of the smaller id; spans of one row: equal masses, the earlier one
            assert res[0][0]["group"] == "v3" and res[0][0]["peak_id"] == ("v3_99" if span == 0 else "v3_100")
    finally:
        d.idx.close()


@GPU
def test_simple_video_index_search_spans_on_fractional_timestamps(gpu_lib):
    from video_quierer_amd.overhaul_index import SimpleVideoIndex
    vecs, video, frame = video_rows(600, 512, seed=911, lengths=[150])
    rng = np.random.default_rng(912)
    names = [f"clip{v}.mp4" for v in video]
    stamps = [round(f * 0.4 + float(rng.uniform(0, 0.3)), 3) for f in frame]      # ~2.5 fps, jittered
    sv = SimpleVideoIndex()
    for e, nm, ts in zip(vecs, names, stamps):
        sv.add_frame(e, nm, ts)
    positions = [int(round(ts * 1000)) for ts in stamps]
    labels, keys = dense_labels(names)
    tie = -np.arange(600)                                          # search's tie rule: the larger frame id first
    stored = np.stack(sv.embeddings)
    q = noisy_steps(vecs, [150 + 60], seed=91)[0]                  # clip1.mp4, around 24 s
    unit = (q / (np.linalg.norm(q) + 1e-10)).astype(np.float32)
    dist = [knn_oracle.distances(stored, unit)]
    seen = set()
    for min_sim, gap_s, len_s in ((0.25, None, None), (0.6, None, None), (0.6, 0.45, None), (0.5, None, 3.0005), (0.25, 0.3999, 1.0)):
        tau = np.float32(1) - np.float32(min_sim)
        gap = NO_LIMIT if gap_s is None else math.floor(gap_s * 1000)
        span = NO_LIMIT if len_s is None else math.floor(len_s * 1000)
        (ans, _, _, _), = span_answer(dist, labels, positions, tie, tau, gap, span, 3)
        got = sv.search_spans(q, 3, min_similarity=min_sim, max_gap_s=gap_s, max_len_s=len_s)
        assert [r["video_name"] for r in got] == [keys[a[0]] for a in ans], (min_sim, gap_s, len_s)
        assert [(r["start"], r["end"], r["peak"]) for r in got] == [tuple(stamps[x] for x in a[4]) for a in ans]
        assert [(r["frames"], r["mass"]) for r in got] == [(a[3], a[2] * 2.0 ** -24) for a in ans]
        assert [r["score"] for r in got] == [1.0 - (float(tau) - a[2] * 2.0 ** -24 / a[3]) for a in ans]
        assert got[0]["video_name"] == "clip1.mp4"
        if gap_s is None and len_s is None:                        # (a limit may cut the query's own frame off the best run)
            assert got[0]["start"] <= stamps[210] <= got[0]["end"]
        seen.add((got[0]["start"], got[0]["end"]))
    assert len(seen) >= 4                                          # the limits and the threshold move the span
