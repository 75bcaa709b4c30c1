"""Warped clip alignment (vq_index_align_clip / HNSWIndex.align_clip): the k videos that show a clip under a monotone time warp.
The expected answer is the definition restated in numpy (tests/align_ref.py, `align_answer` over `align_scan`, which
tests/test_align_cpu.py holds against the cell-by-cell `align_brute`) over the C oracle's exact distances on the exported rows,
with row ties by the id ranks.  Every comparison is exact: the group lists, the bits of D, the costs, the start and end rows
and the alignments.

The rows are video-like (consecutive frames are near-duplicates), as tests/test_distinct_search.py makes them; dim 64 unless
said."""
from ctypes import POINTER, byref, c_float, c_int32, c_int64, c_void_p

import numpy as np
import pytest

from align_ref import align_answer, costs, rank_value
from test_distinct_search import _unit, video_rows
from test_index_host_forms import CANARY, Family, Hip, Out, _data, _hptr, _run_device, _run_host, _same
from test_sequence_search import Data, noisy_steps

GPU = pytest.mark.gpu
DIM = 64
LENGTHS = [1, 2, 3, 7, 63, 64, 65, 300, 700]        # single rows, both sides of a wave and of a 64-row block, several tiles of 256
INF = np.float32(np.inf)
ENV = ("VQ_AMD_ALIGN_LDS_ROWS", "VQ_AMD_ALIGN_DIST_BYTES", "VQ_AMD_ALIGN_BP_BYTES")


def _i32(a):
    return a.ctypes.data_as(POINTER(c_int32))


def c_align(gpu_lib, h, clip, k, max_dist=INF, sel=None, exclude=1, extras=True):
    """The C call.  -> rc, groups [k], D [k], costs [k], rows [k][2], alignment [k][m][2] (the last three None without `extras`)"""
    q = np.ascontiguousarray(clip, dtype=np.float32)
    m = len(q)
    g = np.full(k, -7, np.int32); dd = np.full(k, -7, np.float32)
    cost = np.full(k, -7, np.int64); rows = np.full((k, 2), -7, np.int32); pairs = np.full((k, m, 2), -7, np.int32)
    sel = np.asarray([] if sel is None else sel, dtype=np.int32)
    rc = gpu_lib.load().vq_index_align_clip(h, gpu_lib.fptr(q), m, k, c_float(float(max_dist)), _i32(sel), len(sel), exclude, _i32(g),
                                            gpu_lib.fptr(dd), cost.ctypes.data_as(POINTER(c_int64)) if extras else None,
                                            _i32(rows) if extras else None, _i32(pairs) if extras else None)
    return (rc, g, dd, cost, rows, pairs) if extras else (rc, g, dd, None, None, None)


def assert_c_answer(got, ans, tag=""):
    """got: c_align's arrays; ans: align_answer's list"""
    _, g, dd, cost, rows, pairs = got
    nw = len(ans)
    exp_d = np.array([a[1] for a in ans], np.float32)
    print(f"{tag}: groups got {g[:4].tolist()} want {[a[0] for a in ans][:4]}; D got {dd[:4]} want {exp_d[:4]}")
    assert g[:nw].tolist() == [a[0] for a in ans], f"{tag}: groups differ"
    assert np.array_equal(dd[:nw].view(np.uint32), exp_d.view(np.uint32)), f"{tag}: D differs"
    assert (g[nw:] == -1).all() and np.isposinf(dd[nw:]).all()
    if cost is not None:
        assert cost[:nw].tolist() == [a[2] for a in ans], f"{tag}: costs differ"
        assert rows[:nw].tolist() == [list(a[3]) for a in ans], f"{tag}: start / end rows differ"
        assert pairs[:nw].tolist() == [[list(p) for p in a[4]] for a in ans], f"{tag}: alignments differ"
        assert (cost[nw:] == 0).all() and (rows[nw:] == -1).all() and (pairs[nw:] == -1).all()


def want_for(d, unit, max_dist=INF, k=10, allowed=None):
    return align_answer(d.dist(unit), d.labels, d.positions, d.tie, max_dist, k, allowed)


def upload(d):
    """Labels, ranks and positions go to the device through the wrapper (one tiny call)."""
    d.idx.align_clip([np.ones(d.idx.dimension, np.float32)], 1, group_of=d.group_of, position_of=d.position_of)


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


@pytest.fixture(autouse=True)
def _no_overrides(monkeypatch):
    for name in ENV:
        monkeypatch.delenv(name, raising=False)


def clips_of(rows, first, seed):
    """Clips cut from the video that starts at row `first` (at least 300 rows): name -> unit frames [m][dim]."""
    def cut(frames, s):
        return _unit(noisy_steps(rows, [first + f for f in frames], seed=s, noise=0.1))
    rng = np.random.default_rng(seed)
    out = {"m1": cut([150], seed + 1), "m2": cut([40, 43], seed + 2), "m5 irregular": cut([10, 11, 15, 16, 30], seed + 3),
           "m64 rate 2": cut(range(100, 228, 2), seed + 4),                       # every second stored frame
           "m64 rate 1/2": cut(np.repeat(np.arange(200, 232), 2), seed + 5),      # every stored frame twice
           "m65 irregular": cut(np.cumsum(rng.integers(0, 4, 65)) + 20, seed + 6)}
    return out


def lengths_data():
    def build():
        rows, video, frame = video_rows(sum(LENGTHS), DIM, seed=7007, lengths=LENGTHS)      # one round of LENGTHS: nine groups
        d = Data(rows, list(range(len(rows))), video, frame, group_of=video.__getitem__, position_of=frame.__getitem__)
        d.rows, d.video, d.frame = rows, video, frame
        d.first = {ln: video.index(v) for v, ln in enumerate(LENGTHS)}
        d.clips = clips_of(rows, d.first[700], 70)
        d.clips["m5 of the 300"] = _unit(noisy_steps(rows, [d.first[300] + f for f in (5, 9, 10, 14, 20)], seed=78, noise=0.1))
        upload(d)
        return d
    return cached("lengths", build)


CLIPS = ["m1", "m2", "m5 irregular", "m5 of the 300", "m64 rate 2", "m64 rate 1/2", "m65 irregular"]


# ---- 1. video-like rows: every group length, every clip length, k, max_dist, the filters, the optional outputs ----
@GPU
@pytest.mark.parametrize("clip", CLIPS)
def test_video_like_rows(gpu_lib, clip):
    d = lengths_data()
    unit = d.clips[clip]
    G = len(d.keys)
    full, holding, shared = want_for(d, unit, k=G + 3)
    assert holding == G and not shared                             # on the restatement: every group answers, no two D are equal
    src = LENGTHS.index(300 if "300" in clip else 700)
    assert full[0][0] == src, "the clip's own video comes first"
    if clip.startswith("m64"):                                      # the warp is real: some frame holds several rows, or rows repeat
        pairs = full[0][4]
        assert any(a != b for a, b in pairs) or any(p[1] == q[0] for p, q in zip(pairs, pairs[1:]))
    for k in (1, 4, G + 3):
        got = c_align(gpu_lib, d.idx._h, unit, k)
        gpu_lib.check(got[0])
        assert_c_answer(got, full[:k], tag=f"{clip} k {k}")
        assert d.idx.last_search_stats() == {"verified": G, "rescanned": 0, "exact_fallback": 1}       # no global form, one chunk
        short = c_align(gpu_lib, d.idx._h, unit, k, extras=False)   # the optional outputs NULL
        gpu_lib.check(short[0])
        assert short[1].tobytes() == got[1].tobytes() and short[2].tobytes() == got[2].tobytes()
    # max_dist across the D values: a D hit exactly is inside, the float below it is not
    ds = [a[1] for a in full]
    for md, n_in in ((ds[2], 3), (np.nextafter(ds[2], np.float32(-np.inf)), 2), (ds[-1], G), (np.nextafter(ds[0], np.float32(-np.inf)), 0),
                     (np.float32((float(ds[0]) + float(ds[1])) / 2), 1)):
        want, holding, _ = want_for(d, unit, md, k=G)
        assert holding == n_in and want == full[:n_in]
        got = c_align(gpu_lib, d.idx._h, unit, G, md)
        gpu_lib.check(got[0])
        assert_c_answer(got, want, tag=f"{clip} max_dist {md}")
        assert d.idx.last_search_stats()["verified"] == n_in
    # the filters, in both senses and with both empty lists
    for sel, exclude in (([src, 1, 4], 0), ([4, 1, src, 4], 0), ([src], 1), ([0, 2, 8], 1), ([], 1), ([6], 0)):
        allowed = set(range(G)) - set(sel) if exclude else set(sel)
        want, holding, _ = want_for(d, unit, k=G, allowed=allowed)
        assert holding == len(allowed) and want == [a for a in full if a[0] in allowed]      # a group's result needs no other group
        got = c_align(gpu_lib, d.idx._h, unit, G, sel=sel, exclude=exclude)
        gpu_lib.check(got[0])
        assert_c_answer(got, want, tag=f"{clip} filter {sel} exclude {exclude}")
    none = c_align(gpu_lib, d.idx._h, unit, 3, sel=[], exclude=0)   # an empty `within` list: nothing is allowed
    gpu_lib.check(none[0])
    assert_c_answer(none, [], tag="nothing allowed")
    assert d.idx.last_search_stats() == {"verified": 0, "rescanned": 0, "exact_fallback": 0}
    assert c_align(gpu_lib, d.idx._h, unit, 3, sel=[G], exclude=0)[0] < 0                   # a label the index does not hold


# ---- 2. the same rows through the global form, in three clip chunks, and both: the default run's bits ----
@GPU
@pytest.mark.parametrize("clip", ["m5 irregular", "m64 rate 2", "m65 irregular"])
def test_forced_global_form_and_clip_chunks_give_the_same_bits(gpu_lib, monkeypatch, clip):
    d = lengths_data()
    unit = d.clips[clip]
    m, G = len(unit), len(d.keys)
    ld = (len(d.ids) + 63) // 64 * 64
    want, _, _ = want_for(d, unit, k=G)
    plain = c_align(gpu_lib, d.idx._h, unit, G)
    gpu_lib.check(plain[0])
    assert_c_answer(plain, want, tag="plain")
    per = -(-m // 3)
    chunks = -(-m // per)
    assert chunks == 3

    def same(tag, stats):
        got = c_align(gpu_lib, d.idx._h, unit, G)
        gpu_lib.check(got[0])
        assert d.idx.last_search_stats() == stats, (tag, d.idx.last_search_stats())
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got[1:], plain[1:])), tag
    monkeypatch.setenv("VQ_AMD_ALIGN_LDS_ROWS", "64")               # the groups of 65, 300 and 700 rows take the global form
    same("global form", {"verified": G, "rescanned": 3, "exact_fallback": 1})
    monkeypatch.setenv("VQ_AMD_ALIGN_DIST_BYTES", str(per * ld * 4))
    same("global form, three chunks", {"verified": G, "rescanned": 3, "exact_fallback": 3})
    monkeypatch.delenv("VQ_AMD_ALIGN_LDS_ROWS")
    same("three chunks", {"verified": G, "rescanned": 0, "exact_fallback": 3})
    monkeypatch.setenv("VQ_AMD_ALIGN_BP_BYTES", "1")
    same("three chunks, one winner per batch", {"verified": G, "rescanned": 0, "exact_fallback": 3})
    monkeypatch.setenv("VQ_AMD_ALIGN_LDS_ROWS", "1")                # every group of two rows or more
    same("everything global", {"verified": G, "rescanned": G - 1, "exact_fallback": 3})


# ---- 3. ties: whole plateaus of bit-identical rows, a clip of m copies of one row, string ids ----
def ties_data():
    def build():
        base, _, _ = video_rows(40 + 30 + 90, DIM, seed=8008, lengths=[40, 30, 90])
        # every stored frame three times (video 0), twice (video 1), once with whole stretches frozen (video 2); three rows share
        # every position of videos 0 and 1, so the id ranks order them
        v0, v1 = np.repeat(base[:40], 3, axis=0), np.repeat(base[40:70], 2, axis=0)
        v2 = base[70:].copy()
        v2[20:50] = v2[20]
        v2[60:75] = v2[60]
        rows = np.ascontiguousarray(np.concatenate([v0, v1, v2]))
        video = [0] * 120 + [1] * 60 + [2] * 90
        frame = list(range(120)) + list(range(60)) + list(range(90))
        ids = [f"v{v}_{f}" for v, f in zip(video, frame)]           # "v0_10" < "v0_2": the id order is not the row order
        pos = [f // 3 for f in frame]
        d = Data(rows, ids, [f"v{v}" for v in video], pos, position_of=lambda nid, p=dict(zip(ids, pos)): p[nid])
        d.rows = rows
        upload(d)
        return d
    return cached("ties", build)


@GPU
def test_ties_follow_the_stated_orders(gpu_lib):
    d = ties_data()
    G = 3
    copies = _unit(np.repeat(d.rows[120 + 60 + 25][None], 9, axis=0) * np.float32(3.0))           # nine copies of a frozen row of video 2
    cut = _unit(noisy_steps(d.rows, [30, 36, 42, 48, 49, 50, 60], seed=81, noise=0.05))           # rows of video 0, each stored three times
    exact = _unit(d.rows[[120 + 4, 120 + 6, 120 + 8, 120 + 10]])                                  # stored rows of video 1 themselves
    by_row = False
    for name, unit in (("copies", copies), ("cut", cut), ("exact", exact)):
        want, holding, _ = want_for(d, unit, k=G)
        assert holding == G
        # the id ranks matter: with row numbers as ties the reference names other rows
        other, _, _ = align_answer(d.dist(unit), d.labels, d.positions, np.arange(len(d.ids)), k=G)
        by_row |= [a[3:] for a in other] != [a[3:] for a in want]
        for k in (1, G):
            got = c_align(gpu_lib, d.idx._h, unit, k)
            gpu_lib.check(got[0])
            assert_c_answer(got, want[:k], tag=f"ties {name} k {k}")
    assert by_row, "the string ids change the (position, tie) order"
    # m copies of one row against a plateau of identical rows: every cell of the plateau costs the same, so the later start wins
    # inside a cell, then the shortest stretch, then the earliest start: one row, all nine frames on it
    want, _, _ = want_for(d, copies, k=1)
    (a, b), pairs = want[0][3], want[0][4]
    assert want[0][0] == 2 and a == b and pairs == [(a, a)] * 9
    res = d.idx.align_clip(list(copies), 1, group_of=d.group_of, position_of=d.position_of, alignment=True)
    assert res[0]["group"] == "v2" and res[0]["start_id"] == res[0]["end_id"] == d.ids[a] and res[0]["alignment"] == [(d.ids[a], d.ids[a])] * 9
    assert res[0]["cost"] == want[0][2] and res[0]["distance"].tobytes() == want[0][1].tobytes()


# ---- 4. the winners' tables in batches of one ----
@GPU
def test_alignment_tables_in_batches_of_one_winner(gpu_lib, monkeypatch):
    d = lengths_data()
    unit = d.clips["m64 rate 1/2"]
    G = len(d.keys)
    want, _, _ = want_for(d, unit, k=G)
    plain = c_align(gpu_lib, d.idx._h, unit, G + 2)
    gpu_lib.check(plain[0])
    assert_c_answer(plain, want, tag="one batch")
    monkeypatch.setenv("VQ_AMD_ALIGN_BP_BYTES", str(64 * 700 * 4))  # one winner's table
    for k in (G + 2, 4):
        one = c_align(gpu_lib, d.idx._h, unit, k)
        gpu_lib.check(one[0])
        assert all(a.tobytes() == b[:k].tobytes() for a, b in zip(one[1:], plain[1:])), k
    monkeypatch.setenv("VQ_AMD_ALIGN_BP_BYTES", str(3 * 64 * 700 * 4))
    three = c_align(gpu_lib, d.idx._h, unit, G + 2)
    gpu_lib.check(three[0])
    assert all(a.tobytes() == b.tobytes() for a, b in zip(three[1:], plain[1:]))


# ---- 5. consequences of the definition ----
@GPU
def test_one_frame_is_the_grouped_search(gpu_lib):
    d = lengths_data()
    unit = d.clips["m1"]
    G = len(d.keys)
    dist = d.dist(unit)[0]
    for label in range(G):                                         # every group's best distance is held by one row
        of = dist[d.labels == label]
        assert (of == of.min()).sum() == 1
    grouped = d.idx.search_grouped(unit[0], G, group_of=d.group_of)
    got = c_align(gpu_lib, d.idx._h, unit, G)
    gpu_lib.check(got[0])
    _, g, dd, cost, rows, pairs = got
    assert [d.keys[x] for x in g.tolist()] == [r["group"] for r in grouped]
    assert rows[:, 0].tolist() == rows[:, 1].tolist() == [r["id"] for r in grouped] == pairs[:, 0, 0].tolist() == pairs[:, 0, 1].tolist()
    assert cost.tolist() == costs(np.array([r["distance"] for r in grouped], np.float32)).tolist()
    assert dd.tobytes() == np.array([rank_value(c, 1) for c in cost.tolist()], np.float32).tobytes()


@GPU
def test_a_group_of_one_row_pays_every_frame_on_it(gpu_lib):
    d = lengths_data()
    for clip in ("m5 irregular", "m65 irregular"):
        unit = d.clips[clip]
        got = c_align(gpu_lib, d.idx._h, unit, 1, sel=[0], exclude=0)               # the video of one row
        gpu_lib.check(got[0])
        _, g, dd, cost, rows, pairs = got
        r = d.first[1]
        total = int(costs(np.array([x[r] for x in d.dist(unit)], np.float32)).sum())
        assert g.tolist() == [0] and cost.tolist() == [total] and rows.tolist() == [[r, r]] and (pairs == r).all()
        assert dd.tobytes() == rank_value(total, len(unit)).tobytes()
        # every c >= 0 here: no group does better than its best row frame by frame
        full = c_align(gpu_lib, d.idx._h, unit, len(d.keys))
        for label, c in zip(full[1].tolist(), full[3].tolist()):
            rows_of = np.flatnonzero(d.labels == label)
            per_frame = np.stack([costs(x[rows_of]) for x in d.dist(unit)])
            assert (per_frame >= 0).all() and c >= int(per_frame.min(axis=1).sum())


@GPU
def test_other_groups_do_not_matter_and_a_reversed_clip_differs(gpu_lib):
    d = lengths_data()
    unit = d.clips["m64 rate 2"]
    G = len(d.keys)
    res = d.idx.align_clip(list(unit), G, group_of=d.group_of, position_of=d.position_of, alignment=True)
    assert len(res) == G
    # the same library without the video of 300 rows, under the same ids
    keep = [r for r in range(len(d.ids)) if d.video[r] != LENGTHS.index(300)]
    less = Data(d.rows[keep], keep, [d.video[r] for r in keep], [d.frame[r] for r in keep], group_of=d.video.__getitem__,
                position_of=d.frame.__getitem__)
    try:
        res2 = less.idx.align_clip(list(unit), G, group_of=less.group_of, position_of=less.position_of, alignment=True)
    finally:
        less.idx.close()
    strip = lambda rs: [{k: (v.tobytes() if isinstance(v, np.float32) else v) for k, v in r.items()} for r in rs]
    assert strip(res2) == strip([r for r in res if r["group"] != LENGTHS.index(300)])
    # reversed: another answer, and the restatement's
    back = np.ascontiguousarray(unit[::-1])
    want, _, _ = want_for(d, back, k=G)
    fwd, _, _ = want_for(d, unit, k=G)
    assert want[0][2] > fwd[0][2] and [a[1:] for a in want] != [a[1:] for a in fwd]
    got = c_align(gpu_lib, d.idx._h, back, G)
    gpu_lib.check(got[0])
    assert_c_answer(got, want, tag="reversed")


@GPU
def test_groups_whose_costs_round_to_one_distance_come_by_cost(gpu_lib):
    """Two hundred videos of one or two rows, all nearly opposite to the clip's two frames: every D lies just below 2, where
    fp32 is 2^-23 apart and C / 2 a multiple of 2^-24, so different costs share a D.  The answer is by (C, label) all the same:
    inside the list, and at its end, where the k-th place goes to the cheaper group, not to the smaller label."""
    rng = np.random.default_rng(11)
    q0 = rng.standard_normal(DIM)
    q0 /= np.linalg.norm(q0)
    lens = [1 + (g % 2) for g in range(200)]
    n = sum(lens)
    rows = _unit(-q0[None] + rng.standard_normal((n, DIM)) * 0.0005)
    video = np.repeat(np.arange(200), lens).tolist()
    frame = np.concatenate([np.arange(ln) for ln in lens]).tolist()
    d = Data(rows, list(range(n)), video, frame, group_of=video.__getitem__, position_of=frame.__getitem__)
    try:
        upload(d)
        unit = _unit(np.stack([q0, q0 + rng.standard_normal(DIM) * 0.0005]))
        full, holding, shared = want_for(d, unit, k=200)
        assert holding == 200 and shared
        by_d = sorted(full, key=lambda t: (t[1], t[0]))
        inside = [i for i, (a, b) in enumerate(zip(full, by_d)) if a[0] != b[0]]
        ends = [k for k in range(1, 200) if {a[0] for a in full[:k]} != {a[0] for a in by_d[:k]}]
        assert len(inside) >= 10 and len(ends) >= 5, "the order by (D, label) is another one, also at the end of a short list"
        for k in (ends[0], ends[1], ends[-1], inside[0] + 2, 200):
            got = c_align(gpu_lib, d.idx._h, unit, k)
            gpu_lib.check(got[0])
            assert_c_answer(got, full[:k], tag=f"shared D, k {k}")
            assert (np.diff(got[2]) >= 0).all()
        md = full[ends[0]][1]                                      # a D that several groups hold: all of them are inside
        want, _, _ = want_for(d, unit, md, k=200)
        got = c_align(gpu_lib, d.idx._h, unit, 200, md)
        gpu_lib.check(got[0])
        assert_c_answer(got, want, tag="shared D, max_dist")
    finally:
        d.idx.close()


# ---- 6. the host form against the _device form, on the 300-row index of tests/test_index_host_forms.py ----
@GPU
def test_host_and_device_forms_agree_bit_for_bit(gpu_lib):
    lib = gpu_lib.load()
    d = _data()
    N, K, G = len(d["rows"]), 3, int(d["group"].max()) + 1
    h, empty = c_void_p(), c_void_p()
    gpu_lib.check(lib.vq_index_create(DIM, byref(h)))
    gpu_lib.check(lib.vq_index_create(DIM, byref(empty)))
    gpu_lib.check(lib.vq_index_add(h, _hptr(d["rows"]), N, 0))
    gpu_lib.check(lib.vq_index_set_groups(h, _hptr(d["group"]), N, G))
    gpu_lib.check(lib.vq_index_set_positions(h, _hptr(d["pos"]), N))
    gpu_lib.check(lib.vq_index_set_id_ranks(h, _hptr(d["rank"]), N))
    frames = d["frames"]
    m = len(frames)
    fam = Family("align", "vq_index_align_clip", frames,
                 [Out("groups", np.int32, (K,), -1), Out("dist", np.float32, (K,), float("inf")), Out("cost", np.int64, (K,), 0, True),
                  Out("rows", np.int32, (K, 2), -1, True), Out("align", np.int32, (K, m, 2), -1, True)],
                 lambda q, o: (q, m, K, c_float(0.9), None, 0, 1, *o))
    hip = Hip()
    try:
        host_full, dev_full = _run_host(lib, h, fam, True), _run_device(lib, hip, h, fam, True)
        _same(host_full, dev_full, "every output")
        host_null, dev_null = _run_host(lib, h, fam, False), _run_device(lib, hip, h, fam, False)
        _same(host_null, dev_null, "optional outputs null")
        _same(host_null, {k: host_full[k] for k in host_null}, "null variant against full variant")
        assert host_full["groups"][0] == 0 and (host_full["align"][0] >= 0).all()          # the frames are rows 3, 4, 5 of group 0
        tie = np.asarray(d["rank"], dtype=np.int64)
        from oracle import knn_oracle
        dist = [knn_oracle.distances(d["rows"], q) for q in frames]
        want, _, _ = align_answer(dist, d["group"], d["pos"], tie, np.float32(0.9), K)
        assert_c_answer((0, host_full["groups"], host_full["dist"], host_full["cost"], host_full["rows"], host_full["align"]), want, tag="forms")
        for full in (True, False):
            for got in (_run_host(lib, empty, fam, full), _run_device(lib, hip, empty, fam, full)):
                for o in fam.outs:
                    if o.name in got:
                        assert got[o.name].tobytes() == np.full(o.shape, o.empty, dtype=o.dtype).tobytes(), (o.name, got[o.name])
    finally:
        hip.free()
        lib.vq_index_destroy(h)
        lib.vq_index_destroy(empty)
    assert CANARY == 0x5A


# ---- 7. dim 512, 20,000 rows in about sixty groups, a clip of 130 frames, once; the run repeated ----
@GPU
def test_dim_512_20000_rows_a_clip_of_130_frames(gpu_lib):
    lengths = [333, 1, 700, 64, 257, 500, 100, 45, 900, 430]       # 3,330 rows a round: six rounds and a rest of 20 rows
    rows, video, frame = video_rows(20_000, 512, seed=9009, lengths=lengths)
    d = Data(rows, list(range(len(rows))), video, frame, group_of=video.__getitem__, position_of=frame.__getitem__)
    try:
        upload(d)
        G = len(d.keys)
        assert G == 61
        src = video.index(12)                                      # the second round's video of 700 rows
        assert video.count(12) == 700
        frames = np.cumsum(np.random.default_rng(91).integers(0, 5, 130)) + 50      # irregular strides, some frames repeated
        unit = _unit(noisy_steps(rows, [src + int(f) for f in frames], seed=92, noise=0.1))
        want, holding, _ = want_for(d, unit, k=8)
        assert holding == G and want[0][0] == 12
        first = c_align(gpu_lib, d.idx._h, unit, 8)
        gpu_lib.check(first[0])
        assert_c_answer(first, want, tag="dim 512")
        again = c_align(gpu_lib, d.idx._h, unit, 8)
        gpu_lib.check(again[0])
        assert all(a.tobytes() == b.tobytes() for a, b in zip(first[1:], again[1:])), "two runs, one answer"
    finally:
        d.idx.close()
