"""Host side of the span search without a device: the exported symbols, the plan (query chunks at the 512 MiB rule, the LDS
form's row limit and bytes, the global form's scratch, the environment overrides), the argument checks that come before the
device is touched, the wrappers' checks, and the numpy restatement of the definition (tests/span_ref.py): a hand-worked example
and the O(L^2) form against the prefix/minimum form."""
from ctypes import POINTER, byref, c_float, c_int, c_int32, c_int64

import numpy as np
import pytest

from index_host_fakes import bare_index, fake_device, fake_lib, fill
from span_ref import NO_LIMIT, gains, rank_value, span_answer, span_brute, span_scan

ENV = ("VQ_AMD_SPAN_LDS_ROWS", "VQ_AMD_SPAN_DIST_BYTES")


def _plan(n, n_groups, largest, nq):
    from video_quierer_amd import _lib
    chunks, lds_rows, glob = c_int(), c_int(), c_int()
    lds_bytes, scratch = c_int64(), c_int64()
    _lib.check(_lib.load().vq_debug_span_plan(n, n_groups, largest, nq, byref(chunks), byref(lds_rows), byref(lds_bytes), byref(glob),
                                              byref(scratch)))
    return dict(chunks=chunks.value, lds_rows=lds_rows.value, lds_bytes=lds_bytes.value, global_form=glob.value, scratch=scratch.value)


@pytest.fixture
def no_overrides(monkeypatch):
    for name in ENV:
        monkeypatch.delenv(name, raising=False)
    return monkeypatch


def test_new_symbols_are_exported():
    from video_quierer_amd import _lib
    lib = _lib.load()
    for name in ("vq_index_search_spans", "vq_index_search_spans_device", "vq_debug_span_plan"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert _lib.IDX_NCLASS == 7 and lib.vq_index_profile_class_name(6).decode() == "sequence_dp"
    import video_quierer_amd
    video_quierer_amd.install_dropin()
    from indexes.hnsw import HNSWIndex
    from video_quierer_amd.overhaul_index import SimpleVideoIndex
    assert callable(HNSWIndex.search_spans) and callable(HNSWIndex.search_spans_batch) and callable(SimpleVideoIndex.search_spans)


def test_plan_chunks_keep_the_distances_within_512_mib(no_overrides):
    # 2^27 floats: 1M rows (padded to 64) -> 134 queries fit, so every nq <= 64 is one chunk; 2^22 rows -> 32 queries per chunk
    assert _plan(1_000_000, 2_000, 500, 64)["chunks"] == 1
    assert _plan(2 ** 22, 2_000, 500, 64)["chunks"] == 2 and _plan(2 ** 22, 2_000, 500, 32)["chunks"] == 1
    assert _plan(2 ** 22, 2_000, 500, 33)["chunks"] == 2 and _plan(2 ** 22 + 1, 2_000, 500, 32)["chunks"] == 2     # (rows padded to 64)
    assert _plan(2 ** 27, 2_000, 500, 64)["chunks"] == 64 and _plan(2 ** 31 - 1, 2_000, 500, 5)["chunks"] == 5     # one query at the least
    for n, nq in ((1, 1), (5_000, 64), (3_000_000, 64), (50_000_000, 17)):
        p = _plan(n, 1, 1, nq)
        ld = (n + 63) // 64 * 64
        per = -(-nq // p["chunks"])
        assert per * ld * 4 <= 512 << 20 or per == 1


def test_plan_lds_form_covers_4096_rows_within_a_cu(no_overrides):
    p = _plan(1_000_000, 2_000, 4_096, 8)
    assert p["lds_rows"] == 4_096 and p["global_form"] == 0 and p["scratch"] == 0
    assert p["lds_bytes"] <= 160 << 10                             # the LDS of one gfx950 CU
    assert p["lds_bytes"] == 4_098 * 8 + 3 * 4_096 * 4 + 64 * 4    # prefix sums [rows + 2], three words per row, block minima
    assert p["lds_bytes"] <= 4_096 * 36                            # no more per row than the sequence search's 36 B
    assert 20 * 4_096 <= 160 << 10                                 # the per-row bytes alone
    q = _plan(1_000_000, 2_000, 4_097, 8)                          # global form exactly when the largest group exceeds the limit
    assert q["global_form"] == 1 and q["scratch"] == (1_000_000 + 2_000) * 8 + 3 * 1_000_000 * 4
    assert _plan(1_000_000, 1, 1_000_000, 8)["global_form"] == 1   # one group of a million rows is legal
    small = _plan(1_000_000, 2_000, 500, 8)
    assert small["lds_bytes"] == 514 * 8 + 3 * 512 * 4 + 8 * 4     # sized for the longest group: 500 rows -> 512
    assert small["lds_bytes"] * 8 <= 160 << 10                     # eight such workgroups share a CU


def test_plan_honours_the_overrides(no_overrides):
    mp = no_overrides
    mp.setenv("VQ_AMD_SPAN_LDS_ROWS", "64")
    p = _plan(4_820, 36, 700, 8)
    assert p["lds_rows"] == 64 and p["global_form"] == 1 and p["lds_bytes"] == 66 * 8 + 3 * 64 * 4 + 4
    assert _plan(4_820, 36, 64, 8)["global_form"] == 0 and _plan(4_820, 36, 65, 8)["global_form"] == 1
    mp.setenv("VQ_AMD_SPAN_LDS_ROWS", "100000")                    # never above what the LDS holds
    assert _plan(4_820, 36, 700, 8)["lds_rows"] == 4_096
    mp.delenv("VQ_AMD_SPAN_LDS_ROWS")
    ld = (4_820 + 63) // 64 * 64
    mp.setenv("VQ_AMD_SPAN_DIST_BYTES", str(3 * ld * 4))
    assert _plan(4_820, 36, 700, 8)["chunks"] == 3 and _plan(4_820, 36, 700, 64)["chunks"] == 22 and _plan(4_820, 36, 700, 3)["chunks"] == 1
    mp.setenv("VQ_AMD_SPAN_DIST_BYTES", "1")
    assert _plan(4_820, 36, 700, 8)["chunks"] == 8
    mp.delenv("VQ_AMD_SPAN_DIST_BYTES")
    assert _plan(4_820, 36, 700, 8) == dict(chunks=1, lds_rows=4_096, lds_bytes=706 * 8 + 3 * 704 * 4 + 11 * 4, global_form=0, scratch=0)
    for bad in ((0, 1, 1, 1), (10, 0, 1, 1), (10, 11, 1, 1), (10, 2, 0, 1), (10, 2, 11, 1), (10, 2, 5, 0), (10, 2, 5, 65), (2 ** 31, 2, 5, 1)):
        with pytest.raises(ValueError):
            _plan(*bad)


def test_c_abi_refuses_bad_arguments_before_the_device():
    from video_quierer_amd import _lib
    lib = _lib.load()
    q = np.zeros((65, 8), np.float32); g = np.empty(65 * 1025, np.int32); d = np.empty(65 * 1025, np.float32)
    gp, dp = g.ctypes.data_as(POINTER(c_int32)), d.ctypes.data_as(POINTER(c_float))
    nan = float("nan")
    cases = [(0, 5, .5, 1, 1, "nq"), (65, 5, .5, 1, 1, "nq"), (-1, 5, .5, 1, 1, "nq"), (3, 0, .5, 1, 1, "k "), (3, 1025, .5, 1, 1, "k "),
             (3, 5, nan, 1, 1, "NaN"), (3, 5, .5, -1, 1, "negative"), (3, 5, .5, 1, -1, "negative"), (3, 5, .5, -2 ** 40, 0, "negative")]
    for nq, k, tau, gap, span, word in cases:
        rc = lib.vq_index_search_spans(None, _lib.fptr(q), nq, k, c_float(tau), c_int64(gap), c_int64(span), None, 0, 1, gp, dp, None, None, None)
        assert rc < 0, (nq, k, tau, gap, span)
        assert word in lib.vq_last_error().decode(), lib.vq_last_error()
        assert lib.vq_index_search_spans_device(None, None, nq, k, c_float(tau), c_int64(gap), c_int64(span), None, 0, 1, None, None, None,
                                                None, None) < 0
    # NULL queries or required outputs, a bad filter
    for qq, go, do in ((None, gp, dp), (_lib.fptr(q), None, dp), (_lib.fptr(q), gp, None)):
        assert lib.vq_index_search_spans(None, qq, 3, 5, c_float(.5), c_int64(1), c_int64(1), None, 0, 1, go, do, None, None, None) < 0
        assert "null" in lib.vq_last_error().decode()
    assert lib.vq_index_search_spans(None, _lib.fptr(q), 3, 5, c_float(.5), c_int64(1), c_int64(1), None, 2, 1, gp, dp, None, None, None) < 0
    assert "filter" in lib.vq_last_error().decode()
    assert lib.vq_index_search_spans(None, _lib.fptr(q), 3, 5, c_float(.5), c_int64(1), c_int64(1), None, 0, 2, gp, dp, None, None, None) < 0
    assert "filter" in lib.vq_last_error().decode()


def test_wrapper_argument_checks():
    from video_quierer_amd.indexes.hnsw import HNSWIndex
    from video_quierer_amd.overhaul_index import SimpleVideoIndex
    idx = HNSWIndex.__new__(HNSWIndex)                             # the checks below come before the handle is touched
    idx.entry_point, idx.element_count = None, 0
    q = np.ones(8, np.float32)
    with pytest.raises(TypeError):
        idx.search_spans(q, 5)                                     # max_distance has no default
    with pytest.raises(ValueError):
        idx.search_spans(q, 5, max_distance=float("nan"))
    for kw in (dict(max_gap=-1), dict(max_span=-1), dict(max_gap=-2 ** 40, max_span=3)):
        with pytest.raises(ValueError):
            idx.search_spans(q, 5, max_distance=0.5, **kw)
    with pytest.raises(ValueError):
        idx.search_spans(q, 5, max_distance=0.5, within=["a"], exclude=["b"])
    with pytest.raises(ValueError):
        idx.search_spans(q, 5, max_distance=0.5, within="a")
    with pytest.raises(ValueError):
        idx.search_spans_batch([q] * 65, 5, max_distance=0.5)
    assert idx.search_spans(q, 5, max_distance=0.5) == [] and idx.search_spans_batch([], 5, max_distance=0.5) == []      # an empty index
    assert idx.search_spans_batch([q, q], 5, max_distance=0.5, max_gap=0, max_span=0) == [[], []]
    sv = SimpleVideoIndex()
    for kw in (dict(min_similarity=float("nan")), dict(max_gap_s=-0.5), dict(max_len_s=-1.0), dict(max_len_s=float("nan"))):
        with pytest.raises(ValueError):
            sv.search_spans(q, **kw)
    assert sv.search_spans(q) == []


def test_wrapper_passes_the_limits_and_builds_the_dicts(monkeypatch):
    """On the recording library: None maps to 2^40, the labels of `within` go down sorted, and a canned answer comes back as dicts."""
    ids = ["a_0", "a_1", "a_2", "b_0", "b_1"]
    idx = bare_index(ids, dimension=4)
    seen = []

    def spans(calls, h, q, nq, k, tau, gap, span, labels, n_sel, excl, groups, dist, mass, length, rows):
        seen.append((nq, k, tau, gap, span, [labels[i] for i in range(n_sel)], excl))
        for j in range(nq):
            fill(groups, [1, -1][:k], j * k); fill(dist, [-0.75, np.inf][:k], j * k)
            fill(mass, [3 * 2 ** 22, 0][:k], j * k); fill(length, [2, 0][:k], j * k)
            fill(rows, [3, 4, 4, -1, -1, -1][:3 * k], j * 3 * k)

    fake_lib(monkeypatch, vq_index_search_spans=spans)
    q = np.array([2, 0, 0, 0], np.float32)
    res = idx.search_spans(q, 5, max_distance=0.5)
    assert seen[-1] == (1, 2, 0.5, 2 ** 40, 2 ** 40, [], 1)       # k capped by the groups the index holds
    assert res == [{"group": "b", "mass": 0.75, "frames": 2, "start_id": "b_0", "end_id": "b_1", "peak_id": "b_1", "start": 0, "end": 1,
                    "score": 1.0 - (0.5 - 0.75 / 2)}]
    res = idx.search_spans_batch([q, q], 1, max_distance=np.float32(0.3), max_gap=7, max_span=0, within=["b", "zzz"])
    assert seen[-1] == (2, 1, float(np.float32(0.3)), 7, 0, [1], 0) and len(res) == 2 and res[0] == res[1] and res[0][0]["group"] == "b"
    assert idx.search_spans(q, 5, max_distance=0.5, within=["zzz"]) == [] and idx.search_spans(q, 0, max_distance=0.5) == []
    with pytest.raises(ValueError):
        idx.search_spans(np.ones(5, np.float32), 5, max_distance=0.5)       # the dimension, before the library is called
    assert len(seen) == 2


def test_simple_video_index_maps_seconds_to_milliseconds(monkeypatch):
    from video_quierer_amd.overhaul_index import SimpleVideoIndex
    seen = []

    def spans(calls, h, q, nq, k, tau, gap, span, labels, n_sel, excl, groups, dist, mass, length, rows):
        seen.append((nq, k, tau, gap, span, n_sel, excl))
        fill(groups, [0, -1][:k]); fill(dist, [-1.0, np.inf][:k]); fill(mass, [2 ** 24, 0][:k]); fill(length, [3, 0][:k])
        fill(rows, [0, 2, 1, -1, -1, -1][:3 * k])

    fake_device(monkeypatch, vq_index_search_spans=spans)
    sv = SimpleVideoIndex()
    for i, ts in enumerate((0.5, 1.25, 2.0)):
        sv.add_frame(np.eye(4, dtype=np.float32)[i], "clip.mp4", ts)
    sv.add_frame(np.eye(4, dtype=np.float32)[3], "other.mp4", 0.0)
    res = sv.search_spans(np.ones(4, np.float32), 5, min_similarity=0.25, max_gap_s=1.9999, max_len_s=0.0305)
    tau = float(np.float32(1) - np.float32(0.25))
    assert seen[-1] == (1, 2, tau, 1999, 30, 0, 1)                # floor(x * 1000) ms; unfiltered
    assert res == [{"video_name": "clip.mp4", "start": 0.5, "end": 2.0, "peak": 1.25, "frames": 3, "score": 1.0 - (tau - 1.0 / 3),
                    "mass": 1.0}]
    sv.search_spans(np.ones(4, np.float32), 1)
    assert seen[-1] == (1, 1, tau, 2 ** 40, 2 ** 40, 0, 1)


def test_restatement_on_a_hand_worked_example():
    """tau = .5, distances in eighths (every gain a multiple of u = 2^21), one group of eight rows at positions 0 .. 7:
         d    .5    .25   .375  .875  .125  .5    1.    .125
         w/u   0     2     1    -3     3     0    -4     3
         P/u   0  0     2     3     0     3     3    -1     2
    The largest mass is 3u, held by r1 .. r2, r0 .. r2 (a zero-gain row in front), r4, r4 .. r5 (a zero-gain row behind) and r7.
    The shortest are the single rows r4 and r7; the earlier is r4.  No returned span starts or ends on a zero-gain row."""
    u = 2 ** 21
    pos = list(range(8))
    d = np.array([.5, .25, .375, .875, .125, .5, 1., .125], np.float32)
    w = gains(d, np.float32(.5))
    assert w.tolist() == [0, 2 * u, u, -3 * u, 3 * u, 0, -4 * u, 3 * u]
    w2 = np.array([0, 2, 2, -1, 3, 0, -4, 3], np.int64) * u        # r1 .. r4 holds 6u
    holes = [0, 1, 5, 6, 7, 8, 9, 10]                              # a hole of 4 between r1 and r2
    for one in (span_brute, span_scan):
        assert one(w, pos) == (3 * u, 4, 4, True)
        assert one(w[:7], pos[:7])[:3] == (3 * u, 4, 4)            # without r7: r4 against r1 .. r2 and r4 .. r5, the shorter
        assert one(w[:4], pos[:4])[:3] == (3 * u, 1, 2)            # r1 .. r2, not r0 .. r2
        assert one(w[:2], pos[:2])[:3] == (2 * u, 1, 1) and one(w[:1], pos[:1]) is None       # a zero gain alone is no span
        assert one(w[:4], pos[:4], max_span=0)[:3] == (2 * u, 1, 1)
        assert one(w[:4], pos[:4], max_gap=0)[:3] == (2 * u, 1, 1)                            # every row alone
        assert one(w[:4], [0, 0, 0, 0], max_gap=0, max_span=0)[:3] == (3 * u, 1, 2)           # equal positions: one run
        assert one(w2, pos)[:3] == (6 * u, 1, 4)
        assert one(w2, pos, max_span=2)[:3] == (4 * u, 1, 2)       # r2 .. r4 holds 4u too: as long, later
        assert one(w2, pos, max_span=1)[:3] == (4 * u, 1, 2)
        assert one(w2, holes, max_gap=3)[:3] == (4 * u, 2, 4)      # cut at the hole
        assert one(w2, holes, max_gap=4)[:3] == (6 * u, 1, 4)
        assert one(w2, holes, max_gap=2 ** 40, max_span=6)[:3] == (6 * u, 1, 4) and one(w2, holes, max_span=5)[:3] == (4 * u, 1, 2)
        assert one(-np.abs(w) - 1, pos) is None
    # two groups of the same rows: equal D, the smaller label first; the peak of a span of several rows
    d2 = np.concatenate([d, d])
    labels = np.array([0] * 8 + [1] * 8)
    (ans, decided, holding, group_tie), = span_answer([d2], labels, pos + pos, np.arange(16), np.float32(.5))
    assert holding == 2 and group_tie and decided == {0: True, 1: True}
    assert ans == [(0, np.float32(-.375), 3 * u, 1, (4, 4, 4)), (1, np.float32(-.375), 3 * u, 1, (12, 12, 12))]
    assert rank_value(3 * u) == np.float32(-.375)
    (ans, _, holding, _), = span_answer([d2], labels, pos + pos, np.arange(16)[::-1], np.float32(1.), k=1, allowed={1})
    # tau = 1: w/u = 4 6 5 1 7 4 0 7; the whole group holds 34u, its zero-gain row lies inside the span
    assert holding == 1 and ans == [(1, rank_value(34 * u), 34 * u, 8, (8, 15, 15))]          # peak: .125 twice, the smaller tie
    # tau at a row's exact distance: zero gain, no span; below every distance: nothing
    assert span_answer([d2], labels, pos + pos, np.arange(16), np.float32(.125))[0][2] == 0
    assert span_answer([d2], labels, pos + pos, np.arange(16), np.float32(.1))[0][0] == []


def test_brute_force_agrees_with_the_scan_on_random_integer_cases():
    """A few thousand groups of up to 40 rows with small integer gains (many equal masses), zero gains, equal positions and both
    limits: the O(L^2) form and the prefix/minimum form name the same span."""
    rng = np.random.default_rng(20)
    cases = decided = none = limited = 0
    for _ in range(3_000):
        L = int(rng.integers(1, 41))
        w = rng.integers(-3, 4, L).astype(np.int64) * int(rng.choice([1, 2 ** 21]))
        pos = np.sort(rng.integers(-20, 20, L) * int(rng.choice([1, 1, 2 ** 26])))
        max_gap = int(rng.choice([NO_LIMIT, 2 ** 32, 0, 1, 2, 5, 2 ** 26]))
        max_span = int(rng.choice([NO_LIMIT, 2 ** 32 - 1, 0, 1, 3, 10, 2 ** 28]))
        a, b = span_brute(w, pos, max_gap, max_span), span_scan(w, pos, max_gap, max_span)
        assert (a is None) == (b is None), (w, pos, max_gap, max_span)
        cases += 1
        if a is None:
            none += 1
            continue
        assert a[:3] == b[:3], (w, pos, max_gap, max_span, a, b)
        assert w[a[1]] != 0 and w[a[2]] != 0                       # no zero gain at an end
        decided += a[3]
        limited += a[:3] != span_brute(w, pos)[:3]
    assert cases == 3_000 and decided > 300 and none > 100 and limited > 300, (decided, none, limited)
