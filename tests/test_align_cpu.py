"""Host side of the warped clip alignment without a device: the exported symbols, the plan (clip chunks at the 512 MiB rule,
the LDS form's row limit and bytes, the carried state, the winner batches, the environment overrides, the 1 GiB bound), the
argument checks that come before the device is touched, the wrappers' checks, and the numpy restatement of the definition
(tests/align_ref.py): a hand-worked example, the cell-by-cell form against the prefix form, and the case the feature is for —
a clip at another pace — on the restatement alone."""
import math
from ctypes import POINTER, byref, c_float, c_int, c_int32, c_int64

import numpy as np
import pytest

import match_ref
from align_ref import align_answer, align_brute, align_scan, costs, rank_value
from index_host_fakes import bare_index, fake_device, fake_lib, fill

ENV = ("VQ_AMD_ALIGN_LDS_ROWS", "VQ_AMD_ALIGN_DIST_BYTES", "VQ_AMD_ALIGN_BP_BYTES")


def _plan(n, n_groups, largest, m, k=5, with_align=0):
    from video_quierer_amd import _lib
    chunks, lds_rows, glob, batches = c_int(), c_int(), c_int(), c_int()
    lds_bytes, scratch = c_int64(), c_int64()
    _lib.check(_lib.load().vq_debug_align_plan(n, n_groups, largest, m, k, with_align, byref(chunks), byref(lds_rows), byref(lds_bytes),
                                               byref(glob), byref(scratch), byref(batches)))
    return dict(chunks=chunks.value, lds_rows=lds_rows.value, lds_bytes=lds_bytes.value, global_form=glob.value, scratch=scratch.value,
                batches=batches.value)


@pytest.fixture
def no_overrides(monkeypatch):
    for name in ENV:
        monkeypatch.delenv(name, raising=False)
    return monkeypatch


def test_new_symbols_are_exported():
    from video_quierer_amd import _lib
    lib = _lib.load()
    for name in ("vq_index_align_clip", "vq_index_align_clip_device", "vq_debug_align_plan"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert _lib.IDX_NCLASS == 7 and lib.vq_index_profile_class_name(6).decode() == "sequence_dp"
    import video_quierer_amd
    video_quierer_amd.install_dropin()
    from indexes.hnsw import HNSWIndex
    from video_quierer_amd.overhaul_index import SimpleVideoIndex
    assert callable(HNSWIndex.align_clip) and callable(HNSWIndex.align_group) and callable(SimpleVideoIndex.find_reuse_warped)


def test_plan_chunks_keep_the_distances_within_512_mib(no_overrides):
    # 2^27 floats: 1M rows (padded to 64) -> 134 clip frames per chunk; 2^22 rows -> 32
    assert _plan(1_000_000, 2_000, 500, 134)["chunks"] == 1 and _plan(1_000_000, 2_000, 500, 135)["chunks"] == 2
    assert _plan(1_000_000, 2_000, 500, 4_096)["chunks"] == -(-4_096 // 134)
    assert _plan(2 ** 22, 2_000, 500, 64)["chunks"] == 2 and _plan(2 ** 22, 2_000, 500, 32)["chunks"] == 1
    assert _plan(2 ** 22 + 1, 2_000, 500, 32)["chunks"] == 2      # (rows padded to 64)
    assert _plan(2 ** 31 - 1, 2_000, 500, 5)["chunks"] == 5       # one frame at the least
    for n, m in ((1, 1), (5_000, 4_096), (3_000_000, 640), (50_000_000, 17)):
        p = _plan(n, 1, 1, m)
        ld = (n + 63) // 64 * 64
        per = -(-m // p["chunks"])
        assert per * ld * 4 <= 512 << 20 or per == 1


def test_plan_lds_form_covers_4096_rows_within_a_cu(no_overrides):
    p = _plan(1_000_000, 2_000, 4_096, 8)
    assert p["lds_rows"] == 4_096 and p["global_form"] == 0
    assert p["lds_bytes"] == 4_096 * (8 + 4 + 4)                   # per row: int64 cost, int32 start, int32 row number
    assert p["lds_bytes"] <= 160 << 10                             # the LDS of one gfx950 CU
    assert p["scratch"] == 1_000_000 * 12                          # the carried DP row: int64 cost + int32 start
    assert _plan(1_000_000, 2_000, 4_097, 8)["global_form"] == 1   # the global form exactly above the limit
    assert _plan(1_000_000, 1, 1_000_000, 8)["global_form"] == 1   # one group of a million rows is legal
    small = _plan(1_000_000, 2_000, 500, 8)
    assert small["lds_bytes"] == 512 * 16                          # sized for the longest group: 500 rows -> 512
    assert small["lds_bytes"] * 16 <= 160 << 10                    # sixteen such workgroups share a CU


def test_plan_winner_batches_and_the_1_gib_bound(no_overrides):
    assert _plan(100_000, 50, 2_000, 100, k=10)["batches"] == 0    # no alignment asked for: no table
    # one winner's table: 100 x 2,000 x 4 B = 800,000 B; 256 MiB hold 335 of them
    assert _plan(100_000, 50, 2_000, 100, k=10, with_align=1)["batches"] == 1
    assert _plan(100_000, 5, 2_000, 100, k=1_024, with_align=1)["batches"] == 1        # min(k, groups) winners
    assert _plan(1_000_000, 2_000, 65_536, 4_096, k=10, with_align=1)["batches"] == 10  # 1 GiB each: one winner per batch
    assert _plan(1_000_000, 2_000, 16_384, 4_096, k=10, with_align=1)["batches"] == 10  # 256 MiB each
    assert _plan(1_000_000, 2_000, 8_192, 4_096, k=10, with_align=1)["batches"] == 5
    with pytest.raises(ValueError, match="1 GiB"):
        _plan(1_000_000, 2_000, 65_537, 4_096, k=10, with_align=1)
    assert _plan(1_000_000, 2_000, 65_537, 4_096, k=10)["batches"] == 0                 # without align_out nothing is bounded


def test_plan_honours_the_overrides(no_overrides):
    mp = no_overrides
    mp.setenv("VQ_AMD_ALIGN_LDS_ROWS", "64")
    p = _plan(4_820, 36, 700, 8)
    assert p["lds_rows"] == 64 and p["global_form"] == 1 and p["lds_bytes"] == 64 * 16
    assert _plan(4_820, 36, 64, 8)["global_form"] == 0 and _plan(4_820, 36, 65, 8)["global_form"] == 1
    mp.setenv("VQ_AMD_ALIGN_LDS_ROWS", "100000")                   # never above what the LDS holds
    assert _plan(4_820, 36, 700, 8)["lds_rows"] == 4_096
    mp.delenv("VQ_AMD_ALIGN_LDS_ROWS")
    ld = (4_820 + 63) // 64 * 64
    mp.setenv("VQ_AMD_ALIGN_DIST_BYTES", str(3 * ld * 4))
    assert _plan(4_820, 36, 700, 8)["chunks"] == 3 and _plan(4_820, 36, 700, 64)["chunks"] == 22 and _plan(4_820, 36, 700, 3)["chunks"] == 1
    mp.setenv("VQ_AMD_ALIGN_DIST_BYTES", "1")
    assert _plan(4_820, 36, 700, 8)["chunks"] == 8
    mp.delenv("VQ_AMD_ALIGN_DIST_BYTES")
    mp.setenv("VQ_AMD_ALIGN_BP_BYTES", str(2 * 8 * 700 * 4))       # two winners' tables per batch
    assert _plan(4_820, 36, 700, 8, k=5, with_align=1)["batches"] == 3
    mp.setenv("VQ_AMD_ALIGN_BP_BYTES", "1")                        # one winner at the least
    assert _plan(4_820, 36, 700, 8, k=5, with_align=1)["batches"] == 5
    mp.delenv("VQ_AMD_ALIGN_BP_BYTES")
    assert _plan(4_820, 36, 700, 8, k=5, with_align=1) == dict(chunks=1, lds_rows=4_096, lds_bytes=704 * 16, global_form=0,
                                                               scratch=4_820 * 12, batches=1)
    for bad in ((0, 1, 1, 1), (10, 0, 1, 1), (10, 11, 1, 1), (10, 2, 0, 1), (10, 2, 11, 1), (10, 2, 5, 0), (10, 2, 5, 4_097), (2 ** 31, 2, 5, 1)):
        with pytest.raises(ValueError):
            _plan(*bad)
    for k in (0, 1_025):
        with pytest.raises(ValueError):
            _plan(10, 2, 5, 1, k=k)


def test_c_abi_refuses_bad_arguments_before_the_device():
    from video_quierer_amd import _lib
    lib = _lib.load()
    q = np.zeros((8, 8), np.float32); g = np.empty(1025, np.int32); d = np.empty(1025, np.float32)
    gp, dp = g.ctypes.data_as(POINTER(c_int32)), d.ctypes.data_as(POINTER(c_float))
    nan = float("nan")
    cases = [(0, 5, .5, "m "), (4_097, 5, .5, "m "), (-1, 5, .5, "m "), (3, 0, .5, "k "), (3, 1_025, .5, "k "), (3, 5, nan, "max_dist")]
    for m, k, md, word in cases:
        rc = lib.vq_index_align_clip(None, _lib.fptr(q), m, k, c_float(md), None, 0, 1, gp, dp, None, None, None)
        assert rc < 0, (m, k, md)
        assert word in lib.vq_last_error().decode(), lib.vq_last_error()
        assert lib.vq_index_align_clip_device(None, None, m, k, c_float(md), None, 0, 1, None, None, None, None, None) < 0
        assert word in lib.vq_last_error().decode(), lib.vq_last_error()
    # NULL clip or required outputs, a bad filter
    for qq, go, do in ((None, gp, dp), (_lib.fptr(q), None, dp), (_lib.fptr(q), gp, None)):
        assert lib.vq_index_align_clip(None, qq, 3, 5, c_float(.5), None, 0, 1, go, do, None, None, None) < 0
        assert "null" in lib.vq_last_error().decode()
    assert lib.vq_index_align_clip(None, _lib.fptr(q), 3, 5, c_float(.5), None, 2, 1, gp, dp, None, None, None) < 0
    assert "filter" in lib.vq_last_error().decode()
    assert lib.vq_index_align_clip(None, _lib.fptr(q), 3, 5, c_float(.5), None, 0, 2, gp, dp, None, None, None) < 0
    assert "filter" in lib.vq_last_error().decode()
    assert lib.vq_index_align_clip(None, _lib.fptr(q), 3, 5, c_float(.5), None, -1, 0, gp, dp, None, None, None) < 0
    assert "filter" in lib.vq_last_error().decode()


def test_wrapper_argument_checks():
    from video_quierer_amd.indexes.hnsw import HNSWIndex
    from video_quierer_amd.overhaul_index import SimpleVideoIndex
    idx = HNSWIndex.__new__(HNSWIndex)                             # the checks below come before the handle is touched
    idx.entry_point, idx.element_count = None, 0
    q = np.ones(8, np.float32)
    with pytest.raises(ValueError):
        idx.align_clip([q], 5, max_distance=float("nan"))
    with pytest.raises(ValueError):
        idx.align_clip([], 5)
    with pytest.raises(ValueError):
        idx.align_clip([q] * 4_097, 5)
    with pytest.raises(ValueError):
        idx.align_clip([q], 5, groups="a")
    assert idx.align_clip([q, q], 5) == [] and idx.align_clip([q], 5, max_distance=0.5, groups=["a"], exclude=True) == []     # an empty index
    sv = SimpleVideoIndex()
    with pytest.raises(ValueError):
        sv.find_reuse_warped("a.mp4", min_similarity=float("nan"))
    with pytest.raises(ValueError):
        sv.find_reuse_warped("a.mp4", min_similarity=1.5)
    with pytest.raises(KeyError):
        sv.find_reuse_warped("a.mp4")


def _canned(seen):
    def align(calls, h, q, m, k, max_dist, labels, n_sel, excl, groups, dist, cost, rows, pairs):
        seen.append((m, k, max_dist, [labels[i] for i in range(n_sel)], excl, bool(pairs)))
        fill(groups, [1, -1][:k]); fill(dist, [0.25, np.inf][:k]); fill(cost, [m * 2 ** 22, 0][:k]); fill(rows, [3, 4, -1, -1][:2 * k])
        if pairs:
            fill(pairs, [3, 3] + [4, 4] * (m - 1) + [-1] * (2 * m * (k - 1)))
    return align


def test_wrapper_passes_the_arguments_and_builds_the_dicts(monkeypatch):
    """On the recording library: None maps to +inf, the labels of `groups` go down sorted, and a canned answer comes back as dicts."""
    ids = ["a_0", "a_1", "a_2", "b_0", "b_1"]
    idx = bare_index(ids, dimension=4)
    seen = []
    fake_lib(monkeypatch, vq_index_align_clip=_canned(seen))
    q = np.array([2, 0, 0, 0], np.float32)
    res = idx.align_clip([q, q, q], 5)
    assert seen[-1] == (3, 2, math.inf, [], 1, False)              # k capped by the groups the index holds; nothing excluded
    assert res == [{"group": "b", "distance": np.float32(0.25), "score": np.float32(0.75), "cost": 3 * 2 ** 22, "start_id": "b_0",
                    "end_id": "b_1", "start": 0, "end": 1}]
    res = idx.align_clip([q, q], 1, np.float32(0.3), groups=["b", "zzz"], alignment=True)
    assert seen[-1] == (2, 1, float(np.float32(0.3)), [1], 0, True)
    assert res[0]["alignment"] == [("b_0", "b_0"), ("b_1", "b_1")]
    idx.align_clip([q], 1, groups=["a"], exclude=True)
    assert seen[-1] == (1, 1, math.inf, [0], 1, False)
    assert idx.align_clip([q], 5, groups=["zzz"]) == [] and idx.align_clip([q], 0) == [] and idx.align_clip([q], 5, groups=[]) == []
    with pytest.raises(ValueError):
        idx.align_clip([np.ones(5, np.float32)], 5)                # the dimension, before the library is called
    assert len(seen) == 3


def test_align_group_reads_the_video_in_order_and_excludes_it(monkeypatch):
    ids = ["a_2", "a_0", "a_1", "b_0", "b_1", "a_3", "a_4"]
    idx = bare_index(ids, dimension=4)
    seen, read = [], []

    def read_rows(calls, h, rows, n, out):
        read.append([rows[i] for i in range(n)])
        fill(out, [1.0, 0.0, 0.0, 0.0] * n)

    fake_lib(monkeypatch, vq_index_align_clip=_canned(seen), vq_index_read_rows=read_rows)
    res = idx.align_group("a", 3)
    assert read[-1] == [1, 2, 0, 5, 6]                             # (position, id) order
    assert seen[-1] == (5, 2, math.inf, [0], 1, False) and res[0]["group"] == "b"
    idx.align_group("a", 3, max_frames=2)                          # every ceil(5 / 2) = 3rd frame
    assert read[-1] == [1, 5] and seen[-1][0] == 2
    idx.align_group("a", 3, max_frames=3)                          # every 2nd
    assert read[-1] == [1, 0, 6]
    idx.align_group("a", 3, groups=["a", "b"])                     # itself struck from the list
    assert seen[-1][3:5] == ([1], 0)
    assert idx.align_group("a", 3, groups=["a"]) == []
    with pytest.raises(KeyError):
        idx.align_group("zzz", 3)
    with pytest.raises(ValueError):
        idx.align_group("a", 3, max_frames=0)
    monkeypatch.setattr(type(idx), "ALIGN_MAX_FRAMES", 4)
    with pytest.raises(ValueError, match="max_frames"):
        idx.align_group("a", 3)
    idx.align_group("a", 3, max_frames=4)                          # every 2nd: three frames
    assert read[-1] == [1, 0, 6]


def test_simple_video_index_reports_timestamps(monkeypatch):
    from video_quierer_amd.overhaul_index import SimpleVideoIndex
    seen = []

    def align(calls, h, q, m, k, max_dist, labels, n_sel, excl, groups, dist, cost, rows, pairs):
        seen.append((m, k, max_dist, [labels[i] for i in range(n_sel)], excl))
        fill(groups, [1, -1][:k]); fill(dist, [0.125, np.inf][:k]); fill(cost, [m * 2 ** 21, 0][:k]); fill(rows, [3, 4, -1, -1][:2 * k])

    def read_rows(calls, h, rows, n, out):
        fill(out, [1.0, 0.0, 0.0, 0.0] * n)

    fake_device(monkeypatch, vq_index_align_clip=align, vq_index_read_rows=read_rows)
    sv = SimpleVideoIndex()
    for i, ts in enumerate((0.5, 1.25, 2.0)):
        sv.add_frame(np.eye(4, dtype=np.float32)[i], "clip.mp4", ts)
    sv.add_frame(np.eye(4, dtype=np.float32)[3], "other.mp4", 0.0)
    sv.add_frame(np.eye(4, dtype=np.float32)[3], "other.mp4", 4.0)
    res = sv.find_reuse_warped("clip.mp4", 5, min_similarity=0.75)
    assert seen[-1] == (3, 2, 0.25, [0], 1)                        # the video itself excluded; similarity -> distance
    assert res == [{"video_name": "other.mp4", "score": 0.875, "start": 0.0, "end": 4.0}]
    sv.find_reuse_warped("clip.mp4", 1)
    assert seen[-1] == (3, 1, math.inf, [0], 1)


# ---- the restatement ----
HAND = [[5, -1, -1, 5, 5],
        [5, 5, 5, 0, 5],
        [5, 5, 5, 0, 5]]


def test_restatement_on_a_hand_worked_example():
    """Three clip frames against a group of five rows.  (C, a) per cell, filled by the rules:
         i = 0:  (5,0)  (-1,1)  (-2,1)  (3,1)   (5,4)     (0,2): along the row from (0,1), -2, beats starting there, -1
         i = 1:  (10,0) (4,1)   (3,1)   (-2,1)  (3,1)     (1,3): down the diagonal from (0,2)
         i = 2:  (15,0) (9,1)   (8,1)   (-2,1)  (3,1)     (2,3): straight down from (1,3); (2,4): diagonal and horizontal tie, diagonal
    The best end is b = 3 with C = -2 and a = 1: frame 0 is paired with rows 1 .. 2, frames 1 and 2 with row 3."""
    for one in (align_brute, align_scan):
        assert one(HAND) == (-2, 1, 3, [(1, 2), (3, 3), (3, 3)])
        assert one(HAND[:1]) == (-2, 1, 2, [(1, 2)])               # m = 1: the cheapest stretch of the row
        assert one([[3], [4], [-9]]) == (-2, 0, 0, [(0, 0)] * 3)   # one row: the plain sum
        # equal cost: the later start wins inside a cell, then the shorter stretch, then the earlier start among the ends
        assert one([[0, 0, 0]]) == (0, 0, 0, [(0, 0)])
        assert one([[0, 0, 0], [0, 0, 0]]) == (0, 0, 0, [(0, 0), (0, 0)])
        assert one([[1, 0, 0, 1], [1, 1, 0, 0]])[:3] == (0, 2, 2)
    assert costs(np.array([0.5, 2 ** -25, 3 * 2 ** -25, 200.0, -200.0, np.nan], np.float32)).tolist() == \
        [2 ** 23, 0, 2, 2 ** 31, -2 ** 31, 2 ** 31]                # ties to even; kept within +-2^31; NaN
    assert rank_value(3 * 2 ** 22, 3) == np.float32(0.25)


def test_cell_by_cell_form_agrees_with_the_prefix_form_on_random_integer_tables():
    """Small tables of costs in -2 .. 2 (negative costs, plateaus, many equal keys): costs, starts, ends and alignments agree."""
    rng = np.random.default_rng(31)
    warped = 0
    for t in range(600):
        m, L = int(rng.integers(1, 7)), int(rng.integers(1, 9))
        c = rng.integers(-2, 3, (m, L)).astype(np.int64)
        if t % 3 == 0:
            c = np.repeat(c[:, :max(1, L // 2)], 2, axis=1)[:, :L]  # whole plateaus: neighbouring columns are equal
        a, b = align_brute(c), align_scan(c)
        assert a == b, (c, a, b)
        cost, start, end, pairs = a
        assert pairs[0][0] == start and pairs[-1][1] == end and cost == sum(int(c[i, f:l + 1].sum()) for i, (f, l) in enumerate(pairs))
        assert all(p[0] <= p[1] for p in pairs) and all(q[0] - p[1] in (0, 1) for p, q in zip(pairs, pairs[1:]))
        warped += any(p[0] != p[1] for p in pairs) or any(q[0] == p[1] for p, q in zip(pairs, pairs[1:]))
    assert warped > 200, warped


def _trajectory(rng, n, dim, step):
    x = rng.standard_normal(dim)
    out = np.empty((n, dim), np.float32)
    for i in range(n):
        x = x / np.linalg.norm(x)
        out[i] = x
        x = x + rng.standard_normal(dim) * (step / math.sqrt(dim))
    return out


def _noisy(rng, rows, noise):
    q = rows + rng.standard_normal(rows.shape) * (noise / math.sqrt(rows.shape[1]))
    return (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)


def test_a_clip_at_another_pace_is_found_by_the_warp_and_lost_by_the_diagonal_runs():
    """Three videos of 120 frames, each a smooth trajectory (neighbouring frames 0.02 apart).  A clip that is every second frame of
    frames 30 .. 68 of video 1, with small noise, and one that shows frames 40 .. 59 twice each: the warp names video 1 and the
    stretch to within one stored frame; the best diagonal run at max_miss = 0, at a threshold that admits a frame and its two
    neighbours at the most, covers less than half of either clip."""
    rng = np.random.default_rng(77)
    dim, n = 64, 120
    rows = np.concatenate([_trajectory(rng, n, dim, 0.2) for _ in range(3)])
    labels = np.repeat(np.arange(3), n)
    pos = np.tile(np.arange(n), 3)
    tie = np.arange(3 * n)
    fast = _noisy(rng, rows[n + 30:n + 70:2], 0.03)                # 20 frames at twice the pace
    slow = _noisy(rng, np.repeat(rows[n + 40:n + 60], 2, axis=0), 0.03)      # 40 frames at half the pace
    for clip, first, last in ((fast, n + 30, n + 68), (slow, n + 40, n + 59)):
        dist = (np.float32(1) - (clip.astype(np.float64) @ rows.astype(np.float64).T).astype(np.float32)).astype(np.float32)
        ans, holding, _ = align_answer(dist, labels, pos, tie, k=3)
        assert holding == 3 and ans[0][0] == 1 and ans[0][1] < np.float32(0.1) < ans[1][1]
        (a, b), pairs = ans[0][3], ans[0][4]
        assert abs(a - first) <= 1 and abs(b - last) <= 1, (a, b)
        assert len(pairs) == len(clip) and pairs[0][0] == a and pairs[-1][1] == b
        assert align_answer(dist, labels, pos, tie, max_dist=np.float32(0.1), k=3)[0] == ans[:1]
        assert align_answer(dist[::-1], labels, pos, tie, k=3)[0][0][2] > 4 * ans[0][2]       # the reversed clip fits nowhere
        # the neighbours of the true frame lie about 0.02 away: a threshold of 0.03 hits them, never three frames further
        hit = match_ref.hit_table(dist, np.float32(0.03))
        run = match_ref.best_run(hit, match_ref.order_of(np.flatnonzero(labels == 1), pos, tie), 1, 0)
        assert run is not None and run[1] < len(clip) / 2, run
