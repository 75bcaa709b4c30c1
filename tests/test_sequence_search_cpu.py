"""Host side of the sequence search without a device: the exported symbols, the plan (step chunks at the 512 MiB rule, the LDS
form's row limit, the environment overrides), the argument checks that come before the device is touched, and the numpy
restatement of the definition on a hand-worked example."""
from ctypes import POINTER, byref, c_float, c_int, c_int32, c_int64

import numpy as np
import pytest

from test_sequence_search import group_dp, sequence_answer, set_distance, window_dp

ENV = ("VQ_AMD_SEQ_LDS_ROWS", "VQ_AMD_SEQ_DIST_BYTES", "VQ_AMD_SEQ_BP_BYTES")


def _plan(n, largest, m, k=10):
    from video_quierer_amd import _lib
    chunks, lds_rows, glob, table, slices = c_int(), c_int(), c_int(), c_int(), c_int()
    lds_bytes = c_int64()
    _lib.check(_lib.load().vq_debug_sequence_plan(n, largest, m, k, byref(chunks), byref(lds_rows), byref(glob), byref(lds_bytes),
                                                  byref(table), byref(slices)))
    return dict(chunks=chunks.value, lds_rows=lds_rows.value, global_form=glob.value, lds_bytes=lds_bytes.value,
                table=table.value, slices=slices.value)


@pytest.fixture
def no_overrides(monkeypatch):
    for name in ENV:
        monkeypatch.delenv(name, raising=False)
    return monkeypatch


def test_new_symbols_are_exported():
    from video_quierer_amd import _lib
    lib = _lib.load()
    for name in ("vq_index_search_sequence", "vq_index_search_sequence_device", "vq_debug_sequence_plan"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert _lib.IDX_NCLASS == 7 and lib.vq_index_profile_class_name(6).decode() == "sequence_dp"
    assert lib.vq_index_profile_class_name(2).decode() == "exact_dist_f64chain"
    import video_quierer_amd
    video_quierer_amd.install_dropin()
    from indexes.hnsw import HNSWIndex
    from video_quierer_amd.overhaul_index import SimpleVideoIndex
    assert callable(HNSWIndex.search_sequence) and callable(SimpleVideoIndex.search_storyboard)


def test_plan_chunks_keep_the_distances_within_512_mib(no_overrides):
    # 2^27 floats: 1M rows (padded to 64) -> 134 steps fit, so every m <= 64 is one chunk; 2^22 rows -> 32 steps per chunk
    assert _plan(1_000_000, 500, 64)["chunks"] == 1
    assert _plan(2 ** 22, 500, 64)["chunks"] == 2 and _plan(2 ** 22, 500, 32)["chunks"] == 1
    assert _plan(2 ** 22, 500, 33)["chunks"] == 2 and _plan(2 ** 22 + 1, 500, 32)["chunks"] == 2       # (rows padded to 64)
    assert _plan(2 ** 27, 500, 64)["chunks"] == 64 and _plan(2 ** 31 - 1, 500, 5)["chunks"] == 5       # one step at the least
    for n, m in ((1, 1), (5_000, 64), (3_000_000, 64), (50_000_000, 17)):
        p = _plan(n, 1, m)
        ld = (n + 63) // 64 * 64
        per = -(-m // p["chunks"])
        assert per * ld * 4 <= 512 << 20 or per == 1


def test_plan_lds_form_covers_4096_rows_within_a_cu(no_overrides):
    p = _plan(1_000_000, 4_096, 8)
    assert p["lds_rows"] >= 4_096 and p["global_form"] == 0
    assert p["lds_bytes"] <= 160 << 10                             # the LDS of one gfx950 CU
    assert _plan(1_000_000, p["lds_rows"] + 1, 8)["global_form"] == 1
    assert _plan(1_000_000, 1_000_000, 8)["global_form"] == 1      # one group of a million rows is legal
    small = _plan(1_000_000, 500, 8)
    assert small["lds_bytes"] == 512 * 36 + 8 * 4                  # sized for the longest group: 500 rows -> 512
    assert small["lds_bytes"] * 8 <= 160 << 10                     # eight such workgroups share a CU


def test_plan_chains_table_or_slices(no_overrides):
    assert _plan(1_000_000, 500, 64) | {} == _plan(1_000_000, 500, 64)
    assert _plan(1_000_000, 500, 64)["table"] == 1                 # 63 x 1M x 4 B = 252 MB <= 256 MiB
    p = _plan(2_000_000, 500, 64)
    assert p["table"] == 0 and p["slices"] == 2                    # 33 transitions per slice
    assert _plan(2 ** 27, 500, 64) ["slices"] == 63                 # one transition per slice at the least
    assert _plan(2 ** 27, 500, 1)["slices"] == 0


def test_plan_honours_the_overrides(no_overrides):
    mp = no_overrides
    mp.setenv("VQ_AMD_SEQ_LDS_ROWS", "128")
    p = _plan(4_820, 700, 8)
    assert p["lds_rows"] == 128 and p["global_form"] == 1 and p["lds_bytes"] == 128 * 36 + 2 * 4
    mp.setenv("VQ_AMD_SEQ_LDS_ROWS", "100000")                     # never above what the LDS holds
    assert _plan(4_820, 700, 8)["lds_rows"] == 4_096
    mp.delenv("VQ_AMD_SEQ_LDS_ROWS")
    ld = (4_820 + 63) // 64 * 64
    mp.setenv("VQ_AMD_SEQ_DIST_BYTES", str(3 * ld * 4))
    assert _plan(4_820, 700, 8)["chunks"] == 3 and _plan(4_820, 700, 64)["chunks"] == 22 and _plan(4_820, 700, 3)["chunks"] == 1
    mp.setenv("VQ_AMD_SEQ_DIST_BYTES", "1")
    assert _plan(4_820, 700, 8)["chunks"] == 8
    mp.delenv("VQ_AMD_SEQ_DIST_BYTES")
    mp.setenv("VQ_AMD_SEQ_BP_BYTES", str(2 * 4_820 * 4))
    assert _plan(4_820, 700, 8)["table"] == 0 and _plan(4_820, 700, 8)["slices"] == 4 and _plan(4_820, 700, 3)["table"] == 1
    mp.delenv("VQ_AMD_SEQ_BP_BYTES")
    assert _plan(4_820, 700, 8) == dict(chunks=1, lds_rows=4_096, global_form=0, lds_bytes=704 * 36 + 11 * 4, table=1, slices=0)
    for bad in ((0, 1, 1), (10, 0, 1), (10, 11, 1), (10, 5, 0), (10, 5, 65), (2 ** 31, 5, 1)):
        with pytest.raises(ValueError):
            _plan(*bad)
    with pytest.raises(ValueError):
        _plan(10, 5, 3, k=0)
    with pytest.raises(ValueError):
        _plan(10, 5, 3, k=1025)


def test_c_abi_refuses_bad_arguments_before_the_device():
    from video_quierer_amd import _lib
    lib = _lib.load()
    q = np.zeros((65, 8), np.float32); g = np.empty(1025, np.int32); d = np.empty(1025, np.float32)
    gp, dp = g.ctypes.data_as(POINTER(c_int32)), d.ctypes.data_as(POINTER(c_float))
    for m, k, lo, hi in ((0, 5, 1, 8), (65, 5, 1, 8), (-1, 5, 1, 8), (3, 0, 1, 8), (3, 1025, 1, 8), (3, 5, 0, 8), (3, 5, 9, 8), (3, 5, -2, -1)):
        rc = lib.vq_index_search_sequence(None, _lib.fptr(q), m, k, c_int64(lo), c_int64(hi), None, 0, 1, gp, dp, None)
        assert rc < 0, (m, k, lo, hi)
        msg = lib.vq_last_error().decode()
        assert ("min_gap" in msg) == (lo < 1 or hi < lo), msg
        assert lib.vq_index_search_sequence_device(None, None, m, k, c_int64(lo), c_int64(hi), None, 0, 1, None, None, None) < 0


def test_wrapper_argument_checks():
    from video_quierer_amd.indexes.hnsw import HNSWIndex
    from video_quierer_amd.overhaul_index import SimpleVideoIndex
    idx = HNSWIndex.__new__(HNSWIndex)                             # the checks below come before the handle is touched
    idx.entry_point, idx.element_count = None, 0
    q = np.ones(8, np.float32)
    with pytest.raises(ValueError):
        idx.search_sequence([], 5, max_gap=3)
    with pytest.raises(ValueError):
        idx.search_sequence([q] * 65, 5, max_gap=3)
    for lo, hi in ((0, 3), (4, 3), (-1, -1)):
        with pytest.raises(ValueError):
            idx.search_sequence([q, q], 5, max_gap=hi, min_gap=lo)
    with pytest.raises(TypeError):
        idx.search_sequence([q, q], 5)                             # max_gap has no default
    with pytest.raises(ValueError):
        idx.search_sequence([q], 5, max_gap=3, within=["a"], exclude=["b"])
    assert idx.search_sequence([q, q], 5, max_gap=3) == []         # an empty index
    sv = SimpleVideoIndex()
    with pytest.raises(ValueError):
        sv.search_storyboard([])
    with pytest.raises(ValueError):
        sv.search_storyboard([q] * 65)
    for kw in (dict(max_gap_s=1.0, min_gap_s=2.0), dict(min_gap_s=-1.0), dict(max_gap_s=0.0005)):
        with pytest.raises(ValueError):
            sv.search_storyboard([q, q], **kw)
    assert sv.search_storyboard([q, q]) == []


def test_restatement_on_a_hand_worked_example():
    """Six rows of one group at positions 0 1 2 2 3 5, three steps, gaps 1..2, distances in eighths (every sum exact).
      C_0 = d_0                        = .5   .25  .75  .125 1.   .5
      C_1: r0 -      r1 <- r0: 1.      r2 <- r1: .5     r3 <- r1: .5     r4 <- r3 (.125 beats .25, .75): .625    r5 <- r4: 2.
      C_2: r0 -      r1 - (r0 undefined)      r2 <- r1: 2.      r3 <- r1: 1.5
           r4 <- r2 (.5 = .5: rows 2 and 3 tie, the smaller tie wins): .75       r5 <- r4: .625 + .125 = .75
      end: r4 and r5 tie at .75 -> r4;  D = .75 / 3 = .25;  chain r1 -> r2 -> r4.
    With the ties reversed row 3 beats row 2 and row 5 beats row 4: chain r3 -> r4 -> r5, the same D."""
    pos = [0, 1, 2, 2, 3, 5]
    dist = [np.array(d, np.float32) for d in ([.5, .25, .75, .125, 1., .5], [1., .5, .25, .25, .5, 1.], [1., 1., 1., .5, .25, .125])]
    rows = np.arange(6)
    D, chain, decided = group_dp(dist, rows, pos, np.arange(6), 1, 2)
    assert D == np.float32(0.25) and chain == [1, 2, 4] and decided
    D, chain, decided = group_dp(dist, rows, pos, np.arange(6)[::-1], 1, 2)
    assert D == np.float32(0.25) and chain == [3, 4, 5] and decided
    # gaps 2..2: 0 -> 2 -> (no position 4) ...: r5 <- r4 <- r1 is the only chain (positions 1, 3, 5)
    D, chain, _ = group_dp(dist, rows, pos, np.arange(6), 2, 2)
    assert chain == [1, 4, 5] and D == np.float32((.25 + .5 + .125) / 3)
    assert group_dp(dist, rows, pos, np.arange(6), 3, 3) is None   # 0 -> 3 -> 6, 2 -> 5 -> 8: no third row
    assert group_dp(dist[:1], rows, pos, np.arange(6), 1, 2)[:2] == (np.float32(.125), [3])       # one step: the group's best row
    # two rows at one position never follow each other, whatever the gaps allow
    assert group_dp(dist[:2], np.array([2, 3]), pos, np.arange(6), 1, 2 ** 40) is None
    # the clip search's D ignores the order: .125 + .25 + .125
    assert set_distance(dist, rows) == np.float32(.5 / 3) <= D
    # two groups: labels by (D, label); a group without a chain never appears
    labels = np.array([0, 0, 0, 0, 0, 0, 1, 1], np.int32)
    dist2 = [np.concatenate([d, np.array([.0, .0], np.float32)]) for d in dist]
    ans, _, holding = sequence_answer(dist2, labels, pos + [7, 7], np.arange(8), 1, 2, 5)
    assert holding == 1 and [(g, c) for g, _, c in ans] == [(0, [1, 2, 4])]
    ans, _, holding = sequence_answer(dist2[:1], labels, pos + [7, 7], np.arange(8), 1, 2, 5)
    assert holding == 2 and [(g, float(dd), c) for g, dd, c in ans] == [(1, 0.0, [6]), (0, 0.125, [3])]


def test_window_restatement_agrees_with_the_table_restatement():
    """`window_dp` (long groups at positions 0, 1, 2, ..) against `group_dp`, with planted equal costs so that ties decide."""
    rng = np.random.default_rng(5)
    L, m = 200, 4
    dist = [np.round(rng.uniform(0, 1, L + 7) * 8).astype(np.float32) / 8 for _ in range(m)]      # eighths: many equal costs
    rows = np.arange(3, L + 3)
    pos = np.arange(L + 7) - 3
    tie = rng.permutation(L + 7)
    decided = []
    for min_gap, max_gap in ((1, 2 ** 40), (1, 1), (2, 7), (60, 70), (80, 90), (150, 2 ** 40)):
        a = group_dp(dist, rows, pos, tie, min_gap, max_gap)
        b = window_dp(dist, rows, tie, min_gap, min(max_gap, 10_000))
        assert (a is None) == (b is None), (min_gap, max_gap)
        if a is not None:
            assert a[0].tobytes() == b[0].tobytes() and a[1] == b[1], (min_gap, max_gap)
            decided.append(a[2])
    assert decided[0] and decided[2]                               # the tie chose somewhere where a row has several predecessors
    assert group_dp(dist, rows, pos, tie, 80, 90) is None and group_dp(dist, rows, pos, tie, 60, 70) is not None
