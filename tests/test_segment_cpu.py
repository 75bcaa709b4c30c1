"""Host side of chapter segmentation without a device: the exported symbols, the plan (batches, table bytes, the DP's LDS row
limit and bytes, the global form, launches, pairs, the environment overrides), the argument checks that come before the device
is touched, the numpy restatement of the definition on hand cases with a closed form, the prefix order, and the Python layer
over a recording library."""
import math
from ctypes import POINTER, byref, c_float, c_int, c_int32, c_int64

import numpy as np
import pytest

import segment_ref
from cluster_ref import cancelling_rows
from index_host_fakes import bare_index, fake_device, fake_lib, fill

COST_ENV, LDS_ENV = "VQ_AMD_SEG_COST_BYTES", "VQ_AMD_SEG_LDS_ROWS"
CANCEL_SEED, CANCEL_ROWS, CANCEL_DIM = 4, 96, 16                  # test_segment.py adds the same rows to a device index


def _plan(lengths, dim=512, k=8, max_len=0):
    from video_quierer_amd import _lib
    L = np.ascontiguousarray(lengths, dtype=np.int64)
    batches, lds_rows, glob, launches = c_int(), c_int(), c_int(), c_int()
    table, lds_bytes, pairs = c_int64(), c_int64(), c_int64()
    _lib.check(_lib.load().vq_debug_segment_plan(L.ctypes.data_as(POINTER(c_int64)), len(L), dim, k, max_len, byref(batches), byref(table),
                                                 byref(lds_rows), byref(lds_bytes), byref(glob), byref(launches), byref(pairs)))
    return dict(batches=batches.value, table_bytes=table.value, lds_rows=lds_rows.value, lds_bytes=lds_bytes.value, global_form=glob.value,
                launches=launches.value, pairs=pairs.value)


@pytest.fixture
def no_override(monkeypatch):
    monkeypatch.delenv(COST_ENV, raising=False)
    monkeypatch.delenv(LDS_ENV, raising=False)
    return monkeypatch


def test_new_symbols_are_exported():
    from video_quierer_amd import _lib
    lib = _lib.load()
    for name in ("vq_index_segment_groups", "vq_index_segment_groups_device", "vq_debug_segment_plan"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert _lib.IDX_NCLASS == 7 and lib.vq_index_profile_class_name(2).decode() == "exact_dist_f64chain"
    from video_quierer_amd.indexes.hnsw import HNSWIndex
    from video_quierer_amd.overhaul_index import SimpleVideoIndex
    assert callable(HNSWIndex.segment_group) and callable(HNSWIndex.segment_groups) and callable(SimpleVideoIndex.video_chapters)


# ---- the plan ----
def test_plan_of_the_library_shape_and_of_one_long_video(no_override):
    lib = _plan([500] * 2_000)
    # a batch ends where its prefix rows would pass 512 MiB: 261 groups x 501 rows x 4 KiB; the tables alone would allow 268
    assert lib["batches"] == 8 and lib["table_bytes"] == 261 * 500 * 500 * 8
    assert lib["pairs"] == 2_000 * (500 * 501 // 2) and lib["launches"] == 8 * 4 + 1
    assert lib["lds_rows"] == 4_096 and lib["lds_bytes"] == 2 * 512 * 8 and lib["global_form"] == 0
    one = _plan([4_096])
    assert one == dict(batches=1, table_bytes=4_096 * 4_096 * 8, lds_rows=4_096, lds_bytes=2 * 4_160 * 8, global_form=0, launches=5,
                       pairs=4_096 * 4_097 // 2)
    assert one["lds_bytes"] <= 160 << 10                             # the LDS of one gfx950 CU
    over = _plan([4_097, 10])
    assert over["global_form"] == 1 and over["lds_bytes"] == 2 * 64 * 8          # sized for the longest group that stays in LDS
    banded = _plan([100_000], max_len=7)
    assert banded["table_bytes"] == 100_000 * 7 * 8 and banded["pairs"] == 7 * 100_000 - 21 and banded["global_form"] == 1
    assert _plan([25], max_len=40) == _plan([25])                    # max_len >= L is the same as none
    assert _plan([0, 3])["pairs"] == 6 and _plan([0])["table_bytes"] == 0        # a label without rows costs nothing


def test_plan_batches_follow_the_budget(no_override):
    mp = no_override
    mp.setenv(COST_ENV, str(2 * 100 * 100 * 8))                      # two 100-row tables
    p = _plan([100] * 6, dim=64)
    assert p["batches"] == 3 and p["table_bytes"] == 2 * 100 * 100 * 8 and p["launches"] == 3 * 4 + 1
    assert _plan([100] * 7, dim=64)["batches"] == 4
    assert _plan([300, 1, 1, 300], dim=64)["batches"] == 3           # a group above the budget is a batch of its own
    mp.setenv(COST_ENV, "1")
    assert _plan([5, 6, 7], dim=64)["batches"] == 3                  # at least one group per batch
    mp.setenv(COST_ENV, "0")                                         # not a budget
    assert _plan([100] * 6, dim=64)["batches"] == 1
    mp.delenv(COST_ENV)
    mp.setenv(LDS_ENV, "64")
    p = _plan([64, 65], dim=64)
    assert p["lds_rows"] == 64 and p["global_form"] == 1 and p["lds_bytes"] == 2 * 128 * 8
    mp.setenv(LDS_ENV, "100000")                                     # never above what the LDS form was built for
    assert _plan([5_000], dim=64)["lds_rows"] == 4_096


def test_plan_refuses_what_the_call_refuses(no_override):
    assert _plan([8_192])["pairs"] == 8_192 * 8_193 // 2             # 2^26 pairs exactly: the bound itself is allowed
    with pytest.raises(ValueError, match="group 1 holds 8193 rows.*2\\^26 pairs"):
        _plan([10, 8_193])
    assert _plan([8_193], max_len=8_191)["batches"] == 1             # 2^26 - 1 pairs
    for bad in (dict(lengths=[]), dict(lengths=[5], dim=0), dict(lengths=[5], dim=514), dict(lengths=[5], k=0), dict(lengths=[5], k=65),
                dict(lengths=[5], max_len=-1), dict(lengths=[-1])):
        with pytest.raises(ValueError):
            _plan(**bad)


def test_c_abi_refuses_bad_arguments_before_the_device():
    from video_quierer_amd import _lib
    lib = _lib.load()
    g = np.zeros(4, np.int32)
    cnt, a, b, n, s = (np.empty(4 * 65, np.int32) for _ in range(5))
    f = np.empty(4 * 65, np.float32)
    ip = lambda x: x.ctypes.data_as(POINTER(c_int32))
    fp = f.ctypes.data_as(POINTER(c_float))
    for n_sel, k, pen, max_len, word in ((0, 5, 0.0, 0, "n_sel"), (-2, 5, 0.0, 0, "n_sel"), (4, 0, 0.0, 0, "k 0"), (4, 65, 0.0, 0, "k 65"),
                                         (4, 5, -0.5, 0, "penalty"), (4, 5, math.nan, 0, "penalty"), (4, 5, 0.0, -1, "max_len")):
        rc = lib.vq_index_segment_groups(None, ip(g), n_sel, k, c_float(pen), max_len, ip(cnt), ip(a), ip(b), ip(n), fp, ip(s), None)
        msg = lib.vq_last_error().decode()
        assert rc == -1 and word in msg and "vq_index_segment_groups" in msg, (n_sel, k, pen, max_len, msg)
        assert lib.vq_index_segment_groups_device(None, ip(g), n_sel, k, c_float(pen), max_len, None, None, None, None, None, None, None) == -1
        assert word in lib.vq_last_error().decode()


# ---- the restatement on hand cases with a closed form ----
def one_hot_blocks(lengths=(4, 5, 3), dim=4):
    x = np.zeros((sum(lengths), dim), dtype=np.float32)
    at = 0
    for j, n in enumerate(lengths):
        x[at:at + n, j] = 1.0
        at += n
    return x


def test_one_hot_blocks_have_a_closed_form():
    x = one_hot_blocks()
    order, tie = list(range(12)), np.arange(12)
    P, C = segment_ref.tables(x, order, 12)
    for a0, b0 in ((0, 4), (4, 9), (9, 12)):                         # every pure run costs exactly 0.0
        for a in range(a0, b0):
            for b in range(a + 1, b0 + 1):
                assert C[b][b - a - 1] == 0.0 and not np.signbit(C[b][b - a - 1])
    assert C[9][8] == 9.0 - math.sqrt(16.0 + 25.0)                   # [0, 9): u = (4, 5, 0, 0)
    got = segment_ref.segment(x, order, tie, 5, 0.0, 12)
    assert got["count"] == 3 and got["cuts"] == [(0, 4), (4, 9), (9, 12)]
    assert got["first"].tolist() == [0, 4, 9] and got["last"].tolist() == [3, 8, 11] and got["len"].tolist() == [4, 5, 3]
    assert got["spread"].tolist() == [0.0, 0.0, 0.0] and got["mean_spread"] == 0.0
    assert got["show"].tolist() == [0, 4, 9]                         # all rows of a chapter tie: the smallest tie
    two = segment_ref.segment(x, order, tie, 2, 0.0, 12)
    assert two["cuts"] == [(0, 4), (4, 12)]                          # 8 - sqrt(34) = 2.169 beats 9 - sqrt(41) = 2.597
    assert two["spread"].tobytes() == np.array([0.0, (8.0 - math.sqrt(34.0)) / 8.0], dtype=np.float32).tobytes()
    assert two["mean_spread"] == np.float32((8.0 - math.sqrt(34.0)) / 12.0)
    one = segment_ref.segment(x, order, tie, 1, 0.0, 12)
    assert one["cuts"] == [(0, 12)] and one["spread"][0] == np.float32((12.0 - math.sqrt(50.0)) / 12.0)
    assert segment_ref.segment(x, order, tie, 5, 1e9, 12)["cuts"] == [(0, 12)]           # a huge penalty: one chapter
    assert segment_ref.segment(x, order, tie, 5, 0.25, 12)["cuts"] == [(0, 4), (4, 9), (9, 12)]
    # a reversed tie order picks the other end of each chapter
    assert segment_ref.segment(x, order, 11 - tie, 5, 0.0, 12)["show"].tolist() == [3, 8, 11]
    # the order is (position, tie), not the row number
    pos = np.array([3, 2, 1, 0, 4, 4, 4, 4, 4, 9, 8, 7])
    assert segment_ref.order_of(range(12), pos, tie) == [3, 2, 1, 0, 4, 5, 6, 7, 8, 11, 10, 9]


def test_feasibility_under_max_len():
    x = np.random.default_rng(5).standard_normal((25, 8)).astype(np.float32)
    order, tie = list(range(25)), np.arange(25)
    tab = segment_ref.tables(x, order, 7)
    none = segment_ref.segment(x, order, tie, 3, 0.0, 7, tab)
    assert none["count"] == 0 and len(none["first"]) == 0 and np.isinf(none["mean_spread"])       # 3 x 7 < 25
    four = segment_ref.segment(x, order, tie, 4, 0.0, 7, tab)
    assert four["count"] == 4 and four["len"].sum() == 25 and four["len"].max() <= 7
    assert segment_ref.segment(x, order, tie, 64, 1e9, 7, tab)["count"] == 4             # the fewest chapters that cover the group
    assert segment_ref.segment(x, order, tie, 64, 0.0, 1, segment_ref.tables(x, order, 1))["len"].tolist() == [1] * 25
    assert segment_ref.run_limit(25, 0) == 25 and segment_ref.run_limit(25, 40) == 25 and segment_ref.run_limit(25, 7) == 7


def cancelling_group():
    return cancelling_rows(np.random.default_rng(CANCEL_SEED), CANCEL_ROWS, CANCEL_DIM)


def test_the_prefix_order_is_pinned():
    """On rows whose large terms cancel, a run's direction u is what the prefix additions rounded away: a tree-order prefix gives
    other cost bits than the chain, and with this seed other cuts and spreads for k = 5.  test_segment.py runs the same rows on
    the device with k = 5, so the answer there tells the two orders apart."""
    x = cancelling_group()
    order, tie = list(range(CANCEL_ROWS)), np.arange(CANCEL_ROWS)
    P = segment_ref.prefix_rows(x, order)
    T = segment_ref.tree_prefix_rows(x, order)
    assert np.allclose(P, T, rtol=0, atol=1e-12) and P.tobytes() != T.tobytes()
    C, D = segment_ref.cost_table(P, CANCEL_ROWS), segment_ref.cost_table(T, CANCEL_ROWS)
    ok = ~np.isnan(C)
    differ = int((C[ok].view(np.uint64) != D[ok].view(np.uint64)).sum())
    print(f"{differ} of {int(ok.sum())} costs differ in bits between the chain and the tree prefix")
    assert differ > 0
    chain = [segment_ref.segment(x, order, tie, k, 0.0, CANCEL_ROWS, (P, C)) for k in (2, 5)]
    tree = [segment_ref.segment(x, order, tie, k, 0.0, CANCEL_ROWS, (T, D)) for k in (2, 5)]
    print("chain cuts", [c["cuts"] for c in chain], "tree cuts", [t["cuts"] for t in tree])
    assert any(c["cuts"] != t["cuts"] or c["show"].tolist() != t["show"].tolist() for c, t in zip(chain, tree))


# ---- the Python layer over a recording library ----
IDS = ["a_0", "a_10", "a_2", "b_0", "b_1", "c_0"]                      # string ids: the tie order is uploaded first


def segment_entry(answers):
    """vq_index_segment_groups answering label g with answers[g] = [(first, last, frames, spread, show), ..]; recorded."""
    def entry(calls, h, groups, n_sel, k, penalty, max_len, count, first, last, frames, spread, show, mean):
        labels = [groups[i] for i in range(n_sel)]
        calls.append(("segment", labels, k, penalty, max_len))
        assert not mean
        for e, g in enumerate(labels):
            got = answers.get(g, [])[:k]
            count[e] = len(got)
            ans = got + [(-1, -1, 0, np.inf, -1)] * (k - len(got))
            for j, out in enumerate((first, last, frames, spread, show)):
                fill(out, [a[j] for a in ans], e * k)
    return entry


def test_segment_groups_uploads_in_order_and_shapes_the_result(monkeypatch):
    answers = {0: [(0, 2, 2, 0.25, 0), (1, 1, 1, 0.0, 1)], 1: [(3, 4, 2, 0.125, 4)], 2: []}
    calls = fake_lib(monkeypatch, vq_index_segment_groups=segment_entry(answers))
    idx = bare_index(IDS)
    res = idx.segment_groups(k=3)
    # _prepare's order: tie order, labels, positions (frame_of: a_0, a_10, a_2 -> 0, 10, 2)
    assert [c[0] for c in calls] == ["set_id_ranks", "set_groups", "set_positions", "segment"]
    assert calls[1] == ("set_groups", [0, 0, 0, 1, 1, 2], 3) and calls[2] == ("set_positions", [0, 10, 2, 0, 1, 0])
    assert calls[3] == ("segment", [0, 1, 2], 3, 0.0, 0)
    assert res == {"a": [{"first": "a_0", "last": "a_2", "frames": 2, "spread": np.float32(0.25), "show": "a_0"},
                         {"first": "a_10", "last": "a_10", "frames": 1, "spread": np.float32(0.0), "show": "a_10"}],
                   "b": [{"first": "b_0", "last": "b_1", "frames": 2, "spread": np.float32(0.125), "show": "b_1"}],
                   "c": []}
    assert type(res["a"][0]["spread"]) is np.float32
    del calls[:]
    assert idx.segment_groups(["c", "a", "c"], 300, penalty=0.5, max_len=9) == {"c": [], "a": res["a"]}
    assert calls == [("segment", [2, 0], 64, 0.5, 9)]               # nothing is uploaded twice; a key once; k capped at the limit
    assert idx.segment_group("b", 1) == res["b"]
    del calls[:]
    with pytest.raises(KeyError):
        idx.segment_groups(["a", "nope"])                            # before any device work
    with pytest.raises(KeyError):
        idx.segment_group("nope", 0)
    for bad in (dict(penalty=-1.0), dict(penalty=math.nan), dict(max_len=0), dict(max_len=-3)):
        with pytest.raises(ValueError):
            idx.segment_group("a", 3, **bad)
    assert idx.segment_group("a", 0) == [] and idx.segment_groups(k=-1) == {"a": [], "b": [], "c": []}
    assert idx.segment_groups([]) == {} and calls == []
    assert bare_index([]).segment_groups() == {}


def test_video_chapters_shapes_its_result(monkeypatch):
    from video_quierer_amd.overhaul_index import SimpleVideoIndex
    calls = fake_device(monkeypatch, vq_index_segment_groups=segment_entry({1: [(2, 3, 2, 0.5, 3), (4, 4, 1, 0.0, 4)]}))
    sv = SimpleVideoIndex()
    for i, (name, ts) in enumerate([("x.mp4", 0.0), ("x.mp4", 0.5), ("y.mp4", 0.0), ("y.mp4", 0.75), ("y.mp4", 1.5)]):
        sv.add_frame(np.full(4, i + 1.0, np.float32), name, ts)
    got = sv.video_chapters("y.mp4", 3, penalty=0.25, max_frames=10)
    assert got == [{"start": 0.0, "end": 0.75, "frames": 2, "spread": 0.5, "poster": {"video_name": "y.mp4", "timestamp": 0.75, "frame_id": 3}},
                   {"start": 1.5, "end": 1.5, "frames": 1, "spread": 0.0, "poster": {"video_name": "y.mp4", "timestamp": 1.5, "frame_id": 4}}]
    assert ("segment", [1], 3, 0.25, 10) in calls
    # positions are round(timestamp * 1000) ms
    assert [c for c in calls if c[0] == "set_positions"][-1] == ("set_positions", [0, 500, 0, 750, 1500])
    with pytest.raises(KeyError):
        sv.video_chapters("z.mp4")
    with pytest.raises(KeyError):
        SimpleVideoIndex().video_chapters("y.mp4")
