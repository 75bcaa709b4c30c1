"""Host side of the keyframe summary without a device: the exported symbols, the plan (the LDS form's row limit and bytes, the
wide form, the launch count, the environment override), the argument checks that come before the device is touched, the
Python layer over a recording library, and the numpy restatement of the definition on a hand-worked example."""
import math
from ctypes import POINTER, byref, c_float, c_int, c_int32, c_int64

import numpy as np
import pytest

from index_host_fakes import bare_index, fake_lib, fill
from test_keyframe_summary import mean_direction, summarize

ENV = "VQ_AMD_SUM_LDS_ROWS"
CU_LDS = 160 << 10                                                 # the LDS of one gfx950 CU


def _plan(n, largest, dim=512, k=8):
    from video_quierer_amd import _lib
    lds_rows, wide, launches = c_int(), c_int(), c_int()
    lds_bytes = c_int64()
    _lib.check(_lib.load().vq_debug_summary_plan(n, largest, dim, k, byref(lds_rows), byref(lds_bytes), byref(wide), byref(launches)))
    return dict(lds_rows=lds_rows.value, lds_bytes=lds_bytes.value, wide=wide.value, launches=launches.value)


@pytest.fixture
def no_override(monkeypatch):
    monkeypatch.delenv(ENV, raising=False)
    return monkeypatch


def test_new_symbols_are_exported():
    from video_quierer_amd import _lib
    lib = _lib.load()
    for name in ("vq_index_summarize_groups", "vq_index_summarize_groups_device", "vq_debug_summary_plan"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert _lib.IDX_NCLASS == 7 and lib.vq_index_profile_class_name(6).decode() == "sequence_dp"
    assert lib.vq_index_profile_class_name(2).decode() == "exact_dist_f64chain"        # the class the new launches are accounted under
    import video_quierer_amd
    video_quierer_amd.install_dropin()
    from indexes.hnsw import HNSWIndex
    from video_quierer_amd.overhaul_index import SimpleVideoIndex
    assert callable(HNSWIndex.summarize_group) and callable(HNSWIndex.summarize_groups)
    assert callable(SimpleVideoIndex.video_summary)


def test_plan_lds_form_covers_4096_rows_within_a_cu(no_override):
    for dim in (512, 768):
        p = _plan(1_000_000, 4_096, dim)
        assert p["lds_rows"] >= 4_096 and p["wide"] == 0
        assert p["lds_bytes"] <= CU_LDS
        assert p["lds_bytes"] == dim * 8 + 64 + 1_024 + 4_096 * 14       # the centre in fp64, the fixed words, 14 B per row
        assert _plan(1_000_000, p["lds_rows"] + 1, dim)["wide"] == 1
        assert _plan(1_000_000, 1_000_000, dim)["wide"] == 1             # one group of a million rows is legal
    small = _plan(500_000, 500)                                          # sized for the longest group: 500 rows -> 512
    assert small["lds_bytes"] == 512 * 8 + 64 + 1_024 + 512 * 14 and small["lds_bytes"] * 8 <= CU_LDS
    assert _plan(500_000, 3_600)["lds_bytes"] * 2 <= CU_LDS              # the sampler's cap: two workgroups share a CU


def test_plan_launches_depend_on_the_shapes_and_k_only(no_override):
    for k in (1, 8, 256):
        assert {_plan(n, largest, dim, k)["launches"] for n, largest, dim in ((10, 1, 64), (10**6, 500, 512), (10**9, 4_096, 768))} == {2}
        assert {_plan(n, largest, dim, k)["launches"] for n, largest, dim in ((5_000, 4_097, 64), (10**9, 10**6, 768))} == {2 + 5 + 2 * k}
    for bad in ((0, 1, 512, 8), (10, 0, 512, 8), (10, 11, 512, 8), (10, 5, 0, 8), (10, 5, 514, 8), (10, 5, 512, 0), (10, 5, 512, 257),
                (2 ** 31, 5, 512, 8)):
        with pytest.raises(ValueError):
            _plan(*bad)


def test_plan_honours_the_override_downwards_only(no_override):
    mp = no_override
    mp.setenv(ENV, "64")
    p = _plan(1_500, 700)
    assert p["lds_rows"] == 64 and p["wide"] == 1 and p["lds_bytes"] == 512 * 8 + 64 + 1_024 + 64 * 14
    assert _plan(1_500, 64)["wide"] == 0 and _plan(1_500, 65)["wide"] == 1
    mp.setenv(ENV, "100000")                                             # never above what the LDS form was built for
    assert _plan(10_000, 5_000)["lds_rows"] == 4_096
    mp.setenv(ENV, "0")                                                  # not a limit
    assert _plan(10_000, 5_000)["lds_rows"] == 4_096
    mp.delenv(ENV)
    assert _plan(1_500, 700) == dict(lds_rows=4_096, lds_bytes=512 * 8 + 64 + 1_024 + 704 * 14, wide=0, launches=2)


def test_c_abi_refuses_bad_arguments_before_the_device():
    from video_quierer_amd import _lib
    lib = _lib.load()
    g = np.zeros(4, np.int32); rows = np.empty(4 * 257, np.int32); rad = np.empty(4 * 257, np.float32)
    gp, rp, fp = (a.ctypes.data_as(POINTER(t)) for a, t in ((g, c_int32), (rows, c_int32), (rad, c_float)))
    for n_sel, k, rho in ((4, 0, 0.5), (4, 257, 0.5), (4, -1, 0.5), (0, 5, 0.5), (-3, 5, 0.5), (4, 5, math.nan)):
        rc = lib.vq_index_summarize_groups(None, gp, n_sel, k, c_float(rho), rp, fp, None)
        assert rc == -1, (n_sel, k, rho)
        msg = lib.vq_last_error().decode()
        assert ("NaN" in msg) == math.isnan(rho) and "vq_index_summarize_groups" in msg, msg
        assert lib.vq_index_summarize_groups_device(None, gp, n_sel, k, c_float(rho), None, None, None) == -1


# ---- the Python layer over a recording library ----
IDS = ["a_0", "a_10", "a_2", "b_0", "b_1", "c_0"]                      # string ids: the tie order is uploaded first


def summarize_entry(answers):
    """vq_index_summarize_groups answering label g with answers[g] = [(row, radius, members), ..]; recorded with its arguments."""
    def entry(calls, h, groups, n_sel, k, rho, rows, radius, members):
        labels = [groups[i] for i in range(n_sel)]
        calls.append(("summarize", labels, k, rho))
        for e, g in enumerate(labels):
            ans = (answers.get(g, []) + [(-1, np.inf, 0)] * k)[:k]
            fill(rows, [a[0] for a in ans], e * k)
            fill(radius, [a[1] for a in ans], e * k)
            fill(members, [a[2] for a in ans], e * k)
    return entry


def test_summarize_groups_uploads_in_order_and_shapes_the_result(monkeypatch):
    answers = {0: [(1, 0.25, 2), (2, 0.0, 1)], 1: [(4, 0.125, 2)], 2: [(5, 0.0, 1)]}
    calls = fake_lib(monkeypatch, vq_index_summarize_groups=summarize_entry(answers))
    idx = bare_index(IDS)
    res = idx.summarize_groups(k=2)
    assert [c[0] for c in calls] == ["set_id_ranks", "set_groups", "summarize"]      # _prepare's order: tie order, then labels
    assert calls[1] == ("set_groups", [0, 0, 0, 1, 1, 2], 3) and calls[2] == ("summarize", [0, 1, 2], 2, -math.inf)
    assert res == {"a": [{"id": "a_10", "rank": 0, "radius": np.float32(0.25), "members": 2},
                         {"id": "a_2", "rank": 1, "radius": np.float32(0.0), "members": 1}],
                   "b": [{"id": "b_1", "rank": 0, "radius": np.float32(0.125), "members": 2}],
                   "c": [{"id": "c_0", "rank": 0, "radius": np.float32(0.0), "members": 1}]}
    assert type(res["a"][0]["radius"]) is np.float32
    del calls[:]
    assert idx.summarize_groups(["c", "a", "c"], 300, max_radius=0.5) == {"c": res["c"], "a": res["a"]}
    assert calls == [("summarize", [2, 0], 256, 0.5)]              # nothing is uploaded twice; a key once; k capped at the limit
    assert idx.summarize_group("b", 1) == res["b"]
    del calls[:]
    with pytest.raises(KeyError):
        idx.summarize_groups(["a", "nope"])                        # before any device work
    with pytest.raises(KeyError):
        idx.summarize_group("nope", 0)
    with pytest.raises(ValueError):
        idx.summarize_group("a", 3, max_radius=math.nan)
    assert idx.summarize_group("a", 0) == [] and idx.summarize_groups(k=-1) == {"a": [], "b": [], "c": []}
    assert idx.summarize_groups([]) == {} and calls == []
    assert bare_index([]).summarize_groups() == {}


def test_similar_groups_by_keyframes_makes_these_calls(monkeypatch):
    def read_rows(calls, h, rn, n, out):
        calls.append(("read_rows", [rn[i] for i in range(n)]))
        fill(out, [1.0] * (n * 4))

    def search_set(calls, h, q, m, k, mode, labels, n_sel, excl, groups, dist, rows):
        calls.append(("search_set", m, k, [labels[i] for i in range(n_sel)], excl))
        fill(groups, ([1, 2] + [-1] * k)[:k])
        fill(dist, ([0.25, 0.5] + [np.inf] * k)[:k])

    calls = fake_lib(monkeypatch, vq_index_summarize_groups=summarize_entry({0: [(2, 0.5, 2), (0, 0.0, 1)]}), vq_index_read_rows=read_rows,
                     vq_index_search_set=search_set)
    idx = bare_index(IDS)
    res = idx.similar_groups("a", 2, keyframes=5)
    assert [c for c in calls if c[0] not in ("set_id_ranks", "set_groups")] == [
        ("summarize", [0], 5, -math.inf), ("read_rows", [2, 0]), ("search_set", 2, 2, [0], 1)]
    assert [c[0] for c in calls[:2]] == ["set_id_ranks", "set_groups"]
    assert [(r["group"], r["distance"]) for r in res] == [("b", np.float32(0.25)), ("c", np.float32(0.5))]
    with pytest.raises(ValueError):
        idx.similar_groups("a", 2, keyframes=0)
    with pytest.raises(KeyError):
        idx.similar_groups("nope", 2, keyframes=3)


def test_similar_groups_without_keyframes_keeps_its_limit(monkeypatch):
    calls = fake_lib(monkeypatch)
    idx = bare_index([f"a_{i}" for i in range(4_097)] + ["b_0"])
    with pytest.raises(ValueError, match="4097 rows"):
        idx.similar_groups("a", 3)
    assert calls == []


def test_video_summary_shapes_its_result(monkeypatch):
    from index_host_fakes import fake_device
    from video_quierer_amd.overhaul_index import SimpleVideoIndex
    calls = fake_device(monkeypatch, vq_index_summarize_groups=summarize_entry({1: [(4, 0.5, 2), (2, 0.25, 1), (3, 0.0, 1)]}))
    sv = SimpleVideoIndex()
    for i, (name, ts) in enumerate([("x.mp4", 0.0), ("x.mp4", 0.5), ("y.mp4", 0.0), ("y.mp4", 0.75), ("y.mp4", 1.5)]):
        sv.add_frame(np.full(4, i + 1.0, np.float32), name, ts)
    got = sv.video_summary("y.mp4", 3)
    assert got == [{"video_name": "y.mp4", "timestamp": 1.5, "frame_id": 4, "rank": 0, "radius": 0.5, "members": 2},
                   {"video_name": "y.mp4", "timestamp": 0.0, "frame_id": 2, "rank": 1, "radius": 0.25, "members": 1},
                   {"video_name": "y.mp4", "timestamp": 0.75, "frame_id": 3, "rank": 2, "radius": 0.0, "members": 1}]
    assert [md["frame_id"] for md in sv.video_summary("y.mp4", 3, chronological=True)] == [2, 3, 4]
    assert ("summarize", [1], 3, -math.inf) in calls
    with pytest.raises(KeyError):
        sv.video_summary("z.mp4")
    with pytest.raises(KeyError):
        SimpleVideoIndex().video_summary("y.mp4")


# ---- the restatement ----
def test_restatement_on_a_hand_worked_example():
    """Five rows of one group in dimension 4 (not unit: the definition does not need that), every sum exact:
         r0 = r1 = e0, r2 = e1, r3 = e2, r4 = (.5, .5, 0, 0);  c = (2.5, 1.5, 1, 0)
         1 - x.c = -1.5 -1.5 -.5 0 -1: rows 0 and 1 tie, the smaller tie is the seed.
       s_0 = r0: near = (-, 0, 1, 1, .5), radius 1 (rows 2 and 3 tie -> r2);  d(., r2) = (1, -, 1, .5): nothing is strictly nearer;
       radius 1 -> r3;  radius .5 -> r4 (d(r1, r4) = .5 > 0);  radius 0 -> r1;  radius 0, nothing left."""
    x = np.array([[1, 0, 0, 0], [1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0], [.5, .5, 0, 0]], dtype=np.float32)
    rows, tie = np.arange(5), np.arange(5)
    assert mean_direction(x, rows).tolist() == [2.5, 1.5, 1.0, 0.0]

    def ans(k, rho=-math.inf, t=tie):
        r, rad, mem = summarize(x, rows, t, k, rho)
        return r.tolist(), rad.tolist(), mem.tolist()

    assert ans(5) == ([0, 2, 3, 4, 1], [1.0, 1.0, 0.5, 0.0, 0.0], [1, 1, 1, 1, 1])
    assert ans(9) == ans(5)                                        # kappa = min(k, L)
    assert ans(1) == ([0], [1.0], [5])
    assert ans(2) == ([0, 2], [1.0, 1.0], [4, 1])                  # equal distance keeps the earlier owner
    assert ans(3) == ([0, 2, 3], [1.0, 1.0, 0.5], [3, 1, 1])
    assert ans(5, 0.5) == ans(3) and ans(5, 0.75) == ans(3)        # the shortest prefix whose last radius is <= max_radius
    assert ans(5, 1.0) == ans(1) and ans(5, math.inf) == ans(1)
    assert ans(5, 0.0) == ([0, 2, 3, 4], [1.0, 1.0, 0.5, 0.0], [2, 1, 1, 1])
    # the ties reversed: row 1 is the seed, row 3 goes before row 2
    assert ans(5, t=tie[::-1]) == ([1, 3, 2, 4, 0], [1.0, 1.0, 0.5, 0.0, 0.0], [1, 1, 1, 1, 1])
    # a group is a set of rows of a larger matrix, taken ascending whatever order they are named in
    big = np.concatenate([np.full((3, 4), 9, np.float32), x])
    r, rad, mem = summarize(big, np.array([7, 3, 5, 4, 6]), np.arange(8), 3)
    assert (r.tolist(), rad.tolist(), mem.tolist()) == ([3, 5, 6], [1.0, 1.0, 0.5], [3, 1, 1])
    assert [a.tolist() for a in summarize(x, [2], tie, 4)] == [[2], [0.0], [1]]


def test_mean_direction_adds_block_sums_not_rows():
    """259 rows: the last three are a block of their own.  Block sums: 2^53 + (1 + 1 - 2^53) = 2; row by row both ones would be
    lost in 2^53 and the sum would be 0."""
    x = np.zeros((259, 4), dtype=np.float32)
    x[:, 0] = 1.0
    x[0, 1], x[256, 1], x[257, 1], x[258, 1] = 2.0 ** 53, 1.0, 1.0, -2.0 ** 53
    assert mean_direction(x, np.arange(259)).tolist() == [259.0, 2.0, 0.0, 0.0]
    acc = np.float64(0.0)
    for v in x[:, 1]:
        acc = acc + np.float64(v)
    assert acc == 0.0


def test_restatement_finds_one_keyframe_per_planted_scene():
    rng = np.random.default_rng(31)
    dim, lengths = 64, [40, 3, 90, 17, 50]
    centres = rng.standard_normal((5, dim))
    centres /= np.linalg.norm(centres, axis=1, keepdims=True)
    scene = np.repeat(np.arange(5), lengths)
    x = centres[scene] + rng.standard_normal((200, dim)) * (0.1 / math.sqrt(dim))
    x = (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)
    tie = rng.permutation(200)
    rows, radius, mem = summarize(x, np.arange(200), tie, 5)
    assert sorted(scene[rows].tolist()) == [0, 1, 2, 3, 4]         # one keyframe per scene
    assert scene[rows[0]] == 2 and mem[0] == 90                    # the seed is in the scene that dominates the mean
    assert [int(m) for m in mem] == [lengths[s] for s in scene[rows]] and sorted(mem.tolist()) == [3, 17, 40, 50, 90]
    assert radius[3] > 0.5 > radius[4] and all(a >= b for a, b in zip(radius, radius[1:]))
    for k in (1, 2, 5, 16, 64):                                    # the consequences the header names
        r, rad, m = summarize(x, np.arange(200), tie, k)
        full = summarize(x, np.arange(200), tie, 200)
        assert len(r) == k and r.tolist() == full[0][:k].tolist() and rad.tobytes() == full[1][:k].tobytes() and m.sum() == 200
    r, rad, _ = summarize(x, np.arange(200), tie, 64, 0.5)
    assert len(r) == 5 and rad[-1] <= 0.5 < rad[-2]
