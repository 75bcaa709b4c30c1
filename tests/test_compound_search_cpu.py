"""Host side of the compound search without a device: the exported symbols, the plan against a restatement, the argument checks
that come before the device is touched, the numpy restatement of the definition on a hand-written table, and the Python layer
over a recording stand-in for the library."""
import math
from ctypes import POINTER, byref, c_float, c_int, c_int32, c_int64

import numpy as np
import pytest

from compound_ref import compound_answer, row_distance, struck
from index_host_fakes import bare_index, fake_device, fake_lib, fill

MIB = 1 << 20
INF = float("inf")


def _plan(n, dim, m, k, mode):
    from video_quierer_amd import _lib
    fp16, pool, streams, exact_bytes, eps = c_int(), c_int(), c_int64(), c_int64(), c_float()
    _lib.check(_lib.load().vq_debug_compound_plan(n, dim, m, k, mode, byref(fp16), byref(streams), byref(pool), byref(exact_bytes), byref(eps)))
    return dict(fp16=fp16.value, streams=streams.value, pool=pool.value, exact_bytes=exact_bytes.value, eps=eps.value)


def plan_restated(n, dim, m, k, mode):
    fp16 = mode == 2 or (mode == 0 and dim in (256, 512, 768) and k <= 100 and n >= 262_144)
    pool = (32 if k <= 20 else 64 if k <= 40 else 80 if k <= 64 else 128) if fp16 else 0
    return dict(fp16=int(fp16), streams=-(-n // 128), pool=pool, exact_bytes=m * (-(-n // 64) * 64) * 4)


def test_new_symbols_are_exported():
    from video_quierer_amd import _lib
    lib = _lib.load()
    for name in ("vq_index_search_compound", "vq_index_search_compound_device", "vq_debug_compound_plan"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    import video_quierer_amd
    video_quierer_amd.install_dropin()
    from indexes.hnsw import HNSWIndex, OptimizedHNSWIndex
    from video_quierer_amd.overhaul_index import SimpleVideoIndex
    assert callable(HNSWIndex.search_compound) and callable(OptimizedHNSWIndex.search_compound)
    assert callable(SimpleVideoIndex.search_compound)


def test_plan_matches_its_restatement():
    for dim in (64, 256, 512, 768):
        for n in (1, 127, 128, 129, 16_384, 262_143, 262_144, 1_000_000):
            for m in (1, 3, 16):
                for k in (1, 20, 21, 40, 41, 64, 65, 100, 101, 1024):
                    for mode in (0, 1) + ((2,) if dim != 64 and k <= 100 else ()):
                        got = _plan(n, dim, m, k, mode)
                        eps = got.pop("eps")
                        assert got == plan_restated(n, dim, m, k, mode), (n, dim, m, k, mode)
                        assert got["exact_bytes"] <= 16 * (n + 63) * 4          # 64 MiB per million rows at the most
                        assert (eps == 0.0) == (dim == 64)
    assert _plan(1_000_000, 512, 16, 20, 1)["exact_bytes"] <= 64 * MIB * 1_000_064 // 1_000_000


def test_plan_path_at_the_mode0_edges():
    # the measured crossover (csrc/knn_compound.h CP_FP16_MIN_ROWS), not the plain search's 16,384 rows
    assert _plan(262_143, 512, 3, 10, 0)["fp16"] == 0 and _plan(262_144, 512, 3, 10, 0)["fp16"] == 1
    assert _plan(16_384, 512, 3, 10, 0)["fp16"] == 0
    assert _plan(300_000, 512, 3, 100, 0)["fp16"] == 1 and _plan(300_000, 512, 3, 101, 0)["fp16"] == 0
    assert _plan(1_000_000, 64, 3, 10, 0)["fp16"] == 0
    assert _plan(100, 512, 3, 10, 2)["fp16"] == 1 and _plan(1_000_000, 512, 3, 10, 1)["fp16"] == 0
    for bad in ((0, 512, 1, 1, 0), (2 ** 31, 512, 1, 1, 0), (10, 510, 1, 1, 0), (10, 512, 0, 1, 0), (10, 512, 17, 1, 0), (10, 512, 1, 0, 0),
                (10, 512, 1, 1025, 0), (10, 512, 1, 1, 3), (10, 64, 1, 1, 2), (10, 512, 1, 101, 2)):
        with pytest.raises(ValueError):
            _plan(*bad)


def test_plan_exports_the_bound_of_the_proof():
    """eps = scan_eps_unit(dim) x 1.0001^2 + 2^-21: the scan's bound for norms up to 1.0001 plus half the proof's slack."""
    for dim in (256, 512, 768):
        unit = (2.0 / 2048 + 1.0 / 4194304 + dim / 8388608.0 + 1.0 / 65536 + 2.0 * math.sqrt(dim) / 33554432.0) * 1.02
        assert _plan(4096, dim, 3, 10, 2)["eps"] == pytest.approx(unit * 1.0001 ** 2 + 2.0 ** -21, rel=1e-5)
    assert 1.0e-3 < _plan(4096, 512, 3, 10, 2)["eps"] < _plan(4096, 768, 3, 10, 2)["eps"] < 1.5e-3


def test_arguments_are_refused_before_the_device_is_touched():
    from video_quierer_amd import _lib
    lib = _lib.load()
    q = np.zeros(16 * 4, np.float32); ids = np.zeros(4, np.int32); dist = np.zeros(4, np.float32)
    qp = q.ctypes.data_as(POINTER(c_float))
    out = (ids.ctypes.data_as(POINTER(c_int32)), dist.ctypes.data_as(POINTER(c_float)), None)
    nan = float("nan")

    def clause(*c):
        return (c_int32 * len(c))(*c)
    cases = [
        (0, clause(0), 0.0, 1, 1, b"m 0"), (17, clause(*range(17)), 0.0, 1, 1, b"m 17"), (-1, clause(0), 0.0, 1, 1, b"m -1"),
        (1, clause(0), 0.0, 0, 1, b"k 0"), (1, clause(0), 0.0, 1025, 1, b"k 1025"), (1, clause(0), 0.0, -3, 1, b"k -3"),
        (1, clause(0), nan, 1, 1, b"margin"),
        (1, clause(0), 0.0, 1, 3, b"mode 3"), (1, clause(0), 0.0, 1, -1, b"mode -1"),
        (3, clause(0, 2, 2), 0.0, 1, 1, b"gap"),                      # a gap in the numbering
        (3, clause(-1, 1, 1), 0.0, 1, 1, b"gap"),                     # ... clause 0 missing
        (3, clause(0, 1, 0), 0.0, 1, 1, b"decrease"),                 # a decreasing sequence
        (2, clause(-1, -1), 0.0, 1, 1, b"veto terms only"),           # only -1
        (2, clause(0, 2), 0.0, 1, 1, b"clause_of[1] = 2"),            # a value >= m
        (2, clause(0, 7), 0.0, 1, 1, b"clause_of[1] = 7"),
        (2, clause(0, -2), 0.0, 1, 1, b"clause_of[1] = -2"),
        (1, None, 0.0, 1, 1, b"clause_of is null"),
    ]
    for m, cl, margin, k, mode, word in cases:
        assert lib.vq_index_search_compound(None, qp, m, cl, c_float(margin), k, mode, *out) == -1, word
        assert word in lib.vq_last_error(), (word, lib.vq_last_error())
        assert lib.vq_index_search_compound_device(None, None, m, cl, c_float(margin), k, mode, None, None, None) == -1
        assert word in lib.vq_last_error(), (word, lib.vq_last_error())
    assert not ids.any() and not dist.any()                           # the outputs untouched
    # infinite margins and well-formed structures pass the argument check: what refuses them is the missing handle / library
    for m, cl, margin in ((1, clause(0), INF), (3, clause(0, -1, 0), -INF), (16, clause(*([0] * 8 + [1] * 8)), 0.0), (3, clause(-1, 0, 1), 0.5)):
        assert lib.vq_index_search_compound(None, qp, m, cl, c_float(margin), 1, 0, *out) != 0
        err = lib.vq_last_error()
        assert b"clause" not in err and b"margin" not in err and b" m " not in err, err


def test_the_restatement_on_a_hand_written_table():
    #              row:  0     1     2     3     4     5
    T = np.array([[0.10, 0.50, 0.30, 0.30, 0.90, 0.20],              # term 0
                  [0.80, 0.40, 0.30, 0.30, 0.10, 0.60],              # term 1
                  [0.70, 0.45, 0.90, 0.20, 0.95, 0.25]], np.float32)  # term 2
    tie = np.arange(6)
    f = np.float32
    # all-AND of the three: D = the column maximum
    assert np.array_equal(row_distance(T, [0, 1, 2]), np.array([0.8, 0.5, 0.9, 0.3, 0.95, 0.6], f))
    rows, dist, td = compound_answer(T, [0, 1, 2], 0.0, tie, 3)
    assert rows.tolist() == [3, 1, 5] and np.array_equal(dist, np.array([0.3, 0.5, 0.6], f)) and np.array_equal(td, T[:, [3, 1, 5]].T)
    # the sum of the similarities would have ranked row 0 (one term at 0.1) ... the AND does not: it comes fourth of six
    assert compound_answer(T, [0, 1, 2], 0.0, tie, 6)[0].tolist() == [3, 1, 5, 0, 2, 4]
    # pure OR: the column minimum; rows 0 and 4 tie at 0.1 and come in tie order, either way round
    assert np.array_equal(row_distance(T, [0, 0, 0]), np.array([0.1, 0.4, 0.3, 0.2, 0.1, 0.2], f))
    assert compound_answer(T, [0, 0, 0], 0.0, tie, 4)[0].tolist() == [0, 4, 3, 5]
    assert compound_answer(T, [0, 0, 0], 0.0, tie[::-1], 4)[0].tolist() == [4, 0, 5, 3]
    # mixed: (term 0 OR term 1) AND term 2
    assert np.array_equal(row_distance(T, [0, 0, 1]), np.array([0.7, 0.45, 0.9, 0.3, 0.95, 0.25], f))
    assert compound_answer(T, [0, 0, 1], 0.0, tie, 2)[0].tolist() == [5, 3]
    # a veto term: (term 0 AND term 1), NOT term 2.  D = [0.8, 0.5, 0.3, 0.3, 0.9, 0.6]; struck where T[2] < D + margin
    assert struck(T, [0, 1, -1], 0.0).tolist() == [True, True, False, True, False, True]
    rows, dist, td = compound_answer(T, [0, 1, -1], 0.0, tie, 4)
    assert rows.tolist() == [2, 4, -1, -1] and np.array_equal(dist, np.array([0.3, 0.9, INF, INF], f))
    assert np.array_equal(td[:2], T[:, [2, 4]].T) and np.all(np.isinf(td[2:]))
    assert not struck(T, [0, 1, -1], -INF).any() and struck(T, [0, 1, -1], INF).all()
    assert compound_answer(T, [0, 1, -1], -INF, tie, 6)[0].tolist() == compound_answer(T[:2], [0, 1], 0.0, tie, 6)[0].tolist()
    assert compound_answer(T, [0, 1, -1], INF, tie, 2)[0].tolist() == [-1, -1]
    # strict: row 3 has T[2] = 0.2 and D = 0.3; at margin float32(0.2) - float32(0.3) the limit IS 0.2 -> not struck
    edge = f(0.2) - f(0.3)
    assert f(0.3) + edge == f(0.2) and not struck(T, [0, 1, -1], edge)[3] and struck(T, [0, 1, -1], np.nextafter(edge, f(1)))[3]
    # the veto's position among the terms plays no part; a repeated term in a second clause changes nothing
    assert compound_answer(T[[2, 0, 1]], [-1, 0, 1], 0.0, tie, 4)[0].tolist() == [2, 4, -1, -1]
    assert compound_answer(T[[0, 1, 0]], [0, 1, 2], 0.0, tie, 6)[0].tolist() == compound_answer(T[:2], [0, 1], 0.0, tie, 6)[0].tolist()


def _recording_compound(rows, dists, tds):
    def entry(calls, h, terms, m, clause_of, margin, k, mode, ids, dist, td):
        dim = 4
        calls.append(("compound", np.array([terms[i] for i in range(m * dim)], np.float32).reshape(m, dim),
                      [clause_of[j] for j in range(m)], margin, k, mode))
        fill(ids, (list(rows) + [-1] * k)[:k])
        fill(dist, (list(dists) + [INF] * k)[:k])
        flat = [v for t in tds for v in t]
        fill(td, (flat + [INF] * (k * m))[:k * m])
    return entry


def test_python_layer_flattens_normalises_and_maps(monkeypatch):
    tds = [[0.1, 0.2, 0.3, 0.9], [0.2, 0.1, 0.4, 0.8]]
    calls = fake_lib(monkeypatch, vq_index_search_compound=_recording_compound([2, 0], [0.25, 0.5], tds))
    idx = bare_index(["a_0", "a_1", "b_0"], tie_order="device")
    a, b, c, v = (np.array(x, np.float32) for x in ([2, 0, 0, 0], [0, 3, 0, 0], [0, 0, 4, 0], [0, 0, 0, 5]))
    res = idx.search_compound([a, [b, c]], 5, none_of=[v], margin=0.5)
    (name, terms, clause_of, margin, k, mode), = calls
    assert name == "compound" and clause_of == [0, 1, 1, -1] and margin == 0.5 and k == 3 and mode == 0      # k capped by the size
    assert np.array_equal(terms, np.eye(4, dtype=np.float32))                                                   # normalised as search does
    assert [r["id"] for r in res] == ["b_0", "a_0"]
    assert all(set(r) == {"id", "distance", "score", "term_distances"} for r in res)
    assert [r["distance"] for r in res] == [np.float32(0.25), np.float32(0.5)]
    assert all(type(r["distance"]) is np.float32 and r["score"] == np.float32(1.0) - r["distance"] for r in res)
    assert np.array_equal(np.stack([r["term_distances"] for r in res]), np.array(tds, np.float32))
    # a 2-D array is a clause of alternatives; a bare vector is a clause of one; none_of defaults to nothing
    calls.clear()
    idx.search_compound([np.stack([a, b]), c], 2)
    assert calls[0][2] == [0, 0, 1] and calls[0][3] == 0.0 and calls[0][4] == 2
    calls.clear()
    idx.search_compound([a], 1, margin=-INF)
    assert calls[0][2] == [0] and calls[0][3] == -INF


def test_python_layer_refuses_and_answers_empty(monkeypatch):
    calls = fake_lib(monkeypatch)                                     # no compound entry point: any call to it is an AttributeError
    idx = bare_index(["a_0", "a_1"], tie_order="device")
    a = np.ones(4, np.float32)
    for bad in (dict(all_of=[]), dict(all_of=[[]]), dict(all_of=[a] * 17), dict(all_of=[a] * 9, none_of=[a] * 8),
                dict(all_of=[a], margin=float("nan")), dict(all_of=[np.ones(5, np.float32)]), dict(all_of=[a], none_of=[np.ones(3, np.float32)])):
        with pytest.raises(ValueError):
            idx.search_compound(bad.pop("all_of"), 2, **bad)
    assert idx.search_compound([a], 0) == [] and idx.search_compound([a], -1) == []
    assert bare_index().search_compound([a], 3) == []
    with pytest.raises(ValueError):
        bare_index().search_compound([], 3)                           # the arguments are judged before the empty index answers
    assert calls == []
    from video_quierer_amd.overhaul_index import SimpleVideoIndex
    sv = SimpleVideoIndex()
    assert sv.search_compound([a], 3) == []
    for bad in (dict(all_of=[]), dict(all_of=[a] * 17), dict(all_of=[a], margin=float("nan"))):
        with pytest.raises(ValueError):
            sv.search_compound(bad.pop("all_of"), 3, **bad)


def test_simple_video_index_returns_its_records(monkeypatch):
    tds = [[0.1, 0.3, 0.9], [0.2, 0.4, 0.8]]
    calls = fake_device(monkeypatch, vq_index_search_compound=_recording_compound([1, 2], [0.3, 0.4], tds))
    from video_quierer_amd.overhaul_index import SimpleVideoIndex
    sv = SimpleVideoIndex()
    for i in range(3):
        sv.add_frame(np.eye(4, dtype=np.float32)[i], f"clip{i // 2}", float(i))
    res = sv.search_compound([[3, 0, 0, 0], [0, 2, 0, 0]], 2, none_of=[[0, 0, 0, 9]])
    call = [c for c in calls if c[0] == "compound"][0]
    assert call[2] == [0, 1, -1] and call[3] == 0.0 and call[4] == 2
    assert np.allclose(call[1], np.eye(4, dtype=np.float32)[[0, 1, 3]], atol=1e-6)                # q / (|q| + 1e-10), as search
    assert [r["frame_id"] for r in res] == [1, 2] and [r["video_name"] for r in res] == ["clip0", "clip1"]
    assert all(set(r) == {"video_name", "timestamp", "frame_id", "score", "term_scores"} for r in res)
    assert res[0]["score"] == float(np.float32(1.0) - np.float32(0.3))
    assert res[0]["term_scores"] == [float(np.float32(1.0) - np.float32(d)) for d in tds[0]]
