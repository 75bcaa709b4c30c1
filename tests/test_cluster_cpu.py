"""Host side of library clustering without a device: the exported symbols, the plan against a restatement of its rules, the
argument checks that come before the device is touched, the numpy restatement of the definition (tests/cluster_ref.py) on
hand-made cases, and the Python layer (HNSWIndex.cluster, SimpleVideoIndex.topics) over a recording library."""
from ctypes import POINTER, byref, c_float, c_int, c_int32, c_int64

import numpy as np
import pytest

import cluster_ref
from index_host_fakes import bare_index, fake_device, fake_lib, fill
from test_label_rows_cpu import label_entry

NAMES = ("vq_index_cluster", "vq_index_cluster_device", "vq_debug_cluster_plan", "vq_index_debug_cluster_update")


def _plan(n, dim, P):
    from video_quierer_amd import _lib
    piece, threads, launches = c_int(), c_int(), c_int()
    pieces, blocks, table, sums, scratch = c_int64(), c_int64(), c_int64(), c_int64(), c_int64()
    _lib.check(_lib.load().vq_debug_cluster_plan(n, dim, P, byref(piece), byref(pieces), byref(blocks), byref(table), byref(sums), byref(scratch),
                                                 byref(threads), byref(launches)))
    return dict(piece=piece.value, pieces=pieces.value, blocks=blocks.value, table=table.value, sums=sums.value, scratch=scratch.value,
                threads=threads.value, launches=launches.value)


def plan_restated(n, dim, P):
    """The rules of csrc/knn_cluster.h plan_cluster."""
    pieces, blocks = n // 1024 + min(P, n), -(-n // 1024)
    up4 = lambda v: -(-v // 4) * 4                                        # noqa: E731
    words = 16 + 4 * up4(n) + 5 * up4(P + 1)
    return dict(piece=1024, pieces=pieces, blocks=blocks, table=blocks * P * 4, sums=pieces * dim * 8,
                scratch=blocks * P * 4 + pieces * dim * 8 + 4 * words + 8 * P, threads=-(-(dim // 4) // 64) * 64, launches=6)


def test_new_symbols_are_exported():
    from video_quierer_amd import _lib
    lib = _lib.load()
    for name in NAMES:
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    header = open(_lib.os.path.join(_lib._HERE, "..", "include", "vq_amd.h")).read()
    for name in NAMES:
        assert f"int {name}(" in header
    import video_quierer_amd
    video_quierer_amd.install_dropin()
    from indexes.hnsw import HNSWIndex
    from video_quierer_amd.overhaul_index import SimpleVideoIndex
    assert callable(HNSWIndex.cluster) and callable(SimpleVideoIndex.topics)
    assert _lib.IDX_NCLASS == 7                                            # the new launches are accounted under existing classes


def test_plan_matches_the_restated_rules_and_bounds_the_pieces():
    rng = np.random.default_rng(3)
    for n in (1, 2, 1023, 1024, 1025, 2049, 4097, 16389, 1_000_000, 2 ** 31 - 1):
        for dim in (64, 256, 512, 768, 4096):
            for P in (1, 2, 33, 256, 257, 4096):
                if P > n:
                    continue
                got = _plan(n, dim, P)
                assert got == plan_restated(n, dim, P), (n, dim, P)
                assert got["threads"] * 4 >= dim and got["threads"] % 64 == 0 and got["threads"] <= 1024
        # whatever the clusters' sizes, their pieces fit the grid: sum_j ceil(cnt_j / 1,024) <= floor(n / 1,024) + min(P, n)
        if n <= 1_000_000:
            for P in (1, 3, 257, 4096):
                if P > n:
                    continue
                for _ in range(20):
                    cuts = np.sort(rng.integers(0, n + 1, P - 1))
                    cnt = np.diff(np.concatenate([[0], cuts, [n]]))
                    assert int((-(-cnt // 1024)).sum()) <= _plan(n, 512, P)["pieces"]
    assert _plan(1_000_000, 512, 4096)["sums"] <= 21 << 20                 # about 20 MB of piece sums at 1M x 512, P = 4,096
    for bad in ((0, 512, 1), (2 ** 31, 512, 1), (10, 0, 1), (10, 514, 1), (10, 4100, 1), (10, 512, 0), (10, 512, 11), (10 ** 6, 512, 4097)):
        with pytest.raises(ValueError):
            _plan(*bad)


def test_c_abi_refuses_bad_arguments_before_the_device():
    from video_quierer_amd import _lib
    lib = _lib.load()
    init = np.zeros((4, 8), np.float32)
    rows = np.zeros(4, np.int32)
    cen, dist = np.full((4, 8), -7, np.float32), np.full(64, -7, np.float32)
    out = [np.full(64, -7, np.int32) for _ in range(4)]
    it = c_int(-7)
    fp, ip = (lambda a: a.ctypes.data_as(POINTER(c_float))), (lambda a: a.ctypes.data_as(POINTER(c_int32)))
    for P, iters, a, b in ((0, 5, init, None), (4097, 5, init, None), (-1, 5, None, rows), (4, 0, init, None), (4, 1001, None, rows),
                           (4, 5, init, rows), (4, 5, None, None)):
        args = (fp(a) if a is not None else None, ip(b) if b is not None else None, P, iters, 1)
        assert lib.vq_index_cluster(None, *args, fp(cen), ip(out[0]), fp(dist), ip(out[1]), ip(out[2]), byref(it), ip(out[3])) == -1, (P, iters)
        assert "vq_index_cluster" in lib.vq_last_error().decode()
        assert lib.vq_index_cluster_device(None, *args, fp(cen), None, None, ip(out[1]), ip(out[2])) == -1
        assert "vq_index_cluster_device" in lib.vq_last_error().decode()
    assert lib.vq_index_debug_cluster_update(None, ip(rows), 0, fp(init), fp(cen), ip(out[0])) == -1
    assert (cen == -7).all() and (dist == -7).all() and all((o == -7).all() for o in out) and it.value == -7


# ---- the restatement on hand-made cases (distances in plain numpy: no oracle needed for these) ----
def plain_distances(stored, C):
    return (np.float32(1.0) - (np.asarray(C, np.float32) @ np.asarray(stored, np.float32).T).astype(np.float32)).astype(np.float32)


def test_two_clean_blobs():
    rng = np.random.default_rng(1)
    a = np.array([1.0, 0, 0, 0]) + 0.05 * rng.standard_normal((7, 4))
    b = np.array([0, 0, 1.0, 0]) + 0.05 * rng.standard_normal((5, 4))
    stored = np.concatenate([a, b])
    stored = (stored / np.linalg.norm(stored, axis=1, keepdims=True)).astype(np.float32)[[0, 7, 1, 8, 2, 9, 3, 10, 4, 11, 5, 6]]
    want = np.array([0, 1, 0, 1, 0, 1, 0, 1, 0, 1, 0, 0])
    res = cluster_ref.cluster(stored, stored[[0, 1]], 10, distances=plain_distances)
    assert res["labels"].tolist() == want.tolist() and res["counts"].tolist() == [7, 5]
    assert res["iterations"] == 2 and res["changed"] == [12, 0]            # the first assignment is already the partition
    for j in (0, 1):
        mean = stored[want == j].astype(np.float64).mean(axis=0)
        assert np.allclose(res["centroids"][j], mean / np.linalg.norm(mean), atol=1e-6) and res["centroids"].dtype == np.float32
        assert abs(np.linalg.norm(res["centroids"][j].astype(np.float64)) - 1.0) < 1e-6
        assert want[res["show"][j]] == j and res["distances"][res["show"][j]] == res["distances"][want == j].min()
    # started from two rows of the SAME blob, the other blob pulls one centroid over: labels move for more than one iteration
    res = cluster_ref.cluster(stored, stored[[0, 2]], 10, distances=plain_distances)
    assert res["iterations"] > 2 and res["changed"][-1] == 0 and sorted(res["counts"].tolist()) == [5, 7]


def test_one_cluster_of_opposite_rows_keeps_its_centroid():
    x = np.array([0.6, 0.0, 0.8, 0.0], dtype=np.float32)
    stored = np.stack([x, -x])
    c = np.array([[0.0, 1.0, 0.0, 0.0]], dtype=np.float32)
    res = cluster_ref.cluster(stored, c, 10, distances=plain_distances)
    assert res["iterations"] == 2 and res["changed"] == [2, 0] and res["counts"].tolist() == [2]
    assert res["centroids"].tobytes() == c.tobytes()                      # the zero mean keeps the centroid, bit for bit
    assert res["show"].tolist() == [0]                                    # both rows at distance 1: the smaller tie
    assert cluster_ref.update(stored, [0, 0], c).tobytes() == c.tobytes()
    # an empty cluster keeps its bits too, and is shown by no row
    res = cluster_ref.cluster(stored, np.stack([x, x]), 5, distances=plain_distances)
    assert res["counts"].tolist() == [2, 0] and res["show"].tolist() == [0, -1] and res["centroids"][1].tobytes() == x.tobytes()


def test_the_sum_order_is_part_of_the_definition():
    """2,049 rows in one cluster: three pieces.  On ``cancelling_rows`` the fp32 mean of the definition's order (a chain per
    piece, pieces in order) differs from one chain over all rows and from a pairwise (tree) sum, in every column: an
    implementation that sums in another order cannot pass the stage test of tests/test_cluster.py that uses these rows."""
    n, dim = 2049, 16
    stored = cluster_ref.cancelling_rows(np.random.default_rng(8), n, dim)
    assert np.abs(stored).max() > 0.5 and 0 < np.abs(stored)[np.abs(stored) > 0].min() < 1e-19

    def mean32(s):
        return (s / np.float64(n)).astype(np.float32)

    def tree(v):
        return v[0] if len(v) == 1 else tree(v[:len(v) // 2]) + tree(v[len(v) // 2:])
    chain = cluster_ref.column_sums(stored, np.arange(n))
    one = np.zeros(dim)
    for r in range(n):
        one = one + stored[r].astype(np.float64)
    assert (mean32(chain) != mean32(one)).all()                           # the pieces are part of the order
    assert (mean32(chain) != mean32(tree(list(stored.astype(np.float64))))).all()
    assert (mean32(chain) != mean32(stored.astype(np.float64).sum(axis=0))).any()      # numpy's own sum is pairwise too
    c = np.zeros((1, dim), dtype=np.float32)
    got = cluster_ref.update(stored, np.zeros(n, dtype=np.int64), c)
    assert abs(np.linalg.norm(got[0].astype(np.float64)) - 1.0) < 1e-6    # tiny as the mean is, its direction is a unit vector


# ---- the Python layer over a recording library ----
IDS = ["a_0", "a_10", "a_2", "b_0", "b_1", "c_0"]


def cluster_entry(labels, dists, counts, show, changed, dim=4):
    def entry(calls, h, init, init_rows, P, max_iter, mode, cen, row_label, row_dist, cnt, shw, iterations, chg):
        calls.append(("cluster", None if not init else [[init[j * dim + i] for i in range(dim)] for j in range(P)],
                      None if not init_rows else [init_rows[j] for j in range(P)], P, max_iter, mode))
        fill(cen, [float(i) for i in range(P * dim)])
        fill(row_label, labels)
        fill(row_dist, dists)
        fill(cnt, counts)
        fill(shw, show)
        fill(chg, changed)
        iterations._obj.value = len(changed)
    return entry


def test_cluster_seeds_from_sorted_distinct_rows_and_builds_the_result(monkeypatch):
    calls = fake_lib(monkeypatch, vq_index_cluster=cluster_entry([0, 1, 0, 1, 1, 0], [.1, .2, .3, .4, .5, .6], [3, 3, 0], [2, 1, -1], [6, 2, 0]))
    idx = bare_index(IDS)
    res = idx.cluster(3, seed=11)
    want_rows = sorted(np.random.default_rng(11).choice(6, 3, replace=False).tolist())
    assert [c[0] for c in calls] == ["set_id_ranks", "cluster"]           # string ids: the show rows' ties need the ranks
    assert calls[-1] == ("cluster", None, want_rows, 3, 25, 0) and len(set(want_rows)) == 3
    assert res["centroids"].shape == (3, 4) and res["centroids"].dtype == np.float32 and res["centroids"][1, 2] == 6.0
    assert res["labels"].tolist() == [0, 1, 0, 1, 1, 0] and res["labels"].dtype == np.int32 and res["distances"].dtype == np.float32
    assert res["iterations"] == 3 and res["converged"] is True and res["changed"] == [6, 2, 0]
    assert res["clusters"] == [{"cluster": 0, "size": 3, "id": "a_2", "distance": np.float32(.3), "score": np.float32(1) - np.float32(.3)},
                               {"cluster": 1, "size": 3, "id": "a_10", "distance": np.float32(.2), "score": np.float32(1) - np.float32(.2)},
                               {"cluster": 2, "size": 0, "id": None, "distance": None, "score": None}]
    assert idx.cluster(3)["centroids"].shape == (3, 4) and calls[-1][2] == sorted(np.random.default_rng(0).choice(6, 3, replace=False).tolist())
    # given vectors are normalised the way queries are; the iteration cap and the mode pass through
    calls = fake_lib(monkeypatch, vq_index_cluster=cluster_entry([0] * 6, [.1] * 6, [6, 0], [0, -1], [6, 1]))
    res = idx.cluster(2, init=[np.array([3.0, 0, 0, 4.0]), np.array([0, 2.0, 0, 0])], max_iter=2, mode=1)
    assert calls[-1] == ("cluster", [[np.float32(0.6), 0.0, 0.0, np.float32(0.8)], [0.0, 1.0, 0.0, 0.0]], None, 2, 2, 1)
    assert res["iterations"] == 2 and res["converged"] is False
    for bad in (dict(k=0), dict(k=4097), dict(k=7), dict(k=2, max_iter=0), dict(k=2, max_iter=1001), dict(k=2, init=[np.ones(4)]),
                dict(k=1, init=[np.ones(5)])):
        with pytest.raises(ValueError):
            idx.cluster(**bad)
    calls = fake_lib(monkeypatch)
    res = bare_index([]).cluster(5)
    assert res["clusters"] == [] and res["iterations"] == 0 and res["centroids"].shape == (0, 4) and len(res["labels"]) == 0 and calls == []


def test_topics_orders_by_size_and_counts_videos(monkeypatch):
    from video_quierer_amd.overhaul_index import SimpleVideoIndex
    #              frame: 0  1  2  3  4  5      videos: x x x y y z
    labels, dists = [1, 1, 0, 1, 2, 1], [.5, .25, .3, .75, .1, .2]
    tags = [[(1, 2, 1), (0, 1, 2)], [(1, 1, 3), (2, 1, 4)], [(1, 1, 5)]]
    calls = fake_device(monkeypatch, vq_index_cluster=cluster_entry(labels, dists, [1, 4, 1, 0], [2, 5, 4, -1], [6, 0]),
                        vq_index_label_rows=label_entry(labels, dists, tags))
    sv = SimpleVideoIndex()
    assert sv.topics(3) == []
    for i, (name, ts) in enumerate((("x", 0.0), ("x", 1.5), ("x", 3.0), ("y", 0.0), ("y", 2.0), ("z", 0.5))):
        sv.add_frame(np.eye(4, dtype=np.float32)[i % 4], name, ts)
    res = sv.topics(4, top_videos=2, seed=5, max_iter=7)
    clu = [c for c in calls if c[0] == "cluster"][-1]
    assert clu[2] == sorted(np.random.default_rng(5).choice(6, 4, replace=False).tolist()) and clu[3:] == (4, 7, 0)
    lab = [c for c in calls if c[0] == "label"][-1]
    assert np.array(lab[1]).shape == (4, 4) and lab[1][1] == [4.0, 5.0, 6.0, 7.0] and lab[4:] == (16, True)      # the returned centres, as they are
    assert res == [{"topic": 1, "video_name": "z", "timestamp": 0.5, "frame_id": 5, "score": float(np.float32(1) - np.float32(.2)), "size": 4,
                    "share": 4 / 6, "videos": [{"video_name": "x", "frames": 2}, {"video_name": "y", "frames": 1}]},
                   {"topic": 0, "video_name": "x", "timestamp": 3.0, "frame_id": 2, "score": float(np.float32(1) - np.float32(.3)), "size": 1,
                    "share": 1 / 6, "videos": [{"video_name": "x", "frames": 1}]},
                   {"topic": 2, "video_name": "y", "timestamp": 2.0, "frame_id": 4, "score": float(np.float32(1) - np.float32(.1)), "size": 1,
                    "share": 1 / 6, "videos": [{"video_name": "y", "frames": 1}]}]                                # the empty cluster 3 has no entry
    assert [len(t["videos"]) for t in sv.topics(4, top_videos=0)] == [0, 0, 0]
    with pytest.raises(ValueError):
        sv.topics(4, top_videos=-1)
