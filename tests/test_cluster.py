"""Library clustering (vq_index_cluster / HNSWIndex.cluster / SimpleVideoIndex.topics): exact spherical k-means over the stored
rows.  The expected answer is the definition restated in numpy (tests/cluster_ref.py) over the C oracle's distances on the
exported rows; centroids (as bytes), labels, the float32 bits of the distances, counts, show rows, the number of iterations and
the changed counts must match bit for bit, in every mode, in the host and the device form.

The shapes are the smallest at which each mechanism can break: both sides of the 1,024-entry piece and of the 1,024-row block
of the counting sort; clusters of one, two, three and five pieces with a ragged last one; one to 257 clusters; the row count at
which mode 0 takes the fp16 assignment.  The update is also tested alone (vq_index_debug_cluster_update) on labels the test
writes, among them rows on which the order of the sum decides every bit of the result."""
import ctypes
import math
from ctypes import POINTER, byref, c_float, c_int, c_int32, c_void_p

import numpy as np
import pytest

import cluster_ref
from index_host_fakes import tie_ranks, unit
from test_distinct_search import video_rows
from test_label_rows import c_label, exported, raw_index, stats_of, unit_rows

pytestmark = pytest.mark.gpu
SENTINEL = -7


def _i32(a):
    return a.ctypes.data_as(POINTER(c_int32)) if a is not None else None


def _f32(a):
    return a.ctypes.data_as(POINTER(c_float)) if a is not None else None


def c_cluster(gpu_lib, lib, h, n, dim, P, max_iter, mode, init=None, init_rows=None):
    """vq_index_cluster -> dict(rc, centroids, labels, distances, counts, show, iterations, changed, stats); outputs start as SENTINEL"""
    init = None if init is None else np.ascontiguousarray(init, dtype=np.float32)
    init_rows = None if init_rows is None else np.ascontiguousarray(init_rows, dtype=np.int32)
    out = dict(centroids=np.full((P, dim), SENTINEL, np.float32), labels=np.full(n, SENTINEL, np.int32), distances=np.full(n, SENTINEL, np.float32),
               counts=np.full(P, SENTINEL, np.int32), show=np.full(P, SENTINEL, np.int32), changed=np.full(max(max_iter, 1), SENTINEL, np.int32))
    it = c_int(SENTINEL)
    out["rc"] = lib.vq_index_cluster(h, _f32(init), _i32(init_rows), P, max_iter, mode, _f32(out["centroids"]), _i32(out["labels"]),
                                     _f32(out["distances"]), _i32(out["counts"]), _i32(out["show"]), byref(it), _i32(out["changed"]))
    out["iterations"] = it.value
    out["stats"] = stats_of(gpu_lib, lib, h) if out["rc"] == 0 else None
    return out


class DeviceArrays:
    """hipMalloc'd arrays for the device form, freed on exit."""
    def __enter__(self):
        self.hip, self.ptrs = ctypes.CDLL("libamdhip64.so"), []
        return self

    def __exit__(self, *exc):
        for p in self.ptrs:
            assert self.hip.hipFree(p) == 0

    def alloc(self, nbytes):
        p = c_void_p()
        assert self.hip.hipMalloc(byref(p), ctypes.c_size_t(max(nbytes, 4))) == 0
        self.ptrs.append(p)
        return p

    def up(self, a):
        a = np.ascontiguousarray(a)
        p = self.alloc(a.nbytes)
        assert self.hip.hipMemcpy(p, a.ctypes.data_as(c_void_p), ctypes.c_size_t(a.nbytes), 1) == 0
        return p

    def down(self, p, like):
        host = np.empty_like(like)
        assert self.hip.hipMemcpy(host.ctypes.data_as(c_void_p), p, ctypes.c_size_t(host.nbytes), 2) == 0
        return host


def dev_cluster(gpu_lib, lib, h, n, dim, P, iters, mode, init=None, init_rows=None):
    """vq_index_cluster_device -> dict(centroids, labels, distances, counts, show, stats)"""
    with DeviceArrays() as d:
        di = d.up(np.ascontiguousarray(init, dtype=np.float32)) if init is not None else None
        dr = d.up(np.ascontiguousarray(init_rows, dtype=np.int32)) if init_rows is not None else None
        like = dict(centroids=np.empty((P, dim), np.float32), labels=np.empty(n, np.int32), distances=np.empty(n, np.float32),
                    counts=np.empty(P, np.int32), show=np.empty(P, np.int32))
        ptr = {name: d.alloc(a.nbytes) for name, a in like.items()}
        gpu_lib.check(lib.vq_index_cluster_device(h, di, dr, P, iters, mode, ptr["centroids"], ptr["labels"], ptr["distances"], ptr["counts"], ptr["show"]))
        gpu_lib.check(lib.vq_index_synchronize(h))
        out = {name: d.down(ptr[name], a) for name, a in like.items()}
        out["stats"] = stats_of(gpu_lib, lib, h)
        return out


ARRAYS = ("centroids", "labels", "distances", "counts", "show")


def assert_same(got, want, what):
    """got: c_cluster's dict; want: cluster_ref.cluster's"""
    print(f"{what}: iterations {got['iterations']} want {want['iterations']} changed {got['changed'][:8]} want {want['changed'][:8]} "
          f"counts {got['counts'][:6]} want {want['counts'][:6]} stats {got['stats']}")
    assert got["rc"] == 0, what
    T = want["iterations"]
    assert got["iterations"] == T and got["changed"][:T].tolist() == want["changed"], f"{what}: iterations / changed"
    assert (got["changed"][T:] == SENTINEL).all(), f"{what}: changed is written past the iterations run"
    assert np.array_equal(got["labels"], want["labels"]), f"{what}: labels differ at rows {np.flatnonzero(got['labels'] != want['labels'])[:8]}"
    assert got["distances"].tobytes() == want["distances"].tobytes(), f"{what}: distance bits differ"
    assert np.array_equal(got["counts"], want["counts"]) and np.array_equal(got["show"], want["show"]), f"{what}: counts / show rows"
    bad = np.flatnonzero((got["centroids"].view(np.uint32) != want["centroids"].view(np.uint32)).any(axis=1))
    assert len(bad) == 0, f"{what}: centroid bits differ in clusters {bad[:8]}"
    assert sum(got["stats"]) == len(want["labels"]) and min(got["stats"]) >= 0, f"{what}: stats {got['stats']}"


def assert_bytes(a, b, what, names=ARRAYS):
    for name in names:
        assert a[name].tobytes() == b[name].tobytes(), f"{what}: {name}"


def seed_rows(n, P, seed):
    return np.sort(np.random.default_rng([seed, 5]).choice(n, P, replace=False)).astype(np.int32)


def every_mode_and_form(gpu_lib, lib, h, n, dim, P, max_iter, want, what, modes=(1, 2, 0), **init):
    """The host form in every mode against the restatement; the device form with three iterations to spare against the host form."""
    for mode in modes:
        got = c_cluster(gpu_lib, lib, h, n, dim, P, max_iter, mode, **init)
        assert_same(got, want, f"{what} mode {mode}")
        dev = dev_cluster(gpu_lib, lib, h, n, dim, P, want["iterations"] + (3 if want["changed"][-1] == 0 and want["iterations"] > 1 else 0), mode, **init)
        assert_bytes(dev, got, f"{what} mode {mode} device form")
        assert dev["stats"] == got["stats"], f"{what} mode {mode} device form: stats {dev['stats']} host {got['stats']}"
    return got


# ---- shapes ----
#          n   P  dim max_iter
SHAPES = [(1, 1, 512, 3), (2, 2, 512, 3), (129, 3, 256, 6), (129, 2, 768, 6), (1023, 1, 512, 3), (1024, 1, 512, 3), (1025, 1, 768, 3),
          (2049, 1, 512, 3), (4097, 1, 256, 3), (1025, 2, 512, 6), (4097, 33, 512, 5), (2049, 257, 256, 3)]


@pytest.mark.parametrize("n,P,dim,max_iter", SHAPES)
def test_shapes_every_mode_and_form(gpu_lib, n, P, dim, max_iter):
    """Video-like rows, seeded from stored rows.  P = 1: ONE cluster of n rows, so 1,023 / 1,024 / 1,025 / 2,049 / 4,097 rows
    are one, one, two, three and five pieces, the last one ragged."""
    rows, _, _ = video_rows(n, dim, n + P)
    lib, h = raw_index(gpu_lib, rows)
    stored = exported(gpu_lib, lib, h, n, dim)
    init_rows = seed_rows(n, P, n)
    want = cluster_ref.cluster(stored, stored[init_rows], max_iter)
    assert P > 1 or (want["iterations"] == 2 and want["counts"].tolist() == [n])
    every_mode_and_form(gpu_lib, lib, h, n, dim, P, max_iter, want, f"n {n} P {P} dim {dim}", init_rows=init_rows)
    gpu_lib.check(lib.vq_index_destroy(h))


def test_planted_blobs_of_one_two_three_and_five_pieces(gpu_lib):
    """Four blobs of 1,023 / 1,025 / 2,049 / 4,097 rows, their rows interleaved (a cluster's list is not a run of rows), started
    from one row of each: every cluster is a whole blob from the first assignment on."""
    dim, sizes = 256, (1023, 1025, 2049, 4097)
    rng = np.random.default_rng(44)
    centres = unit_rows(rng, 4, dim)
    owner = rng.permutation(np.repeat(np.arange(4), sizes))
    n = len(owner)
    rows = unit(centres[owner] + 0.3 * rng.standard_normal((n, dim)) / math.sqrt(dim))
    lib, h = raw_index(gpu_lib, rows)
    init_rows = np.array([int(np.flatnonzero(owner == j)[3]) for j in range(4)], dtype=np.int32)
    want = cluster_ref.cluster(rows, rows[init_rows], 4)
    assert want["counts"].tolist() == list(sizes) and np.array_equal(want["labels"], owner) and want["iterations"] == 2
    every_mode_and_form(gpu_lib, lib, h, n, dim, 4, 4, want, "blobs", init_rows=init_rows)
    gpu_lib.check(lib.vq_index_destroy(h))


def test_mode0_takes_the_fp16_assignment_from_16384_rows(gpu_lib):
    """n = 16,384 + 5, P = 256: n x P >= 2^22, so mode 0 assigns on the fp16 path (stats[0] > 0); the answer is the exact one."""
    n, P, dim, max_iter = 16384 + 5, 256, 256, 3
    rows, _, _ = video_rows(n, dim, 163)
    lib, h = raw_index(gpu_lib, rows)
    init_rows = seed_rows(n, P, 163)
    want = cluster_ref.cluster(rows, rows[init_rows], max_iter)
    assert want["iterations"] == 3 and want["changed"][-1] > 0              # still moving when the cap ends it
    got = every_mode_and_form(gpu_lib, lib, h, n, dim, P, max_iter, want, "n 16389", init_rows=init_rows)
    assert got["stats"][0] + got["stats"][1] > 0 and sum(got["stats"]) == n, got["stats"]      # (mode 0 ran last) rows the fp16 pass settled
    assert c_cluster(gpu_lib, lib, h, n, dim, P, max_iter, 1, init_rows=init_rows)["stats"] == [0, 0, n]
    gpu_lib.check(lib.vq_index_destroy(h))


def test_dim64_is_exact_only(gpu_lib):
    n, P, dim = 1025, 5, 64
    rows, _, _ = video_rows(n, dim, 64)
    lib, h = raw_index(gpu_lib, rows)
    init_rows = seed_rows(n, P, 64)
    want = cluster_ref.cluster(rows, rows[init_rows], 6)
    every_mode_and_form(gpu_lib, lib, h, n, dim, P, 6, want, "dim 64", modes=(1, 0), init_rows=init_rows)
    got = c_cluster(gpu_lib, lib, h, n, dim, P, 6, 2, init_rows=init_rows)
    assert got["rc"] == -1 and all((got[name] == SENTINEL).all() for name in ARRAYS + ("changed",)) and got["iterations"] == SENTINEL
    gpu_lib.check(lib.vq_index_destroy(h))


# ---- planted cases ----
def test_video_rows_move_for_several_iterations_and_the_properties_hold(gpu_lib):
    """Labels really move (iterations > 2).  Then: label_rows(centroids) reproduces labels and distances; a repeat is
    bit-identical; `init` vectors equal to the seeded rows give the same bytes as `init_rows`; the three modes agree."""
    n, P, dim = 1500, 5, 512
    rows, _, _ = video_rows(n, dim, 7)
    lib, h = raw_index(gpu_lib, rows)
    init_rows = seed_rows(n, P, 7)
    want = cluster_ref.cluster(rows, rows[init_rows], 25)
    assert want["iterations"] > 2 and want["changed"][-1] == 0 and want["changed"][1] > 0
    got = every_mode_and_form(gpu_lib, lib, h, n, dim, P, 25, want, "video rows", init_rows=init_rows)
    for mode in (1, 2):
        lab = c_label(gpu_lib, lib, h, n, got["centroids"], mode)
        assert np.array_equal(lab["lab"], got["labels"]) and lab["dist"].tobytes() == got["distances"].tobytes(), f"label_rows mode {mode}"
        again = c_cluster(gpu_lib, lib, h, n, dim, P, 25, mode, init_rows=init_rows)
        assert_bytes(again, got, f"repeat mode {mode}", ARRAYS + ("changed",))
        assert again["iterations"] == got["iterations"]
        vec = c_cluster(gpu_lib, lib, h, n, dim, P, 25, mode, init=rows[init_rows])
        assert_bytes(vec, got, f"init vectors mode {mode}", ARRAYS + ("changed",))
    capped = c_cluster(gpu_lib, lib, h, n, dim, P, 2, 1, init_rows=init_rows)      # the cap: the labels belong to the centroids returned
    assert_same(capped, cluster_ref.cluster(rows, rows[init_rows], 2), "max_iter 2")
    gpu_lib.check(lib.vq_index_destroy(h))


def test_duplicate_identical_equal_and_equidistant(gpu_lib):
    dim = 512
    rng = np.random.default_rng(21)
    # duplicate initial centroids: in the first assignment the later one wins no row (equal distances go to the smaller j), shows
    # no row, and the update leaves its bits alone; from the second assignment on it competes where it was left
    n = 300
    rows, _, _ = video_rows(n, dim, 21)
    lib, h = raw_index(gpu_lib, rows)
    init_rows = np.array([10, 200, 10], dtype=np.int32)
    want = cluster_ref.cluster(rows, rows[init_rows], 1)
    assert want["counts"][2] == 0 and want["show"][2] == -1 and want["counts"][0] > 1
    every_mode_and_form(gpu_lib, lib, h, n, dim, 3, 1, want, "duplicate centroids, one assignment", init_rows=init_rows)
    want = cluster_ref.cluster(rows, rows[init_rows], 2)
    assert want["centroids"][2].tobytes() == rows[10].tobytes() and want["centroids"][0].tobytes() != rows[10].tobytes()
    assert want["labels"][10] == 2                           # the row it was copied from now lies at distance 0 of it
    every_mode_and_form(gpu_lib, lib, h, n, dim, 3, 2, want, "duplicate centroids, two assignments", init_rows=init_rows)
    every_mode_and_form(gpu_lib, lib, h, n, dim, 3, 8, cluster_ref.cluster(rows, rows[init_rows], 8), "duplicate centroids", init_rows=init_rows)
    gpu_lib.check(lib.vq_index_destroy(h))
    # identical rows: one cluster takes them all (the smaller j), the others keep their start
    same = np.repeat(unit_rows(rng, 1, dim), 260, axis=0)
    lib, h = raw_index(gpu_lib, same)
    init = unit_rows(rng, 3, dim)
    want = cluster_ref.cluster(same, init, 5)
    assert sorted(want["counts"].tolist()) == [0, 0, 260] and want["show"].max() == 0
    every_mode_and_form(gpu_lib, lib, h, 260, dim, 3, 5, want, "identical rows", init=init)
    gpu_lib.check(lib.vq_index_destroy(h))
    # a row equidistant from two centroids goes to the smaller j; rows equal to a centroid sit at distance ~0
    rows = unit_rows(rng, 200, dim)
    e = np.zeros((2, dim), dtype=np.float32)
    e[0, 3], e[1, 400] = 1.0, 1.0
    rows[0], rows[1], rows[2] = e[0], e[1], (e[0] + e[1]) * np.float32(math.sqrt(0.5))
    lib, h = raw_index(gpu_lib, rows)
    want = cluster_ref.cluster(rows, e, 1)
    assert want["labels"][:3].tolist() == [0, 1, 0] and want["distances"][0] == 0.0 and want["show"].tolist() == [0, 1]
    every_mode_and_form(gpu_lib, lib, h, 200, dim, 2, 1, want, "equidistant", init=e)
    want = cluster_ref.cluster(rows, e[::-1], 1)
    assert want["labels"][:3].tolist() == [1, 0, 0]
    every_mode_and_form(gpu_lib, lib, h, 200, dim, 2, 1, want, "equidistant, swapped", init=e[::-1])
    gpu_lib.check(lib.vq_index_destroy(h))


def test_python_layer_string_ids_ranks_and_lifetimes(gpu_lib):
    """HNSWIndex.cluster over string ids whose order differs from the rows' (ranks are set), with planted duplicate frames: the
    show row of a tie follows the ids.  Then remove_batch and an update of a stored id, each against the restatement again."""
    from video_quierer_amd.indexes.hnsw import OptimizedHNSWIndex
    dim, n, k = 512, 700, 6
    rows, video, frame = video_rows(n, dim, 12, lengths=[1, 7, 63, 64, 65, 300])
    ids = [f"v{v}_{f}" for v, f in zip(video, frame)]
    idx = OptimizedHNSWIndex(dimension=dim)
    idx.add_batch(rows, ids)

    def check(tag, init=None, seed=3):
        stored, cur = idx._export(), list(idx._ids)
        m = len(cur)
        tie = tie_ranks(cur)
        if init is None:
            C1 = stored[np.sort(np.random.default_rng(seed).choice(m, k, replace=False))]
        else:
            C1 = np.ascontiguousarray(idx._unit_rows(init), dtype=np.float32)
        want = cluster_ref.cluster(stored, C1, 25, tie=tie)
        for mode in (1, 2):
            res = idx.cluster(k, init=init, seed=seed, mode=mode)
            assert res["centroids"].tobytes() == want["centroids"].tobytes() and np.array_equal(res["labels"], want["labels"]), f"{tag} mode {mode}"
            assert res["distances"].tobytes() == want["distances"].tobytes() and res["changed"] == want["changed"]
            assert res["iterations"] == want["iterations"] and res["converged"] == (want["changed"][-1] == 0 and want["iterations"] > 1)
            assert res["clusters"] == [{"cluster": j, "size": int(c), "id": cur[r], "distance": want["distances"][r],
                                        "score": np.float32(1.0) - want["distances"][r]} if r >= 0 else
                                       {"cluster": j, "size": 0, "id": None, "distance": None, "score": None}
                                       for j, (c, r) in enumerate(zip(want["counts"], want["show"]))], f"{tag} mode {mode}"
        return want
    check("fresh")
    # the rows closest to a centre, duplicated: "v5_10" sorts before "v5_2" though it is the later row; the tie goes by id
    centre = rows[ids.index("v5_2")]
    init = [centre] + [rows[i] for i in (0, 3, 30, 100, 200)]
    idx.add(centre, "v5_10")                                # both rows now equal the first initial centroid
    want = check("duplicates", init=init)
    cur = list(idx._ids)
    one = cluster_ref.cluster(idx._export(), np.ascontiguousarray(idx._unit_rows(init), dtype=np.float32), 1, tie=tie_ranks(cur))
    assert cur[one["show"][0]] == "v5_10" and cur.index("v5_10") > cur.index("v5_2")
    assert idx.cluster(k, init=init, max_iter=1)["clusters"][0]["id"] == "v5_10"
    idx.remove_batch([i for i in ids if i.startswith("v3_")][::2] + ["v0_0"])
    check("after remove_batch")
    idx.add(np.asarray(rows[400] + 0.01 * rows[0]), "v2_5")  # an id the index holds: its row is replaced
    check("after an update", seed=4)
    idx.close()


def test_topics(gpu_lib):
    from video_quierer_amd.overhaul_index import SimpleVideoIndex
    dim, n, k = 512, 300, 5
    rows, video, frame = video_rows(n, dim, 21, lengths=[40, 100, 160])
    sv = SimpleVideoIndex()
    for r in range(n):
        sv.add_frame(rows[r], f"clip{video[r]}", 0.5 * frame[r])
    res = sv.topics(k, top_videos=2, seed=9)
    C1 = rows[np.sort(np.random.default_rng(9).choice(n, k, replace=False))]
    want = cluster_ref.cluster(rows, C1, 25, tie=-np.arange(n))             # ties: the larger frame id first, as `search`
    order = sorted((j for j in range(k) if want["counts"][j] > 0), key=lambda j: (-want["counts"][j], j))
    assert [t["topic"] for t in res] == order and sum(t["size"] for t in res) == n
    groups = np.asarray(video)
    for t in res:
        j, r = t["topic"], int(want["show"][t["topic"]])
        per_video = np.bincount(groups[want["labels"] == j], minlength=3)
        best = sorted((v for v in range(3) if per_video[v] > 0), key=lambda v: (-per_video[v], v))[:2]
        assert t == {"topic": j, "video_name": f"clip{video[r]}", "timestamp": 0.5 * frame[r], "frame_id": r,
                     "score": float(np.float32(1.0) - want["distances"][r]), "size": int(want["counts"][j]), "share": int(want["counts"][j]) / n,
                     "videos": [{"video_name": f"clip{v}", "frames": int(per_video[v])} for v in best]}


# ---- the update alone, on labels the test writes ----
def c_update(gpu_lib, lib, h, labels, C):
    P, dim = C.shape
    out, counts = np.full((P, dim), SENTINEL, np.float32), np.full(P, SENTINEL, np.int32)
    rc = lib.vq_index_debug_cluster_update(h, _i32(np.ascontiguousarray(labels, dtype=np.int32)), P, _f32(np.ascontiguousarray(C, dtype=np.float32)),
                                           _f32(out), _i32(counts))
    return rc, out, counts


def report_difference(got, want, stored, labels, C, what):
    """Which operation of the update differs, and by how much (printed before the assertion fails)."""
    bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    if len(bad):
        j, i = bad[0]
        rows = np.flatnonzero(labels == j)
        s = cluster_ref.column_sums(stored, rows)
        m = (s / np.float64(len(rows))).astype(np.float32)
        n2 = np.float64(0.0)
        for v in m.astype(np.float64):
            n2 = n2 + v * v
        ulp = np.abs(got[j].astype(np.float64) - want[j].astype(np.float64)) / np.spacing(np.abs(want[j]))
        print(f"{what}: {len(bad)} centroid words differ, first (cluster {j}, column {i}): got {got[j, i]!r} want {want[j, i]!r}; cluster {j}: "
              f"{len(rows)} rows, sum {s[i]!r}, mean {m[i]!r}, n2 {n2!r}, sqrt {np.sqrt(n2)!r}; largest difference {ulp.max():.2f} fp32 ulp; "
              f"all columns scaled alike (a different sqrt or n2): {bool(np.allclose(got[j] / want[j], (got[j] / want[j])[i], rtol=1e-6))}")


STAGE_CASES = ["one label", "alternating", "1024 and 1025", "empty ends", "cancelling", "cancelling 768", "unit rows"]


@pytest.mark.parametrize("case", STAGE_CASES)
def test_stage_update_on_written_labels(gpu_lib, case):
    """The update through vq_index_debug_cluster_update against cluster_ref.update, bit for bit.  Nothing else pins the device's
    fp64 division and square root to correct rounding; `cancelling` pins the order of the sums (a tree-order sum gives other
    bits in every column: tests/test_cluster_cpu.py)."""
    rng = np.random.default_rng([90, STAGE_CASES.index(case)])
    dim = 768 if case == "cancelling 768" else 512 if case != "alternating" else 256
    if case == "one label":
        n, P = 2500, 3
        labels = np.full(n, 1)
    elif case == "alternating":
        n, P = 2051, 2
        labels = np.arange(n) % 2
    elif case == "1024 and 1025":
        n, P = 1024 + 1025 + 7, 3
        labels = rng.permutation(np.repeat([0, 1, 2], [1024, 1025, 7]))
    elif case == "empty ends":
        n, P = 1500, 6
        labels = 1 + rng.integers(0, 4, n)                   # labels 0 and 5 hold no row
    elif case.startswith("cancelling"):
        n, P = 2049 + 300, 2
        labels = rng.permutation(np.repeat([0, 1], [2049, 300]))
    else:
        n, P = 4097, 33
        labels = rng.integers(0, P, n)
    if case.startswith("cancelling"):
        rows = np.empty((n, dim), dtype=np.float32)
        for j in (0, 1):
            rows[labels == j] = cluster_ref.cancelling_rows(rng, int((labels == j).sum()), dim)
    else:
        rows = unit_rows(rng, n, dim) if case == "unit rows" else video_rows(n, dim, 90)[0]
    C = unit_rows(rng, P, dim)
    lib, h = raw_index(gpu_lib, rows)
    stored = exported(gpu_lib, lib, h, n, dim)
    assert stored.tobytes() == rows.tobytes()
    want = cluster_ref.update(stored, labels, C)
    rc, got, counts = c_update(gpu_lib, lib, h, labels, C)
    assert rc == 0 and counts.tolist() == np.bincount(labels, minlength=P).tolist()
    report_difference(got, want, stored, labels, C, case)
    assert got.tobytes() == want.tobytes(), f"{case}: the update's bits differ"
    for j in np.flatnonzero(np.bincount(labels, minlength=P) == 0):
        assert got[j].tobytes() == C[j].tobytes()            # an empty cluster keeps its centroid
    rc2, again, _ = c_update(gpu_lib, lib, h, labels, C)
    assert rc2 == 0 and again.tobytes() == got.tobytes()
    bad = labels.copy()
    bad[n // 2] = P
    rc, out, counts = c_update(gpu_lib, lib, h, bad, C)
    assert rc == -1 and (out == SENTINEL).all() and (counts == SENTINEL).all()
    gpu_lib.check(lib.vq_index_destroy(h))


# ---- refusals ----
def test_refusals_leave_the_outputs_untouched(gpu_lib):
    rng = np.random.default_rng(50)
    n, dim, P = 200, 512, 4
    rows = unit_rows(rng, n, dim)
    init, init_rows = unit_rows(rng, P, dim), np.array([0, 5, 9, 199], dtype=np.int32)
    lib, h = raw_index(gpu_lib, rows)

    def refused(got):
        assert got["rc"] == -1, got["rc"]
        assert all((got[name] == SENTINEL).all() for name in ARRAYS + ("changed",)) and got["iterations"] == SENTINEL
    refused(c_cluster(gpu_lib, lib, h, n, dim, P, 5, 1))                                             # neither init nor init_rows
    refused(c_cluster(gpu_lib, lib, h, n, dim, P, 5, 1, init=init, init_rows=init_rows))             # both
    refused(c_cluster(gpu_lib, lib, h, n, dim, P, 0, 1, init=init))                                  # max_iter out of range
    refused(c_cluster(gpu_lib, lib, h, n, dim, P, 1001, 1, init=init))
    refused(c_cluster(gpu_lib, lib, h, n, dim, n + 1, 5, 1, init=unit_rows(rng, n + 1, dim)))        # more clusters than rows
    refused(c_cluster(gpu_lib, lib, h, n, dim, 4097, 5, 1, init=np.zeros((4097, dim), np.float32)))
    for bad_row in (-1, n):
        r = init_rows.copy()
        r[2] = bad_row
        refused(c_cluster(gpu_lib, lib, h, n, dim, P, 5, 1, init_rows=r))                            # an init row outside [0, n)
    for bad_value in (np.inf, np.nan):
        v = init.copy()
        v[3, 100] = bad_value
        refused(c_cluster(gpu_lib, lib, h, n, dim, P, 5, 2, init=v))                                 # an init value that is not finite
    refused(c_cluster(gpu_lib, lib, h, n, dim, P, 5, 3, init=init))                                  # unknown mode
    refused(c_cluster(gpu_lib, lib, h, n, dim, P, 5, -1, init_rows=init_rows))
    assert c_cluster(gpu_lib, lib, h, n, dim, P, 5, 0, init_rows=init_rows)["rc"] == 0
    gpu_lib.check(lib.vq_index_set_id_ranks(h, _i32(rng.permutation(n).astype(np.int32)), n))
    assert c_cluster(gpu_lib, lib, h, n, dim, P, 5, 0, init_rows=init_rows)["rc"] == 0
    more = unit_rows(rng, 10, dim)
    gpu_lib.check(lib.vq_index_add(h, gpu_lib.fptr(more), 10, 0))
    refused(c_cluster(gpu_lib, lib, h, n + 10, dim, P, 5, 1, init_rows=init_rows))                   # the id ranks are stale now
    with DeviceArrays() as d:
        ptr = [d.alloc(4 * P * dim), d.alloc(4 * P), d.alloc(4 * P), d.up(init_rows)]
        assert lib.vq_index_cluster_device(h, None, ptr[3], P, 5, 1, ptr[0], None, None, ptr[1], ptr[2]) == -1
        assert "stale" in lib.vq_last_error().decode() or "ranks" in lib.vq_last_error().decode()
    gpu_lib.check(lib.vq_index_destroy(h))
    # an empty index: 0, nothing written
    lib, h = raw_index(gpu_lib, np.empty((0, dim), dtype=np.float32))
    got = c_cluster(gpu_lib, lib, h, 4, dim, P, 5, 0, init=init)
    assert got["rc"] == 0 and all((got[name] == SENTINEL).all() for name in ARRAYS + ("changed",)) and got["iterations"] == SENTINEL
    assert got["stats"] == [0, 0, 0]
    gpu_lib.check(lib.vq_index_destroy(h))
