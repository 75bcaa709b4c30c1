"""Zero-shot labelling (vq_index_label_rows / HNSWIndex.label_rows / label_groups / SimpleVideoIndex.tag_videos): which prompt
each row shows, what each group is about.  The expected answer is the definition restated in numpy (tests/label_ref.py) over
the C oracle's distances on the exported rows; labels, the float32 bits of the distances, tags, votes, show rows and
unlabelled counts must match bit for bit, in every mode, in the host and the device form.

The shapes are the smallest at which each mechanism can break: both sides of a 128-row stream, of a 256-row tile and of the
2,048-row range; one, two and three prompt tiles with a ragged last one; two prompt ranges (4,096 prompts); the row count at
which mode 0 changes path."""
import ctypes
import math
from ctypes import POINTER, byref, c_float, c_int, c_int32, c_int64, c_void_p

import numpy as np
import pytest

import label_ref
from index_host_fakes import tie_ranks, unit
from test_distinct_search import video_rows

pytestmark = pytest.mark.gpu
INF = math.inf
SENTINEL = -7


def _i32(a):
    return a.ctypes.data_as(POINTER(c_int32)) if a is not None else None


def _f32(a):
    return a.ctypes.data_as(POINTER(c_float)) if a is not None else None


def unit_rows(rng, n, dim):
    return unit(rng.standard_normal((n, dim)))


def raw_index(gpu_lib, rows, labels=None, ranks=None):
    """rows as given (unit: the library measures them) -> (lib, handle)"""
    lib = gpu_lib.load()
    h = c_void_p()
    gpu_lib.check(lib.vq_index_create(rows.shape[1], byref(h)))
    if len(rows):
        gpu_lib.check(lib.vq_index_add(h, gpu_lib.fptr(np.ascontiguousarray(rows, dtype=np.float32)), len(rows), 0))
    if labels is not None:
        lab = np.ascontiguousarray(labels, dtype=np.int32)
        gpu_lib.check(lib.vq_index_set_groups(h, _i32(lab), len(rows), int(lab.max()) + 1))
    if ranks is not None:
        gpu_lib.check(lib.vq_index_set_id_ranks(h, _i32(np.ascontiguousarray(ranks, dtype=np.int32)), len(rows)))
    return lib, h


def stats_of(gpu_lib, lib, h):
    st = (c_int64 * 3)()
    gpu_lib.check(lib.vq_index_last_search_stats(h, st))
    return list(st)


def c_label(gpu_lib, lib, h, n, prompts, mode, max_dist=INF, m=0, G=0):
    """vq_index_label_rows -> dict(rc, lab, dist, tags, votes, show, unl, stats); outputs start as SENTINEL"""
    prompts = np.ascontiguousarray(prompts, dtype=np.float32)
    out = dict(lab=np.full(n, SENTINEL, np.int32), dist=np.full(n, SENTINEL, np.float32), tags=None, votes=None, show=None, unl=None)
    if m:
        out.update(tags=np.full((G, m), SENTINEL, np.int32), votes=np.full((G, m), SENTINEL, np.int32),
                   show=np.full((G, m), SENTINEL, np.int32), unl=np.full(G, SENTINEL, np.int32))
    out["rc"] = lib.vq_index_label_rows(h, gpu_lib.fptr(prompts), len(prompts), mode, c_float(max_dist), _i32(out["lab"]), _f32(out["dist"]),
                                        m, _i32(out["tags"]), _i32(out["votes"]), _i32(out["show"]), _i32(out["unl"]))
    out["stats"] = stats_of(gpu_lib, lib, h) if out["rc"] == 0 else None
    return out


def plan(gpu_lib, n, dim, P, mode=2, largest_group=0):
    """vq_debug_label_plan -> dict(fp16, eps, pieces: of the longest group, 0 = one workgroup)"""
    a, b, c, t, r, sp, pc = c_int(), c_int(), c_int(), c_int(), c_int(), c_int(), c_int()
    eb, rt, pb, eps, pieces = c_int64(), c_int64(), c_int64(), c_float(), c_int64()
    gpu_lib.check(gpu_lib.load().vq_debug_label_plan(n, dim, P, mode, largest_group, byref(a), byref(b), byref(c), byref(eb), byref(t), byref(r),
                                                     byref(rt), byref(pb), byref(eps), byref(sp), byref(pc), byref(pieces)))
    return dict(fp16=a.value, eps=float(eps.value), pieces=pieces.value)


def plan_eps(gpu_lib, n, dim, P):
    return plan(gpu_lib, n, dim, P)["eps"]


def assert_rows(got, L, best, what):
    print(f"{what}: stats {got['stats']} labels {got['lab'][:6]} want {L[:6]} dist {got['dist'][:3]} want {best[:3]}")
    assert got["rc"] == 0, what
    assert np.array_equal(got["lab"], L), f"{what}: labels differ at rows {np.flatnonzero(got['lab'] != L)[:8]}"
    assert got["dist"].tobytes() == best.tobytes(), f"{what}: distance bits differ"
    assert sum(got["stats"]) == len(L) and min(got["stats"]) >= 0, f"{what}: stats {got['stats']}"


def assert_groups(got, want, what):
    for name, w in zip(("tags", "votes", "show", "unl"), want):
        assert np.array_equal(got[name], w), f"{what}: {name} differ\n{got[name][:4]}\nwant\n{w[:4]}"


def exported(gpu_lib, lib, h, n, dim):
    out = np.empty((n, dim), dtype=np.float32)
    gpu_lib.check(lib.vq_index_export(h, gpu_lib.fptr(out)))
    return out


# ---- shapes: every path against the restatement ----
SHAPES = [(1, 1, 512), (1, 257, 512), (300, 257, 256), (2049, 33, 256), (127, 2, 512), (128, 255, 512), (129, 256, 512), (129, 257, 768), (129, 600, 512),
          (2047, 33, 512), (2048, 5, 768), (2049, 257, 512), (300, 4096, 512)]


@pytest.mark.parametrize("n,P,dim", SHAPES)
def test_shapes_every_mode(gpu_lib, n, P, dim):
    rng = np.random.default_rng([n, P, dim])
    rows, prompts = unit_rows(rng, n, dim), unit_rows(rng, P, dim)
    lib, h = raw_index(gpu_lib, rows)
    L, best = label_ref.row_labels(label_ref.distances(exported(gpu_lib, lib, h, n, dim), prompts))
    for mode in (1, 2, 0):
        got = c_label(gpu_lib, lib, h, n, prompts, mode)
        assert_rows(got, L, best, f"n {n} P {P} dim {dim} mode {mode}")
        if mode != 2:                                       # below 16,384 rows mode 0 is the exact path
            assert got["stats"] == [0, 0, n]
    gpu_lib.check(lib.vq_index_destroy(h))


def test_mode0_switches_path_at_16384_rows(gpu_lib):
    """n = 16,384 + 5: the first row count at which mode 0 can take the fp16 path; it does once n x P reaches 2^22 (P = 256),
    not at P = 5.  The plan says which; the stats must agree, and the answer is the same either way."""
    n, dim = 16384 + 5, 512
    rng = np.random.default_rng(160)
    rows = unit_rows(rng, n, dim)
    lib, h = raw_index(gpu_lib, rows)
    prompts = unit_rows(rng, 5, dim)
    L, best = label_ref.row_labels(label_ref.distances(rows, prompts))
    for mode in (1, 2, 0):
        got = c_label(gpu_lib, lib, h, n, prompts, mode)
        assert_rows(got, L, best, f"P 5 mode {mode}")
        fp16 = plan(gpu_lib, n, dim, 5, mode)["fp16"] == 1
        assert fp16 == (mode == 2) and (got["stats"] == [0, 0, n]) == (not fp16), got["stats"]
    prompts = unit_rows(rng, 256, dim)
    exact = c_label(gpu_lib, lib, h, n, prompts, 1)          # (the exact path is pinned to the oracle above and in every other test)
    assert plan(gpu_lib, n, dim, 256, 0)["fp16"] == 1 and plan(gpu_lib, n - 6, dim, 256, 0)["fp16"] == 0
    for mode in (2, 0):
        got = c_label(gpu_lib, lib, h, n, prompts, mode)
        assert_rows(got, exact["lab"], exact["dist"], f"P 256 mode {mode}")
        assert got["stats"][0] > n // 2, got["stats"]
    gpu_lib.check(lib.vq_index_destroy(h))


def test_dim64_is_exact_only(gpu_lib):
    n, P, dim = 300, 40, 64
    rng = np.random.default_rng(64)
    rows, prompts = unit_rows(rng, n, dim), unit_rows(rng, P, dim)
    lib, h = raw_index(gpu_lib, rows)
    L, best = label_ref.row_labels(label_ref.distances(rows, prompts))
    for mode in (1, 0):
        assert_rows(c_label(gpu_lib, lib, h, n, prompts, mode), L, best, f"dim 64 mode {mode}")
    got = c_label(gpu_lib, lib, h, n, prompts, 2)
    assert got["rc"] == -1 and (got["lab"] == SENTINEL).all() and (got["dist"] == SENTINEL).all()
    gpu_lib.check(lib.vq_index_destroy(h))


# ---- hard data ----
def near(rng, v, eps):
    g = rng.standard_normal(v.shape)
    w = v.astype(np.float64) + eps * g / np.linalg.norm(g)
    return (w / np.linalg.norm(w)).astype(np.float32)


@pytest.mark.parametrize("dim", [512, 768])
def test_duplicates_pairs_and_triples_force_the_rescore_and_the_redo(gpu_lib, dim):
    """Prompts 0/1 are 1e-4 apart (far inside E / 4 ~ 2.7e-4), 5/6/7 a triple that close, 10/11 exact duplicates; the rows lie
    near prompt 0, 5, 10 or nowhere.  A row near the pair has two keys inside 2 E and the third far below: its two candidates
    are re-scored; a row near the triple is filed for the redo; a row near the duplicates must go to the smaller index."""
    rng = np.random.default_rng([77, dim])
    P, n = 40, 400
    prompts = unit_rows(rng, P, dim)
    prompts[1] = near(rng, prompts[0], 1e-4)
    prompts[6], prompts[7] = near(rng, prompts[5], 1e-4), near(rng, prompts[5], 1e-4)
    prompts[11] = prompts[10]
    rows = unit_rows(rng, n, dim)
    for r in range(0, 300):
        rows[r] = near(rng, prompts[(0, 5, 10)[r % 3]], 0.5)
    lib, h = raw_index(gpu_lib, rows)
    L, best = label_ref.row_labels(label_ref.distances(rows, prompts))
    assert not (L == 11).any() and (L == 10).sum() >= 90           # the duplicate never wins
    for mode in (1, 2):
        got = c_label(gpu_lib, lib, h, n, prompts, mode)
        assert_rows(got, L, best, f"dim {dim} mode {mode}")
        if mode == 2:
            assert got["stats"][1] >= 100 and got["stats"][2] >= 90 and got["stats"][0] >= 50, got["stats"]
    gpu_lib.check(lib.vq_index_destroy(h))


def test_identical_rows_and_rows_equal_to_a_prompt(gpu_lib):
    rng = np.random.default_rng(5)
    dim, P = 512, 300
    prompts = unit_rows(rng, P, dim)
    same = np.repeat(unit_rows(rng, 1, dim), 260, axis=0)
    eq = np.concatenate([prompts[[3, 299, 256, 255]], unit_rows(rng, 125, dim)])
    for name, rows in (("identical", same), ("equal", eq)):
        lib, h = raw_index(gpu_lib, rows)
        L, best = label_ref.row_labels(label_ref.distances(rows, prompts))
        if name == "equal":
            assert L[:4].tolist() == [3, 299, 256, 255] and (np.abs(best[:4]) < 1e-6).all()
        for mode in (1, 2):
            assert_rows(c_label(gpu_lib, lib, h, len(rows), prompts, mode), L, best, f"{name} mode {mode}")
        gpu_lib.check(lib.vq_index_destroy(h))


def test_max_dist_is_inclusive_on_the_labelled_side(gpu_lib):
    rng = np.random.default_rng(9)
    n, P, dim = 500, 20, 512
    rows, prompts = unit_rows(rng, n, dim), unit_rows(rng, P, dim)
    lib, h = raw_index(gpu_lib, rows)
    D = label_ref.distances(rows, prompts)
    L0, best = label_ref.row_labels(D)
    r = int(np.argsort(best)[n // 2])
    at = best[r]
    below = np.nextafter(at, np.float32(-np.inf), dtype=np.float32)
    for mode in (1, 2):
        for md, labelled in ((at, True), (below, False)):
            L, b = label_ref.row_labels(D, md)
            assert (L[r] >= 0) == labelled and b.tobytes() == best.tobytes() and 0 < (L < 0).sum() < n
            got = c_label(gpu_lib, lib, h, n, prompts, mode, max_dist=float(md))
            assert_rows(got, L, best, f"mode {mode} max_dist {md!r}")
    gpu_lib.check(lib.vq_index_destroy(h))


def test_prompts_far_from_unit_norm_are_answered_exactly(gpu_lib):
    rng = np.random.default_rng(10)
    n, P, dim = 300, 12, 512
    rows, prompts = unit_rows(rng, n, dim), unit_rows(rng, P, dim)
    lib, h = raw_index(gpu_lib, rows)
    for scale in (1e-5, 1e5):
        p = prompts.copy()
        p[4] = (p[4] * np.float32(scale)).astype(np.float32)
        L, best = label_ref.row_labels(label_ref.distances(rows, p))
        for mode in (1, 2):
            got = c_label(gpu_lib, lib, h, n, p, mode)
            assert_rows(got, L, best, f"scale {scale} mode {mode}")
            assert got["stats"] == [0, 0, n], got["stats"]           # none counted as proven
    gpu_lib.check(lib.vq_index_destroy(h))


# ---- groups ----
def group_case(rng, kind):
    """-> dense labels [n] (every label holds a row)"""
    if kind == "singletons":
        return np.arange(200)
    if kind == "straddle":                                  # groups of 100 rows: most straddle a 128-row stream
        return np.arange(1000) // 100
    if kind == "long":                                      # one group of 5,000 rows among small ones
        return np.concatenate([np.arange(30) // 3, np.full(5000, 10), 11 + np.arange(40) // 4])
    if kind == "longer":                                    # 20,000 rows, not a whole number of pieces, between small groups
        return np.concatenate([np.arange(20) // 5, np.full(20_000, 4), 5 + np.arange(30) // 3])
    if kind == "scattered":
        return rng.permutation(np.arange(900) % 7)
    raise AssertionError(kind)


PIECES = {"singletons": 0, "straddle": 0, "long": 2, "longer": 5, "scattered": 0}      # of the longest group in the split form


@pytest.mark.parametrize("kind", ["singletons", "straddle", "long", "longer", "scattered"])
def test_group_tags(gpu_lib, kind):
    rng = np.random.default_rng([31, len(kind)])
    dim, P = 512, 24
    groups = group_case(rng, kind)
    n, G = len(groups), int(groups.max()) + 1
    assert plan(gpu_lib, n, dim, P, 0, int(np.bincount(groups).max()))["pieces"] == PIECES[kind]     # the form the longest group takes
    rows, _, _ = video_rows(n, dim, 3)
    prompts = unit_rows(rng, P, dim)
    if kind == "longer":                                    # equal best distances in different pieces: the show row follows the ranks
        rows[30 + 9000], rows[30 + 17000] = rows[30 + 100], rows[30 + 100]
    rows[5] = rows[4]                                       # a planted duplicate frame: the show row follows the ranks
    ranks = rng.permutation(n)
    lib, h = raw_index(gpu_lib, rows, groups, ranks)
    D = label_ref.distances(exported(gpu_lib, lib, h, n, dim), prompts)
    md = float(np.sort(label_ref.row_labels(D)[1])[int(n * 0.9)])    # a tenth of the rows unlabelled
    for max_dist in (INF, md):
        L, best = label_ref.row_labels(D, max_dist)
        for m in (1, 3, 16):                                # 16: more slots than voted labels in the small groups
            want = label_ref.group_tags(L, best, groups, ranks, G, m)
            assert kind != "singletons" or m == 1 or (want[0][:, 1:] == -1).all()     # fewer voted labels than slots
            for mode in (1, 2):
                got = c_label(gpu_lib, lib, h, n, prompts, mode, max_dist=max_dist, m=m, G=G)
                what = f"{kind} m {m} mode {mode} max_dist {max_dist}"
                assert_rows(got, L, best, what)
                assert_groups(got, want, what)
    gpu_lib.check(lib.vq_index_destroy(h))


def test_python_layer_string_ids_duplicates_and_lifetimes(gpu_lib):
    """HNSWIndex.label_rows / label_groups over string ids whose order differs from the rows' (ranks are set), with planted
    duplicate frames inside a video: `show` ties follow the ids.  Then remove_batch (labels and ranks are compacted with the
    rows and stay valid) and an update of a stored id (kept), each checked against the restatement again."""
    from video_quierer_amd.indexes.hnsw import OptimizedHNSWIndex
    dim, n, P = 512, 700, 30
    rows, video, frame = video_rows(n, dim, 12, lengths=[1, 7, 63, 64, 65, 300])
    for a, b in ((20, 12), (21, 12), (100, 140)):           # "v2_10" sorts before "v2_2"
        rows[a] = rows[b]
    ids = [f"v{v}_{f}" for v, f in zip(video, frame)]
    prompts = unit_rows(np.random.default_rng(13), P, dim)
    idx = OptimizedHNSWIndex(dimension=dim)
    idx.add_batch(rows, ids)

    def check(tag):
        stored = idx._export()
        cur = list(idx._ids)
        groups, keys = [], {}
        for nid in cur:
            groups.append(keys.setdefault(nid.rsplit("_", 1)[0], len(keys)))
        D = label_ref.distances(stored, np.ascontiguousarray(idx._unit_rows(prompts), dtype=np.float32))   # normalised as `search` does
        for max_distance in (None, float(np.median(label_ref.row_labels(D)[1]))):
            L, best = label_ref.row_labels(D, INF if max_distance is None else max_distance)
            for mode in (1, 2):
                lab, dist = idx.label_rows(prompts, max_distance=max_distance, mode=mode)
                assert np.array_equal(lab, L) and dist.tobytes() == best.tobytes(), f"{tag} mode {mode}"
                idx.search_mode = mode
                res = idx.label_groups(prompts, top=3, max_distance=max_distance)
                tags, votes, show, _ = label_ref.group_tags(L, best, groups, tie_ranks(cur), len(keys), 3)
                sizes = np.bincount(groups)
                assert list(res) == list(keys)
                for g, key in enumerate(keys):
                    want = [{"label": int(j), "votes": int(v), "share": int(v) / int(sizes[g]), "id": cur[r], "distance": best[r]}
                            for j, v, r in zip(tags[g], votes[g], show[g]) if j >= 0]
                    assert res[key] == want, f"{tag} mode {mode} group {key}: {res[key]} want {want}"
    check("fresh")
    idx.remove_batch([i for i in ids if i.startswith("v3_")][::2] + ["v0_0"])
    check("after remove_batch")
    idx.add(np.asarray(prompts[7] + 0.01 * rows[0]), "v2_5")     # an id the index holds: its row is replaced
    check("after an update")
    idx.close()


def test_tag_videos(gpu_lib):
    from video_quierer_amd.overhaul_index import SimpleVideoIndex
    dim, n = 512, 300
    rows, video, frame = video_rows(n, dim, 21, lengths=[40, 100, 160])
    prompts = np.random.default_rng(22).standard_normal((9, dim)).astype(np.float32) * 3.0     # normalised by the call
    sv = SimpleVideoIndex()
    for r in range(n):
        sv.add_frame(rows[r], f"clip{video[r]}", 0.5 * frame[r])
    names = [f"tag{j}" for j in range(9)]
    res = sv.tag_videos(prompts, tags=names, top=2)
    pu = unit(prompts)
    D = label_ref.distances(rows, np.stack([(q / (np.linalg.norm(q) + 1e-10)).astype(np.float32) for q in prompts]))
    L, best = label_ref.row_labels(D)
    groups = np.asarray(video)
    tags, votes, show, _ = label_ref.group_tags(L, best, groups, -np.arange(n), int(groups.max()) + 1, 2)   # ties: the larger frame id first
    assert pu.shape == (9, dim) and list(res) == [f"clip{g}" for g in range(int(groups.max()) + 1)]
    for g in range(int(groups.max()) + 1):
        want = [{"tag": names[j], "frames": int(v), "share": int(v) / int((groups == g).sum()), "timestamp": 0.5 * frame[r], "frame_id": int(r),
                 "score": float(np.float32(1.0) - best[r])} for j, v, r in zip(tags[g], votes[g], show[g]) if j >= 0]
        assert res[f"clip{g}"] == want
    assert [t["tag"] for t in sv.tag_videos(prompts, top=1)["clip0"]] == [int(tags[0][0])]


# ---- the fp16 path cannot pass by always falling back ----
@pytest.mark.parametrize("dim,P,seed", [(512, 257, 1), (512, 600, 2), (768, 257, 3), (768, 600, 4)])
def test_rows_with_a_clear_gap_are_proven(gpu_lib, dim, P, seed):
    """Random unit rows and prompts, n = 4,096.  E: the bound vq_debug_label_plan exports (1.07e-3 at dim 512, 1.11e-3 at 768:
    below 1.5e-3, so P = 600 is tested too).  A row whose best and second-best exact scores differ by more than 4 E has keys
    more than 2 E apart, which is the proof's condition: it must be counted in stats[0].  Scores in fp64 (their error, 1e-16,
    is nothing beside E); the labels and distances are checked against the exact path, which the other tests pin to the oracle."""
    n = 4096
    rng = np.random.default_rng([4096, seed])
    rows, prompts = unit_rows(rng, n, dim), unit_rows(rng, P, dim)
    E = plan_eps(gpu_lib, n, dim, P)
    assert 1.0e-3 < E < 1.5e-3, E
    S = np.sort(rows.astype(np.float64) @ prompts.astype(np.float64).T, axis=1)
    clear = (S[:, -1] - S[:, -2]) > 4 * E
    print(f"dim {dim} P {P} seed {seed}: E {E:.4e} share of rows with a gap above 4 E {clear.mean():.3f}")
    assert clear.mean() >= 0.5                              # so that the check below has teeth
    lib, h = raw_index(gpu_lib, rows)
    exact = c_label(gpu_lib, lib, h, n, prompts, 1)
    got = c_label(gpu_lib, lib, h, n, prompts, 2)
    print(f"stats {got['stats']}")
    assert_rows(got, exact["lab"], exact["dist"], f"dim {dim} P {P}")
    assert np.array_equal(exact["lab"][clear], np.argmax(rows.astype(np.float64) @ prompts.astype(np.float64).T, axis=1)[clear])
    assert got["stats"][0] >= int(clear.sum()), (got["stats"], int(clear.sum()))
    gpu_lib.check(lib.vq_index_destroy(h))


# ---- refusals, repeats, the device form ----
def test_refusals_leave_the_outputs_untouched(gpu_lib):
    rng = np.random.default_rng(50)
    n, dim = 200, 512
    rows, prompts = unit_rows(rng, n, dim), unit_rows(rng, 8, dim)
    lib, h = raw_index(gpu_lib, rows)                       # no group labels

    def refused(got):
        assert got["rc"] == -1, got["rc"]
        for name in ("lab", "dist", "tags", "votes", "show", "unl"):
            assert got[name] is None or (got[name] == SENTINEL).all(), name
    big = np.zeros((4097, dim), dtype=np.float32)
    refused(c_label(gpu_lib, lib, h, n, big, 1))                                    # P out of range
    out = np.full(n, SENTINEL, np.int32)
    assert lib.vq_index_label_rows(h, gpu_lib.fptr(prompts), 0, 1, c_float(INF), _i32(out), None, 0, None, None, None, None) == -1
    assert (out == SENTINEL).all()
    refused(c_label(gpu_lib, lib, h, n, prompts, 1, m=3, G=4))                      # group outputs without labels
    refused(c_label(gpu_lib, lib, h, n, prompts, 3))                                # unknown mode
    refused(c_label(gpu_lib, lib, h, n, prompts, 1, max_dist=math.nan))
    bad = prompts.copy()
    bad[5, 100] = np.inf
    refused(c_label(gpu_lib, lib, h, n, bad, 2))                                    # a prompt that is not finite
    bad[5, 100] = np.nan
    refused(c_label(gpu_lib, lib, h, n, bad, 1))
    groups = np.arange(n) // 50
    gpu_lib.check(lib.vq_index_set_groups(h, _i32(groups.astype(np.int32)), n, 4))
    for m in (0, 17, -1):
        got = dict(tags=np.full((4, 17), SENTINEL, np.int32), votes=np.full((4, 17), SENTINEL, np.int32), show=np.full((4, 17), SENTINEL, np.int32),
                   unl=np.full(4, SENTINEL, np.int32), lab=np.full(n, SENTINEL, np.int32), dist=None)
        got["rc"] = lib.vq_index_label_rows(h, gpu_lib.fptr(prompts), 8, 1, c_float(INF), _i32(got["lab"]), None, m, _i32(got["tags"]),
                                            _i32(got["votes"]), _i32(got["show"]), _i32(got["unl"]))
        refused(got)                                                                # m out of range
    assert c_label(gpu_lib, lib, h, n, prompts, 1, m=16, G=4)["rc"] == 0
    more = unit_rows(rng, 10, dim)
    gpu_lib.check(lib.vq_index_add(h, gpu_lib.fptr(more), 10, 0))
    refused(c_label(gpu_lib, lib, h, n + 10, prompts, 2, m=3, G=4))                 # the labels are stale now
    assert c_label(gpu_lib, lib, h, n + 10, prompts, 2)["rc"] == 0                  # row labels alone need none
    gpu_lib.check(lib.vq_index_destroy(h))
    # an empty index: 0, nothing written
    lib, h = raw_index(gpu_lib, np.empty((0, dim), dtype=np.float32))
    got = c_label(gpu_lib, lib, h, 4, prompts, 0)
    assert got["rc"] == 0 and (got["lab"] == SENTINEL).all() and got["stats"] == [0, 0, 0]
    gpu_lib.check(lib.vq_index_destroy(h))


def test_repeat_is_bit_identical_and_device_form_matches(gpu_lib):
    rng = np.random.default_rng(60)
    n, P, dim, m = 2500, 300, 512, 4
    rows, _, _ = video_rows(n, dim, 61)
    prompts = unit_rows(rng, P, dim)
    prompts[1] = near(rng, prompts[0], 1e-4)
    groups = (np.arange(n) // 90).astype(np.int32)
    G = int(groups.max()) + 1
    lib, h = raw_index(gpu_lib, rows, groups)
    L, best = label_ref.row_labels(label_ref.distances(rows, prompts), 0.95)
    want = label_ref.group_tags(L, best, groups, np.arange(n), G, m)
    hip = ctypes.CDLL("libamdhip64.so")
    ptrs = []

    def dev(nbytes):
        p = c_void_p()
        assert hip.hipMalloc(byref(p), ctypes.c_size_t(nbytes)) == 0
        ptrs.append(p)
        return p
    dp, dl, dd = dev(prompts.nbytes), dev(4 * n), dev(4 * n)
    dt, dv, ds, du = dev(4 * G * m), dev(4 * G * m), dev(4 * G * m), dev(4 * G)
    assert hip.hipMemcpy(dp, prompts.ctypes.data_as(c_void_p), ctypes.c_size_t(prompts.nbytes), 1) == 0
    for mode in (1, 2):
        first = c_label(gpu_lib, lib, h, n, prompts, mode, max_dist=0.95, m=m, G=G)
        assert_rows(first, L, best, f"mode {mode}")
        assert_groups(first, want, f"mode {mode}")
        again = c_label(gpu_lib, lib, h, n, prompts, mode, max_dist=0.95, m=m, G=G)
        for name in ("lab", "dist", "tags", "votes", "show", "unl"):
            assert first[name].tobytes() == again[name].tobytes(), name
        assert first["stats"] == again["stats"]
        gpu_lib.check(lib.vq_index_label_rows_device(h, dp, P, mode, c_float(0.95), dl, dd, m, dt, dv, ds, du))
        gpu_lib.check(lib.vq_index_synchronize(h))
        assert stats_of(gpu_lib, lib, h) == first["stats"]
        for name, p in (("lab", dl), ("dist", dd), ("tags", dt), ("votes", dv), ("show", ds), ("unl", du)):
            host = np.empty_like(first[name])
            assert hip.hipMemcpy(host.ctypes.data_as(c_void_p), p, ctypes.c_size_t(host.nbytes), 2) == 0
            assert host.tobytes() == first[name].tobytes(), f"device form mode {mode}: {name}"
    # the device form with a prompt outside the bound's range: flagged on the device, every row by the exact redo
    scaled = prompts.copy()
    scaled[2] *= np.float32(1e-5)
    Ls, bs = label_ref.row_labels(label_ref.distances(rows, scaled))
    assert hip.hipMemcpy(dp, scaled.ctypes.data_as(c_void_p), ctypes.c_size_t(scaled.nbytes), 1) == 0
    gpu_lib.check(lib.vq_index_label_rows_device(h, dp, P, 2, c_float(INF), dl, dd, 0, None, None, None, None))
    gpu_lib.check(lib.vq_index_synchronize(h))
    assert stats_of(gpu_lib, lib, h) == [0, 0, n]
    hl, hd = np.empty(n, np.int32), np.empty(n, np.float32)
    assert hip.hipMemcpy(hl.ctypes.data_as(c_void_p), dl, ctypes.c_size_t(4 * n), 2) == 0
    assert hip.hipMemcpy(hd.ctypes.data_as(c_void_p), dd, ctypes.c_size_t(4 * n), 2) == 0
    assert np.array_equal(hl, Ls) and hd.tobytes() == bs.tobytes()
    for p in ptrs:
        assert hip.hipFree(p) == 0
    gpu_lib.check(lib.vq_index_destroy(h))
