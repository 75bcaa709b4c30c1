"""CPU (`-m "not gpu"`): the dictated layouts of the exact stage tests (tests/exact_stage_ref.py), on their own.

  - the closed form agrees with the C oracle on every layout class: knn_oracle.topk where ties go by row, the (distance, id) rule of
    test_gpu_parity._expected_in_id_order where id ranks are set, the oracle over the allowed rows under a mask;
  - vq_debug_fallback_plan (host-only) is pinned at the GPU cases' shapes and at 1M, 8M and 2^31 - 1 rows, and keeps inside what
    the kernels' LDS arrays hold over a product of shapes;
  - the case tables cover what they claim: every k, flagged count and dim, every class under every mask and rank kind;
  - the thread-column layout collects the count it is built for: above the 1,024-entry list, its twin at k - 1 inside it;
  - non-vacuity: numpy models of the redo (tile filter + fold, k-way merge with slot bases), of select_small_kernel (threshold,
    collect, rank) and of the chunk lists + merge give the closed form on every case, and each defect planted in them is caught
    by a class CAUGHT_BY names, on every path that has the mechanism;
  - the two debug entries are exported.
"""
import ctypes

import numpy as np
import pytest

import exact_stage_ref as xr
from oracle import knn_oracle


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g
    g.build()
    from video_quierer_amd import _lib
    _lib.load()
    return _lib


def plan(L, n, nq, k):
    return xr.fallback_plan(L.load(), L.check, n, nq, k)


# ---------------------------------------------------------------- closed form against the C oracle
def in_id_order(rows, qs, ids, k, allowed=None):
    """test_gpu_parity._expected_in_id_order over the allowed rows: sorted (distance, id) tuples, tie groups whole"""
    out = []
    keep = np.arange(len(rows)) if allowed is None else np.nonzero(allowed)[0]
    for q in qs:
        d = knn_oracle.distances(rows, q)[keep]
        if not len(d):
            out.append([])
            continue
        kth = np.partition(d, min(k, len(d)) - 1)[min(k, len(d)) - 1]
        cand = np.nonzero(d <= kth)[0]
        out.append(sorted((d[r], int(ids[keep[r]]), int(keep[r])) for r in cand)[:k])
    return out


def check_against_oracle(tag, sc, k):
    got_ids, got_dist = xr.closed_form(sc.a, sc.b, sc.Q, k, sc.tie, sc.allowed)
    if sc.tie is None and sc.allowed is None:
        want_ids, want_dist = knn_oracle.topk(sc.rows, sc.Q.q, k)
        assert xr.same_bits(got_ids, got_dist, want_ids, want_dist), f"{tag}: the closed form differs from knn_oracle.topk"
        return
    ids = np.arange(len(sc.a)) if sc.tie is None else sc.tie
    for j, want in enumerate(in_id_order(sc.rows, sc.Q.q, ids, k, sc.allowed)):
        n_real = len(want)
        assert got_ids[j][:n_real].tolist() == [r for _, _, r in want] and (got_ids[j][n_real:] == -1).all(), f"{tag} query {j}: ids"
        assert np.array_equal(got_dist[j][:n_real].view(np.uint32), np.array([d for d, _, _ in want], np.float32).view(np.uint32)), f"{tag} query {j}"
        assert np.isposinf(got_dist[j][n_real:]).all()


@pytest.mark.parametrize("case", [c for c in xr.fb_cases() if c.n <= 513 or c.ranks == xr.RANKS[xr.FB_CLASSES.index(c.cls) % 3]], ids=xr.fb_id)
def test_closed_form_is_the_oracles_on_the_fallback_layouts(L, case):
    for run in xr.fb_runs(case):
        p = plan(L, case.n, 2 * run.count + 1, run.k)
        S = p.fast_rows if run.count <= xr.FAST_SLOTS else p.rows
        sc = xr.scene(case.cls, case.n, run.k, S, run.dim, 16, case.ranks, run.mask, filler=True)
        n2 = (sc.rows.astype(np.float64) ** 2).sum(axis=1)
        assert 0.5 <= n2.min() and n2.max() < 1.95, "the fp16 path takes near-unit rows only"
        check_against_oracle(f"{xr.fb_id(case)} {run}", sc, run.k)


def EX_SHARE(case):
    """the third of a case's runs (one rank kind) the CPU checks walk"""
    return (xr.EX_CLASSES.index(case.cls) + xr.EX_NS.index(case.n)) % 3


@pytest.mark.parametrize("case", [c for c in xr.ex_cases() if c.n != 32768], ids=xr.ex_id)
def test_closed_form_is_the_oracles_on_the_exact_layouts(case):
    for run in xr.ex_runs(case)[EX_SHARE(case)::3]:
        sc = xr.scene(case.cls, case.n, run.k, xr.SEL_CHUNK, min(run.dim, 100), min(run.nq, 9), run.ranks, None, filler=False)
        check_against_oracle(f"{xr.ex_id(case)} {run}", sc, run.k)


@pytest.mark.parametrize("n,k,about", xr.COLUMN)
def test_thread_columns_collect_the_count_they_are_built_for(n, k, about):
    cls = "ascending" if n <= 1020 else "thread_column"
    for ranks in xr.RANKS:
        sc = xr.scene(cls, n, k, xr.SEL_CHUNK, 64, 8, ranks, None, filler=False)
        check_against_oracle(f"column n={n} k={k}", sc, k)
        d = xr.distances(sc.a, sc.b, sc.Q, 0)
        ids, dist, info = xr.model_select_small(d, sc.tie, k)
        assert xr.same_bits(ids, dist, *xr.topk(d, k, sc.tie))
        rows_per_thread = n // 256
        if cls == "thread_column":
            assert info["c"] == (k - 1) * rows_per_thread + 1, info
            assert (info["c"] > xr.SMALL_LIST) == (about == "overflow") and info["padding"] == 0
        elif about.startswith("padding"):
            pieces = (n + 3) // 4
            assert pieces < min(k, n) <= 256 and info["padding"] > 0 and info["c"] == n + info["padding"], info      # the empty key is the threshold
            assert (info["c"] <= xr.SMALL_LIST) == (about == "padding-list")
        else:
            assert info["padding"] == 0 and info["c"] <= xr.SMALL_LIST
    if about == "overflow":                                       # the smallest overflowing k of each n has its fitting twin at k - 1
        k0 = min(kk for nn, kk, ab in xr.COLUMN if nn == n and ab == "overflow")
        assert (n, k0 - 1, "fits") in xr.COLUMN


def test_thread_ownership_is_the_kernels():
    """piece p = rows 4p .. 4p + 3 goes to thread p & 255: p0 = tid + 1024 i, pieces p0, p0 + 256, p0 + 512, p0 + 768"""
    owner = np.full(40000, -1)
    for tid in range(256):
        for p0 in range(tid, 10000, 1024):
            for u in range(4):
                owner[4 * (p0 + 256 * u):4 * (p0 + 256 * u) + 4] = tid
    assert np.array_equal(owner, xr.thread_of(np.arange(40000)))


# ---------------------------------------------------------------- the plan
PINNED = [((1, 1, 1), (1, 256, 1, 256, 8, 64)), ((513, 147, 10), (2, 512, 1, 768, 152, 1520)), ((16385, 147, 100), (33, 512, 9, 2048, 152, 211200)),
          ((16385, 1, 1), (33, 512, 9, 2048, 8, 2112)), ((89 * 2048 + 1, 1000, 100), (357, 512, 90, 2048, 928, 8352000)),
          ((1 << 20, 32, 10), (2048, 512, 512, 2048, 32, 1310720)), ((1 << 23, 1000, 100), (4096, 2048, 4096, 2048, 16, 26214400)),
          ((2 ** 31 - 1, 4096, 100), (4096, 524288, 4096, 524288, 16, 26214400))]


@pytest.mark.parametrize("args,want", PINNED)
def test_fallback_plan_is_pinned(L, args, want):
    assert tuple(plan(L, *args)) == want


def test_fallback_plan_keeps_inside_the_kernels_arrays(L):
    for n in (1, 2, 255, 256, 257, 511, 512, 513, 2047, 2048, 2049, 16385, 100_000, 1 << 20, (1 << 21) + 1, 1 << 23, (1 << 23) + 1, 10 ** 9, 2 ** 31 - 1):
        for nq in (1, 7, 8, 9, 64, 65, 1000, 4096, 100_000):
            for k in (1, 10, 99, 100):
                p = plan(L, n, nq, k)
                for splits, rows in ((p.fast_splits, p.fast_rows), (p.splits, p.rows)):
                    assert 1 <= splits <= xr.MAX_SPLITS and rows % xr.TILE == 0 and splits * rows >= n and (splits - 1) * rows < n, (n, nq, k, p)
                assert p.round_q % xr.QG == 0 and p.round_q >= xr.QG
                assert p.partial >= max(p.round_q * p.splits, xr.FAST_SLOTS * p.fast_splits) * k
                assert p.round_q * p.splits * k * 8 <= max(64 << 20, xr.QG * p.splits * k * 8)
    assert xr.KMAX <= 255                                        # fallback_merge_kernel keeps a list's position in a uint8_t
    for bad in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (1, 1, 101), (2 ** 31, 1, 1)):
        out = (ctypes.c_int64 * 6)()
        assert L.load().vq_debug_fallback_plan(*bad, out) != 0


def test_the_gpu_shapes_reach_what_they_name(L):
    p = plan(L, 513, 147, 10)
    assert p.fast_splits == 2 and 513 - p.fast_rows == 1 and p.splits == 1
    p = plan(L, 16385, 147, 100)
    assert p.splits == 9 and 16385 - 8 * p.rows == 1 and p.round_q >= 147
    n, nq, k = 89 * 2048 + 1, 1000, 100
    p = plan(L, n, nq, k)
    r = xr.rounds(p, nq, nq)
    assert p.round_q < nq - 64 and [x[1] for x in r] == [64, 928, 8] and [x[0] for x in r] == [0, 64, 992] and n - 89 * p.rows == 1
    assert len(xr.rounds(plan(L, 16385, 147, 100), 147, 73)) == 2 and len(xr.rounds(plan(L, 16385, 129, 100), 129, 64)) == 1


def test_the_case_tables_cover_what_they_claim():
    for n in xr.FB_NS[1:]:
        runs = [(c, r) for c in xr.fb_cases() if c.n == n for r in xr.fb_runs(c)]
        assert {r.k for _, r in runs} == set(xr.FB_KS) and {r.count for _, r in runs} == set(xr.FB_COUNTS) and {r.dim for _, r in runs} == set(xr.FB_DIMS)
        assert {(c.cls, r.mask) for c, r in runs} == {(cls, m) for cls in xr.FB_CLASSES for m in xr.MASKS}
        assert {(c.cls, c.ranks) for c, _ in runs} == {(cls, rk) for cls in xr.FB_CLASSES for rk in xr.RANKS}
        assert {(r.mask, r.exclude) for _, r in runs} >= {(m, e) for m in xr.MASKS[1:] for e in (0, 1)}
        assert {(r.count, r.mask is None) for _, r in runs} >= {(c, m) for c in xr.FB_COUNTS for m in (True, False)}
    runs = [(c, r) for c in xr.ex_cases() for r in xr.ex_runs(c)]
    assert {c.n for c, _ in runs} == set(xr.EX_NS) and {r.dim for _, r in runs} == set(xr.EX_DIMS)
    for n in xr.EX_NS:
        assert {r.k for c, r in runs if c.n == n} == set(xr.EX_KS) and {r.nq for c, r in runs if c.n == n} == set(xr.EX_NQS)
        paths = {xr.exact_path(n, r.nq, r.dim) for c, r in runs if c.n == n}
        assert paths == ({"small", "chunks"} if n <= xr.SMALL_MAX_N else {"chunks"})
    assert {(xr.exact_path(c.n, r.nq, r.dim), r.dim) for c, r in runs} >= {("chunks", 1540), ("small", 1536)}
    assert all(r.k <= 1024 for _, r in runs)
    flags = xr.fb_flags(73)
    assert len(flags) == 147 and set(flags[::2].tolist()) == {0, 1} and not set(flags[1::2].tolist()) & {0, 1} and len(set(flags[1::2].tolist())) > 3
    ids, dist = xr.sentinels(147, 100)
    assert len(np.unique(ids)) == ids.size and len(np.unique(dist.view(np.uint32))) == dist.size and np.isnan(dist).all() and (ids < -1).all()


# ---------------------------------------------------------------- the models, clean and with planted defects
# the flagged-list positions the models work out: the special queries, a positive e0 query, the bulk round's first and last
def model_slots(count):
    return sorted({s for s in (0, 1, 2, 3, 4, 5, 6, 7, 63, 64, 65, count - 1) if 0 <= s < count})


def fallback_model_cases(L):
    """-> [(path, class, tag, run(defect) -> ok)]"""
    out = []
    for case in xr.fb_cases():
        if case.n > 513 and case.ranks != xr.RANKS[xr.FB_CLASSES.index(case.cls) % 3]:
            continue
        for run in xr.fb_runs(case):
            if run.count == 0:
                continue
            flags = xr.fb_flags(run.count)
            p = plan(L, case.n, len(flags), run.k)
            S = p.fast_rows if run.count <= xr.FAST_SLOTS else p.rows
            sc = xr.scene(case.cls, case.n, run.k, S, 64, len(flags), case.ranks, run.mask, filler=True)
            only = model_slots(run.count)
            which = [2 * s + 1 for s in only]
            want = xr.closed_form(sc.a, sc.b, sc.Q, run.k, sc.tie, sc.allowed, which)
            out.append(("fallback", case.cls, f"{xr.fb_id(case)} {run}", make_fb_runner(sc, run.k, flags, p, only, which, want)))
    n, nq, k = 89 * 2048 + 1, 1000, 100
    p = plan(L, n, nq, k)
    sc = xr.scene("last_row", n, k, p.rows, 64, nq, None, None, filler=True)
    only = [0, 63, 64, 991, 992, 999]
    want = xr.closed_form(sc.a, sc.b, sc.Q, k, None, None, only)
    out.append(("fallback", "last_row", "bulk rounds", make_fb_runner(sc, k, np.full(nq, 2, np.int32), p, only, only, want)))
    return out


def make_fb_runner(sc, k, flags, p, only, which, want):
    def run(defect):
        ids, dist, counters = xr.model_fallback(sc, k, flags, p, defect, only)
        flagged = int(((flags < 0) | (flags >= 2)).sum())
        assert counters == [flagged, int((flags == 0).sum()), int((flags == 1).sum()), flagged]
        return xr.same_bits(ids[which], dist[which], want[0][which], want[1][which])
    return run


def exact_model_cases():
    out = []
    for case in xr.ex_cases():
        if case.n == 32768:
            continue
        ri = EX_SHARE(case)
        for run in xr.ex_runs(case)[4 * ri:4 * ri + 4]:
            nq = min(run.nq, 8)
            sc = xr.scene(case.cls, case.n, run.k, xr.SEL_CHUNK, 4, nq, run.ranks, None, filler=False)
            path = xr.exact_path(case.n, run.nq, run.dim)
            want = xr.closed_form(sc.a, sc.b, sc.Q, run.k, sc.tie)
            out.append((path, case.cls, f"{xr.ex_id(case)} {run}", make_ex_runner(sc, run.k, nq, path, want)))
    for n, k, about in xr.COLUMN:
        for ranks in xr.RANKS:
            cls = "ascending" if n <= 1020 else "thread_column"
            sc = xr.scene(cls, n, k, xr.SEL_CHUNK, 4, 8, ranks, None, filler=False)
            out.append(("small", cls, f"column n={n} k={k} {ranks}", make_ex_runner(sc, k, 8, "small", xr.closed_form(sc.a, sc.b, sc.Q, k, sc.tie))))
    return out


def make_ex_runner(sc, k, nq, path, want):
    def run(defect):
        return all(xr.same_bits(*xr.model_exact(sc, k, j, path, defect), want[0][j], want[1][j]) for j in range(nq))
    return run


_cases = {}


def model_cases(L):
    if not _cases:
        _cases["all"] = fallback_model_cases(L) + exact_model_cases()
    return _cases["all"]


def test_the_models_give_the_closed_form(L):
    cases = model_cases(L)
    assert {path for path, _, _, _ in cases} == {"fallback", "small", "chunks"}
    for path, cls, tag, run in cases:
        assert run(None), f"{path} model, {tag}: differs from the closed form"


# the classes that must catch each defect: at least one of them, on every path that has the mechanism
CAUGHT_BY = {
    "no_displace": ("descending", "last_rows", "last_row"), "ragged_tile_dropped": ("last_row", "last_rows"),
    "merge_one_per_list": ("one_split", "last_rows", "alternating"), "no_slot_base": ("last_row",),
    "mask_ignored": ("ascending", "descending", "plateau_k"), "tie_by_row": ("plateau_k", "plateau_tile", "plateau_split", "plateau_chunk"),
    "unsigned_bits": ("signs",), "list_truncated": ("thread_column",), "threshold_low": ("one_per_split", "thread_column"),
    "chunk_tail_real": ("last_row", "last_rows", "ascending"),
}


@pytest.mark.parametrize("defect", xr.DEFECTS)
def test_each_planted_defect_is_caught(L, defect):
    assert set(CAUGHT_BY) == set(xr.DEFECTS) == set(xr.MECHANISM)
    caught = {}
    for path, cls, tag, run in model_cases(L):
        if path in xr.MECHANISM[defect] and not run(defect):
            caught.setdefault(path, set()).add(cls)
    print(defect, {p: sorted(c) for p, c in caught.items()})
    for path in xr.MECHANISM[defect]:
        assert caught.get(path, set()) & set(CAUGHT_BY[defect]), f"{defect} on the {path} path: caught only by {sorted(caught.get(path, ()))}"


def test_the_debug_entries_are_exported(L):
    for name in ("vq_debug_fallback_plan", "vq_index_debug_fallback"):
        assert name in L.SIGNATURES and hasattr(L.load(), name)
