"""GPU: pass 3 of an fp16 search (the exact redo) and the exact selection kernels, on distances the test dictates
(tests/exact_stage_ref.py).

Pass 1 is held to the key contract (tests/test_scan_stages.py) and pass 2 to soundness (tests/test_rescore_stages.py); here
  - vq_index_debug_fallback runs collect_flags_kernel and the search's own launch_fallback on flags the test wrote: the flagged
    slots must equal the closed form bit for bit, every other slot must keep the sentinel the test put there, and the counters
    must be {flagged, flags == 0, flags == 1, flagged};
  - vq_index_search(mode = 1) runs exact_dist(_small)_kernel and select_small_kernel or select_chunk_kernel + merge_topk_kernel
    on the same layouts;
  - vq_index_add(normalize = 1) + vq_index_export is held to knn_oracle.normalize_rows.
Ids and distances are compared as bits everywhere: no tolerance.  The layouts put the k best rows where the data-dependent
branches are (every tile displacing the list, one list supplying all k, empty splits, a plateau over a boundary, a threshold that
admits more keys than the list holds, negative distances); each case derives its shapes from vq_debug_fallback_plan and fails if
the plan no longer gives the geometry it names.  One line per case (the case, the branches reached, the seconds) is appended to
the file $VQ_EXACT_OUT names; profiles/exact_stages/outcomes.txt is one run.

Rows go in with normalize = 0 (except in the normalise test), so the fp32 data given IS the data stored.
"""
import ctypes
import os
import time

import numpy as np
import pytest

import exact_stage_ref as xr
from oracle import knn_oracle
from test_scan_stages import Index

pytestmark = pytest.mark.gpu
MODE_EXACT, MODE_FP16 = 1, 2


def record(line):
    print(line)
    out = os.environ.get("VQ_EXACT_OUT")
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def set_ranks(ix, rank):
    if rank is not None:
        ix.L.check(ix.lib.vq_index_set_id_ranks(ix.h, ix.L.i32ptr(rank), len(rank)))


def run_fallback(ix, qs, k, flags, ids0, dist0, filt=None):
    """the entry on copies of the initial results -> ids, dist, counters"""
    qs, flags = np.ascontiguousarray(qs, np.float32), np.ascontiguousarray(flags, np.int32)
    ids, dist, counters = ids0.copy(), dist0.copy(), np.zeros(4, np.int32)
    sel, n_sel, exclude = (None, 0, 0) if filt is None else (ix.L.i32ptr(filt[0]), len(filt[0]), filt[1])
    ix.L.check(ix.lib.vq_index_debug_fallback(ix.h, ix.L.fptr(qs), len(qs), k, ix.L.i32ptr(flags), sel, n_sel, exclude, ix.L.i32ptr(ids),
                                              ix.L.fptr(dist), ix.L.i32ptr(counters)))
    return ids, dist, counters.tolist()


def search_exact(ix, qs, k):
    qs = np.ascontiguousarray(qs, np.float32)
    ids, dist = np.empty((len(qs), k), np.int32), np.empty((len(qs), k), np.float32)
    ix.L.check(ix.lib.vq_index_search(ix.h, ix.L.fptr(qs), len(qs), k, MODE_EXACT, ix.L.i32ptr(ids), ix.L.fptr(dist)))
    return ids, dist


def assert_lists(tag, ids, dist, want_ids, want_dist, which):
    for j in which:
        assert xr.same_bits(ids[j], dist[j], want_ids[j], want_dist[j]), \
            f"{tag} query {j}: the list differs from the closed form\n got  {ids[j][:12]} {dist[j][:12]}\n want {want_ids[j][:12]} {want_dist[j][:12]}"


def fallback_branches(plan, nq, count, k, want_ids, want_dist, flagged, allowed):
    """what the expected lists say the kernels went through"""
    tags = [f"rounds={len(xr.rounds(plan, nq, count))}"]
    geo = [(S, splits) for _, _, S, splits in xr.rounds(plan, nq, count)]
    for S, splits in dict.fromkeys(geo):
        lists = [want_ids[j][want_ids[j] >= 0] // S for j in flagged]
        if any(len(l) == k and k > 1 and (l == l[0]).all() for l in lists):
            tags.append("pos=k")
        if any(len(l) == k == splits and len(set(l.tolist())) == k for l in lists):
            tags.append("one-per-split")
        if allowed is not None and splits > 1:
            full = [bool(allowed[s * S:(s + 1) * S].any()) for s in range(splits)]
            if any(full) and not all(full):
                tags.append("empty-split")
    if any((want_dist[j] < 0).any() and (want_dist[j][want_ids[j] >= 0] >= 0).any() for j in flagged):
        tags.append("neg-to-pos")
    if any((want_ids[j] < 0).any() for j in flagged):
        tags.append("short")
    return " ".join(dict.fromkeys(tags))


def fallback_once(gpu_lib, monkeypatch, tag, cls, n, ranks, run, twice=False):
    """one layout, one entry call -> the branch tags"""
    flags = xr.fb_flags(run.count)
    nq, k = len(flags), run.k
    plan = xr.fallback_plan(gpu_lib.load(), gpu_lib.check, n, nq, k)
    S = plan.fast_rows if run.count <= xr.FAST_SLOTS else plan.rows
    sc = xr.scene(cls, n, k, S, run.dim, nq, ranks, run.mask, filler=True)
    flagged = np.nonzero((flags < 0) | (flags >= 2))[0]
    assert len(flagged) == run.count
    want_ids, want_dist = xr.closed_form(sc.a, sc.b, sc.Q, k, sc.tie, sc.allowed, flagged)
    ids0, dist0 = xr.sentinels(nq, k)
    with Index(gpu_lib, monkeypatch, run.dim) as ix:
        ix.add(sc.rows)
        set_ranks(ix, sc.tie)
        filt = None
        if sc.allowed is not None:
            lab, G, sel, exclude = xr.labels_of(sc.allowed, run.exclude)
            ix.set_groups(lab, G)
            filt = (sel, exclude)
        ids, dist, counters = run_fallback(ix, sc.Q.q, k, flags, ids0, dist0, filt)
        again = run_fallback(ix, sc.Q.q, k, flags, ids0, dist0, filt) if twice else None
    assert counters == [run.count, int((flags == 0).sum()), int((flags == 1).sum()), run.count], f"{tag}: counters {counters}"
    assert_lists(tag, ids, dist, want_ids, want_dist, flagged)
    rest = np.setdiff1d(np.arange(nq), flagged)
    assert xr.same_bits(ids[rest], dist[rest], ids0[rest], dist0[rest]), f"{tag}: an unflagged query's slots changed"
    if twice:
        assert xr.same_bits(again[0], again[1], ids, dist) and again[2] == counters, f"{tag}: the second run left other bits"
    return fallback_branches(plan, nq, run.count, k, want_ids, want_dist, flagged, sc.allowed)


def test_the_plans_give_the_geometry_the_cases_name(gpu_lib):
    lib = gpu_lib.load()
    p = xr.fallback_plan(lib, gpu_lib.check, 1, 1, 1)
    assert (p.fast_splits, p.splits) == (1, 1)
    p = xr.fallback_plan(lib, gpu_lib.check, 513, 147, 10)
    assert (p.fast_splits, p.fast_rows, p.splits) == (2, 512, 1) and 513 - p.fast_rows == 1              # two fast splits, a 1-row tail
    p = xr.fallback_plan(lib, gpu_lib.check, 16385, 147, 100)
    assert (p.splits, p.rows) == (9, 2048) and 16385 - 8 * p.rows == 1 and p.fast_splits == 33 and p.round_q >= 147


@pytest.mark.parametrize("case", xr.fb_cases(), ids=xr.fb_id)
def test_fallback_on_written_flags(gpu_lib, monkeypatch, case):
    t0 = time.perf_counter()
    out = []
    for i, run in enumerate(xr.fb_runs(case)):
        tag = f"fallback {xr.fb_id(case)} mask={run.mask} k={run.k} flagged={run.count} dim={run.dim}"
        out.append(f"[{run.mask or 'all'} k{run.k} f{run.count} d{run.dim}: {fallback_once(gpu_lib, monkeypatch, tag, case.cls, case.n, case.ranks, run, twice=i == 0)}]")
    record(f"fallback {xr.fb_id(case):<34} {' '.join(out)}  {time.perf_counter() - t0:.1f} s")


@pytest.mark.parametrize("mask,ranks", [(None, None), ("stripes", "random")])
def test_fallback_gaussian_rows_against_the_oracle(gpu_lib, monkeypatch, mask, ranks):
    """the fp64 chain over every dimension (the dictated layouts use three components)"""
    n, dim, k, count = 16385, 128, 32, 9
    flags = xr.fb_flags(count)
    rows, qs = xr.gaussian(np.random.default_rng([71, n]), n, len(flags), dim, unit=True)
    tie, allowed = xr.rank_of(ranks, n), xr.allowed_rows(mask, n, k, 512)
    flagged = np.nonzero((flags < 0) | (flags >= 2))[0]
    want_ids, want_dist = xr.oracle_expected(knn_oracle, rows, qs, k, tie, allowed)
    ids0, dist0 = xr.sentinels(len(flags), k)
    with Index(gpu_lib, monkeypatch, dim) as ix:
        ix.add(rows)
        set_ranks(ix, tie)
        filt = None
        if allowed is not None:
            lab, G, sel, exclude = xr.labels_of(allowed, 1)
            ix.set_groups(lab, G)
            filt = (sel, exclude)
        ids, dist, counters = run_fallback(ix, qs, k, flags, ids0, dist0, filt)
    assert counters[0] == count
    assert_lists(f"fallback gaussian mask={mask} ranks={ranks}", ids, dist, want_ids, want_dist, flagged)
    record(f"fallback gaussian n={n} dim={dim} k={k} mask={mask} ranks={ranks}: the C oracle's lists")


def test_fallback_runs_several_bulk_rounds(gpu_lib, monkeypatch):
    """1,000 flagged queries whose per-split lists take more than the 64 MiB a bulk round has: two bulk rounds, the last one
    ragged; every query has a scale of its own, so a list filed under another round's slot shows"""
    t0 = time.perf_counter()
    lib, dim, nq, k = gpu_lib.load(), 64, 1000, 100
    n = 89 * 2048 + 1                                            # 90 bulk splits of 2,048 rows, the last one a single row
    plan = xr.fallback_plan(lib, gpu_lib.check, n, nq, k)
    assert plan.round_q < nq - xr.FAST_SLOTS and (plan.splits, plan.rows) == (90, 2048) and n - 89 * plan.rows == 1, plan
    rnds = xr.rounds(plan, nq, nq)
    assert len(rnds) >= 3 and rnds[-1][1] < plan.round_q and rnds[-1][1] % xr.QG == 0 and sum(r[1] for r in rnds) == nq, rnds
    sc = xr.scene("last_row", n, k, plan.rows, dim, nq, None, None, filler=True)
    flags = np.full(nq, 2, np.int32)
    want_ids, want_dist = xr.closed_form(sc.a, sc.b, sc.Q, k)
    ids0, dist0 = xr.sentinels(nq, k)
    with Index(gpu_lib, monkeypatch, dim) as ix:
        ix.add(sc.rows)
        ids, dist, counters = run_fallback(ix, sc.Q.q, k, flags, ids0, dist0)
    assert counters == [nq, 0, 0, nq]
    assert_lists("bulk rounds", ids, dist, want_ids, want_dist, range(nq))
    record(f"fallback bulk rounds n={n} nq={nq} k={k}: rounds={len(rnds)} (slots {[r[1] for r in rnds]}) round_q={plan.round_q} "
           f"{time.perf_counter() - t0:.1f} s")


def test_flag_collection_beyond_one_pass_of_the_workgroup(gpu_lib, monkeypatch):
    """2,100 queries: collect_flags_kernel takes three passes of 1,024 flags and carries the list position across them"""
    n, dim, nq, k = 513, 64, 2100, 10
    flags = np.array([(0, 1, 2, 9)[(j * 7 // 3) % 4] for j in range(nq)], np.int32)
    flagged = np.nonzero(flags >= 2)[0]
    assert (flagged < 1024).sum() > xr.FAST_SLOTS and (flagged >= 2048).any()
    plan = xr.fallback_plan(gpu_lib.load(), gpu_lib.check, n, nq, k)
    sc = xr.scene("plateau_split", n, k, plan.rows, dim, nq, "random", None, filler=True)
    want_ids, want_dist = xr.closed_form(sc.a, sc.b, sc.Q, k, sc.tie, None, flagged)
    ids0, dist0 = xr.sentinels(nq, k)
    with Index(gpu_lib, monkeypatch, dim) as ix:
        ix.add(sc.rows)
        set_ranks(ix, sc.tie)
        ids, dist, counters = run_fallback(ix, sc.Q.q, k, flags, ids0, dist0)
    assert counters == [len(flagged), int((flags == 0).sum()), int((flags == 1).sum()), len(flagged)]
    assert_lists("flag collection", ids, dist, want_ids, want_dist, flagged)
    rest = np.setdiff1d(np.arange(nq), flagged)
    assert xr.same_bits(ids[rest], dist[rest], ids0[rest], dist0[rest])
    record(f"fallback flag collection nq={nq}: {len(flagged)} flagged, rounds={len(xr.rounds(plan, nq, len(flagged)))}")


@pytest.mark.parametrize("k,count", [(10, 9), (32, 73)])
def test_fallback_merges_exactly_one_result_per_split(gpu_lib, monkeypatch, k, count):
    """as many splits as results, the last split a single row: every merge list gives its head and is never read again"""
    nq = 2 * count + 1
    per = 512 if count <= xr.FAST_SLOTS else 2048
    n = (k - 1) * per + 1
    plan = xr.fallback_plan(gpu_lib.load(), gpu_lib.check, n, nq, k)
    assert ((plan.fast_splits, plan.fast_rows) if count <= xr.FAST_SLOTS else (plan.splits, plan.rows)) == (k, per), plan
    tags = fallback_once(gpu_lib, monkeypatch, f"one per split k={k} flagged={count}", "one_per_split", n, None, xr.FbRun(None, k, count, 64, 0))
    assert "one-per-split" in tags, tags
    record(f"fallback one result per split n={n} k={k} flagged={count}: {tags}")


def test_fallback_entry_is_the_products_redo(gpu_lib, monkeypatch):
    """an all-tied index: the fp16 search cannot prove any query and redoes them all; the entry, fed those flags, gives its bits"""
    n, dim, nq, k = 16385, 64, 9, 10
    rows = np.zeros((n, dim), np.float32)
    rows[:, 3] = 1.0
    qs = np.zeros((nq, dim), np.float32)
    qs[:, 3] = 0.5 + np.arange(nq) / 32.0
    qs[:, 5] = 1.0                                               # (no row has this component)
    with Index(gpu_lib, monkeypatch, dim) as ix:
        ix.add(rows)
        p_ids, p_dist = ix.search(qs, k)
        stats = (ctypes.c_int64 * 3)()
        ix.L.check(ix.lib.vq_index_last_search_stats(ix.h, stats))
        assert list(stats) == [0, 0, nq], f"the search redid {list(stats)}"
        ids0, dist0 = xr.sentinels(nq, k)
        ids, dist, counters = run_fallback(ix, qs, k, np.full(nq, 2, np.int32), ids0, dist0)
    assert counters == [nq, 0, 0, nq] and xr.same_bits(ids, dist, p_ids, p_dist)
    assert (ids == np.arange(k)).all() and (dist == (np.float32(1.0) - qs[:, 3])[:, None]).all()
    record(f"fallback parity n={n} nq={nq} k={k}: vq_index_search(mode 2) redid {list(stats)}, the entry gives the same bits")


# ---------------------------------------------------------------- exact mode
def exact_once(gpu_lib, monkeypatch, tag, cls, n, run):
    sc = xr.scene(cls, n, run.k, xr.SEL_CHUNK, run.dim, run.nq, run.ranks, None, filler=False)
    want_ids, want_dist = xr.closed_form(sc.a, sc.b, sc.Q, run.k, sc.tie)
    with Index(gpu_lib, monkeypatch, run.dim) as ix:
        ix.add(sc.rows)
        set_ranks(ix, sc.tie)
        ids, dist = search_exact(ix, sc.Q.q, run.k)
    assert_lists(tag, ids, dist, want_ids, want_dist, range(run.nq))
    path = xr.exact_path(n, run.nq, run.dim)
    tags = [path]
    if path == "small":
        infos = [xr.model_select_small(xr.distances(sc.a, sc.b, sc.Q, j), sc.tie, run.k)[2] for j in range(run.nq)]
        tags += sorted({i["branch"] for i in infos}) + (["padding"] if any(i["padding"] and i["branch"] == "list" for i in infos) else [])
    if ((want_dist < 0).any(axis=1) & ((want_dist >= 0) & (want_ids >= 0)).any(axis=1)).any():
        tags.append("neg-to-pos")
    return "+".join(tags), sc


@pytest.mark.parametrize("case", xr.ex_cases(), ids=xr.ex_id)
def test_exact_mode_on_dictated_layouts(gpu_lib, monkeypatch, case):
    t0 = time.perf_counter()
    out = []
    for run in xr.ex_runs(case):
        tag = f"exact {xr.ex_id(case)} ranks={run.ranks} nq={run.nq} k={run.k} dim={run.dim}"
        out.append(f"[{run.ranks or 'rows'} q{run.nq} k{run.k} d{run.dim}: {exact_once(gpu_lib, monkeypatch, tag, case.cls, case.n, run)[0]}]")
    record(f"exact {xr.ex_id(case):<24} {' '.join(out)}  {time.perf_counter() - t0:.1f} s")


@pytest.mark.parametrize("n,k,about", xr.COLUMN)
@pytest.mark.parametrize("ranks", xr.RANKS)
def test_select_small_thread_columns(gpu_lib, monkeypatch, n, k, about, ranks):
    """k - 1 threads own every near row: the threshold admits (k - 1) x rows per thread + 1 keys, more than the list holds"""
    t0 = time.perf_counter()
    cls = "ascending" if n <= 1020 else "thread_column"
    branch, sc = exact_once(gpu_lib, monkeypatch, f"column n={n} k={k} {ranks}", cls, n, xr.ExRun(ranks, 8, k, 64))
    info = xr.model_select_small(xr.distances(sc.a, sc.b, sc.Q, 0), sc.tie, k)[2]
    if cls == "thread_column":
        assert info["c"] == (k - 1) * (n // 256) + 1
    assert (info["c"] > xr.SMALL_LIST) == (about in ("overflow", "padding")) and (info["padding"] > 0) == about.startswith("padding"), info
    record(f"exact column n={n} k={k} ranks={ranks}: query 0 collects c={info['c']} ({info['padding']} padding) -> {info['branch']}; "
           f"all queries {branch}  {time.perf_counter() - t0:.1f} s")


@pytest.mark.parametrize("n,nq,dim,k", [(1020, 8, 36, 10), (1020, 9, 100, 257), (8193, 1, 1540, 9), (8193, 8, 100, 256), (8193, 33, 4, 255),
                                        (32769, 2, 36, 1024)])
def test_exact_mode_gaussian_rows_at_ragged_dims(gpu_lib, monkeypatch, n, nq, dim, k):
    rows, qs = xr.gaussian(np.random.default_rng([73, n, dim]), n, nq, dim, unit=False)
    want_ids, want_dist = knn_oracle.topk(rows, qs, k)
    with Index(gpu_lib, monkeypatch, dim) as ix:
        ix.add(rows)
        ids, dist = search_exact(ix, qs, k)
    assert_lists(f"exact gaussian n={n} nq={nq} dim={dim} k={k}", ids, dist, want_ids, want_dist, range(nq))
    record(f"exact gaussian n={n} nq={nq} dim={dim} k={k}: {xr.exact_path(n, nq, dim)}, the C oracle's lists")


@pytest.mark.parametrize("dim", [4, 36, 100, 516])
def test_device_normalise_is_the_oracles(gpu_lib, monkeypatch, dim):
    for n in (1, 127, 128, 129, 300):
        rows = (np.random.default_rng([79, n, dim]).standard_normal((n, dim)) * 3.0).astype(np.float32)
        got = np.empty_like(rows)
        with Index(gpu_lib, monkeypatch, dim) as ix:
            ix.L.check(ix.lib.vq_index_add(ix.h, ix.L.fptr(rows), n, 1))
            ix.L.check(ix.lib.vq_index_export(ix.h, ix.L.fptr(got)))
        assert np.array_equal(got.view(np.uint32), knn_oracle.normalize_rows(rows).view(np.uint32)), f"dim {dim} n {n}"
    record(f"normalise dim={dim} n in (1, 127, 128, 129, 300): the C oracle's bits")
