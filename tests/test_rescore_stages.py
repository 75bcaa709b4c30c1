"""GPU: pass 2 of every fp16 search, the re-score kernels, stage-tested on key tables the test writes (tests/rescore_stage_ref.py).

Pass 1 meets the key contract (tests/test_scan_stages.py).  Here vq_index_debug_rescore runs the product's re-score launch on
tables that sit at the EDGE of that contract: every key moved by up to 0.97 E against the proof, and the row that decides the proof
hidden behind each truncating container in turn (a stream's second key, the (C+1)-th key, a share's floor, the collected list,
the first re-score pass).  Two assertions:
  - soundness, for every table of every class: where the flag is 0 or 1, ids and distances equal oracle.knn_oracle.topk on the
    same fp32 rows bit for bit (with id ranks: its (distance, rank) order).  Nothing is asserted about the lists of a flagged query;
  - completeness, per class: the flag the documented rule requires (0 proven, 1 proven after stream rescans, 2 flagged).
Each case asks vq_debug_scan_plan for the kernel and key layout it is about and fails on any other; writes the table, reads it
back through vq_index_debug_read_scan_keys and requires the same words; runs the entry twice and requires identical bits.  The
state histogram of each case is appended to the file $VQ_RESCORE_OUT names (profiles/rescore_stages/outcomes.txt is one run).

Rows go in with normalize = 0, so the fp32 data given IS the data stored.
"""
import collections
import ctypes
import os
import time

import numpy as np
import pytest

import rescore_stage_ref as rr
import scan_stage_ref as ref
from test_scan_stages import Index

pytestmark = pytest.mark.gpu


def record(line):
    print(line)
    out = os.environ.get("VQ_RESCORE_OUT")
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def histogram(hist):
    return "  ".join(f"{cls}:{''.join(str(s) for s in sorted(states))}" for cls, states in hist.items())


def set_reversed_ranks(ix, n):
    rank = np.arange(n, dtype=np.int32)[::-1].copy()                  # ids reversed: among exact ties the LATER row comes first
    ix.L.check(ix.lib.vq_index_set_id_ranks(ix.h, ix.L.i32ptr(rank), n))
    return rank


def rescore_twice(ix, case_id, qs, k, keys, layout):
    """the entry on the table, the table read back, the entry again: the same words, the same bits -> ids, dist, flags"""
    ids, dist, flags = rr.run_rescore(ix.lib, ix.L.check, ix.h, qs, k, keys)
    info, back = ix.keys()
    assert info == dict(q0=0, cur=len(qs), layout=layout, streams=keys.shape[1], masked=0), info
    assert np.array_equal(back, keys), f"{case_id}: the table read back differs from the table written"
    ids2, dist2, flags2 = rr.run_rescore(ix.lib, ix.L.check, ix.h, qs, k, keys)
    assert np.array_equal(flags, flags2) and set(flags.tolist()) <= {0, 1, 2}, (flags, flags2)
    proven = flags != 2
    assert np.array_equal(ids[proven], ids2[proven]) and np.array_equal(dist[proven].view(np.uint32), dist2[proven].view(np.uint32)), \
        f"{case_id}: the second run left other bits"
    return ids, dist, flags


def check_sound(case_id, cls, j, flag, ids, dist, want_ids, want_dist):
    if flag == 2:
        return
    assert np.array_equal(ids, want_ids) and np.array_equal(dist.view(np.uint32), want_dist.view(np.uint32)), \
        f"{case_id} query {j} ({cls}): flag {flag}, yet the list differs from the oracle's\n got  {ids}\n want {want_ids}"


@pytest.mark.parametrize("case", rr.CASES, ids=lambda c: c.id)
def test_rescore_on_written_keys(gpu_lib, monkeypatch, case):
    t0 = time.perf_counter()
    hist = collections.OrderedDict()
    for sc in case.scenes(gpu_lib.load()):
        with Index(gpu_lib, monkeypatch, case.dim, case.env) as ix:
            plan = ix.plan(case.n, case.nq, case.k)
            got = (int(plan.rescore), int(plan.layout), int(plan.streams), int(plan.chunks))
            assert got == (case.rescore, case.layout, case.streams, 1), f"{case.id}: the plan is {got}"
            ix.add(sc.rows)
            rank = set_reversed_ranks(ix, case.n) if case.reversed_ranks else None
            ids, dist, flags = rescore_twice(ix, case.id, sc.qs, case.k, sc.keys, case.layout)
        want_ids, want_dist = rr.expected(sc.rows, sc.clean_qs, case.k, rank)
        for j, sp in enumerate(sc.specs):
            hist.setdefault(sp.cls, set()).add(int(flags[j]))
            check_sound(case.id, sp.cls, j, flags[j], ids[j], dist[j], want_ids[j], want_dist[j])
            assert sp.required is None or flags[j] == sp.required, \
                f"{case.id} query {j} ({sp.cls}): flag {flags[j]}, the class requires {sp.required} (table at {sc.worst:.3f} E)"
            if flags[j] != 2:
                assert set(sp.must_hold) <= set(ids[j].tolist())
    took = time.perf_counter() - t0
    record(f"{case.id:<58} {histogram(hist)}" + (f"  [{took:.1f} s, table and oracle included]" if case.streams > 8000 else ""))


@pytest.mark.parametrize("rescore,layout,dim,n,nq,k", rr.SHORT)
def test_short_tables_are_flagged(gpu_lib, monkeypatch, rescore, layout, dim, n, nq, k):
    """fewer rows than k, or fewer keys than k: nothing can be proven"""
    rng = np.random.default_rng([43, rescore, n])
    with Index(gpu_lib, monkeypatch, dim) as ix:
        plan = ix.plan(n, nq, k)
        assert (plan.rescore, plan.layout, plan.chunks) == (rescore, layout, 1)
        geo = rr.Geo(ix.lib, layout, int(plan.streams), n)
        sc = rr.gaussian_scene(rng, geo, dim, nq, "random")
        ix.add(sc.rows)
        _, _, flags = rescore_twice(ix, f"short {rr.PARAMS[rescore]} n={n} k={k}", sc.qs, k, sc.keys, layout)
    assert (flags == 2).all(), flags
    record(f"short {rr.PARAMS[rescore].name} L{layout} d{dim} n={n} q{nq} k{k}: all 2")


# the real class: the keys a scan left, fed back in, must give what the product gave.  (rescore, dim, n, nq, k, env)
REAL = [(rr.SMALL32, 256, 513 * 128 - 37, 1, 10, {}), (rr.SMALL32, 512, 65 * 128 - 37, 3, 20, {}), (rr.SMALL64, 256, 129 * 128 - 37, 3, 40, {}),
        (rr.LARGE1, 768, 300 * 128 - 37, 3, 21, {}), (rr.XLARGE1, 256, 300 * 128 - 37, 1, 100, {}), (rr.BATCH8, 192, 376 * 128 - 987, 9, 10, {}),
        (rr.BATCH8, 128, 384 * 128 - 2011, 9, 20, {}), (rr.LARGE4, 192, 504 * 128 - 987, 5, 64, {}), (rr.XLARGE4, 128, 512 * 128 - 2011, 5, 100, {}),
        (rr.LARGE4, 256, 300 * 128 - 37, 5, 64, {"VQ_AMD_RESCORE_QPW4": 1})]


@pytest.mark.parametrize("cls", ["gaussian", "midpoints"])
@pytest.mark.parametrize("rescore,dim,n,nq,k,env", REAL)
def test_rescore_on_the_scans_own_keys_is_the_product(gpu_lib, monkeypatch, cls, rescore, dim, n, nq, k, env):
    rows, qs = ref.input_class(cls, np.random.default_rng([47, rescore, dim, n]), n, nq, dim)
    with Index(gpu_lib, monkeypatch, dim, env) as ix:
        plan = ix.plan(n, nq, k)
        assert (plan.rescore, plan.chunks) == (rescore, 1)
        ix.add(rows)
        p_ids, p_dist = ix.search(qs, k)
        stats = (ctypes.c_int64 * 3)()
        ix.L.check(ix.lib.vq_index_last_search_stats(ix.h, stats))
        info, keys = ix.keys()
        case_id = f"real {cls} {rr.PARAMS[rescore]} d{dim} n={n} q{nq} k{k}"
        ids, dist, flags = rescore_twice(ix, case_id, qs, k, keys, int(plan.layout))
    counts = [int((flags == s).sum()) for s in (0, 1, 2)]
    assert counts == list(stats), f"{case_id}: flags {counts}, the search counted {list(stats)}"
    want_ids, want_dist = rr.expected(rows, qs, k)
    for j in range(nq):
        check_sound(case_id, "real", j, flags[j], ids[j], dist[j], p_ids[j], p_dist[j])
        check_sound(case_id, "real", j, 0, p_ids[j], p_dist[j], want_ids[j], want_dist[j])      # (and the product's answer is the oracle's)
    record(f"{case_id:<58} states {counts}")
