"""CPU (`-m "not gpu"`): the key tables the re-score stage tests write (tests/rescore_stage_ref.py), on their own.

  - every class's tables pass scan_stage_ref.check_keys (Scene raises otherwise), for each container parameter set:
    (8, 6, 32), (4, 10, 80), (4, 12, 128), (1, 10, 80), (1, 12, 128) and the two one-query kernels;
  - model_state, the documented proof rule restated in numpy, gives every table's required state, and a sound answer wherever it
    proves one: the classes' expectations follow from the rule, not from what a kernel happened to do;
  - non-vacuity: each defect planted in the model is caught by at least one class, through the soundness rule (flag 0 or 1 with
    a list that differs from the oracle's) or through a required state;
  - the shapes of the GPU cases give the re-score kernel and key layout they name (vq_debug_scan_plan is host-only), and the
    debug entry is exported.
"""
import ctypes

import numpy as np
import pytest

import rescore_stage_ref as rr
from oracle import knn_oracle


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g
    g.build()
    from video_quierer_amd import _lib
    _lib.load()
    return _lib


_prepared = {}


def prepared(case, lib):
    """every query of the case: (spec, keys, oracle distances, E, |q|^2, the expected list, geo); built once"""
    if case.id not in _prepared:
        rank = np.arange(case.n, dtype=np.int32)[::-1].copy() if case.reversed_ranks else None
        out = []
        for sc in case.scenes(lib):
            for j, sp in enumerate(sc.specs):
                d32 = knn_oracle.distances(sc.rows, sc.clean_qs[j])
                q2 = float((sc.qs[j].astype(np.float64) ** 2).sum())
                want = rr.expected(sc.rows, sc.clean_qs[j:j + 1], case.k, rank)[0][0]
                out.append((sp, sc.keys[j], d32, sc.E[j], q2, want, sc.geo, rank))
        _prepared[case.id] = out
    return _prepared[case.id]


def verdicts(case, lib, defect=None, planted_only=False):
    """-> [(class, required, state, sound, info)] of every query of the case under the model"""
    out = []
    for sp, keys, d32, E, q2, want, geo, rank in prepared(case, lib):
        if planted_only and sp.required is None:
            continue
        state, ids, info = rr.model_state(keys, d32, E, case.P, case.k, geo, q2, defect, rank)
        sound = state == 2 or np.array_equal(ids, want)
        if state != 2 and sound:
            assert set(sp.must_hold) <= set(ids.tolist()), f"{case.id} {sp.cls}: the answer lacks a row the class is about"
        out.append((sp.cls, sp.required, state, sound, info))
    return out


CPU_CASES = [c for c in rr.CASES if c.cpu]
_cache = {}


def clean(case, lib):
    if case.id not in _cache:
        _cache[case.id] = verdicts(case, lib)
    return _cache[case.id]


def test_every_parameter_set_is_covered():
    assert {c.P.name for c in CPU_CASES} == {p.name for p in rr.PARAMS.values()}
    assert {(p.QPW, p.KEEP, p.C) for p in rr.PARAMS.values() if p.kind == "batch"} == {(8, 6, 32), (4, 10, 80), (4, 12, 128), (1, 10, 80), (1, 12, 128)}
    for name in rr.CLASSES:
        assert any(name in c.classes for c in CPU_CASES), name


@pytest.mark.parametrize("case", CPU_CASES, ids=lambda c: c.id)
def test_tables_are_inside_the_contract_and_the_rule_gives_the_required_state(L, case):
    for cls, required, state, sound, info in clean(case, L.load()):
        assert sound, f"{cls}: the rule itself proves a wrong list ({info})"
        assert required is None or state == required, f"{cls}: the rule gives state {state}, the class requires {required} ({info})"
        if cls.startswith("hidden-deep"):
            assert info["pass2"], "hidden-deep: the second re-score pass did not run"


# the classes that must catch each defect (at least one of them, on some parameter set that has the container)
CAUGHT_BY = {
    "eps_095": ("hidden(1)",), "eps_105": ("no-rescan",), "no_rest_bound": ("rest-bound",), "no_share_floor": ("share-floor",),
    "no_second_key": ("hidden(1)", "hidden(4)"), "second_key_first_pass_only": ("hidden-deep(1)",), "fifth_rescan_dropped": ("hidden(5)",),
    "rescanned_candidates_stay": ("hidden(4)",), "no_norm_gate": ("norm-gate(0.24)", "norm-gate(4.1)", "norm-gate(nan)"),
}
DEFECT_CASES = [c for c in CPU_CASES if not c.reversed_ranks]


@pytest.mark.parametrize("defect", rr.DEFECTS)
def test_each_planted_defect_is_caught(L, defect):
    assert set(CAUGHT_BY) == set(rr.DEFECTS)
    caught = set()
    for case in DEFECT_CASES:
        if defect == "no_share_floor" and case.P.kind != "batch":
            continue
        if defect == "second_key_first_pass_only" and case.P.kind != "small":
            continue
        base = clean(case, L.load())
        for (cls, required, state, sound, _), (_, _, state0, sound0, _) in zip(verdicts(case, L.load(), defect), base):
            assert sound0 and (required is None or state0 == required)
            if not sound or (required is not None and state != required):
                caught.add((case.P.name, cls, "unsound" if not sound else f"state {state} for {required}"))
    print(defect, sorted(caught))
    hit = {cls for _, cls, _ in caught}
    assert hit & set(CAUGHT_BY[defect]), f"{defect}: caught only by {sorted(hit)}"
    # every kernel that has the container catches it
    kernels = {c.P.name for c in DEFECT_CASES if not (defect == "no_share_floor" and c.P.kind != "batch")
               and not (defect == "second_key_first_pass_only" and c.P.kind != "small")}
    assert {name for name, _, _ in caught} == kernels, f"{defect}: not caught on {sorted(kernels - {n for n, _, _ in caught})}"


def test_keys_are_packed_to_the_nearest_word_and_sorted():
    rng = np.random.default_rng(3)
    v = rng.uniform(-1, 1, 1000).astype(np.float32)
    loc = rng.integers(0, 128, 1000)
    w = rr.pack_index(v, loc)
    assert ((w & 127) == loc).all()
    assert (np.abs(w.view(np.float32).astype(np.float64) - v) <= 64 * np.spacing(np.abs(v)).astype(np.float64)).all()


@pytest.mark.parametrize("case", rr.CASES, ids=lambda c: c.id)
def test_the_case_shapes_reach_the_kernel_they_name(L, case, monkeypatch):
    for name in ("VQ_AMD_SCAN", "VQ_AMD_SCAN_SMALL", "VQ_AMD_SCAN_RB", "VQ_AMD_RESCORE_QPW4", "VQ_AMD_RESCORE_SMALL64"):
        monkeypatch.delenv(name, raising=False)
    for name, v in case.env.items():
        monkeypatch.setenv(name, str(v))
    p = L.ScanPlanC()
    L.check(L.load().vq_debug_scan_plan(case.dim, case.n, case.nq, case.k, 0, ctypes.byref(p)))
    assert (p.rescore, p.layout, p.streams, p.chunks) == (case.rescore, case.layout, case.streams, 1)
    assert p.rescore_files_flags == int(case.P.kind == "small" and case.nq == 1)


@pytest.mark.parametrize("rescore,layout,dim,n,nq,k", rr.SHORT)
def test_the_short_shapes_reach_the_kernel_they_name(L, rescore, layout, dim, n, nq, k):
    p = L.ScanPlanC()
    L.check(L.load().vq_debug_scan_plan(dim, n, nq, k, 0, ctypes.byref(p)))
    assert (p.rescore, p.layout) == (rescore, layout) and (n < k or 2 * p.streams < k)


def test_the_debug_entry_is_exported(L):
    assert "vq_index_debug_rescore" in L.SIGNATURES and hasattr(L.load(), "vq_index_debug_rescore")
