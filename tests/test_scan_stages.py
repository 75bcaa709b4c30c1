"""GPU: pass 1 of every fp16 search, stage-tested against fp64 scores (tests/scan_stage_ref.py).

Each case builds one small index, asks vq_debug_scan_plan which kernel the search will run (and fails if it is not the one the
case is about), searches once in mode 2, reads the scan's keys (or group maxima) back through vq_index_debug_read_scan_keys /
_group_best and hands them to the checker: every (query, stream) pair — two distinct rows of the stream, each key within E of
the exact score of the row it names, key1 >= key2, and every row the stream did not emit at or below key2 + E — or every
(query, group) pair.  Then it searches again and asserts the same bits.  The only tolerance is E = eps_unit(dim) max|row| |q|,
restated in scan_stage_ref.py from the derivation in csrc/knn_scan_f16.h.  Each check prints max(error / E);
profiles/scan_stages/ratios.txt is the table of one run ($VQ_SCAN_RATIOS_OUT names the file the lines are appended to).

Rows go in with normalize = 0, so the fp32 data given IS the data stored, and the reference needs nothing back from the device.
"""
import ctypes
import os

import numpy as np
import pytest

import scan_stage_ref as ref

pytestmark = pytest.mark.gpu

SWITCHES = ("VQ_AMD_SCAN", "VQ_AMD_SCAN_SMALL", "VQ_AMD_SCAN_RB", "VQ_AMD_RESCORE_QPW4", "VQ_AMD_RESCORE_SMALL64")
MODE_FP16 = 2
K = 5
I_MFMA_SCAN = 4                     # vq_index_profile_class_name(4) == "scan_f16_mfma_top2"
TILE128, STREAM, FOLD = 1, 3, 5


def record(case, stage, ratio):
    line = f"{case:<58} {stage:<10} {ratio:.4g}"
    print(line)
    out = os.environ.get("VQ_SCAN_RATIOS_OUT")
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


class Index:
    """A vq_index handle over the C ABI; the switches in `env` are in the environment when it is created (they are read then)."""

    def __init__(self, L, monkeypatch, dim, env=None):
        self.L, self.lib = L, L.load()
        for name in SWITCHES:
            monkeypatch.delenv(name, raising=False)
        for name, v in (env or {}).items():
            monkeypatch.setenv(name, str(v))
        self.dim = dim
        self.h = ctypes.c_void_p()
        L.check(self.lib.vq_index_create(dim, ctypes.byref(self.h)))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.lib.vq_index_destroy(self.h)

    def plan(self, n, nq, k=K):
        p = self.L.ScanPlanC()
        self.L.check(self.lib.vq_debug_scan_plan(self.dim, n, nq, k, 0, ctypes.byref(p)))
        return p

    def add(self, rows):
        rows = np.ascontiguousarray(rows, np.float32)
        self.L.check(self.lib.vq_index_add(self.h, self.L.fptr(rows), len(rows), 0))

    def set_groups(self, labels, G):
        lab = np.ascontiguousarray(labels, np.int32)
        self.L.check(self.lib.vq_index_set_groups(self.h, self.L.i32ptr(lab), len(lab), G))

    def search(self, qs, k=K):
        qs = np.ascontiguousarray(qs, np.float32)
        ids, dist = np.empty((len(qs), k), np.int32), np.empty((len(qs), k), np.float32)
        self.L.check(self.lib.vq_index_search(self.h, self.L.fptr(qs), len(qs), k, MODE_FP16, self.L.i32ptr(ids), self.L.fptr(dist)))
        return ids, dist

    def search_filtered(self, qs, sel, exclude, k=K):
        qs, sel = np.ascontiguousarray(qs, np.float32), np.ascontiguousarray(sel, np.int32)
        ids, dist = np.empty((len(qs), k), np.int32), np.empty((len(qs), k), np.float32)
        self.L.check(self.lib.vq_index_search_filtered(self.h, self.L.fptr(qs), len(qs), k, MODE_FP16, self.L.i32ptr(sel), len(sel), exclude,
                                                       self.L.i32ptr(ids), self.L.fptr(dist)))
        return ids, dist

    def search_grouped(self, qs, sel=None, exclude=0, k=K):
        qs = np.ascontiguousarray(qs, np.float32)
        g, r, d = (np.empty((len(qs), k), t) for t in (np.int32, np.int32, np.float32))
        if sel is None:
            self.L.check(self.lib.vq_index_search_grouped(self.h, self.L.fptr(qs), len(qs), k, MODE_FP16, self.L.i32ptr(g), self.L.i32ptr(r),
                                                          self.L.fptr(d)))
        else:
            sel = np.ascontiguousarray(sel, np.int32)
            self.L.check(self.lib.vq_index_search_grouped_filtered(self.h, self.L.fptr(qs), len(qs), k, MODE_FP16, self.L.i32ptr(sel), len(sel),
                                                                   exclude, self.L.i32ptr(g), self.L.i32ptr(r), self.L.fptr(d)))
        return g, r, d

    def scan_launches(self, run):
        """run() between the profile brackets -> launches of the scan class"""
        ms, launches = (ctypes.c_float * self.L.IDX_NCLASS)(), (ctypes.c_int * self.L.IDX_NCLASS)()
        assert self.lib.vq_index_profile_class_name(I_MFMA_SCAN).decode() == "scan_f16_mfma_top2"
        self.L.check(self.lib.vq_index_profile_begin(self.h))
        run()
        self.L.check(self.lib.vq_index_profile_end(self.h, ms, launches))
        return launches[I_MFMA_SCAN]

    def keys(self):
        return ref.read_scan_keys(self.lib, self.L.check, self.h)

    def group_best(self):
        return ref.read_group_best(self.lib, self.L.check, self.h)


def check_plain(ix, case, rows, qs, plan, search=None, allowed_rows=None, masked=0):
    """One search, the keys against the checker, a second search, the same bits.  -> the keys"""
    search = search or (lambda: ix.search(qs))
    search()
    info, keys = ix.keys()
    assert info == dict(q0=0, cur=len(qs), layout=int(plan.layout), streams=int(plan.streams), masked=masked), info
    table = ref.row_table(ix.lib, info["layout"], info["streams"])
    record(case, "keys", ref.check_keys(keys, rows, qs, table, allowed_rows))
    search()
    info2, again = ix.keys()
    assert info2 == info and np.array_equal(keys, again), f"{case}: the second search left other key bits"
    return keys


def plain_case(gpu_lib, monkeypatch, case, cls, dim, n, nq, env, want, seed=0):
    """want: the plan's scalars the case is about (scan, and what else decides the kernel instance or its blocking)"""
    with Index(gpu_lib, monkeypatch, dim, env) as ix:
        plan = ix.plan(n, nq)
        got = {name: int(getattr(plan, name)) for name in want}
        assert got == want and plan.chunks == 1, f"{case}: the plan is {got}, chunks {plan.chunks}"
        rows, qs = ref.input_class(cls, np.random.default_rng([17, dim, n, nq, seed]), n, nq, dim)
        ix.add(rows)
        check_plain(ix, f"{case} {cls} dim={dim} n={n} nq={nq}", rows, qs, plan)


# ---------------------------------------------------------------- 128 x 1024 tile (scan_f16_top2_kernel): dim % 128 != 0
N_TILE = 2 * 1024 + 129            # three ranges; the last: one full stream pair, a stream with one valid row, streams with none
TILE_CASES = [("gaussian", 192, N_TILE, 130), ("gaussian", 320, N_TILE, 130), ("gaussian", 192, 1, 130), ("gaussian", 192, 1024, 130)] + \
             [(cls, 64, N_TILE, 130) for cls in ref.INPUT_CLASSES]


@pytest.mark.parametrize("cls,dim,n,nq", TILE_CASES)
def test_tile128_scan(gpu_lib, monkeypatch, cls, dim, n, nq):
    plain_case(gpu_lib, monkeypatch, "tile128", cls, dim, n, nq, None, dict(scan=TILE128, layout=1, q_tiles=2, ranges=(n + 1023) // 1024))


# ---------------------------------------------------------------- 256 x 2048 fold (scan5_f16_top2_kernel), the default
N_FOLD = 2 * 2048 + 65
FOLD_CASES = [
    # default blocking (rb = 2): five ranges = a second range group holding one ragged range; nine query tiles = a second block of them
    ("gaussian", 512, 4 * 2048 + 2048 - 63, 2100, {}, dict(scan=FOLD, rb=2, ranges=5, q_tiles=9)),
    ("gaussian", 768, N_FOLD, 257, {}, dict(scan=FOLD, rb=2, ranges=3, q_tiles=2)),
    ("gaussian", 1024, N_FOLD, 257, {}, dict(scan=FOLD, rb=2, ranges=3, q_tiles=2)),
    ("gaussian", 128, 33 * 2048 - 1000, 300, {"VQ_AMD_SCAN_RB": 5}, dict(scan=FOLD, rb=5, ranges=33, q_tiles=2)),
    ("gaussian", 128, 2 * 2048 + 1, 33 * 256 - 5, {"VQ_AMD_SCAN_RB": 0}, dict(scan=FOLD, rb=0, ranges=3, q_tiles=33)),
    ("gaussian", 512, 1, 1, {"VQ_AMD_SCAN_SMALL": 0}, dict(scan=FOLD, rb=2, ranges=1, q_tiles=1)),
    ("gaussian", 512, 2048, 1, {"VQ_AMD_SCAN_SMALL": 0}, dict(scan=FOLD, rb=2, ranges=1, q_tiles=1)),
] + [(cls, 128, N_FOLD, 257, {}, dict(scan=FOLD, rb=2, ranges=3, q_tiles=2)) for cls in ref.INPUT_CLASSES]


@pytest.mark.parametrize("cls,dim,n,nq,env,want", FOLD_CASES)
def test_fold_scan(gpu_lib, monkeypatch, cls, dim, n, nq, env, want):
    plain_case(gpu_lib, monkeypatch, "fold rb=%d" % want["rb"], cls, dim, n, nq, env, dict(want, layout=2))


# ---------------------------------------------------------------- streaming (scan3_f16_top2_kernel)
STREAM_NQ = (1, 3, 4, 5, 16, 17, 33, 96)      # fused conversion; one group; two groups per pass and more than one pass (768: one group per pass)


def stream_want(dim, nq):
    nqg = 2 if nq > 16 and dim <= 512 else 1
    return dict(scan=STREAM, layout=3, fused_q=int(nq <= 4), nqg=nqg, scan_grid_y=-(-nq // (16 * nqg)))


@pytest.mark.parametrize("dim", [256, 512, 768])
@pytest.mark.parametrize("n", [1, 127, 128, 129, 6 * 128 + 1])      # the last: seven streams = a last workgroup with three live waves, a one-row stream
def test_stream_scan(gpu_lib, monkeypatch, dim, n):
    rng = np.random.default_rng([19, dim, n])
    rows, qs = ref.input_class("gaussian", rng, n, max(STREAM_NQ), dim)
    with Index(gpu_lib, monkeypatch, dim) as ix:
        ix.add(rows)
        got = {}
        for nq in STREAM_NQ:
            plan, want = ix.plan(n, nq), stream_want(dim, nq)
            assert {name: int(getattr(plan, name)) for name in want} == want and plan.chunks == 1, (nq, want)
            got[nq] = check_plain(ix, f"stream gaussian dim={dim} n={n} nq={nq}", rows, qs[:nq], plan)
        # the fused form rounds the queries as the conversion kernel does: the same keys, bit for bit
        assert np.array_equal(got[3], got[5][:3]), "fused 3-query keys differ from the same queries' keys in a 5-query call"
        assert np.array_equal(got[4], got[16][:4])


@pytest.mark.parametrize("cls", ref.INPUT_CLASSES)
@pytest.mark.parametrize("nq", [3, 33])
def test_stream_scan_input_classes(gpu_lib, monkeypatch, cls, nq):
    plain_case(gpu_lib, monkeypatch, "stream", cls, 512, 6 * 128 + 1, nq, None, stream_want(512, nq))


# ---------------------------------------------------------------- masked streaming scan (filtered search, fp16 path)
def masked_labels():
    """Five streams in one index: 0 uniform (label 0); 1 uniform (label 1); 2 mixed, its labels changing off a lane's 4-row boundary
    (local 10), on it (16, 36) and off it again (63); 3 label 6 but for ONE row of label 5; 4 ragged (37 rows, labels 7 | 8)."""
    lab = [0] * 128 + [1] * 128 + [2] * 10 + [3] * 6 + [4] * 20 + [3] * 27 + [2] * 65 + [6] * 77 + [5] + [6] * 50 + [7] * 20 + [8] * 17
    return np.array(lab, np.int64), 9


MASK_SEL = [0, 2, 5, 7]            # `within`: stream 1 is not read, stream 3 holds one allowed row; `exclude`: stream 0 is not read, stream 3 holds 127


@pytest.mark.parametrize("cls,dim,nq,exclude", [("gaussian", 256, nq, ex) for nq in (1, 17) for ex in (0, 1)] +
                         [("gaussian", 768, 17, 0)] + [(cls, 512, 17, ex) for cls in ref.INPUT_CLASSES for ex in (0, 1)])
def test_masked_stream_scan(gpu_lib, monkeypatch, cls, dim, nq, exclude):
    labels, G = masked_labels()
    n = len(labels)
    rows, qs = ref.input_class(cls, np.random.default_rng([23, dim, nq, exclude]), n, nq, dim)
    allowed_groups = np.isin(np.arange(G), MASK_SEL) != bool(exclude)
    allowed_rows = allowed_groups[labels]
    sl = ref.stream_labels(labels)
    assert list(sl) == [0, 1, -1, -1, -1] and allowed_rows[3 * 128:4 * 128].sum() == (127 if exclude else 1)
    with Index(gpu_lib, monkeypatch, dim) as ix:
        ix.add(rows)
        ix.set_groups(labels, G)
        plan = ix.plan(n, nq)                     # (the masked path has no plan of its own: the streaming scan's stream count and layout)
        assert (plan.scan, plan.layout, plan.streams) == (STREAM, 3, 5)
        case = f"masked {'exclude' if exclude else 'within'} {cls} dim={dim} n={n} nq={nq}"
        keys = check_plain(ix, case, rows, qs, plan, lambda: ix.search_filtered(qs, MASK_SEL, exclude), allowed_rows, masked=1)
        # the path: one scan launch between the profile brackets, and the stream the filter rules out was not read (bare sentinels)
        assert ix.scan_launches(lambda: ix.search_filtered(qs, MASK_SEL, exclude)) == 1
        skipped = 0 if exclude else 1
        assert (keys[:, skipped, :] == np.float32(-3.0e38).view(np.uint32)).all()


# ---------------------------------------------------------------- group-max scan (scan3_group_max_kernel), plain and masked
def group_labels():
    """1,000 rows: group 0 spans three whole streams and 40 rows more; groups of 1 and 3 rows; labels alternating 3, 4 (runs of one);
    a run ending inside a lane's four rows (local 73 of stream 3) and the next on the boundary (80); label 7 in two separate streams
    (3 into 4, and 6), its first run crossing a stream boundary; a ragged last stream."""
    lab = [0] * 424 + [1] + [2] * 3 + [3, 4] * 12 + [5] * 6 + [6] * 6 + [7] * 50 + [8] * 300 + [7] * 30 + [9] * 156
    return np.array(lab, np.int64), 10


def group_inputs(cls, rng, n, nq, dim):
    """The class's rows and queries; `gaussian` here is a cluster (every pairwise score positive), and query 0 is a stored row
    negated: every score negative, the lower half of the order-preserving key."""
    if cls != "gaussian":
        return ref.input_class(cls, rng, n, nq, dim)
    c = ref.gaussian_unit(rng, 1, dim)
    rows = ref.unit(0.6 * c + ref.gaussian_unit(rng, n, dim))
    qs = ref.unit(0.3 * c + ref.gaussian_unit(rng, nq, dim))
    qs[0] = -rows[3]
    assert (ref.exact_scores(rows, qs[:1]) < 0).all()
    return rows, qs


def check_groups(ix, case, rows, qs, labels, G, search, allowed_groups=None):
    search()
    info, best = ix.group_best()
    assert info == dict(q0=0, cur=len(qs), n_groups=G), info
    record(case, "group_max", ref.check_group_best(best, rows, qs, labels, G, allowed_groups))
    search()
    info2, again = ix.group_best()
    assert info2 == info and np.array_equal(best.view(np.uint32), again.view(np.uint32)), f"{case}: the second search left other bits"


GROUP_SEL = [0, 3, 5, 7]
GROUP_CASES = [("gaussian", dim, nq, flt) for dim in (256, 512) for nq in (1, 16, 17) for flt in (None, 0, 1)] + \
              [("gaussian", 768, 17, None)] + [(cls, 256, 16, flt) for cls in ref.INPUT_CLASSES[1:] for flt in (None, 0)]


@pytest.mark.parametrize("cls,dim,nq,flt", GROUP_CASES)
def test_group_max_scan(gpu_lib, monkeypatch, cls, dim, nq, flt):
    labels, G = group_labels()
    n = len(labels)
    rows, qs = group_inputs(cls, np.random.default_rng([29, dim, nq]), n, nq, dim)
    allowed = None if flt is None else np.isin(np.arange(G), GROUP_SEL) != bool(flt)
    with Index(gpu_lib, monkeypatch, dim) as ix:
        ix.add(rows)
        ix.set_groups(labels, G)
        how = "plain" if flt is None else "exclude" if flt else "within"
        search = (lambda: ix.search_grouped(qs)) if flt is None else (lambda: ix.search_grouped(qs, GROUP_SEL, flt))
        check_groups(ix, f"group_max {how} {cls} dim={dim} n={n} nq={nq}", rows, qs, labels, G, search, allowed)
        assert ix.scan_launches(search) == 1          # the fp16 path: one group-max scan per call


def test_group_max_scan_one_group(gpu_lib, monkeypatch):
    n, dim, nq = 1000, 256, 17
    rows, qs = group_inputs("gaussian", np.random.default_rng(31), n, nq, dim)
    labels = np.zeros(n, np.int64)
    info = (ctypes.c_int64 * 3)()
    with Index(gpu_lib, monkeypatch, dim) as ix:
        ix.add(rows)
        ix.set_groups(labels, 1)
        assert ix.lib.vq_index_debug_read_group_best(ix.h, info, None, 0) == -3          # VQ_ERR_STATE: no group-max scan yet
        check_groups(ix, f"group_max plain G=1 dim={dim} n={n} nq={nq}", rows, qs, labels, 1, lambda: ix.search_grouped(qs, k=1))


# ---------------------------------------------------------------- state: the keys follow the CURRENT rows
@pytest.mark.parametrize("dim,n,nq,env,scan", [(512, 6 * 128 + 1, 3, None, STREAM), (128, N_FOLD, 257, None, FOLD), (192, N_TILE, 130, None, TILE128)])
def test_keys_follow_updated_and_removed_rows(gpu_lib, monkeypatch, dim, n, nq, env, scan):
    L = gpu_lib
    rng = np.random.default_rng([37, dim])
    rows, qs = ref.input_class("gaussian", rng, n, nq, dim)
    info = (ctypes.c_int64 * 5)()
    with Index(L, monkeypatch, dim, env) as ix:
        assert ix.lib.vq_index_debug_read_scan_keys(ix.h, info, None, 0) == -3           # VQ_ERR_STATE: nothing scanned yet
        ix.add(rows)
        assert ix.lib.vq_index_debug_read_scan_keys(ix.h, info, None, 0) == -3
        ix.search(qs)
        ix.keys()
        # a few rows, one in the last (ragged) stream, become near copies of query 0: a stale fp16 copy would keep them out of their streams' keys
        upd = np.array([5, 700 % n, n - 1], np.int64)
        new = ref.unit(qs[0][None, :] + 0.05 * ref.gaussian_unit(rng, len(upd), dim))
        L.check(ix.lib.vq_index_update_rows(ix.h, L.fptr(new), L.i64ptr(upd), len(upd), 0))
        assert ix.lib.vq_index_debug_read_scan_keys(ix.h, info, None, 0) == -3           # the rows changed: the old keys are not handed out
        rows = rows.copy()
        rows[upd] = new
        rm = np.array([5, 17], np.int64)             # one of the updated rows goes, every row behind it moves down
        L.check(ix.lib.vq_index_remove_rows(ix.h, L.i64ptr(rm), len(rm)))
        assert ix.lib.vq_index_debug_read_scan_keys(ix.h, info, None, 0) == -3
        rows = np.delete(rows, rm, axis=0)
        plan = ix.plan(len(rows), nq)
        assert plan.scan == scan
        check_plain(ix, f"state update+remove scan={scan} dim={dim} n={len(rows)} nq={nq}", rows, qs, plan)
