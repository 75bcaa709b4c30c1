"""Chapter segmentation on the device (vq_index_segment_groups / HNSWIndex.segment_groups / SimpleVideoIndex.video_chapters)
against the numpy restatement of the definition (tests/segment_ref.py) over vq_index_export's rows: counts, first / last / show
rows and lengths as integers, spreads and mean spreads as fp32 bits.

One index per dimension of 594 rows in ten groups whose lengths sit on both sides of the pair kernel's edges (a thread's rows
change at 32, the tile at 64) and span several tiles (300); rows of the groups are interleaved, positions are not monotone in
row order and repeat, so that the tie (the row number, or the id rank) decides."""
import ctypes
from ctypes import POINTER, byref, c_float, c_int, c_int32, c_int64, c_void_p

import numpy as np
import pytest

import segment_ref
from test_segment_cpu import CANCEL_DIM, CANCEL_ROWS, cancelling_group, one_hot_blocks

GPU = pytest.mark.gpu
LENGTHS = [1, 2, 3, 31, 32, 33, 63, 64, 65, 300]
KS, PENALTIES, MAX_LENS = (1, 2, 5, 64), (0.0, 0.05, 1e9), (0, 1, 7)
COST_ENV, LDS_ENV = "VQ_AMD_SEG_COST_BYTES", "VQ_AMD_SEG_LDS_ROWS"


def _i32(a):
    return a.ctypes.data_as(POINTER(c_int32))


def _f32(a):
    return a.ctypes.data_as(POINTER(c_float))


def scene_rows(rng, L, dim):
    """A video of a few scenes: per scene a random direction, its frames that direction plus noise (not normalised here)."""
    out, left = [], L
    while left:
        n = int(min(left, rng.integers(1, max(2, L // 3) + 1)))
        centre = rng.standard_normal(dim)
        out.append(centre + 0.05 * rng.standard_normal((n, dim)))
        left -= n
    return np.concatenate(out).astype(np.float32)


class Index:
    """A C-level index: rows as given (normalised by the add unless normalize=0), labels, positions, optional id ranks; the
    restatement's per-group tables are cached per run limit."""

    def __init__(self, lib_mod, rows, labels, pos, ranks=None, normalize=1):
        self.m, self.lib = lib_mod, lib_mod.load()
        self.h = c_void_p()
        self.m.check(self.lib.vq_index_create(rows.shape[1], byref(self.h)))
        self.dim = rows.shape[1]
        self.n = 0
        self.add(rows, normalize)
        self.set(labels, pos, ranks)

    def add(self, rows, normalize=1):
        rows = np.ascontiguousarray(rows, dtype=np.float32)
        self.m.check(self.lib.vq_index_add(self.h, _f32(rows), len(rows), normalize))
        self.n += len(rows)

    def set(self, labels, pos, ranks=None, which=("ranks", "groups", "positions")):
        self.labels, self.pos = np.ascontiguousarray(labels, dtype=np.int32), np.ascontiguousarray(pos, dtype=np.int32)
        self.ranks = None if ranks is None else np.ascontiguousarray(ranks, dtype=np.int32)
        self.n_groups = int(self.labels.max()) + 1
        if "ranks" in which:
            self.m.check(self.lib.vq_index_set_id_ranks(self.h, None if self.ranks is None else _i32(self.ranks), 0 if self.ranks is None else self.n))
        if "groups" in which:
            self.m.check(self.lib.vq_index_set_groups(self.h, _i32(self.labels), self.n, self.n_groups))
        if "positions" in which:
            self.m.check(self.lib.vq_index_set_positions(self.h, _i32(self.pos), self.n))
        self.refresh()

    def refresh(self):
        self.stored = np.empty((self.n, self.dim), dtype=np.float32)
        self.m.check(self.lib.vq_index_export(self.h, _f32(self.stored)))
        self.tie = np.arange(self.n) if self.ranks is None else self.ranks
        self.sizes = np.bincount(self.labels, minlength=self.n_groups)
        self.order = [segment_ref.order_of(np.flatnonzero(self.labels == g), self.pos, self.tie) for g in range(self.n_groups)]
        self._tables, self._want = {}, {}

    def want(self, g, k, penalty, max_len):
        L = int(self.sizes[g])
        W = segment_ref.run_limit(L, max_len)
        if (g, W) not in self._tables:
            self._tables[g, W] = segment_ref.tables(self.stored, self.order[g], W)
        at = (g, W, min(k, L), float(np.float32(penalty)))
        if at not in self._want:
            self._want[at] = segment_ref.segment(self.stored, self.order[g], self.tie, k, penalty, W, self._tables[g, W])
        return self._want[at]

    def call(self, groups, k, penalty=0.0, max_len=0, show=True, mean=True):
        """vq_index_segment_groups -> (rc, dict of arrays)"""
        g = np.ascontiguousarray(groups, dtype=np.int32)
        out = dict(count=np.full(len(g), -7, np.int32), first=np.full((len(g), k), -7, np.int32), last=np.full((len(g), k), -7, np.int32),
                   len=np.full((len(g), k), -7, np.int32), spread=np.full((len(g), k), -7.0, np.float32),
                   show=np.full((len(g), k), -7, np.int32), mean_spread=np.full(len(g), -7.0, np.float32))
        rc = self.lib.vq_index_segment_groups(self.h, _i32(g), len(g), k, c_float(penalty), max_len, _i32(out["count"]), _i32(out["first"]),
                                              _i32(out["last"]), _i32(out["len"]), _f32(out["spread"]), _i32(out["show"]) if show else None,
                                              _f32(out["mean_spread"]) if mean else None)
        return rc, out

    def expected(self, groups, k, penalty, max_len):
        """The restatement's answer in the C layout: -1 / -1 / 0 / +inf / -1 in the unused slots."""
        n = len(groups)
        out = dict(count=np.zeros(n, np.int32), first=np.full((n, k), -1, np.int32), last=np.full((n, k), -1, np.int32),
                   len=np.zeros((n, k), np.int32), spread=np.full((n, k), np.inf, np.float32), show=np.full((n, k), -1, np.int32),
                   mean_spread=np.full(n, np.inf, np.float32))
        for e, g in enumerate(groups):
            w = self.want(int(g), k, penalty, max_len)
            c = w["count"]
            out["count"][e] = c
            for name in ("first", "last", "len", "spread", "show"):
                out[name][e, :c] = w[name]
            out["mean_spread"][e] = w["mean_spread"]
        return out

    def stats(self):
        st = (c_int64 * 3)()
        self.m.check(self.lib.vq_index_last_search_stats(self.h, st))
        return list(st)

    def plan(self, groups, k, max_len):
        L = np.ascontiguousarray(self.sizes[np.asarray(groups)], dtype=np.int64)
        batches, lds_rows, glob, launches = c_int(), c_int(), c_int(), c_int()
        table, lds_bytes, pairs = c_int64(), c_int64(), c_int64()
        self.m.check(self.lib.vq_debug_segment_plan(L.ctypes.data_as(POINTER(c_int64)), len(L), self.dim, k, max_len, byref(batches), byref(table),
                                                    byref(lds_rows), byref(lds_bytes), byref(glob), byref(launches), byref(pairs)))
        return dict(batches=batches.value, pairs=pairs.value, global_form=glob.value)

    def close(self):
        if self.h:
            self.lib.vq_index_destroy(self.h)
            self.h = c_void_p()


def same(got, want, what):
    for name in ("count", "first", "last", "len", "show"):
        assert np.array_equal(got[name], want[name]), f"{what}: {name} differ\n got {got[name]}\nwant {want[name]}"
    for name in ("spread", "mean_spread"):
        assert got[name].tobytes() == want[name].tobytes(), f"{what}: {name} bits differ\n got {got[name]}\nwant {want[name]}"


_CACHE = {}


def planted(gpu_lib, dim, ranked):
    """594 rows: the groups' rows interleaved by a permutation, so positions fall as often as they rise along the rows; position =
    3 * (frame // 2): two frames share each position and the tie decides; id ranks, when set, are another permutation."""
    if (dim, ranked) not in _CACHE:
        rng = np.random.default_rng(9_000 + dim)
        rows = np.concatenate([scene_rows(rng, L, dim) for L in LENGTHS])
        labels = np.concatenate([np.full(L, g) for g, L in enumerate(LENGTHS)])
        frame = np.concatenate([np.arange(L) for L in LENGTHS])
        perm = rng.permutation(len(rows))
        ranks = rng.permutation(len(rows)) if ranked else None
        # dense labels in order of first appearance are not needed at this level: any labelling with every label used is legal
        _CACHE[dim, ranked] = Index(gpu_lib, rows[perm], labels[perm], 3 * (frame[perm] // 2), ranks)
    return _CACHE[dim, ranked]


@pytest.fixture(scope="module", autouse=True)
def _close_indexes():
    yield
    for d in _CACHE.values():
        d.close()
    _CACHE.clear()


class DeviceOut:
    """Device buffers for the _device form of up to n_sel x k slots, on a stream of their own."""

    def __init__(self, n_sel, k):
        self.hip = ctypes.CDLL("libamdhip64.so")
        self.shape = (n_sel, k)
        self.ptr = {}
        for name, words in (("count", n_sel), ("first", n_sel * k), ("last", n_sel * k), ("len", n_sel * k), ("spread", n_sel * k),
                            ("show", n_sel * k), ("mean_spread", n_sel)):
            p = c_void_p()
            assert self.hip.hipMalloc(byref(p), ctypes.c_size_t(words * 4)) == 0
            self.ptr[name] = p

    def args(self):
        return [self.ptr[name] for name in ("count", "first", "last", "len", "spread", "show", "mean_spread")]

    def read(self, n_sel, k):
        out = {}
        for name, p in self.ptr.items():
            a = np.empty(n_sel if name in ("count", "mean_spread") else (n_sel, k), dtype=np.float32 if "spread" in name else np.int32)
            assert self.hip.hipMemcpy(a.ctypes.data_as(c_void_p), p, ctypes.c_size_t(a.nbytes), 2) == 0
            out[name] = a
        return out

    def free(self):
        for p in self.ptr.values():
            self.hip.hipFree(p)


# ---- 1. the sweep ----
@GPU
@pytest.mark.parametrize("ranked", [False, True])
@pytest.mark.parametrize("dim", [512, 64, 72])
def test_every_group_against_the_restatement(gpu_lib, monkeypatch, dim, ranked):
    """dim 72 is not a multiple of the 32 staged columns: the last chunk is partial."""
    monkeypatch.delenv(COST_ENV, raising=False)
    monkeypatch.delenv(LDS_ENV, raising=False)
    d = planted(gpu_lib, dim, ranked)
    assert sorted(d.sizes.tolist()) == LENGTHS
    groups = np.arange(d.n_groups, dtype=np.int32)
    dev = DeviceOut(len(groups), 64)
    try:
        for max_len in MAX_LENS:
            for k in KS:
                plan = d.plan(groups, k, max_len)
                for penalty in PENALTIES:
                    what = f"dim {dim} ranks {ranked} k {k} penalty {penalty} max_len {max_len}"
                    rc, got = d.call(groups, k, penalty, max_len)
                    gpu_lib.check(rc)
                    want = d.expected(groups, k, penalty, max_len)
                    same(got, want, what)
                    st = d.stats()
                    assert st == [int((want["count"] > 0).sum()), plan["pairs"], plan["batches"]], (what, st, plan)
                    gpu_lib.check(d.lib.vq_index_segment_groups_device(d.h, _i32(groups), len(groups), k, c_float(penalty), max_len, *dev.args()))
                    gpu_lib.check(d.lib.vq_index_synchronize(d.h))
                    same(dev.read(len(groups), k), got, what + " (device form)")
    finally:
        dev.free()
    # what the definition promises, on the restatement's own numbers
    big = int(np.argmax(d.sizes))
    for g in range(d.n_groups):
        L = int(d.sizes[g])
        assert d.want(g, 1, 0.0, 0)["cuts"] == [(0, L)]                                       # k = 1: the whole video
        assert d.want(g, 64, 1e9, 0)["cuts"] == [(0, L)]                                      # a huge penalty: one chapter
        assert d.want(g, 64, 0.0, 1)["count"] == min(64, L) * (L <= 64)                       # max_len 1: L chapters, or none
        assert d.want(g, 5, 0.0, 7)["count"] == (min(5, L) if L <= 35 else 0)
    assert 1 < d.want(big, 64, 0.05, 0)["count"] < 64                                         # the penalty chooses the number


# ---- 2. batches and both DP forms give the same bits ----
@GPU
def test_batches_and_both_dp_forms_give_the_defaults_bits(gpu_lib, monkeypatch):
    monkeypatch.delenv(COST_ENV, raising=False)
    monkeypatch.delenv(LDS_ENV, raising=False)
    d = planted(gpu_lib, 512, True)
    groups = np.arange(d.n_groups, dtype=np.int32)
    base = {}
    for k, penalty, max_len in ((5, 0.0, 0), (64, 0.05, 0), (64, 0.0, 7)):
        rc, base[k, penalty, max_len] = d.call(groups, k, penalty, max_len)
        gpu_lib.check(rc)
        assert d.stats()[2] == 1 and d.plan(groups, k, max_len) ["global_form"] == 0
    monkeypatch.setenv(COST_ENV, str(800_000))                     # one 300-row table (720,000 B) and little else
    monkeypatch.setenv(LDS_ENV, "64")                              # 65 and 300 rows: the global form, beside the LDS form
    for (k, penalty, max_len), want in base.items():
        plan = d.plan(groups, k, max_len)
        assert plan["global_form"] == 1 and (plan["batches"] >= 3 or max_len)
        rc, got = d.call(groups, k, penalty, max_len)
        gpu_lib.check(rc)
        same(got, want, f"overrides, k {k} penalty {penalty} max_len {max_len}")
        assert d.stats()[1:] == [plan["pairs"], plan["batches"]]
    monkeypatch.setenv(COST_ENV, "1")                              # a batch per group
    rc, got = d.call(groups, 5, 0.0, 0)
    gpu_lib.check(rc)
    same(got, base[5, 0.0, 0], "a batch per group")
    assert d.stats()[2] == d.n_groups


# ---- 3. the device form twice without a wait; duplicates; NULL outputs ----
@GPU
def test_device_form_twice_without_a_wait_and_duplicate_labels(gpu_lib, monkeypatch):
    monkeypatch.delenv(COST_ENV, raising=False)
    monkeypatch.setenv(LDS_ENV, "64")                              # both DP forms in each call
    d = planted(gpu_lib, 512, True)
    big, one = int(np.argmax(d.sizes)), int(np.argmin(d.sizes))
    calls = [(np.array([big, one, big, 3, big], dtype=np.int32), 8, 0.02, 0), (np.arange(d.n_groups, dtype=np.int32), 5, 0.0, 40)]
    want = []
    for g, k, penalty, max_len in calls:
        rc, got = d.call(g, k, penalty, max_len)
        gpu_lib.check(rc)
        same(got, d.expected(g, k, penalty, max_len), "host form")           # duplicates: each entry on its own, identically
        want.append(got)
    assert want[0]["first"][0].tobytes() == want[0]["first"][2].tobytes() == want[0]["first"][4].tobytes()
    rc, bare = d.call(calls[0][0], 8, 0.02, 0, show=False, mean=False)         # show_out / mean_spread_out may be NULL
    gpu_lib.check(rc)
    assert (bare["show"] == -7).all() and (bare["mean_spread"] == -7).all()
    assert all(bare[name].tobytes() == want[0][name].tobytes() for name in ("count", "first", "last", "len", "spread"))
    hip = ctypes.CDLL("libamdhip64.so")
    stream = c_void_p()
    assert hip.hipStreamCreate(byref(stream)) == 0
    outs = [DeviceOut(len(g), k) for g, k, _, _ in calls] + [DeviceOut(len(calls[0][0]), calls[0][1])]
    try:
        gpu_lib.check(d.lib.vq_index_set_stream(d.h, stream))
        for (g, k, penalty, max_len), o in zip(calls + calls[:1], outs):          # back to back, nothing read back in between
            gpu_lib.check(d.lib.vq_index_segment_groups_device(d.h, _i32(g), len(g), k, c_float(penalty), max_len, *o.args()))
        assert hip.hipStreamSynchronize(stream) == 0
        for (g, k, _, _), o, ref in zip(calls + calls[:1], outs, want + want[:1]):
            same(o.read(len(g), k), ref, "device form, queued without a wait")
    finally:
        gpu_lib.check(d.lib.vq_index_set_stream(d.h, None))
        for o in outs:
            o.free()
        hip.hipStreamDestroy(stream)
    rc, _ = d.call([0, d.n_groups], 4)
    assert rc < 0 and b"outside" in d.lib.vq_last_error()
    rc, _ = d.call([-1], 4)
    assert rc < 0 and b"outside" in d.lib.vq_last_error()


# ---- 4. closed form and the prefix order, on the device ----
@GPU
def test_one_hot_closed_form_and_cancelling_rows_on_the_device(gpu_lib, monkeypatch):
    monkeypatch.delenv(COST_ENV, raising=False)
    monkeypatch.delenv(LDS_ENV, raising=False)
    x = one_hot_blocks()
    d = Index(gpu_lib, x, np.zeros(12, np.int32), np.arange(12))
    try:
        assert d.stored.tobytes() == x.tobytes()
        rc, got = d.call([0], 5)
        gpu_lib.check(rc)
        assert got["count"][0] == 3 and got["first"][0].tolist() == [0, 4, 9, -1, -1] and got["last"][0].tolist() == [3, 8, 11, -1, -1]
        assert got["len"][0].tolist() == [4, 5, 3, 0, 0] and got["show"][0].tolist() == [0, 4, 9, -1, -1]
        assert got["spread"][0].tobytes() == np.array([0, 0, 0, np.inf, np.inf], np.float32).tobytes() and got["mean_spread"][0] == 0.0
        rc, got = d.call([0], 2)
        gpu_lib.check(rc)
        assert got["first"][0].tolist() == [0, 4] and got["last"][0].tolist() == [3, 11]
        same(got, d.expected([0], 2, 0.0, 0), "one-hot, k 2")
    finally:
        d.close()
    y = cancelling_group()
    d = Index(gpu_lib, y, np.zeros(CANCEL_ROWS, np.int32), np.arange(CANCEL_ROWS), normalize=0)
    try:
        assert d.stored.tobytes() == y.tobytes() and d.dim == CANCEL_DIM
        for k in (2, 5):                                           # k = 5: a tree-order prefix gives other cuts (test_segment_cpu.py)
            rc, got = d.call([0], k)
            gpu_lib.check(rc)
            same(got, d.expected([0], k, 0.0, 0), f"cancelling rows, k {k}")
    finally:
        d.close()


# ---- 5. an empty index, labels without rows, the quadratic bound ----
@GPU
def test_empty_index_dense_labels_and_the_pair_bound(gpu_lib):
    """The C definition gives empty slots to a label that holds no row.  The index keeps its labels dense (vq_index_set_groups
    refuses a label without rows, vq_index_remove_rows renumbers them away), so no call sequence reaches that case: what can be
    checked is that refusal, and the empty index, whose every slot is empty."""
    lib = gpu_lib.load()
    h = c_void_p()
    gpu_lib.check(lib.vq_index_create(4, byref(h)))
    d = Index.__new__(Index)
    d.m, d.lib, d.h, d.dim, d.n = gpu_lib, lib, h, 4, 0
    try:
        rc, got = d.call([0, 5], 3)
        gpu_lib.check(rc)
        assert (got["count"] == 0).all() and (got["first"] == -1).all() and (got["last"] == -1).all() and (got["len"] == 0).all()
        assert np.isinf(got["spread"]).all() and (got["show"] == -1).all() and np.isinf(got["mean_spread"]).all()
        assert d.stats() == [0, 0, 0]
        dev = DeviceOut(2, 3)
        try:
            gpu_lib.check(lib.vq_index_segment_groups_device(h, _i32(np.array([0, 5], np.int32)), 2, 3, c_float(0.0), 0, *dev.args()))
            gpu_lib.check(lib.vq_index_synchronize(h))
            same(dev.read(2, 3), got, "empty index, device form")
        finally:
            dev.free()
        rows = np.tile(np.eye(4, dtype=np.float32), (2_049, 1))[:8_194]        # 8,193 rows of one group and one more
        d.add(rows)
        lab = np.zeros(8_194, np.int32)
        lab[-1] = 2
        assert lib.vq_index_set_groups(h, _i32(lab), 8_194, 3) < 0 and b"no rows" in lib.vq_last_error()
        lab[-1] = 1
        d.set(lab, np.arange(8_194))
        rc, _ = d.call([1, 0], 4)
        msg = lib.vq_last_error()
        assert rc == -1 and b"group 0 holds 8193 rows" in msg and b"2^26 pairs" in msg, msg
        rc, got = d.call([1, 0], 4, 0.0, 2)                        # with a run limit the same group is fine: period-4 one-hot rows
        gpu_lib.check(rc)
        assert got["count"].tolist() == [1, 0]                     # 4 x 2 < 8,193
    finally:
        d.close()


# ---- 6. lifetime ----
@GPU
def test_lifetime_after_add_and_remove_rows(gpu_lib, monkeypatch):
    monkeypatch.delenv(COST_ENV, raising=False)
    monkeypatch.delenv(LDS_ENV, raising=False)
    rng = np.random.default_rng(77)
    lengths = [40, 70, 9]
    rows = np.concatenate([scene_rows(rng, L, 64) for L in lengths])
    labels = np.concatenate([np.full(L, g) for g, L in enumerate(lengths)])
    perm = rng.permutation(len(rows))
    rows, labels = rows[perm], labels[perm]
    pos = rng.integers(0, 30, len(rows))
    n = 100
    d = Index(gpu_lib, rows[:n], labels[:n], pos[:n], rng.permutation(n))
    lib = d.lib
    try:
        rc, got = d.call([0, 1, 2], 5, 0.01)
        gpu_lib.check(rc)
        same(got, d.expected([0, 1, 2], 5, 0.01, 0), "fresh")
        d.add(rows[n:])                                            # stale after an add: refused until all three are set again
        rc, _ = d.call([0, 1, 2], 5)
        assert rc < 0 and b"ranks" in lib.vq_last_error()
        d.set(labels, pos, rng.permutation(len(rows)), which=("ranks",))
        rc, _ = d.call([0, 1, 2], 5)
        assert rc < 0 and b"labels" in lib.vq_last_error()
        d.set(labels, pos, d.ranks, which=("groups",))
        rc, _ = d.call([0, 1, 2], 5)
        assert rc < 0 and b"positions" in lib.vq_last_error()
        d.set(labels, pos, d.ranks, which=("positions",))
        rc, got = d.call([0, 1, 2], 5, 0.01)
        gpu_lib.check(rc)
        same(got, d.expected([0, 1, 2], 5, 0.01, 0), "after add")
        gone = np.flatnonzero(labels == 0)[::2].astype(np.int64)   # every other row of group 0
        gpu_lib.check(lib.vq_index_remove_rows(d.h, gone.ctypes.data_as(POINTER(c_int64)), len(gone)))
        rc, _ = d.call([0, 1, 2], 5)                               # removal compacts labels and ranks; the positions are stale
        assert rc < 0 and b"positions" in lib.vq_last_error()
        keep = np.setdiff1d(np.arange(len(rows)), gone)
        d.n = len(keep)
        order = np.argsort(d.ranks[keep], kind="stable")           # the surviving rows' ranks, made dense again, keep their order
        dense = np.empty(len(keep), np.int64)
        dense[order] = np.arange(len(keep))
        d.set(labels[keep], pos[keep], dense, which=("positions",))
        rc, got = d.call([0, 1, 2], 5, 0.01)
        gpu_lib.check(rc)
        same(got, d.expected([0, 1, 2], 5, 0.01, 0), "after removal")
        assert d.sizes.tolist() == [20, 70, 9]
    finally:
        d.close()


# ---- 7. Python end to end ----
@GPU
def test_video_chapters_end_to_end(gpu_lib, monkeypatch):
    monkeypatch.delenv(COST_ENV, raising=False)
    monkeypatch.delenv(LDS_ENV, raising=False)
    from video_quierer_amd.overhaul_index import SimpleVideoIndex
    rng = np.random.default_rng(812)
    lengths = {"a.mp4": 20, "b.mp4": 33, "c.mp4": 12}
    frames = [(name, i) for name, L in lengths.items() for i in range(L)]
    frames = [frames[i] for i in rng.permutation(len(frames))]     # the videos' frames arrive interleaved and out of order
    vec = {name: scene_rows(rng, L, 512) for name, L in lengths.items()}
    stamp = {name: np.round(np.sort(rng.uniform(0, 60, L)), 3) for name, L in lengths.items()}
    sv = SimpleVideoIndex()
    for name, i in frames:
        sv.add_frame(vec[name][i], name, float(stamp[name][i]))
    stored = np.stack(sv.embeddings)
    tie = -np.arange(len(frames))                                  # search's tie rule: the larger frame id first
    pos = np.array([int(round(md["timestamp"] * 1000)) for md in sv.metadata])
    for name, L in lengths.items():
        rows = [r for r, md in enumerate(sv.metadata) if md["video_name"] == name]
        order = segment_ref.order_of(rows, pos, tie)
        for k, penalty, cap in ((4, 0.0, None), (8, 0.3, None), (8, 0.0, 5)):
            want = segment_ref.segment(stored, order, tie, k, penalty, segment_ref.run_limit(L, cap))
            got = sv.video_chapters(name, k, penalty=penalty, max_frames=cap)
            print(name, k, penalty, cap, [(c["start"], c["end"], c["frames"]) for c in got])
            assert [c["frames"] for c in got] == want["len"].tolist() and len(got) == want["count"]
            assert [c["start"] for c in got] == [sv.metadata[r]["timestamp"] for r in want["first"]]
            assert [c["end"] for c in got] == [sv.metadata[r]["timestamp"] for r in want["last"]]
            assert [c["spread"] for c in got] == [float(s) for s in want["spread"]]
            assert [c["poster"] for c in got] == [sv.metadata[r] for r in want["show"]]
            assert all(a["end"] <= b["start"] for a, b in zip(got, got[1:])) and sum(c["frames"] for c in got) == L
    by_group = sv._device(ranks=True).segment_groups(k=4, group_of=sv._group_fn, position_of=sv._pos_fn)
    assert sorted(by_group) == sorted(lengths) and all(len(v) == 4 for v in by_group.values())
    with pytest.raises(KeyError):
        sv.video_chapters("nope.mp4")
