"""GPU: pass 1 of the four fp16 paths on the streamed 256 x 256 mainloop (csrc/scan_stream256.h), stage-tested against fp64
scores (tests/tile_stage_ref.py): neighbors_tile_kernel, label_tile_kernel, match_tile_kernel and set_group_max_kernel.

Each case builds one small index with normalize = 0 (the fp32 data given IS the data stored), asserts from the plan entry or
the read-back's own words that the tile path answers and the call is not flagged, calls once in mode 2, reads back what the
tile kernel left (vq_index_debug_read_scan_keys / _label_parts / _match_bits / _group_best) and hands it to the checker; then it
calls again and asserts the same bits.  The only tolerance is E = eps_unit(dim) max|row| |q| (for the filed band of the match
scan 2 E + MATCH_SLACK + 2^-22), restated in the reference.  Each check prints `case / stage / ratio`;
profiles/tile_scan_stages/ratios.txt is the table of one run ($VQ_SCAN_RATIOS_OUT names the file the lines are appended to).
"""
import ctypes
import os

import numpy as np
import pytest

import scan_stage_ref as ref
import tile_stage_ref as tile

pytestmark = pytest.mark.gpu

MODE_FP16 = 2
K = 3
ERR_STATE = -3
CHUNK_ENV, CAP_ENV = "VQ_AMD_NEIGHBORS_CHUNK", "VQ_AMD_MATCH_FILED_CAP"


def record(case, stage, ratio):
    line = f"{case:<66} {stage:<10} {ratio:.4g}"
    print(line)
    out = os.environ.get("VQ_SCAN_RATIOS_OUT")
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def u32ptr(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))


class Index:
    """A vq_index handle over the C ABI, rows stored as given."""

    def __init__(self, L, monkeypatch, dim, rows, labels=None, positions=False, env=None):
        self.L, self.lib, self.dim = L, L.load(), dim
        for name in (CHUNK_ENV, CAP_ENV):
            monkeypatch.delenv(name, raising=False)
        for name, v in (env or {}).items():
            monkeypatch.setenv(name, str(v))
        self.h = ctypes.c_void_p()
        L.check(self.lib.vq_index_create(dim, ctypes.byref(self.h)))
        self.add(rows)
        if labels is not None:
            self.set_groups(labels, positions)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.lib.vq_index_destroy(self.h)

    def add(self, rows):
        rows = np.ascontiguousarray(rows, np.float32)
        self.L.check(self.lib.vq_index_add(self.h, self.L.fptr(rows), len(rows), 0))
        self.n = len(rows)

    def set_groups(self, labels, positions=False):
        lab = np.ascontiguousarray(labels, np.int32)
        self.G = int(lab.max()) + 1
        self.L.check(self.lib.vq_index_set_groups(self.h, self.L.i32ptr(lab), len(lab), self.G))
        if positions:                                # the shared-footage search walks each group by position: the row order
            pos = np.arange(len(lab), dtype=np.int32)
            self.L.check(self.lib.vq_index_set_positions(self.h, self.L.i32ptr(pos), len(pos)))

    def stats(self):
        st = (ctypes.c_int64 * 3)()
        self.L.check(self.lib.vq_index_last_search_stats(self.h, st))
        return [int(v) for v in st]

    # ---- the four calls
    def neighbors_rc(self, asked, exclude, m=None):
        m = len(asked) if asked is not None else (self.n if m is None else m)
        ids, dist = np.empty((m, K), np.int32), np.empty((m, K), np.float32)
        ptr = None if asked is None else self.L.i64ptr(np.ascontiguousarray(asked, np.int64))
        return self.lib.vq_index_neighbors(self.h, ptr, m, K, exclude, MODE_FP16, self.L.i32ptr(ids), self.L.fptr(dist))

    def neighbors(self, asked, exclude):
        self.L.check(self.neighbors_rc(asked, exclude))

    def label(self, prompts):
        prompts = np.ascontiguousarray(prompts, np.float32)
        lab, dist = np.empty(self.n, np.int32), np.empty(self.n, np.float32)
        self.L.check(self.lib.vq_index_label_rows(self.h, self.L.fptr(prompts), len(prompts), MODE_FP16, ctypes.c_float(np.inf), self.L.i32ptr(lab),
                                                  self.L.fptr(dist), 0, None, None, None, None))

    def match(self, qs, max_dist):
        qs = np.ascontiguousarray(qs, np.float32)
        out = [np.empty(K, np.int32) for _ in range(6)] + [np.empty(K, np.float32)]
        self.L.check(self.lib.vq_index_match_runs(self.h, self.L.fptr(qs), len(qs), K, ctypes.c_float(max_dist), 2, 0, MODE_FP16, None, 0, 1,
                                                  *(self.L.i32ptr(a) for a in out[:6]), self.L.fptr(out[6])))

    def search_set(self, qs, sel=None, exclude=1):
        """sel = None: unfiltered (an empty exclude list)"""
        qs = np.ascontiguousarray(qs, np.float32)
        g, d = np.empty(K, np.int32), np.empty(K, np.float32)
        s = None if sel is None else np.ascontiguousarray(sel, np.int32)
        self.L.check(self.lib.vq_index_search_set(self.h, self.L.fptr(qs), len(qs), K, MODE_FP16, None if s is None else self.L.i32ptr(s),
                                                  0 if s is None else len(s), exclude, self.L.i32ptr(g), self.L.fptr(d), None))

    # ---- the read-backs
    def keys(self):
        return ref.read_scan_keys(self.lib, self.L.check, self.h)

    def label_parts(self):
        return tile.read_label_parts(self.lib, self.L.check, self.h)

    def match_bits(self):
        return tile.read_match_bits(self.lib, self.L.check, self.h)

    def group_best(self):
        return ref.read_group_best(self.lib, self.L.check, self.h), tile.read_group_scan_kind(self.lib, self.L.check, self.h)

    def reader_codes(self):
        i = (ctypes.c_int64 * 6)()
        return [self.lib.vq_index_debug_read_scan_keys(self.h, i, None, 0), self.lib.vq_index_debug_read_group_best(self.h, i, None, 0),
                self.lib.vq_index_debug_group_scan_kind(self.h, i), self.lib.vq_index_debug_read_label_parts(self.h, i, None, 0),
                self.lib.vq_index_debug_read_match_bits(self.h, i, None, 0, None, 0)]


def stored_rows(cls, rng, n, dim):
    """the class's rows for a scan whose queries are stored rows: qnorm (a class of the QUERIES) is a second unnormalised seed"""
    if cls == "qnorm":
        return ref.unnormalised_rows(np.random.default_rng([43, dim, n]), n, dim)
    return ref.input_class(cls, rng, n, 1, dim)[0]


# ---------------------------------------------------------------- library neighbours (neighbors_tile_kernel)
def neighbor_labels(n):
    """Runs that change off a lane's 4-row boundary (row 10), on it (16), across a 256-row tile (250 .. 261) and across the
    2,048-row range (2040 .. 2059); a one-row group (300); one group that is a whole 128-row stream (stream 5 of range 0, its
    rows spread over the eight tiles); dense labels."""
    if n < 16:
        return (np.arange(n) % 2).astype(np.int64) if n > 1 else np.zeros(1, np.int64)
    cuts = [c for c in (10, 16, 250, 262, 300, 301, 1000, 2040, 2060) if c < n]
    lab = np.searchsorted(np.array(cuts), np.arange(n), side="right").astype(np.int64)
    lab[tile.stream_of(np.arange(n)) == 5] = len(cuts) + 1
    return np.unique(lab, return_inverse=True)[1].astype(np.int64)


def neighbor_plan(ix, m, exclude):
    fp16, chunk_rows, chunks, key_bytes, kind, eps = ctypes.c_int(), ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int(), ctypes.c_float()
    ix.L.check(ix.lib.vq_debug_neighbors_plan(ix.n, ix.dim, m, K, exclude, MODE_FP16, ctypes.byref(fp16), ctypes.byref(chunk_rows), ctypes.byref(chunks),
                                              ctypes.byref(key_bytes), ctypes.byref(kind), ctypes.byref(eps)))
    return fp16.value, chunk_rows.value, chunks.value


def neighbor_case(L, monkeypatch, cls, dim, n, m, exclude, chunk=None):
    """m = None: every row; else a row list of m entries (repeats allowed, the last row among them)"""
    rng = np.random.default_rng([47, dim, n, 0 if m is None else m, exclude])
    rows = stored_rows(cls, rng, n, dim)
    asked = None if m is None else np.append(rng.integers(0, n, m - 1), n - 1).astype(np.int64)
    who = np.arange(n) if asked is None else asked
    labels = neighbor_labels(n)
    tags = labels if exclude else np.arange(n)
    case = f"neighbours {cls} dim={dim} n={n} {'all' if m is None else 'list m=%d' % m} exclude={exclude}" + (f" chunk={chunk}" if chunk else "")
    with Index(L, monkeypatch, dim, rows, labels if exclude else None, env={CHUNK_ENV: chunk} if chunk else None) as ix:
        fp16, chunk_rows, chunks = neighbor_plan(ix, len(who), exclude)
        want_chunk = tile.round_up(chunk, 256) if chunk else tile.round_up(len(who), 256)
        assert fp16 == 1 and chunk_rows == want_chunk and chunks == -(-len(who) // want_chunk), (case, fp16, chunk_rows, chunks)
        q0 = (chunks - 1) * chunk_rows
        ix.neighbors(asked, exclude)
        info, keys = ix.keys()
        streams = tile.round_up(n, tile.RANGE) // 128
        assert info == dict(q0=q0, cur=len(who) - q0, layout=2, streams=streams, masked=2), (case, info)
        st = ix.stats()
        assert st[0] + st[2] == len(who), (case, st)             # the tile path answered: every asked row proven or redone exactly
        table = ref.row_table(ix.lib, 2, streams)
        allowed = tile.allowed_from_tags(tags[who[q0:]], tags)
        record(case, "keys", ref.check_keys(keys, rows, rows[who[q0:]], table, allowed))
        ix.neighbors(asked, exclude)
        info2, again = ix.keys()
        assert info2 == info and np.array_equal(keys, again), f"{case}: the second call left other key bits"
    return keys


NB_N = (2, 255, 257, 2048, 2049, 2048 + 257)
NB_CASES = [("gaussian", 256, n, m, ex) for n in NB_N for m in (None, 1, 257) for ex in (0, 1)] + \
           [("gaussian", dim, 2305, None, ex) for dim in (512, 768) for ex in (0, 1)] + \
           [(cls, 256, 2305, None, 1) for cls in ref.INPUT_CLASSES[1:]] + [("identical", 256, 2305, None, 0)]


@pytest.mark.parametrize("cls,dim,n,m,exclude", NB_CASES)
def test_neighbors_tile_scan(gpu_lib, monkeypatch, cls, dim, n, m, exclude):
    neighbor_case(gpu_lib, monkeypatch, cls, dim, n, m, exclude)


def test_neighbors_tile_scan_second_chunk(gpu_lib, monkeypatch):
    neighbor_case(gpu_lib, monkeypatch, "gaussian", 256, 300, None, 1, chunk=256)           # two chunks: the keys read are rows 256 .. 299's


def test_neighbors_tile_scan_one_row(gpu_lib, monkeypatch):
    """n = 1, exclude = 0: the only pair is struck, every key must read "no row" (or the call refuses the shape)"""
    rows = ref.gaussian_unit(np.random.default_rng(53), 1, 256)
    with Index(gpu_lib, monkeypatch, 256, rows) as ix:
        rc = ix.neighbors_rc(None, 0)
        if rc != 0:
            assert rc == -1
            return
        info, keys = ix.keys()
        assert info == dict(q0=0, cur=1, layout=2, streams=16, masked=2)
        assert (keys.view(np.float32) < ref.NO_ROW_BELOW).all()
        record("neighbours gaussian dim=256 n=1 all exclude=0", "keys",
               ref.check_keys(keys, rows, rows, ref.row_table(ix.lib, 2, 16), np.zeros((1, 1), bool)))


# ---------------------------------------------------------------- zero-shot labelling (label_tile_kernel)
def label_plan(ix, P):
    v = [ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int64(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int64(), ctypes.c_int64(),
         ctypes.c_float(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int64()]
    ix.L.check(ix.lib.vq_debug_label_plan(ix.n, ix.dim, P, MODE_FP16, 0, *(ctypes.byref(x) for x in v)))
    return dict(fp16=v[0].value, prompt_tiles=v[4].value, prompt_ranges=v[5].value, row_tiles=v[6].value)


LABEL_P = (1, 2, 3, 255, 257, 2048, 2049, 4096)
LABEL_CASES = [("gaussian", 512, n, P) for n in (1, 257) for P in LABEL_P] + \
              [("gaussian", dim, 257, P) for dim in (256, 768) for P in (257, 2049)] + [(cls, 512, 257, 600) for cls in ref.INPUT_CLASSES]


@pytest.mark.parametrize("cls,dim,n,P", LABEL_CASES)
def test_label_tile_scan(gpu_lib, monkeypatch, cls, dim, n, P):
    rows, prompts = ref.input_class(cls, np.random.default_rng([59, dim, n, P]), n, P, dim)      # qnorm: the prompts' norms
    case = f"label {cls} dim={dim} n={n} P={P}"
    with Index(gpu_lib, monkeypatch, dim, rows) as ix:
        n_pad, ranges = tile.label_shape(n, P)
        plan = label_plan(ix, P)
        assert plan == dict(fp16=1, prompt_tiles=-(-P // 256), prompt_ranges=ranges, row_tiles=n_pad // 256), (case, plan)
        ix.label(prompts)
        info, parts = ix.label_parts()                   # (a flagged call is refused here: VQ_ERR_STATE)
        assert info == dict(n=n, n_pad=n_pad, ranges=ranges, P=P), (case, info)
        st = ix.stats()
        assert sum(st) == n, (case, st)
        record(case, "parts", tile.check_label_parts(parts, n, rows, prompts))
        ix.label(prompts)
        info2, again = ix.label_parts()
        assert info2 == info and np.array_equal(parts[:, :, :n], again[:, :, :n]), f"{case}: the second call left other bits"


# ---------------------------------------------------------------- shared-footage search (match_tile_kernel)
def match_plan(ix, m):
    v = [ctypes.c_int(), ctypes.c_int64(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int64(), ctypes.c_int64(),
         ctypes.c_int(), ctypes.c_int64(), ctypes.c_int()]
    ix.L.check(ix.lib.vq_debug_match_plan(ix.n, ix.G, ix.dim, m, MODE_FP16, *(ctypes.byref(x) for x in v)))
    return dict(fp16=v[0].value, q_tiles=v[4].value, ranges=v[5].value, filed_cap=v[7].value)


def match_case(L, monkeypatch, cls, dim, m, n, cap=None):
    rows, qs, max_dist = tile.match_inputs(cls, dim, m, n)
    ex = ref.exact_scores(rows, qs)
    assert tile.threshold_conditions(ex, max_dist) == (True, True)          # before the GPU call: a pair beside T, none inside 2^-21
    case = f"match {cls} dim={dim} m={m} n={n}" + (f" cap={cap}" if cap else "")
    with Index(L, monkeypatch, dim, rows, np.arange(n) // 64, positions=True, env={CAP_ENV: cap} if cap else None) as ix:
        plan = match_plan(ix, m)
        assert plan["fp16"] == 1 and plan["q_tiles"] == -(-m // 256) and plan["ranges"] == -(-n // 2048), (case, plan)
        assert plan["filed_cap"] == (cap if cap else 16 << 20)
        ix.match(qs, max_dist)
        info, bits, filed = ix.match_bits()
        assert (info["m"], info["W"], info["n"], info["cap"]) == (m, (n + 31) // 32, n, plan["filed_cap"]), (case, info)
        if cap:
            # the list overflowed: the exact redo rewrote the whole table
            assert info["flag"] == 2 and info["cursor"] > cap and ix.stats()[2] == 2, (case, info)
            tile.check_match_bits(bits, filed, info, rows, qs, max_dist, redone=True)
            record(case, "bits", 0.0)
        else:
            assert info["flag"] == 0 and ix.stats()[1:] == [info["cursor"], 0], (case, info, ix.stats())
            record(case, "bits+filed", tile.check_match_bits(bits, filed, info, rows, qs, max_dist))
        ix.match(qs, max_dist)
        info2, again, filed2 = ix.match_bits()
        assert np.array_equal(bits, again), f"{case}: the second call left other bits"
        if not cap:
            assert info2 == info and np.array_equal(np.sort(filed), np.sort(filed2)), f"{case}: the second call filed other pairs"


@pytest.mark.parametrize("cls,dim,m,n", tile.MATCH_CASES)
def test_match_tile_scan(gpu_lib, monkeypatch, cls, dim, m, n):
    match_case(gpu_lib, monkeypatch, cls, dim, m, n)


def test_match_tile_scan_filed_list_overflows(gpu_lib, monkeypatch):
    match_case(gpu_lib, monkeypatch, "identical", 512, 257, 2348, cap=100)      # one query's 2,348 equal scores sit beside T


# ---------------------------------------------------------------- clip search (set_group_max_kernel)
GROUP_SEL = [0, 3, 5, 7]


def set_labels(n):
    """n = 1,000: test_scan_stages.group_labels (restated); else runs of 100 rows with a short first one"""
    if n == 1000:
        lab = [0] * 424 + [1] + [2] * 3 + [3, 4] * 12 + [5] * 6 + [6] * 6 + [7] * 50 + [8] * 300 + [7] * 30 + [9] * 156
        return np.array(lab, np.int64)
    return ((np.arange(n) + 63) // 100).astype(np.int64)


SET_CASES = [("gaussian", 256, m, n, flt) for m in (17, 255, 257, 273) for n in (1000, 2348) for flt in (False, True)] + \
            [("gaussian", dim, m, 1000, flt) for dim in (512, 768) for m in (257, 273) for flt in (False, True)] + \
            [(cls, 256, m, 1000, flt) for cls in ref.INPUT_CLASSES[1:] for m, flt in ((257, False), (255, True), (273, False))]


@pytest.mark.parametrize("cls,dim,m,n,flt", SET_CASES)
def test_set_group_max_tile_scan(gpu_lib, monkeypatch, cls, dim, m, n, flt):
    """The record is the LAST query chunk's.  m = 257 runs as a chunk of 256 queries (set_group_max_kernel) and a chunk of one
    (the streaming scan): the case asserts that the tile kernel ran and checks the chunk that is left; m = 273 leaves a
    second chunk of 17 queries, which the tile kernel scans (q0 = 256)."""
    rows, qs = ref.input_class(cls, np.random.default_rng([61, dim, m, n]), n, m, dim)
    labels = set_labels(n)
    case = f"set {cls} dim={dim} m={m} n={n} {'within' if flt else 'plain'}"
    with Index(gpu_lib, monkeypatch, dim, rows, labels) as ix:
        G = ix.G
        allowed = np.isin(np.arange(G), GROUP_SEL) if flt else None
        search = (lambda: ix.search_set(qs, GROUP_SEL, 0)) if flt else (lambda: ix.search_set(qs))
        search()
        (info, best), kind = ix.group_best()
        chunks = -(-m // 256)
        q0 = (chunks - 1) * 256
        last_tile = m - q0 > 16
        assert info == dict(q0=q0, cur=m - q0, n_groups=G), (case, info)
        assert kind == dict(kind=3 if last_tile else 2, chunks=chunks, tile_chunks=chunks if last_tile else chunks - 1), (case, kind)
        assert kind["tile_chunks"] >= 1, f"{case}: set_group_max_kernel did not run"
        record(case + ("" if last_tile else " (streaming chunk)"), "group_max", ref.check_group_best(best, rows, qs[q0:], labels, G, allowed))
        search()
        (info2, again), kind2 = ix.group_best()
        assert (info2, kind2) == (info, kind) and np.array_equal(best.view(np.uint32), again.view(np.uint32)), f"{case}: the second call left other bits"


# ---------------------------------------------------------------- state: the records follow the CURRENT rows
def test_records_follow_updated_and_removed_rows(gpu_lib, monkeypatch):
    L = gpu_lib
    dim, n, m, P = 256, 600, 40, 300
    rng = np.random.default_rng(67)
    rows, qs = ref.input_class("gaussian", rng, n, m, dim)
    prompts = ref.gaussian_unit(rng, P, dim)

    def all_calls(ix, rows, case):
        labels = (np.arange(len(rows)) // 64).astype(np.int64)
        ix.set_groups(labels, positions=True)
        table = ref.row_table(ix.lib, 2, 16)
        tags = np.arange(len(rows))
        ix.neighbors(None, 0)
        record(case, "keys", ref.check_keys(ix.keys()[1], rows, rows, table, tile.allowed_from_tags(tags, tags)))
        ix.label(prompts)
        record(case, "parts", tile.check_label_parts(ix.label_parts()[1], len(rows), rows, prompts))
        max_dist = tile.choose_max_dist(ref.exact_scores(rows, qs))
        ix.match(qs, max_dist)
        info, bits, filed = ix.match_bits()
        record(case, "bits+filed", tile.check_match_bits(bits, filed, info, rows, qs, max_dist))
        ix.search_set(qs)
        (info, best), kind = ix.group_best()
        assert kind["kind"] == 3
        record(case, "group_max", ref.check_group_best(best, rows, qs, labels, ix.G))

    with Index(L, monkeypatch, dim, rows) as ix:
        assert ix.reader_codes() == [ERR_STATE] * 5                                          # nothing scanned yet
        all_calls(ix, rows, f"state first dim={dim} n={n}")
        assert ix.reader_codes() == [0] * 5
        # a few rows, one in the last (ragged) tile, become near copies of query 0 / of each other: stale fp16 copies would show
        upd = np.array([5, 300, n - 1], np.int64)
        new = ref.unit(qs[0][None, :] + 0.05 * ref.gaussian_unit(rng, len(upd), dim))
        L.check(ix.lib.vq_index_update_rows(ix.h, L.fptr(new), L.i64ptr(upd), len(upd), 0))
        assert ix.reader_codes() == [ERR_STATE] * 5                                          # the rows changed: nothing old is handed out
        rows = rows.copy()
        rows[upd] = new
        rm = np.array([5, 17], np.int64)                 # one of the updated rows goes, every row behind it moves down
        L.check(ix.lib.vq_index_remove_rows(ix.h, L.i64ptr(rm), len(rm)))
        assert ix.reader_codes() == [ERR_STATE] * 5
        rows = np.delete(rows, rm, axis=0)
        ix.n = len(rows)
        all_calls(ix, rows, f"state update+remove dim={dim} n={len(rows)}")
