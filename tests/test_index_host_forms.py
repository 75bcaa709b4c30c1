"""The two forms of every search family, side by side: a host form's arrays must equal, bit for bit, what its _device form
leaves in device memory — on a small index, with and without the optional outputs, and on an empty index, where the expected
values are written out below.  The calls go through ctypes on the C entry points; the device arrays come from hipMalloc.

This is a test of the host layer (one list of outputs per family, laid out, filled and copied back by shared helpers), not of
the scans: every call runs mode 1 at dim 64."""
import ctypes
from ctypes import POINTER, byref, c_float, c_int, c_int32, c_int64, c_void_p

import numpy as np
import pytest

GPU = pytest.mark.gpu
DIM, N, K = 64, 300, 3
LENGTHS = (120, 1, 59, 40, 50, 30)          # six groups, one of a single row
INF = float("inf")
CANARY = 0x5A
I32, F32, I64 = np.int32, np.float32, np.int64
CTYPE = {np.dtype(I32): c_int32, np.dtype(F32): c_float, np.dtype(I64): c_int64}


def _unit(a):
    a = np.asarray(a, dtype=np.float64)
    return np.ascontiguousarray(a / np.linalg.norm(a, axis=1, keepdims=True), dtype=F32)


def _hptr(a):
    return a.ctypes.data_as(POINTER(CTYPE[a.dtype]))


class Out:
    """One output array of a family: its dtype and shape, whether the call may leave it out, and the value every slot
    holds after a call on an empty index (None: the call writes nothing there)."""

    def __init__(self, name, dtype, shape, empty, optional=False):
        self.name, self.dtype, self.shape, self.empty, self.optional = name, np.dtype(dtype), tuple(shape), empty, optional


class Family:
    """host / device: the entry points' names.  q: the query array both forms read (None: the family takes none).
    args(q, o): the argument list behind the handle, given the query pointer and the output pointers in `outs` order."""

    def __init__(self, name, host, q, outs, args):
        self.name, self.host, self.device, self.q, self.outs, self.args = name, host, host + "_device", q, outs, args


def _data():
    rng = np.random.default_rng(20260307)
    rows = _unit(rng.standard_normal((N, DIM)))
    group = np.repeat(np.arange(len(LENGTHS), dtype=I32), LENGTHS)
    pos = np.concatenate([np.arange(L, dtype=I32) for L in LENGTHS])
    rank = rng.permutation(N).astype(I32)
    near = lambda r: _unit(rows[r] + 0.02 * rng.standard_normal((len(r), DIM)))
    return dict(rows=rows, group=group, pos=pos, rank=rank, queries=near([10, 200]), one_query=near([140]), frames=near([3, 4, 5]),
                prompts=_unit(rng.standard_normal((4, DIM))))


def _families(d):
    G = len(LENGTHS)
    sel = np.array([0, 2], dtype=I32)                       # two listed groups
    init_rows = np.array([0, 130, 200, 260], dtype=I32)
    clause_of = np.array([0, 0, 1, -1], dtype=I32)
    nb_rows = np.array([0, 120, 121, 250, 299], dtype=I64)
    q, frames, prompts = d["queries"], d["frames"], d["prompts"]
    nq, m, P = len(q), len(frames), len(prompts)
    ids = lambda n, nm="ids": Out(nm, I32, (n, K), -1)
    dist = lambda n, nm="dist": Out(nm, F32, (n, K), INF)
    fams = [
        Family("plain", "vq_index_search", q, [ids(nq), dist(nq)], lambda q, o: (q, nq, K, 1, *o)),
        Family("grouped", "vq_index_search_grouped", q, [ids(nq, "groups"), ids(nq, "rows"), dist(nq)], lambda q, o: (q, nq, K, 1, *o)),
        Family("distinct", "vq_index_search_distinct", q, [ids(nq), dist(nq)], lambda q, o: (q, nq, K, 1, 2, *o)),
        Family("diverse", "vq_index_search_diverse", q, [ids(nq), dist(nq)], lambda q, o: (q, nq, K, 1, 0.1, *o)),
        Family("filtered", "vq_index_search_filtered", q, [ids(nq), dist(nq)], lambda q, o: (q, nq, K, 1, _hptr(sel), 2, 0, *o)),
        Family("grouped filtered", "vq_index_search_grouped_filtered", q, [ids(nq, "groups"), ids(nq, "rows"), dist(nq)],
               lambda q, o: (q, nq, K, 1, _hptr(sel), 2, 0, *o)),
        Family("set", "vq_index_search_set", frames, [Out("groups", I32, (K,), -1), Out("dist", F32, (K,), INF), Out("match", I32, (K, m), -1, True)],
               lambda q, o: (q, m, K, 1, None, 0, 1, *o)),
        Family("sequence", "vq_index_search_sequence", frames,
               [Out("groups", I32, (K,), -1), Out("dist", F32, (K,), INF), Out("chain", I32, (K, m), -1, True)],
               lambda q, o: (q, m, K, 1, 1000, None, 0, 1, *o)),
    ]
    for name, sq in (("spans", q), ("spans, one query", d["one_query"])):     # the block that mixes widths, at 6 and at 3 slots
        n1 = len(sq)
        fams.append(Family(name, "vq_index_search_spans", sq,
                           [ids(n1, "groups"), dist(n1), Out("mass", I64, (n1, K), 0, True), Out("len", I32, (n1, K), 0, True),
                            Out("rows", I32, (n1, K, 3), -1, True)],
                           lambda q, o, n1=n1: (q, n1, K, 0.9, 5, 1 << 40, None, 0, 1, *o)))
    fams += [
        Family("summarize", "vq_index_summarize_groups", None, [ids(2, "rows"), dist(2, "radius"), Out("members", I32, (2, K), 0, True)],
               lambda q, o: (_hptr(sel), 2, K, -INF, *o)),
        Family("segment", "vq_index_segment_groups", None,
               [Out("count", I32, (2,), 0), ids(2, "first"), ids(2, "last"), Out("len", I32, (2, K), 0), dist(2, "spread"),
                Out("show", I32, (2, K), -1, True), Out("mean_spread", F32, (2,), INF, True)],
               lambda q, o: (_hptr(sel), 2, K, 0.0, 0, *o)),
        Family("label", "vq_index_label_rows", prompts,
               [Out("row_label", I32, (N,), None, True), Out("row_dist", F32, (N,), None, True), Out("tags", I32, (G, 2), None, True),
                Out("votes", I32, (G, 2), None, True), Out("show", I32, (G, 2), None, True), Out("unlabelled", I32, (G,), None, True)],
               lambda q, o: (q, P, 1, INF, o[0], o[1], 2, *o[2:])),
        Family("compound", "vq_index_search_compound", prompts,
               [Out("ids", I32, (K,), -1), Out("dist", F32, (K,), INF), Out("term_dist", F32, (K, P), INF, True)],
               lambda q, o: (q, P, _hptr(clause_of), -INF, K, 1, *o)),
        Family("match", "vq_index_match_runs", frames,
               [Out("groups", I32, (K,), -1), Out("hits", I32, (K,), 0), Out("span", I32, (K,), 0), Out("q_first", I32, (K,), -1),
                Out("row_first", I32, (K,), -1), Out("row_last", I32, (K,), -1), Out("mean_dist", F32, (K,), INF)],
               lambda q, o: (q, m, K, 0.5, 1, 1, 1, None, 0, 1, *o)),
        Family("neighbours", "vq_index_neighbors", None, [Out("ids", I32, (5, K), None), Out("dist", F32, (5, K), None)],
               lambda q, o: (_hptr(nb_rows), 5, K, 1, 1, *o)),
    ]
    # the arrays the lambdas point into must outlive the calls
    return fams, (sel, init_rows, clause_of, nb_rows)


class Hip:
    def __init__(self):
        self.hip = ctypes.CDLL("libamdhip64.so")
        self.ptrs = []

    def array(self, host):
        """Device memory holding a copy of `host` (the blocking copy is done before any call is queued)."""
        p = c_void_p()
        assert self.hip.hipMalloc(byref(p), ctypes.c_size_t(max(host.nbytes, 8))) == 0
        self.ptrs.append(p)
        assert self.hip.hipMemcpy(p, host.ctypes.data_as(c_void_p), ctypes.c_size_t(host.nbytes), 1) == 0
        return p

    def read(self, p, like):
        got = np.empty_like(like)
        assert self.hip.hipMemcpy(got.ctypes.data_as(c_void_p), p, ctypes.c_size_t(got.nbytes), 2) == 0
        return got

    def free(self):
        for p in self.ptrs:
            self.hip.hipFree(p)
        self.ptrs = []


def _canary(dtype, shape):
    dtype = np.dtype(dtype)
    return np.frombuffer(bytes([CANARY]) * (int(np.prod(shape)) * dtype.itemsize), dtype=dtype).reshape(shape).copy()


def _canaries(fam, full):
    """name -> an array of canary bytes for every output this variant gives (optional ones only in the full variant)."""
    return {o.name: _canary(o.dtype, o.shape) for o in fam.outs if full or not o.optional}


def _run_host(lib, h, fam, full):
    arrs = _canaries(fam, full)
    o = [_hptr(arrs[x.name]) if x.name in arrs else None for x in fam.outs]
    rc = getattr(lib, fam.host)(h, *fam.args(_hptr(fam.q) if fam.q is not None else None, o))
    assert rc == 0, (fam.name, lib.vq_last_error())
    return arrs


def _run_device(lib, hip, h, fam, full):
    """Canaries go down, the device form runs on the index's stream, the arrays come back after a wait on that stream."""
    want = _canaries(fam, full)
    dev = {name: hip.array(a) for name, a in want.items()}
    dq = hip.array(fam.q) if fam.q is not None else None
    o = [dev.get(x.name) for x in fam.outs]
    rc = getattr(lib, fam.device)(h, *fam.args(dq, o))
    assert rc == 0, (fam.name, lib.vq_last_error())
    assert lib.vq_index_synchronize(h) == 0
    return {name: hip.read(p, want[name]) for name, p in dev.items()}


def _cluster(lib, hip, h, init_rows, full, host):
    """The clustering call, whose two forms take different arguments (the host form also reports its iterations)."""
    P, iters = 4, 3
    shapes = dict(centroids=(F32, (P, DIM)), row_label=(I32, (N,)), row_dist=(F32, (N,)), counts=(I32, (P,)), show_rows=(I32, (P,)))
    arrs = {k: _canary(t, s) for k, (t, s) in shapes.items() if full or k not in ("row_label", "row_dist")}
    if host:
        it, changed = c_int(-7), np.full(iters, -7, dtype=I32)
        p = {k: _hptr(a) for k, a in arrs.items()}
        rc = lib.vq_index_cluster(h, None, _hptr(init_rows), P, iters, 1, p["centroids"], p.get("row_label"), p.get("row_dist"), p["counts"],
                                  p["show_rows"], byref(it), _hptr(changed))
        assert rc == 0, lib.vq_last_error()
        return arrs, it.value
    dev = {k: hip.array(a) for k, a in arrs.items()}
    rc = lib.vq_index_cluster_device(h, None, hip.array(init_rows), P, iters, 1, dev["centroids"], dev.get("row_label"), dev.get("row_dist"),
                                     dev["counts"], dev["show_rows"])
    assert rc == 0, lib.vq_last_error()
    assert lib.vq_index_synchronize(h) == 0
    return {k: hip.read(p, arrs[k]) for k, p in dev.items()}, None


def _same(a, b, what):
    assert a.keys() == b.keys(), what
    for name in a:
        assert a[name].tobytes() == b[name].tobytes(), (what, name, a[name], b[name])


@pytest.fixture(scope="module")
def setup(gpu_lib):
    lib = gpu_lib.load()
    d = _data()
    h = c_void_p()
    gpu_lib.check(lib.vq_index_create(DIM, byref(h)))
    gpu_lib.check(lib.vq_index_add(h, _hptr(d["rows"]), N, 0))
    gpu_lib.check(lib.vq_index_set_groups(h, _hptr(d["group"]), N, len(LENGTHS)))
    gpu_lib.check(lib.vq_index_set_positions(h, _hptr(d["pos"]), N))
    gpu_lib.check(lib.vq_index_set_id_ranks(h, _hptr(d["rank"]), N))
    empty = c_void_p()
    gpu_lib.check(lib.vq_index_create(DIM, byref(empty)))
    fams, keep = _families(d)
    hip = Hip()
    yield lib, hip, h, empty, fams, keep
    hip.free()
    lib.vq_index_destroy(h)
    lib.vq_index_destroy(empty)


@GPU
def test_host_and_device_forms_agree_bit_for_bit(setup):
    lib, hip, h, _, fams, _ = setup
    for fam in fams:
        host_full, dev_full = _run_host(lib, h, fam, True), _run_device(lib, hip, h, fam, True)
        _same(host_full, dev_full, (fam.name, "every output"))
        host_null, dev_null = _run_host(lib, h, fam, False), _run_device(lib, hip, h, fam, False)
        _same(host_null, dev_null, (fam.name, "optional outputs null"))
        _same(host_null, {k: host_full[k] for k in host_null}, (fam.name, "null variant against full variant"))
        hip.free()
    # the calls answered: slots were written (a canary left everywhere would also compare equal)
    plain = _run_host(lib, h, fams[0], True)
    assert (plain["ids"] >= 0).all() and np.isfinite(plain["dist"]).all()


@GPU
def test_span_block_mixes_widths_in_every_slot(setup):
    """Masses (64-bit), lengths and rows (3 words per slot) behind groups and distances in one block: at nq = 2, k = 3 and at one
    query, where the 32-bit fields are 12 bytes long and the 64-bit field behind them needs the layout's 8-byte alignment."""
    lib, hip, h, _, fams, _ = setup
    for fam in (f for f in fams if f.host == "vq_index_search_spans"):
        host, dev = _run_host(lib, h, fam, True), _run_device(lib, hip, h, fam, True)
        for o in fam.outs:
            a, b = host[o.name].reshape(-1, *o.shape[2:]), dev[o.name].reshape(-1, *o.shape[2:])
            for slot in range(len(a)):
                assert a[slot].tobytes() == b[slot].tobytes(), (fam.name, o.name, slot, a[slot], b[slot])
        assert (host["groups"] >= 0).any() and (host["len"][host["groups"] >= 0] >= 1).all()      # spans were found and finished
        hip.free()


@GPU
def test_cluster_forms_agree(setup):
    lib, hip, h, _, _, keep = setup
    init_rows = keep[1]
    for full in (True, False):
        host, T = _cluster(lib, hip, h, init_rows, full, True)
        dev, _ = _cluster(lib, hip, h, init_rows, full, False)
        assert 1 <= T <= 3
        _same(host, dev, ("cluster", full))
        if full:
            first = host
        else:
            _same(host, {k: first[k] for k in host}, "cluster: null variant against full variant")
        assert host["counts"].sum() == N and (host["show_rows"] >= 0).all()
        hip.free()


@GPU
def test_empty_index_answers(setup):
    """Both forms, both variants, on an index of dim 64 that holds no row: -1 for rows and groups, +inf for distances (term
    distances and mean spreads too), 0 for lengths, counts, members, hits, spans and masses.  The labelling, clustering and
    (m = 0) neighbours calls return 0 and leave the caller's arrays as they were."""
    lib, hip, _, empty, fams, keep = setup
    for fam in fams:
        if fam.host == "vq_index_neighbors":                # no row to ask for and no labels: rows = NULL, m = 0, exclude = 0
            fam = Family(fam.name, fam.host, None, fam.outs, lambda q, o: (None, 0, K, 0, 1, *o))
        for full in (True, False):
            for got in (_run_host(lib, empty, fam, full), _run_device(lib, hip, empty, fam, full)):
                for o in fam.outs:
                    if o.name not in got:
                        continue
                    if o.empty is None:
                        assert got[o.name].tobytes() == bytes([CANARY]) * got[o.name].nbytes, (fam.name, o.name)
                    else:
                        assert got[o.name].tobytes() == np.full(o.shape, o.empty, dtype=o.dtype).tobytes(), (fam.name, o.name, got[o.name])
        hip.free()
    for full in (True, False):
        for host in (True, False):
            got, _ = _cluster(lib, hip, empty, keep[1], full, host)
            for name, a in got.items():
                assert a.tobytes() == bytes([CANARY]) * a.nbytes, ("cluster", name)
    hip.free()
