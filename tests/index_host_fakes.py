"""What the CPU tests of the index's Python layer share: a bare ``HNSWIndex`` (no library handle, no device) over a given id
list, and a recording stand-in for libvq_amd whose entry points a test file composes from the defaults below and its own
canned answers.  (The GPU suites take ``unit`` and ``tie_ranks`` from here.)"""
import threading

import numpy as np


def bare_index(ids=(), *, dimension=4, identity=False, tie_order="stale"):
    """An index holding ``ids`` as the rows 0..n-1 of a matrix nobody stored; ``identity`` / ``tie_order`` as the test needs them
    (the default is what a freshly added block of non-integer ids leaves: no ranks on the device yet)."""
    from video_quierer_amd.indexes.hnsw import MODE_AUTO, HNSWIndex
    idx = HNSWIndex.__new__(HNSWIndex)
    idx._h, idx.dimension, idx.lock, idx.search_mode, idx.search_times = None, dimension, threading.RLock(), MODE_AUTO, []
    idx._reset_host_state()
    idx._ids.extend(ids)
    idx._row_of.update((nid, r) for r, nid in enumerate(idx._ids))
    idx._identity, idx._tie_order = identity, tie_order
    idx.element_count = len(idx._ids)
    idx.entry_point = idx._ids[0] if idx._ids else None
    return idx


def fill(ptr, values, start=0):
    """Write ``values`` through a ctypes pointer, from element ``start``."""
    for i, v in enumerate(values, start):
        ptr[i] = v


def nothing(*outs):
    """A canned search answer: no row at any rank (-1 in every integer output, inf in the distances)."""
    def answer(n):
        for ptr, empty in outs:
            fill(ptr, [empty] * n)
    return answer


# -- the default entry points: record the call as ("name", ...) and answer "nothing" ---------------------------------------
def _set_groups(calls, h, ptr, n, n_groups):
    calls.append(("set_groups", [ptr[i] for i in range(n)], n_groups))


def _set_id_ranks(calls, h, ptr, n):
    calls.append(("set_id_ranks", n))


def _set_positions(calls, h, ptr, n):
    calls.append(("set_positions", [ptr[i] for i in range(n)]))


def _remove_rows(calls, h, ptr, n):
    calls.append(("remove", [ptr[i] for i in range(n)]))


def _search(calls, h, q, nq, k, mode, ids, dist):
    calls.append(("search", k))
    nothing((ids, -1), (dist, np.inf))(nq * k)


def _search_grouped(calls, h, q, nq, k, mode, groups, rows, dist):
    calls.append(("search_grouped", k))
    nothing((groups, -1), (rows, -1), (dist, np.inf))(nq * k)


DEFAULTS = {"vq_index_set_groups": _set_groups, "vq_index_set_id_ranks": _set_id_ranks, "vq_index_set_positions": _set_positions,
            "vq_index_remove_rows": _remove_rows, "vq_index_search": _search, "vq_index_search_grouped": _search_grouped}


def fake_lib(monkeypatch, **entry_points):
    """Put a recording library in place of libvq_amd and return its list of calls.  Every entry point is a function
    ``f(calls, *c_arguments)`` that appends what the test wants to see and fills the outputs; it succeeds (returns 0) unless it
    returns something else.  ``entry_points`` (``vq_index_search_set=...``) are added to DEFAULTS or replace one of them; an
    entry point nobody gave is an AttributeError, so a test also pins which calls are NOT made."""
    from video_quierer_amd import _lib
    calls = []

    class FakeLib:
        pass

    def bind(fn):
        def call(*args):
            rc = fn(calls, *args)
            return 0 if rc is None else rc
        return call

    lib = FakeLib()
    for name, fn in {**DEFAULTS, **entry_points}.items():
        setattr(lib, name, bind(fn))
    monkeypatch.setattr(_lib, "load", lambda: lib)
    return calls


def ranked_search(rows, dists):
    """``vq_index_search`` over an index whose exhaustive answer to every query is ``rows`` at ``dists`` (ascending): a call
    with k gets the first k of them; recorded as ("search", nq, k, mode)."""
    def entry(calls, h, q, nq, k, mode, ids, dist):
        calls.append(("search", nq, k, mode))
        for j in range(nq):
            fill(ids, (list(rows) + [-1] * k)[:k], j * k)
            fill(dist, (list(dists) + [np.inf] * k)[:k], j * k)
    return entry


def fake_device(monkeypatch, **entry_points):
    """``fake_lib`` for tests in which an ``HNSWIndex`` is really constructed (``SimpleVideoIndex`` builds its own): no GPU is
    bound, creation succeeds, and appended blocks are recorded as ("add", rows, normalize)."""
    from video_quierer_amd import _lib
    monkeypatch.setattr(_lib, "init", lambda device=None: 0)

    def add(calls, h, ptr, n, normalize):
        calls.append(("add", n, normalize))

    return fake_lib(monkeypatch, vq_index_create=lambda calls, dim, h: None, vq_index_add=add, **entry_points)


# -- shared by the GPU suites of the search families ------------------------------------------------------------------------
def unit(qs):
    return np.stack([q / np.linalg.norm(q) for q in qs]).astype(np.float32)


def tie_ranks(ids):
    """Each row's position in the id order (what ``sorted((distance, id))`` falls back to on equal distances)."""
    order = sorted(range(len(ids)), key=ids.__getitem__)
    rank = np.empty(len(ids), dtype=np.int64)
    rank[order] = np.arange(len(ids))
    return rank
