"""Drop-in for the reference's ``indexes.hnsw`` module (reference
src/indexes/hnsw.py): ``HNSWIndex`` / ``OptimizedHNSWIndex`` with the same
constructor, methods, result dicts and pickle layout — but ``search`` is an
EXACT scan of a device-resident matrix in libvq_amd (no graph walk), i.e. what
the reference itself returns once ``ef_search >= N``:

    distance_i = fp32(1 - fp32(dot(x_i, q))),  k smallest by (distance, id).

The graph parameters (M, ef_construction, ef_search, max_M,
level_generation_factor) are accepted and echoed by ``get_stats`` but have no
effect.  There is no CPU path: without the library or a gfx950 device
construction raises.
"""
from __future__ import annotations

import ctypes
import hashlib
import math
import os
import pickle
import threading
import time
from collections.abc import Iterable, Mapping
from concurrent.futures import ThreadPoolExecutor
from itertools import compress
from ctypes import c_float, c_int64, c_void_p
from typing import Callable, Dict, Hashable, List, Optional, Sequence, Tuple

import numpy as np

from video_quierer_amd import _lib

MODE_AUTO, MODE_EXACT, MODE_FP16 = 0, 1, 2
GROUP_OF = Optional[Callable[[Hashable], Hashable]]      # node id -> group key (None: video_of)
POSITION_OF = Optional[Callable[[Hashable], int]]        # node id -> integer position (None: frame_of)


def video_of(node_id: Hashable) -> Hashable:
    """The default group of a node id for ``search_grouped``: the reference caller's frame ids are ``f"{video_id}_{i}"``
    (video_search_system.py:164-166), so a string id's video is everything before its LAST underscore (video ids may
    contain ``_``); any other id is its own group."""
    return node_id.rsplit("_", 1)[0] if isinstance(node_id, str) else node_id


def frame_of(node_id: Hashable) -> int:
    """The default position of a node id for ``search_distinct``: the integer after the LAST underscore of a string id (the
    reference caller's ``f"{video_id}_{i}"``), or an int id itself.  Anything else is a ``ValueError`` naming the id."""
    if isinstance(node_id, (int, np.integer)) and not isinstance(node_id, bool):
        return int(node_id)
    if isinstance(node_id, str) and "_" in node_id:
        try:
            return int(node_id.rsplit("_", 1)[1])
        except ValueError:
            pass
    raise ValueError(f"frame_of: id {node_id!r} carries no frame number (pass position_of=)")


class _RowState:
    """Per-row int32 state derived from the ids through a caller's mapping (group labels, positions) and mirrored on the device.
    Kept like the tie order: only rows added since the last call are mapped, the first search that needs the state after an add
    or a removal uploads it; another mapping or another id list (``load``) maps everything again.  Never saved."""

    def __init__(self, fn: Callable[[Hashable], Hashable], ids: List[Hashable]):
        self.fn, self.ids = fn, ids
        self.values = np.empty(0, dtype=np.int32)
        self.uploaded = -1                        # rows the device copy covers

    @classmethod
    def current(cls, held, fn, ids):
        """``held`` while it belongs to this mapping and this id list (an add only appends to the list), else a fresh state."""
        if held is not None and held.fn is fn and held.ids is ids and len(held.values) <= len(ids):
            return held
        return cls(fn, ids)

    def extend(self) -> bool:
        """Map the rows added since the last call; True when the device copy is stale."""
        n = len(self.ids)
        if len(self.values) < n:
            self.values = np.concatenate([self.values, self._map(self.ids[len(self.values):])])
        return self.uploaded != n

    def sync(self, h):
        """``extend``, and upload when the device copy is stale."""
        if self.extend():
            _lib.check(self._upload(h, _lib.i32ptr(self.values), len(self.values)))
            self.uploaded = len(self.values)
        return self


class _Positions(_RowState):
    """int32 positions of the rows for ``vq_index_set_positions``."""

    def _map(self, ids) -> np.ndarray:
        fn = self.fn
        new = np.array([int(fn(nid)) for nid in ids], dtype=np.int64)
        if len(new) and (new.min() < -2 ** 31 or new.max() >= 2 ** 31):
            raise ValueError("positions must fit a 32-bit signed integer")
        return new.astype(np.int32)

    def _upload(self, h, ptr, n):
        return _lib.load().vq_index_set_positions(h, ptr, n)

    def compact(self, keep: np.ndarray) -> None:
        """The positions of the surviving rows; vq_index_remove_rows drops the device's, so an upload is due."""
        self.values = self.values[keep]
        self.uploaded = -1


class _GroupLabels(_RowState):
    """Dense int labels of the rows for ``vq_index_set_groups``: group keys are numbered in the order in which they first appear."""

    def __init__(self, fn, ids):
        super().__init__(fn, ids)
        self.index: Dict[Hashable, int] = {}
        self.keys: List[Hashable] = []

    @property
    def labels(self) -> np.ndarray:
        return self.values

    def _map(self, ids) -> np.ndarray:
        index, keys, fn = self.index, self.keys, self.fn
        new = np.empty(len(ids), dtype=np.int32)
        for j, nid in enumerate(ids):
            key = fn(nid)
            g = index.get(key)
            if g is None:
                g = index[key] = len(keys)
                keys.append(key)
            new[j] = g
        return new

    def _upload(self, h, ptr, n):
        return _lib.load().vq_index_set_groups(h, ptr, n, len(self.keys))

    def compact(self, keep: np.ndarray, current: bool) -> None:
        """The labels of the surviving rows (``keep`` = per-row mask), renumbered as vq_index_remove_rows renumbers the device
        labels: groups left without rows are dropped, the others keep their order.  ``current``: the device held these labels
        for every row before the removal (it then keeps them, renumbered, and no upload is due)."""
        labels = self.values[keep]
        alive = np.bincount(labels, minlength=len(self.keys)) > 0
        self.values = (np.cumsum(alive, dtype=np.int64) - 1)[labels].astype(np.int32)
        if not alive.all():
            self.keys = [key for key, a in zip(self.keys, alive.tolist()) if a]
            self.index = {key: g for g, key in enumerate(self.keys)}
        self.uploaded = len(self.values) if current else -1


_ONE = np.float32(1.0)


def _scored(d: np.float32) -> Dict:
    """The tail of every result dict: the scan's distance and the score the reference derives from it (hnsw.py:271-277)."""
    return {"distance": d, "score": _ONE - d}


def _hits(to_id, rows: List[int], dist: np.ndarray) -> List[Dict]:
    """One query's ``[{'id', 'distance', 'score'}]`` from its row numbers (a list; -1 = no row) and distances."""
    return [{"id": to_id(r), **_scored(d)} for r, d in zip(rows, dist) if r >= 0]


def host_tie_order(run, kk: int, n: int, tie_key, finite_only: bool = False) -> List[List]:
    """The (distance, id) order where the device cannot give it (it orders equal distances by row): ``run(fetch)`` returns the
    (rows, distances) of the ``fetch`` best rows per query; fetch more than ``kk`` until no group of equal distances is cut at
    rank ``kk`` (``n`` rows can come back at the most), then sort every query's candidates by ``(distance, tie_key(row))`` on
    the host.  Returns the first ``kk`` pairs per query.  ``finite_only``: a run of inf (fewer than kk rows allowed) is no tie."""
    fetch = min(n, kk + 8)
    while True:
        rows, dist = run(fetch)
        cut = dist[:, kk - 1] == dist[:, fetch - 1]
        if finite_only:
            cut &= np.isfinite(dist[:, kk - 1])
        if fetch >= n or not np.any(cut):
            break
        fetch = min(n, fetch * 2)
    return [sorted((d, tie_key(r)) for r, d in zip(rr, rd) if r >= 0)[:kk] for rr, rd in zip(rows.tolist(), dist)]


class _RowView(Mapping):
    """Read-only ``id -> stored row`` view of an index (``HNSWIndex.data``)."""

    def __init__(self, index):
        self._index = index

    def __len__(self):
        return len(self._index._ids)

    def __iter__(self):
        return iter(self._index._ids)

    def __contains__(self, node_id):
        return node_id in self._index._row_of

    def __getitem__(self, node_id):
        idx = self._index
        with idx.lock:
            row = idx._row_of[node_id]                       # KeyError for an unknown id, as a dict would
            out = np.empty((1, idx.dimension), dtype=np.float32)
            rn = (ctypes.c_int64 * 1)(row)
            _lib.check(_lib.load().vq_index_read_rows(idx._h, rn, 1, _lib.fptr(out)))
        return out[0]

    def items(self):
        rows = self._index._export()
        return [(i, rows[r]) for r, i in enumerate(self._index._ids)]

    def values(self):
        rows = self._index._export()
        return [rows[r] for r in range(len(self._index._ids))]


class HNSWIndex:
    def __init__(self, dimension: int = 512, M: int = 16, ef_construction: int = 200, ef_search: int = 50,
                 max_M: int = 16, level_generation_factor: float = 1.0 / math.log(2.0), num_threads: int = 4,
                 device: Optional[int] = None):
        # reference :25-57
        self.dimension = dimension
        self.M = M
        self.max_M = max_M
        self.ef_construction = ef_construction
        self.ef_search = ef_search
        self.level_generation_factor = level_generation_factor
        self.num_threads = num_threads

        self.entry_point = None
        self.element_count = 0
        self.lock = threading.RLock()
        self.thread_pool = ThreadPoolExecutor(max_workers=num_threads)
        self.build_time = 0
        self.search_times: List[float] = []
        self.search_mode = MODE_AUTO

        self._reset_host_state()
        _lib.init(device)
        h = c_void_p()
        _lib.check(_lib.load().vq_index_create(int(dimension), ctypes.byref(h)))
        self._h = h

    def _reset_host_state(self) -> None:
        """All the host knows about the rows of an empty index (``__init__``, ``load``)."""
        self._ids: List[Hashable] = []            # row -> caller id
        self._row_of: Dict[Hashable, int] = {}    # caller id -> row
        self._identity = True                     # ids are exactly 0..n-1 in row order
        # (distance, id) tie order on the device (vq_index_set_id_ranks): "stale" until the ranks of the current ids
        # have been uploaded, "device" afterwards, "host" when the ids cannot be put in one order (see _sync_tie_order)
        self._tie_order = "device"
        self._groups, self._positions = None, None

    # derived per-row state of the grouped / distinct searches, made by the first search that needs it (_sync_groups,
    # _sync_positions).  Declared on the class as well, so an index that was never given any (one made without __init__)
    # reads "none yet" like a fresh one.
    _groups: Optional[_GroupLabels] = None
    _positions: Optional[_Positions] = None

    # -- reference-shaped views of the state (hnsw.py:44-49) ---------------------
    @property
    def data(self) -> "Mapping[Hashable, np.ndarray]":
        """The reference's ``self.data`` dict (id -> stored unit vector, hnsw.py:44) as a read-only view of the device matrix:
        a lookup fetches that one row, iteration / ``len`` / ``in`` touch no device memory, ``items()`` / ``values()`` / ``dict(...)``
        export the matrix once.  (Round 2 exported every row on every access.)"""
        return _RowView(self)

    @property
    def levels(self) -> Dict[Hashable, int]:
        return {i: 0 for i in self._ids}          # exact index: a single flat level

    @property
    def graph(self) -> dict:
        return {0: {i: set() for i in self._ids}}

    def _export(self) -> np.ndarray:
        n = len(self._ids)
        rows = np.empty((n, self.dimension), dtype=np.float32)
        if n:
            _lib.check(_lib.load().vq_index_export(self._h, _lib.fptr(rows)))
        return rows

    # -- build --------------------------------------------------------------------
    @staticmethod
    def _unit(vector) -> np.ndarray:
        v = np.asarray(vector)
        return (v / np.linalg.norm(v)).astype(np.float32, copy=False)     # hnsw.py:157 (no zero guard)

    @classmethod
    def _unit_rows(cls, vectors) -> np.ndarray:
        """Row-wise ``v / np.linalg.norm(v)`` for a block (reference :157, :250) with the per-row Python loop taken out.
        For a 1-D float32 vector ``np.linalg.norm`` is ``sqrt(v.dot(v))`` — BLAS sdot; ``np.matmul`` of a stack of
        (1, d) @ (d, 1) products runs that same dot per row, so the norms (and ``v / norm`` in float32) are the reference's
        bits, 6x faster than the loop.  That equivalence is numpy's implementation, not its contract: a sample of rows (a
        fixed spread + 16 random ones per call) is checked against ``np.linalg.norm`` on every call and any difference (or
        any other dtype) takes the per-row loop.  A SAMPLE: "stored rows == reference .data" is asserted on whole matrices
        by the golden tests (1k rows bit for bit, sha256 of all rows at 10k and 100k), not by this guard."""
        vs = vectors if isinstance(vectors, np.ndarray) else None
        if vs is None:
            try:
                vs = np.asarray(vectors)
            except ValueError:
                vs = None
        if vs is None or vs.ndim != 2 or vs.dtype != np.float32 or vs.shape[0] < 8:
            return np.stack([cls._unit(v) for v in vectors])
        vs = np.ascontiguousarray(vs)
        with np.errstate(invalid="ignore", divide="ignore"):
            norms = np.sqrt(np.matmul(vs[:, None, :], vs[:, :, None]).reshape(-1))
            n = vs.shape[0]
            # a fixed spread of rows plus a fresh random set on every call: the equivalence is sampled, not proven — a row
            # outside both sets that differed would go unnoticed (numpy would have to pick another kernel for some rows of ONE
            # matmul: its batched (1, d) @ (d, 1) loop calls the same dot per row), which is why every golden test also
            # compares the stored rows with the reference's `.data` bit for bit, whole matrices, sha256 at 10k / 100k rows
            probe = np.unique(np.concatenate([[0, n - 1], np.linspace(0, n - 1, 16).astype(np.int64),
                                              np.random.default_rng().integers(0, n, 16)]))
            for i in probe:
                ref = np.linalg.norm(vs[i])
                if not (norms[i] == ref or (np.isnan(norms[i]) and np.isnan(ref))):
                    return np.stack([cls._unit(v) for v in vs])
            return vs / norms[:, None]

    @staticmethod
    def _ids_are_rows(ids: Sequence[Hashable], base: int) -> bool:
        """Are `ids` exactly base, base + 1, ... (integers)?  Ids are any hashable: a ragged mix (tuples of different lengths, a
        str beside a tuple) makes ``np.asarray`` raise — that is simply "no"."""
        if not ids or not isinstance(ids[0], (int, np.integer)) or not isinstance(ids[-1], (int, np.integer)):
            return False
        if isinstance(ids, range):
            return ids.step == 1 and ids.start == base
        try:
            arr = np.asarray(ids)
        except (ValueError, TypeError):
            return False
        return bool(arr.ndim == 1 and arr.dtype.kind in "iu" and np.array_equal(arr, np.arange(base, base + len(ids))))

    def _sync_tie_order(self) -> None:
        """The reference returns ``sorted(candidates)[:k]`` over (distance, id) tuples (hnsw.py:269 / :518): rows at equal
        distance come back in id order.  The device orders by (distance, rank of the row's id) once it has the ranks
        (vq_index_set_id_ranks); they are recomputed here, lazily, by the first search after new ids came in.  ``sorted``
        compares ids only where distances tie, so the reference tolerates ids that have no common order (an int beside a
        str) as long as no tie meets them; a global ranking cannot — such an index keeps the host-side path (over-fetch,
        re-sort per query)."""
        if self._tie_order != "stale":
            return
        ids = self._ids
        n = len(ids)
        order = None
        if type(ids[0]) is str and type(ids[-1]) is str and all(type(i) is str for i in ids):
            try:
                arr = np.array(ids)                                  # '<U..': numpy compares code points, as str does
                if arr.dtype.kind == "U" and arr.shape == (n,):
                    cand = np.argsort(arr, kind="stable")
                    srt = arr[cand]
                    if n < 2 or bool(np.all(srt[1:] > srt[:-1])):    # strict: two ids numpy cannot tell apart (trailing NULs) -> Python
                        order = cand
            except (ValueError, TypeError):
                order = None
        if order is None:
            try:
                order = np.fromiter(sorted(range(n), key=ids.__getitem__), dtype=np.int64, count=n)
            except TypeError:                                        # no total order over these ids
                _lib.check(_lib.load().vq_index_set_id_ranks(self._h, None, 0))
                self._tie_order = "host"
                return
        rank = np.empty(n, dtype=np.int32)
        rank[order] = np.arange(n, dtype=np.int32)
        _lib.check(_lib.load().vq_index_set_id_ranks(self._h, _lib.i32ptr(rank), n))
        self._tie_order = "device"

    def add(self, vector: np.ndarray, node_id: Hashable) -> None:
        self.add_batch([vector], [node_id])                               # reference :150-229

    def add_batch(self, vectors: Sequence[np.ndarray], node_ids: Sequence[Hashable]) -> None:
        """Reference :231-236 (a per-vector loop there); here one device append."""
        node_ids = list(node_ids)
        n = min(len(vectors), len(node_ids))                              # zip semantics
        if n == 0:
            return
        t0 = time.time()
        with self.lock:
            vs = np.asarray(vectors[:n] if not isinstance(vectors, np.ndarray) else vectors[:n])
            if vs.ndim != 2 or vs.shape[1] != self.dimension:
                raise ValueError(f"vectors must be [n,{self.dimension}], got {vs.shape}")
            # row-wise `v / np.linalg.norm(v)` exactly as the reference computes it (:157)
            unit = self._unit_rows(vs)
            unit = np.ascontiguousarray(unit, dtype=np.float32)
            ids_n = node_ids[:n]
            if self._row_of.keys().isdisjoint(ids_n) and len(set(ids_n)) == n:
                # the ingest case (video_search_system.py:168-176: every frame id is new): no per-id walk
                self._append_stored(unit, ids_n)
            else:
                fresh_rows, fresh_ids = [], []
                upd_rows, upd_src = [], []                               # re-added ids: (stored row, batch position), in call order
                seen_now: Dict[Hashable, int] = {}
                for j, nid in enumerate(ids_n):
                    if nid in self._row_of:
                        upd_rows.append(self._row_of[nid]); upd_src.append(j)
                    elif nid in seen_now:                                # later duplicate wins (dict semantics)
                        fresh_rows[seen_now[nid]] = j
                    else:
                        seen_now[nid] = len(fresh_rows)
                        fresh_rows.append(j)
                        fresh_ids.append(nid)
                if upd_rows:
                    self._overwrite(upd_rows, unit if len(upd_src) == n else np.ascontiguousarray(unit[upd_src]))
                if fresh_rows:
                    self._append_stored(unit if len(fresh_rows) == n else np.ascontiguousarray(unit[fresh_rows]), fresh_ids)
                self.element_count += n - len(fresh_ids)                  # reference counts every add (:229), re-adds included
        self.build_time += time.time() - t0

    def add_device(self, d_rows: int, n: int, node_ids: Sequence[Hashable], normalize: bool = True) -> None:
        """Append n device-resident fp32 rows (e.g. straight from the encoder) without a host round trip."""
        node_ids = list(node_ids)
        if len(node_ids) != n:
            raise ValueError("node_ids must have n entries")
        with self.lock:
            if not self._row_of.keys().isdisjoint(node_ids) or len(set(node_ids)) != n:
                raise ValueError("add_device: ids must be new and unique")
            _lib.check(_lib.load().vq_index_add_device(self._h, c_void_p(d_rows), n, int(bool(normalize))))
            self._commit_rows(node_ids)

    def _append_stored(self, rows: np.ndarray, node_ids: Sequence[Hashable]) -> None:
        """Append a block of fp32 rows stored AS GIVEN (the library measures them, vq_index_add normalize=0; a block that is
        not unit-norm still searches exactly, on the fp32 scan) under new, unique ids of the caller's choice."""
        node_ids = list(node_ids)
        with self.lock:
            _lib.check(_lib.load().vq_index_add(self._h, _lib.fptr(rows), len(node_ids), 0))
            self._commit_rows(node_ids)

    def _commit_rows(self, node_ids: List[Hashable]) -> None:
        """The host's side of an append: ``node_ids`` (new, unique) name the rows the device just added at its end."""
        base = len(self._ids)
        identity = self._identity and self._ids_are_rows(node_ids, base)     # decided before anything changes
        self._row_of.update(zip(node_ids, range(base, base + len(node_ids))))     # (a per-id loop here cost 45 ms per 250k rows)
        self._ids.extend(node_ids)
        self._identity = identity
        if not identity:
            self._tie_order = "stale"
        self.element_count += len(node_ids)                               # reference counts every add (:229)
        if self.entry_point is None:
            self.entry_point = self._ids[0]

    def _replace_ids(self, node_ids: List[Hashable]) -> None:
        """Rename every row (a caller whose ids are positions renumbers them after a removal).  The new ids must sort as the old
        ones did: ranks, labels and positions on the device stay as they are."""
        with self.lock:
            if len(node_ids) != len(self._ids):
                raise ValueError("_replace_ids: one id per row")
            self._ids[:] = node_ids                                       # in place: the derived state holds this list
            self._row_of = {nid: r for r, nid in enumerate(node_ids)}
            self.entry_point = node_ids[0] if node_ids else None

    def _overwrite(self, rows: Sequence[int], unit_vecs: np.ndarray) -> None:
        """Re-adding an id replaces its vector (a dict assignment in the reference, hnsw.py:160): the stored rows are
        replaced in place on the device — fp32 master, fp16 scan copy, norm range — in one call; a row named twice
        keeps its last vector, as sequential assignments would leave it."""
        rn = np.ascontiguousarray(rows, dtype=np.int64)
        _lib.check(_lib.load().vq_index_update_rows(self._h, _lib.fptr(unit_vecs), _lib.i64ptr(rn), len(rn), 0))

    # -- removal (reference: `del self.data[node_id]`; video_search_system.py:427-463 delete_video) -------------------
    def remove(self, node_id: Hashable) -> None:
        """Take one id out of the index; ``KeyError`` for an unknown id, as ``del`` on the reference's ``data`` dict."""
        self.remove_batch([node_id])

    def remove_batch(self, node_ids: Sequence[Hashable]) -> int:
        """Take the given ids out of the index, all or none: an unknown id raises ``KeyError`` before anything changes.  An id
        named twice is removed once.  The survivors keep their order; returns the number of rows removed."""
        with self.lock:
            row_of = self._row_of
            rows = np.fromiter({row_of[nid] for nid in node_ids}, dtype=np.int64)
            return self._remove_rows(np.sort(rows))

    def remove_group(self, group: Hashable, group_of: GROUP_OF = None) -> int:
        """Take every row of one group out (default ``video_of``: the caller's ``delete_video(video_id)``); returns the number
        of rows removed (0 for a group the index does not hold).  The rows are found through the host group labels."""
        with self.lock:
            rows = self._group_rows(group, group_of)
            return 0 if rows is None else self._remove_rows(rows)

    def _group_rows(self, group: Hashable, group_of: GROUP_OF) -> Optional[np.ndarray]:
        """The rows of one group, ascending, through the host labels (nothing is uploaded); None for a group the index lacks."""
        gl = self._group_labels(group_of)
        gl.extend()
        g = gl.index.get(group)
        return None if g is None else np.flatnonzero(gl.labels == g).astype(np.int64)

    def _remove_rows(self, rows: np.ndarray) -> int:
        """rows: sorted, unique, valid row numbers.  The device compacts the matrix, the id ranks and the group labels
        (vq_index_remove_rows); the host follows: ``_ids`` in place, ``_row_of`` for the rows that moved, the group labels
        renumbered the same way, so neither the next search nor the next grouped search uploads anything."""
        m = len(rows)
        if m == 0:
            return 0
        ids = self._ids
        n = len(ids)
        # derived state of a replaced id list is mapped again on its next use; the rest gets every row mapped (no upload)
        gl, ps = (st if st is not None and st.ids is ids else None for st in (self._groups, self._positions))
        for st in (gl, ps):
            if st is not None:
                st.extend()
        current = gl is not None and gl.uploaded == n
        rows = np.ascontiguousarray(rows, dtype=np.int64)
        _lib.check(_lib.load().vq_index_remove_rows(self._h, _lib.i64ptr(rows), m))
        keep = np.ones(n, dtype=bool)
        keep[rows] = False
        first = int(rows[0])
        row_of = self._row_of
        for r in rows.tolist():
            del row_of[ids[r]]
        tail = list(compress(ids[first:], keep[first:].tolist()))
        ids[first:] = tail                                       # in place: the group labels hold this list
        row_of.update(zip(tail, range(first, first + len(tail))))
        # ids 0..n-1 lose that property once a survivor moves; they still increase with the row, so ties keep coming back in id
        # order without ranks
        self._identity = self._identity and not tail
        self.element_count -= m
        self.entry_point = ids[0] if ids else None
        if gl is not None:
            gl.compact(keep, current)
        if ps is not None:
            ps.compact(keep)
        return m

    # -- query --------------------------------------------------------------------
    def _raw_search(self, unit_queries: np.ndarray, k: int):
        nq = unit_queries.shape[0]
        ids = np.empty((nq, k), dtype=np.int32)
        dist = np.empty((nq, k), dtype=np.float32)
        _lib.check(_lib.load().vq_index_search(self._h, _lib.fptr(unit_queries), nq, k, int(self.search_mode),
                                               _lib.i32ptr(ids), _lib.fptr(dist)))
        return ids, dist

    def _id_of(self):
        """The function that maps a row number to the caller's id."""
        return int if self._identity else self._ids.__getitem__

    def _host_ties(self) -> bool:
        """Do the ids lack a common order (``_sync_tie_order`` has run), so that (distance, id) is established on the host?"""
        return not self._identity and self._tie_order != "device"

    def _search_many(self, queries: Sequence[np.ndarray], k: int) -> List[List[Dict]]:
        # the plain search is the latency path (one synchronous call per query in the reference caller): its few steps are
        # spelt out here instead of going through _prepare
        n = len(self._ids)
        unit = np.ascontiguousarray(self._unit_rows(queries), dtype=np.float32)
        if unit.shape[1] != self.dimension:
            raise ValueError(f"query dimension {unit.shape[1]} != index dimension {self.dimension}")
        kk = min(k, n)
        if kk <= 0:
            return [[] for _ in queries]          # reference: sorted(candidates)[:0] == [] (hnsw.py:269)
        if not self._identity:
            self._sync_tie_order()
        if self._host_ties():
            # ids without a common order: the library orders ties by row, the reference by id (hnsw.py:269/518)
            best = host_tie_order(lambda fetch: self._raw_search(unit, fetch), kk, n, self._ids.__getitem__)
            return [[{"id": i, **_scored(d)} for d, i in cand] for cand in best]
        # row numbers, or the caller's ids (strings f"{video_id}_{i}", video_search_system.py:164-166) with their ranks on the
        # device: it already ordered by (distance, id) — exactly k results fetched, rows mapped to ids, nothing re-sorted
        rows, dist = self._raw_search(unit, kk)
        to_id = self._id_of()
        return [_hits(to_id, rr, rd) for rr, rd in zip(rows.tolist(), dist)]

    def search(self, query: np.ndarray, k: int = 5) -> List[Dict]:
        """Reference :238-280 / :488-528."""
        if self.entry_point is None or self.element_count == 0:
            return []
        t0 = time.time()
        with self.lock:
            res = self._search_many([query], k)[0]
        self.search_times.append((time.time() - t0) * 1000)
        return res

    def search_batch(self, queries: List[np.ndarray], k: int = 5) -> List[List[Dict]]:
        """Reference :282-300 (a thread fan-out serialised by the index lock); here one batched scan."""
        if len(queries) == 0:
            return []
        if self.entry_point is None or self.element_count == 0:
            return [[] for _ in queries]
        t0 = time.time()
        with self.lock:
            res = self._search_many(queries, k)
        per = (time.time() - t0) * 1000 / len(queries)
        self.search_times.extend([per] * len(queries))
        return res

    def search_device(self, d_queries: int, nq: int, k: int, d_ids: int, d_dist: int, mode: Optional[int] = None) -> None:
        """Device pointers in/out (unit fp32 queries; int32 ROW numbers; fp32 distances); asynchronous.  Rows at equal
        distance come back in the order of their ids (as `search` returns them) unless the ids have no common order."""
        with self.lock:
            if not self._identity:
                self._sync_tie_order()
            _lib.check(_lib.load().vq_index_search_device(self._h, c_void_p(d_queries), int(nq), int(k),
                                                          int(self.search_mode if mode is None else mode),
                                                          c_void_p(d_ids), c_void_p(d_dist)))

    # -- what every other search family does before its C call ------------------------------------------------------------
    def _empty(self) -> bool:
        return self.entry_point is None or self.element_count == 0

    def _group_labels(self, group_of: GROUP_OF) -> _GroupLabels:
        """The host's labels under ``group_of`` (default ``video_of``); nothing is mapped or uploaded yet."""
        self._groups = _GroupLabels.current(self._groups, video_of if group_of is None else group_of, self._ids)
        return self._groups

    def _sync_groups(self, group_of: GROUP_OF) -> _GroupLabels:
        return self._group_labels(group_of).sync(self._h)

    def _sync_positions(self, position_of: POSITION_OF) -> _Positions:
        self._positions = _Positions.current(self._positions, frame_of if position_of is None else position_of, self._ids)
        return self._positions.sync(self._h)

    @staticmethod
    def _filter_arg(within, exclude, required: bool = False) -> Optional[Tuple[List[Hashable], bool]]:
        """(group keys, exclude?) of a ``within`` / ``exclude`` pair, each an iterable of keys; None when neither is given."""
        if within is None and exclude is None and not required:
            return None
        if (within is None) == (exclude is None):
            raise ValueError("give exactly one of `within` and `exclude` (an iterable of group keys)")
        keys = within if within is not None else exclude
        if isinstance(keys, (str, bytes)) or not isinstance(keys, Iterable):
            raise ValueError("`within` / `exclude` take an iterable of group keys (a list of video ids), not one key")
        return list(keys), exclude is not None

    def _prepare(self, queries, k: int, *, given: bool = False, group_of: GROUP_OF = None, positions: bool = False,
                 position_of: POSITION_OF = None, flt: Optional[Tuple[List[Hashable], bool]] = None, what: str = "query",
                 groups: bool = True):
        """The common start of the grouped, filtered, distinct, clip and sequence searches, under the lock, in the order the
        callers rely on: the queries normalised as ``search`` does (``given``: fp32 [nq][dim], used as they are), their
        dimension checked; then the answers that need no device (k <= 0, an empty index, an empty ``within``: None is
        returned and the caller answers empty); then the device is given what the C call needs: the tie order, the group
        labels under ``group_of``, the positions under ``position_of`` if asked for, in that order, each uploaded only when
        stale.  ``flt`` (``_filter_arg``) becomes the ascending labels of the keys the index holds (unknown keys hold no
        rows); a ``within`` that names none of them is None again, after the uploads.  Without ``flt`` nothing is excluded.
        ``groups=False`` (a call that reads neither labels nor ranks: ``label_rows``) maps and uploads neither; its group labels are None.
        Returns (unit queries, group labels, positions or None, filter labels, exclude flag)."""
        unit = queries if given else np.ascontiguousarray(self._unit_rows(queries), dtype=np.float32)
        if unit.shape[1] != self.dimension:
            raise ValueError(f"{what} dimension {unit.shape[1]} != index dimension {self.dimension}")
        keys, excl = flt if flt is not None else ((), True)
        if k <= 0 or not self._ids or (not excl and not keys):
            return None
        gl = None
        if groups:
            if not self._identity:
                self._sync_tie_order()
            gl = self._sync_groups(group_of)
        ps = self._sync_positions(position_of) if positions else None
        index = gl.index if gl is not None else {}
        labels = np.array(sorted({index[key] for key in keys if key in index}), dtype=np.int32)
        if not excl and len(labels) == 0:
            return None
        return unit, gl, ps, labels, excl

    # -- grouped query: the k best videos, one best frame each ----------------------------
    def search_grouped(self, query: np.ndarray, k: int = 5, group_of: GROUP_OF = None, *,
                       within: Optional[Iterable[Hashable]] = None, exclude: Optional[Iterable[Hashable]] = None) -> List[Dict]:
        """The k best GROUPS (videos) for one query, each with its best row: ``[{'group', 'id', 'distance', 'score'}]``.
        Exactly the plain search's exhaustive (distance, id) list with every row dropped whose group came earlier — what
        video_search_system.py:296-342 builds from ``search(q, k * 2)`` (it returns fewer than k videos once the top 2k
        frames span fewer than k of them; this never does while the index holds k groups).  ``group_of`` maps a node id to
        its group key (default ``video_of``: the caller's ``f"{video_id}_{i}"`` convention); a caller holding the metadata
        passes ``lambda nid: meta[nid]['video_id']`` — keep passing the SAME callable, a different one relabels every row.
        ``within`` / ``exclude`` (at most one, an iterable of group keys) restrict the search to those groups or to all the
        others, exactly as ``search_filtered`` does."""
        return self.search_grouped_batch([query], k, group_of, within=within, exclude=exclude)[0]

    def search_grouped_batch(self, queries: List[np.ndarray], k: int = 5, group_of: GROUP_OF = None, *,
                             within: Optional[Iterable[Hashable]] = None,
                             exclude: Optional[Iterable[Hashable]] = None) -> List[List[Dict]]:
        """``search_grouped`` for a batch of queries, one device pass."""
        flt = self._filter_arg(within, exclude)
        if len(queries) == 0:
            return []
        if self._empty():
            return [[] for _ in queries]
        with self.lock:
            ready = self._prepare(queries, k, group_of=group_of, flt=flt)
            if ready is None:
                return [[] for _ in queries]
            unit, gl, _, labels, excl = ready
            nq, kk = unit.shape[0], min(int(k), len(gl.keys))
            groups = np.empty((nq, kk), dtype=np.int32)
            rows = np.empty((nq, kk), dtype=np.int32)
            dist = np.empty((nq, kk), dtype=np.float32)
            out = _lib.i32ptr(groups), _lib.i32ptr(rows), _lib.fptr(dist)
            if flt is None:
                _lib.check(_lib.load().vq_index_search_grouped(self._h, _lib.fptr(unit), nq, kk, int(self.search_mode), *out))
            else:
                _lib.check(_lib.load().vq_index_search_grouped_filtered(self._h, _lib.fptr(unit), nq, kk, int(self.search_mode),
                                                                        _lib.i32ptr(labels), len(labels), int(excl), *out))
            keys, to_id = gl.keys, self._id_of()
            return [[{"group": keys[g], "id": to_id(r), **_scored(d)} for g, r, d in zip(rg, rr, rd) if r >= 0]
                    for rg, rr, rd in zip(groups.tolist(), rows.tolist(), dist)]

    # -- distinct moments: the k best rows, two of one group at least min_gap positions apart ------------
    def search_distinct(self, query: np.ndarray, k: int = 5, min_gap: int = 1, *, group_of: GROUP_OF = None,
                        position_of: POSITION_OF = None) -> List[Dict]:
        """The k best distinct MOMENTS for one query: ``[{'id', 'group', 'position', 'distance', 'score'}]``.  Exactly the plain
        search's exhaustive (distance, id) list, walked in order, with every row dropped that lies less than ``min_gap``
        positions from an already kept row of the same group.  ``min_gap=0`` is ``search``; a gap above every position
        difference is ``search_grouped``'s rows.  ``group_of`` as ``search_grouped``; ``position_of`` maps a node id to an
        integer position that fits 32 bits (default ``frame_of``: the frame number of ``f"{video_id}_{i}"``; pass timestamps
        in ms and a gap in ms alike) — keep passing the SAME callables, a different one maps every row again."""
        return self.search_distinct_batch([query], k, min_gap, group_of=group_of, position_of=position_of)[0]

    def search_distinct_batch(self, queries: List[np.ndarray], k: int = 5, min_gap: int = 1, *, group_of: GROUP_OF = None,
                              position_of: POSITION_OF = None) -> List[List[Dict]]:
        """``search_distinct`` for a batch of queries, one device pass."""
        if int(min_gap) < 0:
            raise ValueError(f"min_gap must be >= 0, got {min_gap}")
        if len(queries) == 0:
            return []
        if self._empty():
            return [[] for _ in queries]
        with self.lock:
            return self._distinct_many(queries, k, int(min_gap), group_of, position_of)

    def _distinct_many(self, queries, k: int, min_gap: int, group_of, position_of, given: bool = False) -> List[List[Dict]]:
        """``given``: see ``_prepare`` (SimpleVideoIndex normalises by its own rule).  min_gap: checked."""
        ready = self._prepare(queries, k, given=given, group_of=group_of, positions=True, position_of=position_of)
        if ready is None:
            return [[] for _ in queries]
        unit, gl, ps, _, _ = ready
        nq, kk = unit.shape[0], min(int(k), len(self._ids))
        rows = np.empty((nq, kk), dtype=np.int32)
        dist = np.empty((nq, kk), dtype=np.float32)
        _lib.check(_lib.load().vq_index_search_distinct(self._h, _lib.fptr(unit), nq, kk, int(self.search_mode), min_gap,
                                                        _lib.i32ptr(rows), _lib.fptr(dist)))
        keys, labels, pos, to_id = gl.keys, gl.labels, ps.values, self._id_of()
        return [[{"id": to_id(r), "group": keys[labels[r]], "position": int(pos[r]), **_scored(d)} for r, d in zip(rr, rd) if r >= 0]
                for rr, rd in zip(rows.tolist(), dist)]

    # -- diverse search: the k best rows, no two of them closer than min_distance to each other ------------
    DIVERSE_MAX_K = 256

    def search_diverse(self, query: np.ndarray, k: int = 5, min_distance: float = 0.05) -> List[Dict]:
        """The k best frames that do not look alike: ``[{'id', 'distance', 'score'}]``, ``search``'s dicts.  Exactly the plain
        search's exhaustive (distance, id) list, walked in order, with every row dropped whose cosine distance to an already
        kept row is below ``min_distance`` (fp32, strict) — a static shot, an intro that sits in every episode or a bit-exact
        re-upload then takes one slot, whichever video the copies sit in.  ``min_distance=0`` is ``search``; at most 256
        results per query.  Needs neither groups nor positions."""
        return self.search_diverse_batch([query], k, min_distance)[0]

    def search_diverse_batch(self, queries: List[np.ndarray], k: int = 5, min_distance: float = 0.05) -> List[List[Dict]]:
        """``search_diverse`` for a batch of queries, one device pass."""
        min_dist = np.float32(min_distance)
        if not min_dist >= 0:                                     # (NaN too)
            raise ValueError(f"min_distance must be >= 0, got {min_distance}")
        if len(queries) == 0:
            return []
        if self._empty():
            return [[] for _ in queries]
        with self.lock:
            return self._diverse_many(queries, k, min_dist)

    def _diverse_many(self, queries, k: int, min_dist: np.float32, given: bool = False) -> List[List[Dict]]:
        """``given``: see ``_prepare`` (SimpleVideoIndex normalises by its own rule).  min_dist: checked."""
        ready = self._prepare(queries, k, given=given, groups=False)
        if ready is None:
            return [[] for _ in queries]
        if not self._identity:
            self._sync_tie_order()
        unit = ready[0]
        nq, kk = unit.shape[0], min(int(k), len(self._ids))
        rows = np.empty((nq, kk), dtype=np.int32)
        dist = np.empty((nq, kk), dtype=np.float32)
        _lib.check(_lib.load().vq_index_search_diverse(self._h, _lib.fptr(unit), nq, kk, int(self.search_mode), float(min_dist),
                                                       _lib.i32ptr(rows), _lib.fptr(dist)))
        to_id = self._id_of()
        return [_hits(to_id, rr, rd) for rr, rd in zip(rows.tolist(), dist)]

    # -- compound search: the k best rows that match ALL of several prompts, and none of the vetoed ones ------------
    COMPOUND_MAX_TERMS = 16

    @staticmethod
    def _compound_terms(all_of, none_of) -> Tuple[List[np.ndarray], np.ndarray]:
        """``all_of`` / ``none_of`` flattened into the C call's (term vectors, clause_of): an entry of ``all_of`` is one vector
        (a clause of one term) or a sequence of vectors (alternatives: any of them satisfies the clause); the veto terms of
        ``none_of`` follow with clause -1."""
        terms, clause_of = [], []
        for c, entry in enumerate(all_of):
            if len(entry) == 0:
                raise ValueError(f"clause {c} of all_of holds no vector")
            alts = [entry] if np.ndim(entry[0]) == 0 else list(entry)
            terms.extend(alts)
            clause_of.extend([c] * len(alts))
        if not terms:
            raise ValueError("search_compound needs at least one vector in all_of")
        for v in none_of:
            terms.append(v)
            clause_of.append(-1)
        if len(terms) > HNSWIndex.COMPOUND_MAX_TERMS:
            raise ValueError(f"a compound query holds at most {HNSWIndex.COMPOUND_MAX_TERMS} terms, got {len(terms)}")
        return terms, np.array(clause_of, dtype=np.int32)

    def search_compound(self, all_of, k: int = 5, *, none_of=(), margin: float = 0.0) -> List[Dict]:
        """The k best frames that match ALL of several prompts: ``search``'s dicts plus ``'term_distances'`` (float32 [m]: the
        frame's distance to every term, ``all_of``'s vectors in order, then ``none_of``'s — which term held the frame back).
        An entry of ``all_of`` is one vector, or a sequence of vectors that are alternatives for that clause.  A frame's
        distance is that of its WORST clause (the max over the clauses of the min over a clause's alternatives), so a frame
        that shows one prompt very well and another not at all does not beat a frame that shows both — what adding the
        prompt vectors cannot give.  A frame is struck when a ``none_of`` vector lies closer to it than that distance plus
        ``margin`` (float32, strict): ``margin=0`` drops frames that show the unwanted prompt better than the wanted
        combination, ``-inf`` drops nothing.  Every vector is normalised as ``search`` normalises its query; at most 16
        vectors in all.  Exact in every mode (vq_index_search_compound)."""
        terms, clause_of = self._compound_terms(all_of, none_of)
        mg = np.float32(margin)
        if mg != mg:
            raise ValueError("margin is NaN")
        if self._empty():
            return []
        with self.lock:
            return self._compound(terms, clause_of, k, mg)

    def _compound(self, terms, clause_of: np.ndarray, k: int, margin: np.float32, given: bool = False) -> List[Dict]:
        """``given``: see ``_prepare`` (SimpleVideoIndex normalises by its own rule).  clause_of, margin: checked."""
        ready = self._prepare(terms, k, given=given, groups=False, what="term")
        if ready is None:
            return []
        if not self._identity:
            self._sync_tie_order()
        unit = ready[0]
        m, kk = unit.shape[0], min(int(k), len(self._ids))
        rows = np.empty(kk, dtype=np.int32)
        dist = np.empty(kk, dtype=np.float32)
        td = np.empty((kk, m), dtype=np.float32)
        _lib.check(_lib.load().vq_index_search_compound(self._h, _lib.fptr(unit), m, _lib.i32ptr(clause_of), float(margin), kk,
                                                        int(self.search_mode), _lib.i32ptr(rows), _lib.fptr(dist), _lib.fptr(td)))
        to_id = self._id_of()
        return [{"id": to_id(r), **_scored(d), "term_distances": t} for r, d, t in zip(rows.tolist(), dist, td) if r >= 0]

    # -- filtered query: the plain search within, or excluding, a set of groups (videos) -------------
    def search_filtered(self, query: np.ndarray, k: int = 5, *, within: Optional[Iterable[Hashable]] = None,
                        exclude: Optional[Iterable[Hashable]] = None, group_of: GROUP_OF = None) -> List[Dict]:
        """``search`` restricted to the rows of some groups (videos): ``within=[video_id]`` searches inside one video,
        ``exclude=[video_of(frame_id)]`` finds more like a frame from the other videos, ``within=collection`` searches a set.
        Exactly one of ``within`` / ``exclude`` is given, as an iterable of group keys (``group_of`` as ``search_grouped``;
        unknown keys hold no rows).  The result is what ``search`` returns on an index holding only the allowed rows: the same
        dicts, distances and (distance, id) order, exact for any k however few rows the filter allows."""
        return self.search_filtered_batch([query], k, within=within, exclude=exclude, group_of=group_of)[0]

    def search_filtered_batch(self, queries: List[np.ndarray], k: int = 5, *, within: Optional[Iterable[Hashable]] = None,
                              exclude: Optional[Iterable[Hashable]] = None, group_of: GROUP_OF = None) -> List[List[Dict]]:
        """``search_filtered`` for a batch of queries (one filter for all of them), one device pass."""
        flt = self._filter_arg(within, exclude, required=True)
        if len(queries) == 0:
            return []
        if self._empty():
            return [[] for _ in queries]
        with self.lock:
            ready = self._prepare(queries, k, group_of=group_of, flt=flt)
            if ready is None:
                return [[] for _ in queries]                 # nothing allowed: no device call
            unit, _, _, labels, excl = ready
            nq, n = unit.shape[0], len(self._ids)
            kk = min(int(k), n)

            def run(fetch):
                rows = np.empty((nq, fetch), dtype=np.int32)
                dist = np.empty((nq, fetch), dtype=np.float32)
                _lib.check(_lib.load().vq_index_search_filtered(self._h, _lib.fptr(unit), nq, fetch, int(self.search_mode),
                                                                _lib.i32ptr(labels), len(labels), int(excl), _lib.i32ptr(rows),
                                                                _lib.fptr(dist)))
                return rows, dist

            if self._host_ties():                            # as _search_many; fewer than kk allowed rows end in inf: no tie
                best = host_tie_order(run, kk, n, self._ids.__getitem__, finite_only=True)
                return [[{"id": i, **_scored(d)} for d, i in cand] for cand in best]
            rows, dist = run(kk)
            to_id = self._id_of()
            return [_hits(to_id, rr, rd) for rr, rd in zip(rows.tolist(), dist)]

    # -- clip query: the k groups (videos) most similar to a SET of frames -------------------------
    SET_MAX_QUERIES = 4096        # vq_index_search_set: query frames per call

    def _search_set(self, queries, k: int, flt, group_of, matches: bool, given: bool = False) -> List[Dict]:
        """queries: at most SET_MAX_QUERIES frames (``given``: see ``_prepare``).  flt: ``_filter_arg``'s."""
        ready = self._prepare(queries, k, given=given, group_of=group_of, flt=flt)
        if ready is None:
            return []
        unit, gl, _, labels, excl = ready
        m, kk = unit.shape[0], min(int(k), len(gl.keys), 1024)
        groups = np.empty(kk, dtype=np.int32)
        dist = np.empty(kk, dtype=np.float32)
        rows = np.empty((kk, m), dtype=np.int32) if matches else None
        _lib.check(_lib.load().vq_index_search_set(self._h, _lib.fptr(unit), m, kk, int(self.search_mode), _lib.i32ptr(labels), len(labels),
                                                   int(excl), _lib.i32ptr(groups), _lib.fptr(dist), _lib.i32ptr(rows) if matches else None))
        keys, to_id = gl.keys, self._id_of()
        out = []
        for j, (g, d) in enumerate(zip(groups.tolist(), dist)):
            if g < 0:
                break
            out.append({"group": keys[g], **_scored(d)})
            if matches:
                out[-1]["matches"] = [to_id(r) for r in rows[j].tolist()]
        return out

    def search_set(self, queries: Sequence[np.ndarray], k: int = 5, *, within: Optional[Iterable[Hashable]] = None,
                   exclude: Optional[Iterable[Hashable]] = None, group_of: GROUP_OF = None, matches: bool = False) -> List[Dict]:
        """The k GROUPS (videos) most similar to a set of query frames (a clip, several example frames, several prompts):
        ``[{'group', 'distance', 'score'[, 'matches']}]``.  Every query frame (normalised as ``search`` does) takes its
        smallest distance to a row of the group; ``distance`` is the mean of those over the frames (added in fp64 in the
        frames' order, rounded once to float32), ``score = float32(1) - distance``; groups come back by (distance, order in
        which the groups first appeared in the index).  One-directional: the video's other frames cost nothing, so a short
        clip finds the long video it was cut from.  ``matches=True`` adds, per result, the node id of the matching row for
        every query frame (ties inside a group by id, as ``search``).  ``within`` / ``exclude`` / ``group_of`` as
        ``search_grouped``; giving neither searches every group.  At most 4,096 frames and 1,024 results."""
        flt = self._filter_arg(within, exclude)
        if len(queries) == 0:
            raise ValueError("search_set needs at least one query frame")
        if self._empty() or k <= 0:
            return []
        if len(queries) > self.SET_MAX_QUERIES:
            raise ValueError(f"a clip query holds at most {self.SET_MAX_QUERIES} frames, got {len(queries)}")
        with self.lock:
            return self._search_set(queries, k, flt, group_of, matches)

    def similar_groups(self, group: Hashable, k: int = 5, *, within: Optional[Iterable[Hashable]] = None,
                       group_of: GROUP_OF = None, matches: bool = False, keyframes: Optional[int] = None) -> List[Dict]:
        """"More like this video": ``search_set`` with the stored rows of ``group`` (in row order) as the query set and
        ``group`` itself excluded; ``within`` restricts the answer to those groups.  ``KeyError`` for a group the index does
        not hold, ``ValueError`` for a group of more than 4,096 rows.  ``keyframes=m`` (m >= 1) sends the group's m-keyframe
        summary (``summarize_group``, in selection order) instead of all its rows: a group of any length is then accepted."""
        if within is not None:
            within = self._filter_arg(within, None)[0]
        if keyframes is not None and int(keyframes) < 1:
            raise ValueError(f"keyframes must be >= 1, got {keyframes}")
        with self.lock:
            rn = self._group_rows(group, group_of)
            if rn is None:
                raise KeyError(group)
            if keyframes is None and len(rn) > self.SET_MAX_QUERIES:
                raise ValueError(f"group {group!r} holds {len(rn)} rows; a clip query holds at most {self.SET_MAX_QUERIES}")
            if k <= 0:
                return []
            if keyframes is not None:
                rows, _, _ = self._summarize([self._groups.index[group]], int(keyframes), None, group_of)
                rn = rows[0][rows[0] >= 0].astype(np.int64)
            # one include list: `within` without the group itself; without `within`, one exclude list
            flt = ([key for key in within if key != group], False) if within is not None else ([group], True)
            if not flt[1] and not flt[0]:
                return []
            unit = np.empty((len(rn), self.dimension), dtype=np.float32)
            _lib.check(_lib.load().vq_index_read_rows(self._h, _lib.i64ptr(rn), len(rn), _lib.fptr(unit)))
            return self._search_set(unit, k, flt, group_of, matches, given=True)

    # -- keyframe summary: the k most representative rows of a group (video) -------------------------
    SUMMARY_MAX_K = 256           # vq_index_summarize_groups: keyframes per group

    def _summarize(self, labels: List[int], k: int, max_radius: Optional[float], group_of: GROUP_OF):
        """labels: dense labels of the host's labels under ``group_of`` (at least one), k >= 1, the index not empty; under the
        lock.  One device call -> (rows, radius, members), each [len(labels)][min(k, SUMMARY_MAX_K)]; -1 / inf / 0 in unused slots."""
        rho = -math.inf if max_radius is None else float(max_radius)
        if math.isnan(rho):
            raise ValueError("max_radius must not be NaN (None: no early stop)")
        self._prepare(np.empty((0, self.dimension), dtype=np.float32), k, given=True, group_of=group_of, what="index")
        lab = np.ascontiguousarray(labels, dtype=np.int32)
        kk = min(int(k), self.SUMMARY_MAX_K)
        rows = np.empty((len(lab), kk), dtype=np.int32)
        radius = np.empty((len(lab), kk), dtype=np.float32)
        members = np.empty((len(lab), kk), dtype=np.int32)
        _lib.check(_lib.load().vq_index_summarize_groups(self._h, _lib.i32ptr(lab), len(lab), kk, rho, _lib.i32ptr(rows), _lib.fptr(radius),
                                                         _lib.i32ptr(members)))
        return rows, radius, members

    def summarize_groups(self, groups: Optional[Iterable[Hashable]] = None, k: int = 5, *, max_radius: Optional[float] = None,
                         group_of: GROUP_OF = None) -> Dict[Hashable, List[Dict]]:
        """The k most representative rows (keyframes) of each listed group (default: every group the index holds), from one
        device call: ``{group: [{'id', 'rank', 'radius', 'members'}]}``, each list in selection order.  Greedy farthest-point
        selection on the stored rows: the first keyframe is the row most like the group's mean direction, every further one
        the row farthest (in ``search``'s distance, ties by id as ``search``) from the keyframes chosen so far; ``radius`` is
        the distance of the farthest remaining row once this keyframe is in (it never increases: every row of the group lies
        within ``radius`` of one of the keyframes up to this one), ``members`` the number of rows, the keyframe included, that
        the keyframe is the nearest of (first-chosen on equal distance).  The list for k is a prefix of the list for k + 1.
        ``max_radius`` stops as soon as ``radius <= max_radius`` (at least one keyframe is always returned); a group of fewer
        than k rows returns them all.  ``group_of`` as ``search_grouped``; a key the index does not hold raises ``KeyError``
        before any device work; a key named twice is answered once.  At most 256 keyframes per group."""
        with self.lock:
            gl = self._group_labels(group_of)
            gl.extend()
            keys = list(gl.keys) if groups is None else list(dict.fromkeys(groups))
            labels = [gl.index[key] for key in keys]                 # KeyError: before any device work
            if k <= 0 or not keys:
                return {key: [] for key in keys}
            rows, radius, members = self._summarize(labels, k, max_radius, group_of)
            to_id = self._id_of()
            return {key: [{"id": to_id(r), "rank": t, "radius": d, "members": m} for t, (r, d, m) in enumerate(zip(rr, rd, rm)) if r >= 0]
                    for key, rr, rd, rm in zip(keys, rows.tolist(), radius, members.tolist())}

    def summarize_group(self, group: Hashable, k: int = 5, *, max_radius: Optional[float] = None, group_of: GROUP_OF = None) -> List[Dict]:
        """``summarize_groups`` for one group: ``[{'id', 'rank', 'radius', 'members'}]`` in selection order.  ``KeyError`` for a
        group the index does not hold, ``[]`` for k <= 0."""
        return self.summarize_groups([group], k, max_radius=max_radius, group_of=group_of)[group]

    # -- chapter segmentation: each group (video) cut into at most k coherent runs of frames -------------------------
    SEGMENT_MAX_K = 64            # vq_index_segment_groups: chapters per group

    def _segment(self, labels: List[int], k: int, penalty: float, max_len: Optional[int], group_of: GROUP_OF, position_of: POSITION_OF):
        """labels: dense labels of the host's labels under ``group_of`` (at least one), k >= 1, the index not empty; under the
        lock.  One device call -> (count [n], first, last, frames, spread, show: each [n][min(k, SEGMENT_MAX_K)])."""
        pen, cap = float(penalty), 0 if max_len is None else int(max_len)
        if not pen >= 0:                                          # (NaN too)
            raise ValueError(f"penalty must be >= 0, got {penalty}")
        if max_len is not None and cap < 1:
            raise ValueError(f"max_len must be >= 1 (None: no limit), got {max_len}")
        self._prepare(np.empty((0, self.dimension), dtype=np.float32), k, given=True, group_of=group_of, positions=True,
                      position_of=position_of, what="index")
        lab = np.ascontiguousarray(labels, dtype=np.int32)
        kk = min(int(k), self.SEGMENT_MAX_K)
        count = np.empty(len(lab), dtype=np.int32)
        first, last, frames, show = (np.empty((len(lab), kk), dtype=np.int32) for _ in range(4))
        spread = np.empty((len(lab), kk), dtype=np.float32)
        _lib.check(_lib.load().vq_index_segment_groups(self._h, _lib.i32ptr(lab), len(lab), kk, pen, cap, _lib.i32ptr(count), _lib.i32ptr(first),
                                                       _lib.i32ptr(last), _lib.i32ptr(frames), _lib.fptr(spread), _lib.i32ptr(show), None))
        return count, first, last, frames, spread, show

    def segment_groups(self, groups: Optional[Iterable[Hashable]] = None, k: int = 8, *, penalty: float = 0.0, max_len: Optional[int] = None,
                       group_of: GROUP_OF = None, position_of: POSITION_OF = None) -> Dict[Hashable, List[Dict]]:
        """Chapters: each listed group (default: every group the index holds), walked by (position, id), cut into at most k
        contiguous runs of rows that point the same way, from one device call: ``{group: [{'first', 'last', 'frames', 'spread',
        'show'}]}``, each list in time order.  The cut is the optimal one (a dynamic programme over all contiguous runs) for
        the cost "rows of the run times their mean cosine distance to the run's mean direction", summed over the runs, plus
        ``penalty`` per chapter: ``penalty=0`` gives the best split into at most k parts, a larger one fewer chapters.
        ``first`` / ``last`` are the ids of a chapter's first and last row, ``frames`` its number of rows, ``spread`` that mean
        distance (float32), ``show`` the id of the row most like the chapter as a whole.  ``max_len`` caps the rows of a
        chapter (a group that k chapters of that length cannot cover returns ``[]``).  ``group_of`` as ``search_grouped``,
        ``position_of`` as ``search_distinct``; a key the index does not hold raises ``KeyError`` before any device work; a key
        named twice is answered once.  At most 64 chapters per group; a group of more than 8,192 rows needs ``max_len``."""
        with self.lock:
            gl = self._group_labels(group_of)
            gl.extend()
            keys = list(gl.keys) if groups is None else list(dict.fromkeys(groups))
            labels = [gl.index[key] for key in keys]                 # KeyError: before any device work
            if k <= 0 or not keys:
                return {key: [] for key in keys}
            count, first, last, frames, spread, show = self._segment(labels, k, penalty, max_len, group_of, position_of)
            to_id = self._id_of()
            return {key: [{"first": to_id(a), "last": to_id(b), "frames": n, "spread": d, "show": to_id(s)}
                          for a, b, n, d, s in zip(fa[:c], la[:c], na[:c], da[:c], sa[:c])]
                    for key, c, fa, la, na, da, sa in zip(keys, count.tolist(), first.tolist(), last.tolist(), frames.tolist(), spread, show.tolist())}

    def segment_group(self, group: Hashable, k: int = 8, *, penalty: float = 0.0, max_len: Optional[int] = None, group_of: GROUP_OF = None,
                      position_of: POSITION_OF = None) -> List[Dict]:
        """``segment_groups`` for one group: ``[{'first', 'last', 'frames', 'spread', 'show'}]`` in time order.  ``KeyError`` for a
        group the index does not hold, ``[]`` for k <= 0."""
        return self.segment_groups([group], k, penalty=penalty, max_len=max_len, group_of=group_of, position_of=position_of)[group]

    # -- zero-shot labelling: which prompt each row shows, what each group (video) is about --------------
    LABEL_MAX_PROMPTS = 4096      # vq_index_label_rows: prompts per call
    LABEL_MAX_TAGS = 16           # ... tags per group

    def _label(self, prompts, mode: int, max_distance: Optional[float], top: int, group_of: GROUP_OF, given: bool = False):
        """One device call, under the lock.  prompts: 1 .. LABEL_MAX_PROMPTS vectors (``given``: see ``_prepare``); top > 0 asks
        for the group outputs.  None for an empty index, else (labels [n], distances [n], group labels (None without ``top``), tags, votes, show rows
        [G][min(top, LABEL_MAX_TAGS)], unlabelled [G]); the last four None without ``top``."""
        if len(prompts) == 0:
            raise ValueError("labelling needs at least one prompt")
        if len(prompts) > self.LABEL_MAX_PROMPTS:
            raise ValueError(f"a vocabulary holds at most {self.LABEL_MAX_PROMPTS} prompts, got {len(prompts)}")
        rho = math.inf if max_distance is None else float(max_distance)
        if math.isnan(rho):
            raise ValueError("max_distance must not be NaN (None: every row is labelled)")
        m = min(int(top), self.LABEL_MAX_TAGS)
        ready = self._prepare(prompts, 1, given=given, group_of=group_of, what="prompt", groups=m > 0)    # row labels alone need no labels or ranks
        if ready is None:
            return None
        unit, gl = ready[0], ready[1]
        n, G = len(self._ids), len(gl.keys) if m > 0 else 0
        labels = np.empty(n, dtype=np.int32)
        dist = np.empty(n, dtype=np.float32)
        tags = votes = show = unl = None
        if m > 0:
            tags, votes, show = (np.empty((G, m), dtype=np.int32) for _ in range(3))
            unl = np.empty(G, dtype=np.int32)
        _lib.check(_lib.load().vq_index_label_rows(self._h, _lib.fptr(unit), unit.shape[0], int(mode), rho, _lib.i32ptr(labels),
                                                   _lib.fptr(dist), max(m, 0), *(_lib.i32ptr(a) if m > 0 else None for a in (tags, votes, show, unl))))
        return labels, dist, gl, tags, votes, show, unl

    def label_rows(self, prompts: Sequence[np.ndarray], *, max_distance: Optional[float] = None, mode: int = MODE_AUTO):
        """Zero-shot labels: for every stored row the prompt it is closest to.  Returns ``(labels int32 [n], distances float32
        [n])`` in row order (the order of ``add``): ``labels[r]`` is the index into ``prompts`` with the smallest
        ``search`` distance to row r (prompts normalised as ``search`` normalises queries; two prompts at the same distance:
        the smaller index), ``distances[r]`` that distance.  ``max_distance``: a row farther than this from every prompt gets
        label -1 ("none of the above"; its distance is still reported; a row exactly at ``max_distance`` keeps its label).
        Exact in every mode; ``mode`` as ``search_mode`` (0 auto, 1 exact path, 2 fp16 path).  At most 4,096 prompts."""
        with self.lock:
            res = self._label(prompts, mode, max_distance, 0, None)
        if res is None:
            return np.empty(0, dtype=np.int32), np.empty(0, dtype=np.float32)
        return res[0], res[1]

    def _label_groups(self, prompts, top: int, group_of: GROUP_OF, max_distance: Optional[float], given: bool = False) -> Dict[Hashable, List[Dict]]:
        """``label_groups`` under the lock (``given``: see ``_prepare``)."""
        if int(top) <= 0:
            raise ValueError(f"top must be >= 1, got {top}")
        res = self._label(prompts, self.search_mode, max_distance, top, group_of, given=given)
        if res is None:
            return {}
        _, dist, gl, tags, votes, show, _ = res
        rows_of = np.bincount(gl.labels, minlength=len(gl.keys))
        to_id = self._id_of()
        return {key: [{"label": j, "votes": v, "share": v / int(rows_of[g]), "id": to_id(r), "distance": dist[r]}
                      for j, v, r in zip(tags[g].tolist(), votes[g].tolist(), show[g].tolist()) if j >= 0]
                for g, key in enumerate(gl.keys)}

    def label_groups(self, prompts: Sequence[np.ndarray], top: int = 3, *, group_of: GROUP_OF = None,
                     max_distance: Optional[float] = None) -> Dict[Hashable, List[Dict]]:
        """What every group (video) is about, from one device call: ``{group: [{'label', 'votes', 'share', 'id', 'distance'}]}``.
        Every row votes for its ``label_rows`` label; a group's list holds its ``top`` most voted labels (at most 16; more
        votes first, the smaller index on equal votes; labels nobody voted for never appear).  ``votes`` is the number of the
        group's rows with that label, ``share`` votes over ALL the group's rows (rows that ``max_distance`` leaves unlabelled
        vote for nothing but still count here), ``id`` and ``distance`` those of the group's row that shows the label best (the
        smallest distance, ties by id as ``search``).  ``group_of`` as ``search_grouped``."""
        with self.lock:
            return self._label_groups(prompts, top, group_of, max_distance)

    # -- library clustering: the themes of everything stored, nobody's query needed ----------------------
    CLUSTER_MAX = 4096            # vq_index_cluster: clusters per call
    CLUSTER_MAX_ITER = 1000       # ... iterations

    def _cluster(self, k: int, max_iter: int, init, seed, mode: int, given: bool = False):
        """One device call, under the lock.  None for an empty index, else (centroids [k][dim], labels [n], distances [n],
        counts [k], show rows [k], iterations, changed [iterations])."""
        k, max_iter = int(k), int(max_iter)
        if not 1 <= k <= self.CLUSTER_MAX:
            raise ValueError(f"k must be in [1, {self.CLUSTER_MAX}], got {k}")
        if not 1 <= max_iter <= self.CLUSTER_MAX_ITER:
            raise ValueError(f"max_iter must be in [1, {self.CLUSTER_MAX_ITER}], got {max_iter}")
        if self._empty():
            return None
        n = len(self._ids)
        if k > n:
            raise ValueError(f"{k} clusters for an index of {n} rows")
        unit = rows = None
        if init is None:
            rows = np.sort(np.random.default_rng(seed).choice(n, k, replace=False)).astype(np.int32)
        else:
            unit = init if given else np.ascontiguousarray(self._unit_rows(init), dtype=np.float32)
            if unit.shape != (k, self.dimension):
                raise ValueError(f"init must hold {k} vectors of dimension {self.dimension}, got shape {unit.shape}")
        if not self._identity:
            self._sync_tie_order()                # the show rows' ties follow the ids, as `search` orders them
        centroids = np.empty((k, self.dimension), dtype=np.float32)
        labels, counts, show = np.empty(n, dtype=np.int32), np.empty(k, dtype=np.int32), np.empty(k, dtype=np.int32)
        dist = np.empty(n, dtype=np.float32)
        changed = np.zeros(max_iter, dtype=np.int32)
        iterations = ctypes.c_int(0)
        _lib.check(_lib.load().vq_index_cluster(self._h, _lib.fptr(unit) if unit is not None else None,
                                                _lib.i32ptr(rows) if rows is not None else None, k, max_iter, int(mode), _lib.fptr(centroids),
                                                _lib.i32ptr(labels), _lib.fptr(dist), _lib.i32ptr(counts), _lib.i32ptr(show),
                                                ctypes.byref(iterations), _lib.i32ptr(changed)))
        return centroids, labels, dist, counts, show, iterations.value, changed[:iterations.value]

    def cluster(self, k: int, *, max_iter: int = 25, init=None, seed=0, mode: int = MODE_AUTO) -> Dict:
        """Spherical k-means over every stored row, exact and reproducible: the same rows, ``k``, ``init`` / ``seed`` give the
        same bits on every run (the device sums in a fixed order; include/vq_amd.h vq_index_cluster has the definition).
        ``init``: k start vectors (normalised as ``search`` normalises queries); None: k distinct stored rows drawn by
        ``np.random.default_rng(seed)``, in ascending row order.  Every iteration assigns each row to its closest centroid
        (``label_rows``' rule: equal distances go to the smaller cluster number) and moves each centroid to the normalised
        mean of its rows; a cluster that loses all its rows keeps its centroid.  It stops when no row changes cluster, or
        after ``max_iter`` assignments.  Returns ``{'centroids' float32 [k][dim], 'labels' int32 [n], 'distances' float32 [n],
        'clusters', 'iterations', 'converged', 'changed'}``: labels and distances are ``label_rows(centroids)`` in row order;
        ``clusters[j]`` is ``{'cluster': j, 'size', 'id', 'distance', 'score'}`` with the row closest to the centroid (ties by id
        as ``search``; ``id`` None for an empty cluster); ``changed[t]`` the rows that changed cluster in assignment t + 1 (all
        of them in the first); ``converged``: the last assignment changed nothing.  ``mode`` as ``label_rows``.  At most 4,096
        clusters, at most as many as rows.  An empty index: no clusters."""
        with self.lock:
            res = self._cluster(k, max_iter, init, seed, mode)
        if res is None:
            return {"centroids": np.empty((0, self.dimension), dtype=np.float32), "labels": np.empty(0, dtype=np.int32),
                    "distances": np.empty(0, dtype=np.float32), "clusters": [], "iterations": 0, "converged": True, "changed": []}
        centroids, labels, dist, counts, show, iterations, changed = res
        to_id = self._id_of()
        clusters = [{"cluster": j, "size": c, "id": to_id(r), **_scored(dist[r])} if r >= 0 else
                    {"cluster": j, "size": c, "id": None, "distance": None, "score": None}
                    for j, (c, r) in enumerate(zip(counts.tolist(), show.tolist()))]
        changed = changed.tolist()
        return {"centroids": centroids, "labels": labels, "distances": dist, "clusters": clusters, "iterations": iterations,
                "converged": iterations > 1 and changed[-1] == 0, "changed": changed}

    # -- sequence query: the k groups (videos) that show a list of steps in order -------------------
    SEQ_MAX_STEPS = 64            # vq_index_search_sequence: steps per call

    def _search_sequence(self, steps, k: int, min_gap: int, max_gap: int, flt, group_of, position_of, given: bool = False) -> List[Dict]:
        """steps: 1 to SEQ_MAX_STEPS of them (``given``: see ``_prepare``).  flt: ``_filter_arg``'s.  min_gap / max_gap: checked."""
        ready = self._prepare(steps, k, given=given, group_of=group_of, positions=True, position_of=position_of, flt=flt, what="step")
        if ready is None:
            return []
        unit, gl, ps, labels, excl = ready
        m, kk = unit.shape[0], min(int(k), len(gl.keys), 1024)
        groups = np.empty(kk, dtype=np.int32)
        dist = np.empty(kk, dtype=np.float32)
        rows = np.empty((kk, m), dtype=np.int32)
        _lib.check(_lib.load().vq_index_search_sequence(self._h, _lib.fptr(unit), m, kk, min_gap, max_gap, _lib.i32ptr(labels), len(labels),
                                                        int(excl), _lib.i32ptr(groups), _lib.fptr(dist), _lib.i32ptr(rows)))
        keys, pos, to_id = gl.keys, ps.values, self._id_of()
        out = []
        for j, (g, d) in enumerate(zip(groups.tolist(), dist)):
            if g < 0:
                break
            chain = rows[j].tolist()
            out.append({"group": keys[g], **_scored(d), "chain": [to_id(r) for r in chain], "positions": [int(pos[r]) for r in chain]})
        return out

    def search_sequence(self, steps: Sequence[np.ndarray], k: int = 5, *, max_gap: int, min_gap: int = 1,
                        within: Optional[Iterable[Hashable]] = None, exclude: Optional[Iterable[Hashable]] = None,
                        group_of: GROUP_OF = None, position_of: POSITION_OF = None) -> List[Dict]:
        """The k GROUPS (videos) that show the ``steps`` IN ORDER (a storyboard of prompts, the frames of a clip):
        ``[{'group', 'distance', 'score', 'chain', 'positions'}]``.  A chain is one row of the group per step whose positions
        increase by ``min_gap`` .. ``max_gap`` from step to step (``1 <= min_gap <= max_gap``); its cost adds the steps'
        distances (normalised as ``search`` does) in fp64 in step order, a step always continuing the cheapest admissible
        chain so far (ties by id, as ``search``).  ``distance`` is the group's cheapest chain over the number of steps, rounded
        once to float32; ``chain`` its node ids in step order, ``positions`` their positions.  Groups without any chain do not
        appear; groups come back by (distance, order in which the groups first appeared in the index).  One step is
        ``search_grouped``; ``search_set`` of the same steps never scores a group worse.  ``group_of`` / ``within`` /
        ``exclude`` as ``search_grouped``, ``position_of`` as ``search_distinct`` (timestamps in ms with gaps in ms alike).
        At most 64 steps and 1,024 results."""
        flt = self._filter_arg(within, exclude)
        if len(steps) == 0:
            raise ValueError("search_sequence needs at least one step")
        if len(steps) > self.SEQ_MAX_STEPS:
            raise ValueError(f"a sequence query holds at most {self.SEQ_MAX_STEPS} steps, got {len(steps)}")
        lo, hi = int(min_gap), int(max_gap)
        if lo < 1 or hi < lo:
            raise ValueError(f"the gaps must satisfy 1 <= min_gap <= max_gap, got min_gap={min_gap}, max_gap={max_gap}")
        if self._empty() or k <= 0:
            return []
        with self.lock:
            return self._search_sequence(steps, k, lo, min(hi, 2 ** 62), flt, group_of, position_of)

    # -- span query: the k groups (videos) with the best time span for a query, from where to where ----
    SPAN_MAX_QUERIES = 64         # vq_index_search_spans: queries per call
    SPAN_NO_LIMIT = 2 ** 40       # what None means for max_gap / max_span (positions are 32-bit)

    @staticmethod
    def _span_args(max_distance, max_gap, max_span) -> Tuple[np.float32, int, int]:
        tau = np.float32(max_distance)
        if tau != tau:
            raise ValueError("max_distance is NaN")
        gap = HNSWIndex.SPAN_NO_LIMIT if max_gap is None else int(max_gap)
        span = HNSWIndex.SPAN_NO_LIMIT if max_span is None else int(max_span)
        if gap < 0 or span < 0:
            raise ValueError(f"max_gap and max_span must be >= 0 (None: no limit), got max_gap={max_gap}, max_span={max_span}")
        return tau, min(gap, 2 ** 62), min(span, 2 ** 62)

    def _search_spans(self, queries, k: int, tau: np.float32, max_gap: int, max_span: int, flt, group_of, position_of,
                      given: bool = False) -> List[List[Dict]]:
        """queries: 1 to SPAN_MAX_QUERIES of them (``given``: see ``_prepare``).  flt: ``_filter_arg``'s.  tau and limits: checked."""
        ready = self._prepare(queries, k, given=given, group_of=group_of, positions=True, position_of=position_of, flt=flt)
        if ready is None:
            return [[] for _ in queries]
        unit, gl, ps, labels, excl = ready
        nq, kk = unit.shape[0], min(int(k), len(gl.keys), 1024)
        groups = np.empty((nq, kk), dtype=np.int32)
        dist = np.empty((nq, kk), dtype=np.float32)
        mass = np.empty((nq, kk), dtype=np.int64)
        length = np.empty((nq, kk), dtype=np.int32)
        rows = np.empty((nq, kk, 3), dtype=np.int32)
        _lib.check(_lib.load().vq_index_search_spans(self._h, _lib.fptr(unit), nq, kk, float(tau), max_gap, max_span, _lib.i32ptr(labels),
                                                     len(labels), int(excl), _lib.i32ptr(groups), _lib.fptr(dist),
                                                     mass.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), _lib.i32ptr(length),
                                                     _lib.i32ptr(rows)))
        keys, pos, to_id = gl.keys, ps.values, self._id_of()
        out = []
        for gq, mq, lq, rq in zip(groups.tolist(), mass.tolist(), length.tolist(), rows.tolist()):
            res = []
            for g, s, n, (a, b, p) in zip(gq, mq, lq, rq):
                if g < 0:
                    break
                m = s * 2.0 ** -24                              # (exact: |s| < 2^53)
                res.append({"group": keys[g], "mass": m, "frames": n, "start_id": to_id(a), "end_id": to_id(b), "peak_id": to_id(p),
                            "start": int(pos[a]), "end": int(pos[b]), "score": 1.0 - (float(tau) - m / n)})
            out.append(res)
        return out

    def search_spans(self, query: np.ndarray, k: int = 5, *, max_distance: float, max_gap: Optional[int] = None,
                     max_span: Optional[int] = None, within: Optional[Iterable[Hashable]] = None,
                     exclude: Optional[Iterable[Hashable]] = None, group_of: GROUP_OF = None,
                     position_of: POSITION_OF = None) -> List[Dict]:
        """The k GROUPS (videos) with the best TIME SPAN for one query — "where does it happen, from when to when":
        ``[{'group', 'mass', 'frames', 'start_id', 'end_id', 'peak_id', 'start', 'end', 'score'}]``.  Every row gains
        ``max_distance - distance`` (the query normalised as ``search`` does; the gain is kept as an integer multiple of
        2^-24), so rows closer than ``max_distance`` add to a span and rows farther away cost it.  A span is a run of
        consecutive rows of one group in position order in which neighbours lie at most ``max_gap`` positions apart and the
        first and the last at most ``max_span`` (``None``: no limit); a group answers with its span of the largest summed gain
        (``mass``; then the shortest, then the earliest), and groups without a span of positive mass do not appear.  Groups
        come back by mass, largest first (ties: the order in which the groups first appeared in the index).  ``frames`` is the
        number of rows in the span, ``start`` / ``end`` the positions of its first and last row (``start_id`` / ``end_id``),
        ``peak_id`` its best single row (ties by id, as ``search``); ``score`` = ``1 - (max_distance - mass / frames)`` is the
        mean similarity over the span, good to the gain's rounding.  ``max_span=0`` on distinct positions is
        ``search_grouped`` below ``max_distance``.  ``group_of`` / ``within`` / ``exclude`` as ``search_grouped``,
        ``position_of`` as ``search_distinct`` (timestamps in ms with limits in ms alike).  At most 1,024 results."""
        return self.search_spans_batch([query], k, max_distance=max_distance, max_gap=max_gap, max_span=max_span, within=within,
                                       exclude=exclude, group_of=group_of, position_of=position_of)[0]

    def search_spans_batch(self, queries: Sequence[np.ndarray], k: int = 5, *, max_distance: float, max_gap: Optional[int] = None,
                           max_span: Optional[int] = None, within: Optional[Iterable[Hashable]] = None,
                           exclude: Optional[Iterable[Hashable]] = None, group_of: GROUP_OF = None,
                           position_of: POSITION_OF = None) -> List[List[Dict]]:
        """``search_spans`` for a batch of at most 64 queries, one device pass; a group's span for one query does not depend on
        the other queries."""
        flt = self._filter_arg(within, exclude)
        tau, gap, span = self._span_args(max_distance, max_gap, max_span)
        if len(queries) > self.SPAN_MAX_QUERIES:
            raise ValueError(f"a span search takes at most {self.SPAN_MAX_QUERIES} queries, got {len(queries)}")
        if len(queries) == 0:
            return []
        if self._empty() or k <= 0:
            return [[] for _ in queries]
        with self.lock:
            return self._search_spans(queries, k, tau, gap, span, flt, group_of, position_of)

    # -- shared footage: the k groups (videos) that reuse a run of a clip's frames, and where -------
    MATCH_MAX_FRAMES = 4096      # vq_index_match_runs: clip frames per call

    @staticmethod
    def _match_args(max_distance, min_len, max_miss) -> Tuple[np.float32, int, int]:
        md = np.float32(max_distance)
        if md != md:
            raise ValueError("max_distance is NaN")
        if int(min_len) < 1 or int(max_miss) < 0:
            raise ValueError(f"shared runs need min_len >= 1 and max_miss >= 0, got min_len={min_len}, max_miss={max_miss}")
        return md, int(min_len), min(int(max_miss), 2 ** 31 - 1)

    def _shared_runs(self, frames, k: int, max_dist: np.float32, min_len: int, max_miss: int, flt, group_of, position_of,
                     given: bool = False) -> List[Dict]:
        """frames: 1 to MATCH_MAX_FRAMES of them, in time order (``given``: see ``_prepare``).  flt: ``_filter_arg``'s."""
        ready = self._prepare(frames, k, given=given, group_of=group_of, positions=True, position_of=position_of, flt=flt, what="frame")
        if ready is None:
            return []
        unit, gl, ps, labels, excl = ready
        m, kk = unit.shape[0], min(int(k), len(gl.keys), 1024)
        ints = np.empty((6, kk), dtype=np.int32)              # group, hits, span, q_first, row_first, row_last
        mean = np.empty(kk, dtype=np.float32)
        _lib.check(_lib.load().vq_index_match_runs(self._h, _lib.fptr(unit), m, kk, max_dist, min_len, max_miss, int(self.search_mode),
                                                   _lib.i32ptr(labels), len(labels), int(excl), *(_lib.i32ptr(ints[a]) for a in range(6)),
                                                   _lib.fptr(mean)))
        keys, pos, to_id = gl.keys, ps.values, self._id_of()
        out = []
        for (g, hits, span, q_first, first, last), d in zip(ints.T.tolist(), mean):
            if g < 0:
                break
            out.append({"group": keys[g], "hits": hits, "span": span, "query_first": q_first, "first": to_id(first), "last": to_id(last),
                        "positions": (int(pos[first]), int(pos[last])), **_scored(d)})
        return out

    def shared_runs(self, frames: Sequence[np.ndarray], k: int = 5, *, max_distance: float, min_len: int = 3, max_miss: int = 0,
                    within: Optional[Iterable[Hashable]] = None, exclude: Optional[Iterable[Hashable]] = None,
                    group_of: GROUP_OF = None, position_of: POSITION_OF = None) -> List[Dict]:
        """The k GROUPS (videos) that contain the same footage as the clip ``frames`` (in time order), and where:
        ``[{'group', 'hits', 'span', 'query_first', 'first', 'last', 'positions', 'distance', 'score'}]``.  Clip frame i HITS a
        stored frame when their distance (the clip normalised as ``search`` does) is at most ``max_distance``.  A video's
        frames are taken in (position, id) order; a run is a stretch of hits along one diagonal — clip frame i against the
        video's frame i + offset — that no gap of more than ``max_miss`` misses interrupts, trimmed to its first and last hit,
        with at least ``min_len`` hits.  Per video its best run (most hits, then the shortest span, the smallest offset, the
        earliest start): ``hits``, ``span`` (clip frames from its first to its last hit), ``query_first`` (the clip frame it
        starts at), ``first`` / ``last`` (node ids of the video's frames at its ends) and their ``positions``, ``distance`` the
        mean distance over the hits, ``score = float32(1) - distance``.  Videos come back by (most hits, shortest span, order
        in which the groups first appeared in the index); a video without a run does not appear.  ``group_of`` / ``within`` /
        ``exclude`` as ``search_grouped``, ``position_of`` as ``search_distinct``.  At most 4,096 frames and 1,024 results;
        the clip times the index's rows is bounded (4,096 frames against a million rows)."""
        flt = self._filter_arg(within, exclude)
        if len(frames) == 0:
            raise ValueError("shared_runs needs at least one frame")
        if len(frames) > self.MATCH_MAX_FRAMES:
            raise ValueError(f"a clip holds at most {self.MATCH_MAX_FRAMES} frames, got {len(frames)}")
        md, lo, miss = self._match_args(max_distance, min_len, max_miss)
        if self._empty() or k <= 0:
            return []
        with self.lock:
            return self._shared_runs(frames, k, md, lo, miss, flt, group_of, position_of)

    def shared_runs_of(self, group: Hashable, k: int = 5, *, max_distance: float, min_len: int = 3, max_miss: int = 0,
                       within: Optional[Iterable[Hashable]] = None, group_of: GROUP_OF = None,
                       position_of: POSITION_OF = None) -> List[Dict]:
        """"Which videos reuse footage of this one": ``shared_runs`` with the stored rows of ``group``, in (position, id) order,
        as the clip and ``group`` itself excluded; ``within`` restricts the answer to those groups.  ``KeyError`` for a group
        the index does not hold, ``ValueError`` for a group of more than 4,096 rows."""
        if within is not None:
            within = self._filter_arg(within, None)[0]
        md, lo, miss = self._match_args(max_distance, min_len, max_miss)
        with self.lock:
            rn = self._group_rows(group, group_of)
            if rn is None:
                raise KeyError(group)
            if len(rn) > self.MATCH_MAX_FRAMES:
                raise ValueError(f"group {group!r} holds {len(rn)} rows; a clip holds at most {self.MATCH_MAX_FRAMES}")
            if k <= 0:
                return []
            flt = ([key for key in within if key != group], False) if within is not None else ([group], True)
            if not flt[1] and not flt[0]:
                return []
            self._positions = _Positions.current(self._positions, frame_of if position_of is None else position_of, self._ids)
            self._positions.extend()
            pos, ids = self._positions.values, self._ids
            try:
                rn = np.array(sorted(rn.tolist(), key=lambda r: (int(pos[r]), ids[r])), dtype=np.int64)
            except TypeError:                                 # ids without a total order: rows at one position stay in row order
                rn = np.array(sorted(rn.tolist(), key=lambda r: int(pos[r])), dtype=np.int64)
            unit = np.empty((len(rn), self.dimension), dtype=np.float32)
            _lib.check(_lib.load().vq_index_read_rows(self._h, _lib.i64ptr(rn), len(rn), _lib.fptr(unit)))
            return self._shared_runs(unit, k, md, lo, miss, flt, group_of, position_of, given=True)

    # -- warped alignment: the k groups (videos) that show a clip at any pace, and from where to where ----
    ALIGN_MAX_FRAMES = 4096      # vq_index_align_clip: clip frames per call

    @staticmethod
    def _align_args(max_distance, groups, exclude) -> Tuple[np.float32, Optional[Tuple[List[Hashable], bool]]]:
        md = np.float32(np.inf if max_distance is None else max_distance)
        if md != md:
            raise ValueError("max_distance is NaN")
        if groups is None:
            return md, None
        if isinstance(groups, (str, bytes)) or not isinstance(groups, Iterable):
            raise ValueError("`groups` takes an iterable of group keys (a list of video ids), not one key")
        return md, (list(groups), bool(exclude))

    def _align_clip(self, frames, k: int, max_dist: np.float32, flt, group_of, position_of, alignment: bool,
                    given: bool = False) -> List[Dict]:
        """frames: 1 to ALIGN_MAX_FRAMES of them, in time order (``given``: see ``_prepare``).  flt: ``_align_args``'s."""
        ready = self._prepare(frames, k, given=given, group_of=group_of, positions=True, position_of=position_of, flt=flt, what="frame")
        if ready is None:
            return []
        unit, gl, ps, labels, excl = ready
        m, kk = unit.shape[0], min(int(k), len(gl.keys), 1024)
        groups = np.empty(kk, dtype=np.int32)
        dist = np.empty(kk, dtype=np.float32)
        cost = np.empty(kk, dtype=np.int64)
        ends = np.empty((kk, 2), dtype=np.int32)
        pairs = np.empty((kk, m, 2), dtype=np.int32) if alignment else None
        _lib.check(_lib.load().vq_index_align_clip(self._h, _lib.fptr(unit), m, kk, float(max_dist), _lib.i32ptr(labels), len(labels),
                                                   int(excl), _lib.i32ptr(groups), _lib.fptr(dist),
                                                   cost.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), _lib.i32ptr(ends),
                                                   _lib.i32ptr(pairs) if alignment else None))
        keys, pos, to_id = gl.keys, ps.values, self._id_of()
        out = []
        for j, (g, d, c, (a, b)) in enumerate(zip(groups.tolist(), dist, cost.tolist(), ends.tolist())):
            if g < 0:
                break
            hit = {"group": keys[g], **_scored(d), "cost": c, "start_id": to_id(a), "end_id": to_id(b), "start": int(pos[a]),
                   "end": int(pos[b])}
            if alignment:
                hit["alignment"] = [(to_id(first), to_id(last)) for first, last in pairs[j].tolist()]
            out.append(hit)
        return out

    def align_clip(self, frames: Sequence[np.ndarray], k: int = 5, max_distance: Optional[float] = None, *, group_of: GROUP_OF = None,
                   position_of: POSITION_OF = None, groups: Optional[Iterable[Hashable]] = None, exclude: bool = False,
                   alignment: bool = False) -> List[Dict]:
        """The k GROUPS (videos) that show the clip ``frames`` (in time order) AT ANY PACE — played faster or slower, or sampled
        at another rate — and from where to where: ``[{'group', 'distance', 'score', 'cost', 'start_id', 'end_id', 'start',
        'end'}]``.  A subsequence dynamic time warp: a video's frames are taken in (position, id) order; a path pairs every clip
        frame, in order, with one or more consecutive stored frames (a stored frame may serve several clip frames), from any
        start to any end; its ``cost`` adds the paired distances (the clip normalised as ``search`` does), each kept as an
        integer multiple of 2^-24.  Per video the cheapest path (then the later start; among ends: the shortest stretch, the
        earliest); ``distance`` is its cost per clip frame, ``score = float32(1) - distance``; ``start_id`` / ``end_id`` the
        stored frames at its ends and ``start`` / ``end`` their positions.  Videos with ``distance`` above ``max_distance`` do
        not appear (``None``: no limit); they come back cheapest first (ties: the order in which the groups first appeared in
        the index).  ``alignment=True`` adds ``'alignment'``: per clip frame the ``(first_id, last_id)`` of the stored frames
        paired with it.  ``groups`` restricts the search to those group keys, or with ``exclude=True`` to all the others.
        ``group_of`` as ``search_grouped``, ``position_of`` as ``search_distinct``.  At most 4,096 frames and 1,024 results;
        with ``alignment`` the clip times the longest video searched is bounded (2^28 cells)."""
        md, flt = self._align_args(max_distance, groups, exclude)
        if len(frames) == 0:
            raise ValueError("align_clip needs at least one frame")
        if len(frames) > self.ALIGN_MAX_FRAMES:
            raise ValueError(f"a clip holds at most {self.ALIGN_MAX_FRAMES} frames, got {len(frames)}")
        if self._empty() or k <= 0:
            return []
        with self.lock:
            return self._align_clip(frames, k, md, flt, group_of, position_of, bool(alignment))

    def align_group(self, group: Hashable, k: int = 5, max_distance: Optional[float] = None, *, group_of: GROUP_OF = None,
                    position_of: POSITION_OF = None, groups: Optional[Iterable[Hashable]] = None, alignment: bool = False,
                    max_frames: Optional[int] = None) -> List[Dict]:
        """"Which videos show this one at any pace": ``align_clip`` with the stored rows of ``group``, in (position, id) order, as
        the clip and ``group`` itself excluded; ``groups`` restricts the answer to those groups.  ``max_frames`` takes every
        ceil(L / max_frames)-th of the video's L frames as the clip.  ``KeyError`` for a group the index does not hold,
        ``ValueError`` for a clip of more than 4,096 frames (pass ``max_frames``)."""
        md, flt = self._align_args(max_distance, groups, False)
        if max_frames is not None and int(max_frames) < 1:
            raise ValueError(f"max_frames must be >= 1, got {max_frames}")
        with self.lock:
            rn = self._group_rows(group, group_of)
            if rn is None:
                raise KeyError(group)
            stride = 1 if max_frames is None else -(-len(rn) // int(max_frames))
            if -(-len(rn) // stride) > self.ALIGN_MAX_FRAMES:
                raise ValueError(f"group {group!r} holds {len(rn)} rows; a clip holds at most {self.ALIGN_MAX_FRAMES} "
                                 "(pass max_frames= to take every ceil(L / max_frames)-th frame)")
            if k <= 0:
                return []
            flt = ([key for key in flt[0] if key != group], False) if flt is not None else ([group], True)
            if not flt[1] and not flt[0]:
                return []
            self._positions = _Positions.current(self._positions, frame_of if position_of is None else position_of, self._ids)
            self._positions.extend()
            pos, ids = self._positions.values, self._ids
            try:
                rn = np.array(sorted(rn.tolist(), key=lambda r: (int(pos[r]), ids[r])), dtype=np.int64)
            except TypeError:                                 # ids without a total order: rows at one position stay in row order
                rn = np.array(sorted(rn.tolist(), key=lambda r: int(pos[r])), dtype=np.int64)
            rn = np.ascontiguousarray(rn[::stride])
            unit = np.empty((len(rn), self.dimension), dtype=np.float32)
            _lib.check(_lib.load().vq_index_read_rows(self._h, _lib.i64ptr(rn), len(rn), _lib.fptr(unit)))
            return self._align_clip(unit, k, md, flt, group_of, position_of, bool(alignment), given=True)

    # -- library neighbours: every stored row's nearest rows elsewhere ------------------------
    NEIGHBORS_MAX_K = 1024

    def _neighbors(self, rows: Optional[np.ndarray], k: int, other_groups: bool, group_of: GROUP_OF, mode: int):
        """One device call, under the lock.  rows: int64 row numbers, or None for every row.  (rows int32 [m][k], distances
        float32 [m][k]); unused slots -1 / inf."""
        k = int(k)
        if not 1 <= k <= self.NEIGHBORS_MAX_K:
            raise ValueError(f"k must be in 1 .. {self.NEIGHBORS_MAX_K}, got {k}")
        if int(mode) not in (MODE_AUTO, 1, 2):
            raise ValueError(f"mode {mode} unknown (0 auto, 1 exact path, 2 fp16 path)")
        m = len(self._ids) if rows is None else len(rows)
        out_rows = np.full((m, k), -1, dtype=np.int32)
        out_dist = np.full((m, k), np.inf, dtype=np.float32)
        if m == 0 or self._empty():
            return out_rows, out_dist
        if not self._identity:
            self._sync_tie_order()
        if other_groups:
            self._sync_groups(group_of)
        _lib.check(_lib.load().vq_index_neighbors(self._h, None if rows is None else _lib.i64ptr(rows), m, k, 1 if other_groups else 0,
                                                  int(mode), _lib.i32ptr(out_rows), _lib.fptr(out_dist)))
        return out_rows, out_dist

    def _rows_of_ids(self, ids: Iterable[Hashable]) -> np.ndarray:
        try:
            return np.array([self._row_of[i] for i in ids], dtype=np.int64)
        except KeyError as e:
            raise KeyError(f"id {e.args[0]!r} is not in the index") from None

    def neighbors(self, k: int = 5, *, ids: Optional[Iterable[Hashable]] = None, other_groups: bool = False,
                  group_of: GROUP_OF = None, mode: int = MODE_AUTO) -> Tuple[np.ndarray, np.ndarray]:
        """The library's neighbour table: for every stored row (``ids=None``, in add order) or for the rows of ``ids`` (in
        their order; repeats allowed) the ``k`` nearest OTHER stored rows.  ``other_groups=False``: every row but the row
        itself.  ``other_groups=True``: only rows of other groups (videos, under ``group_of``, default ``video_of``) — "where
        else does this frame appear".  Returns ``(rows int32 [m][k], distances float32 [m][k])`` in ROW numbers (``index._ids[r]``
        is the id), nearest first by ``search``'s (distance, id) order (ids without a common order: equal distances in row
        order); a row with fewer than ``k`` eligible rows has -1 / inf in its unused slots.  The distances are ``search``'s, bit
        for bit: line r is what ``search_filtered(stored row r, k, exclude=[group of r])`` (or ``search(row r, k + 1)`` without
        r) returns.  Exact in every mode; ``mode`` as ``search_mode`` (2 takes k <= 100).  ``KeyError`` for an unknown id."""
        with self.lock:
            rows = None if ids is None else self._rows_of_ids(ids)
            return self._neighbors(rows, k, other_groups, group_of, mode)

    def neighbors_of(self, node_id: Hashable, k: int = 5, *, other_groups: bool = False, group_of: GROUP_OF = None) -> List[Dict]:
        """"More like this frame": the ``k`` nearest other stored rows of one stored id (``other_groups``: of other videos only),
        as ``search`` returns them: ``[{'id', 'distance', 'score'}]``.  ``KeyError`` for an unknown id."""
        with self.lock:
            rows = self._rows_of_ids([node_id])
            if k <= 0:
                return []
            out_rows, out_dist = self._neighbors(rows, k, other_groups, group_of, self.search_mode)
            return _hits(self._id_of(), out_rows[0].tolist(), out_dist[0])

    def synchronize(self) -> None:
        _lib.check(_lib.load().vq_index_synchronize(self._h))

    def set_stream(self, hip_stream: int) -> None:
        _lib.check(_lib.load().vq_index_set_stream(self._h, c_void_p(hip_stream or None)))

    def size(self) -> int:
        return self.element_count                                          # reference :302-304

    # -- persistence (reference :306-380: pickle + sha256 sidecar) ------------------
    def save(self, filepath: str) -> None:
        """Reference :306-339: same pickle keys, HIGHEST_PROTOCOL, SHA-256 sidecar.  The index is exact, so ``levels``
        and ``graph`` are flat: the reference class LOADS such a file (same rows, ids and parameters) but its graph
        walk has nothing to walk — a reference user re-adds the rows; files written by the
        reference load here and answer as the reference does.  The extra key ``exact_index`` marks files from here."""
        with self.lock:
            save_data = {
                "dimension": self.dimension, "M": self.M, "max_M": self.max_M,
                "ef_construction": self.ef_construction, "ef_search": self.ef_search,
                "level_generation_factor": self.level_generation_factor,
                "data": dict(self.data.items()), "levels": self.levels, "graph": self.graph,
                "entry_point": self.entry_point, "element_count": self.element_count,
                "exact_index": True,     # extra key: no navigable graph in this file
            }
            d = os.path.dirname(filepath)
            if d:
                os.makedirs(d, exist_ok=True)
            with open(filepath, "wb") as f:
                pickle.dump(save_data, f, protocol=pickle.HIGHEST_PROTOCOL)
            with open(filepath, "rb") as f:
                checksum = hashlib.sha256(f.read()).hexdigest()
            with open(filepath + ".sha256", "w") as f:
                f.write(checksum)

    def load(self, filepath: str) -> None:
        """Reference :341-380 (checksum check, missing sidecar tolerated, ValueError on mismatch).  Only ``data`` (and
        the parameters) are used; the rows are stored as given and MEASURED by the library (vq_index_add
        normalize=0, ``_append_stored``): a file whose rows are not unit-norm still searches exactly, on the fp32 scan."""
        try:
            with open(filepath, "rb") as f:
                current = hashlib.sha256(f.read()).hexdigest()
            with open(filepath + ".sha256", "r") as f:
                expected = f.read().strip()
            if current != expected:
                raise ValueError("Index file corrupted (checksum mismatch)")
        except FileNotFoundError:
            print("Warning: No checksum file found, skipping verification")
        with open(filepath, "rb") as f:
            s = pickle.load(f)
        with self.lock:
            if s["dimension"] != self.dimension:
                lib = _lib.load()
                lib.vq_index_destroy(self._h)
                h = c_void_p()
                _lib.check(lib.vq_index_create(int(s["dimension"]), ctypes.byref(h)))
                self._h = h
            else:
                _lib.check(_lib.load().vq_index_clear(self._h))
            self.dimension = s["dimension"]
            self.M, self.max_M = s["M"], s["max_M"]
            self.ef_construction, self.ef_search = s["ef_construction"], s["ef_search"]
            self.level_generation_factor = s["level_generation_factor"]
            self._reset_host_state()
            ids = list(s["data"].keys())
            if ids:                                                      # stored rows are already unit
                self._append_stored(np.ascontiguousarray(np.stack([np.asarray(s["data"][i], dtype=np.float32) for i in ids])), ids)
            self.entry_point = s["entry_point"]
            self.element_count = s["element_count"]

    # -- stats (reference :382-402) ---------------------------------------------------
    def get_stats(self) -> Dict:
        if self.search_times:
            avg = sum(self.search_times) / len(self.search_times)
            p95 = np.percentile(self.search_times, 95)
        else:
            avg = p95 = 0
        return {
            "element_count": self.element_count,
            "entry_point_level": 0,
            "avg_search_time_ms": avg,
            "p95_search_time_ms": p95,
            "total_searches": len(self.search_times),
            "dimension": self.dimension,
            "M": self.M,
            "ef_search": self.ef_search,
        }

    def last_search_stats(self) -> Dict[str, int]:
        st = (c_int64 * 3)()
        _lib.check(_lib.load().vq_index_last_search_stats(self._h, st))
        return {"verified": int(st[0]), "rescanned": int(st[1]), "exact_fallback": int(st[2])}

    def profile_begin(self) -> None:
        _lib.check(_lib.load().vq_index_profile_begin(self._h))

    def profile_end(self) -> Dict[str, dict]:
        lib = _lib.load()
        ms = (c_float * _lib.IDX_NCLASS)()
        cnt = (ctypes.c_int * _lib.IDX_NCLASS)()
        _lib.check(lib.vq_index_profile_end(self._h, ms, cnt))
        return {lib.vq_index_profile_class_name(i).decode(): {"ms": float(ms[i]), "launches": int(cnt[i])}
                for i in range(_lib.IDX_NCLASS)}

    def close(self) -> None:
        if getattr(self, "_h", None):
            _lib.load().vq_index_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class OptimizedHNSWIndex(HNSWIndex):
    """Reference :405-528.  ``use_numpy_optimization`` is accepted for signature
    compatibility; both classes run the same device scan."""

    def __init__(self, *args, use_numpy_optimization=True, **kwargs):
        super().__init__(*args, **kwargs)
        self.use_numpy_optimization = use_numpy_optimization
