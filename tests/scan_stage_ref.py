"""Stage reference of the index's fp16 scans (pass 1 of every fp16 search), in numpy and fp64.

What a scan is, restated from the kernels' comments (csrc/knn_scan_f16.h, knn_scan_small.h, knn_scan_fold.h, knn_grouped.h):
rows and queries are rounded to fp16 (round to nearest even), every (query, row) score is the fp32-accumulated sum of the
exact fp16 products, and per (query, stream of 128 rows) only the best two scores survive, as KEYS: the fp32 score with the
row's 7-bit index inside its stream written over the low mantissa bits.  Rows past the end of the index, and rows a filter
disallows, score as a large negative finite sentinel ("no row"); a stream the masked scan skips has two bare sentinels.  The
group-max scan keeps, per (query, group label), the largest score of the group's rows (no index bits).

The exact re-score behind the scan proves its answer from one sentence: "rows a stream did not emit <= that stream's 2nd
key", up to E = eps_unit(dim) * max|row| * |q|.  check_keys asserts that sentence, and everything else the keys must be,
for EVERY (query, stream); check_group_best does the same for every (query, group).  emulate_* is a plain numpy scan, so
that the checker can be shown sound (the reference itself stays inside E) and not vacuous (planted defects are caught)
without a GPU.

E is restated here term by term and never read from the library.
"""
from __future__ import annotations

import ctypes

import numpy as np

STREAM_ROWS = 128
NO_ROW_BELOW = np.float32(-1.0e38)                 # a key below this names no row (the kernels' sentinel is -3.0e38, or -inf)
SENTINEL = np.float32(-3.0e38)


# ---------------------------------------------------------------- the bound
def eps_unit(dim: int) -> float:
    """Worst |fp16 score - exact score| for a unit row and a unit query; scales with |row| |q| (its last term aside).
    operand rounding: both operands carry a relative error of 2^-11 (half an ulp of an 11-bit significand):
                      (1 + 2^-11)^2 - 1 = 2 * 2^-11 + 2^-22, times sum|x_i q_i| <= |x||q| (Cauchy-Schwarz)
    accumulation:     dim fp32 additions of exact products, each within one ulp (2^-23, truncating adders allowed) of a
                      partial sum bounded by sum|x_i q_i| <= |x||q|, in any order
    index bits:       the low 7 bits of the fp32 score are overwritten: < 2^7 ulps = 2^-16 relative
    subnormals:       an element below fp16's normal range is rounded with ABSOLUTE error 2^-25; over dim elements of one
                      operand against the other's norm: 2^-25 sqrt(dim) |other|, for either operand
    plus 2 % for the fp32 arithmetic the device evaluates the bound in."""
    operand = 2.0 * 2.0 ** -11 + 2.0 ** -22
    accumulation = dim * 2.0 ** -23
    index_bits = 2.0 ** -16
    subnormal = 2.0 * np.sqrt(float(dim)) * 2.0 ** -25
    return (operand + accumulation + index_bits + subnormal) * 1.02


def bound(rows: np.ndarray, queries: np.ndarray) -> np.ndarray:
    """E per query [nq], fp64.  The largest row norm, never below 1 (the index's measured range starts at [1, 1] and only widens)."""
    dim = rows.shape[1]
    rmax = max(1.0, float(np.sqrt((rows.astype(np.float64) ** 2).sum(1).max()))) if len(rows) else 1.0
    return eps_unit(dim) * rmax * np.sqrt((queries.astype(np.float64) ** 2).sum(1))


def exact_scores(rows: np.ndarray, queries: np.ndarray) -> np.ndarray:
    """[nq][n] fp64 scores of the fp32 data as given: one matmul."""
    return queries.astype(np.float64) @ rows.astype(np.float64).T


# ---------------------------------------------------------------- geometry, through the library's own row functions
_tables: dict = {}


def row_table(lib, layout: int, streams: int) -> np.ndarray:
    """[streams][128] int64: the row every (stream, local index) names, by vq_debug_scan_row_of (pure host)."""
    key = (layout, streams)
    if key not in _tables:
        f = lib.vq_debug_scan_row_of
        _tables[key] = np.array([[f(layout, s, l) for l in range(STREAM_ROWS)] for s in range(streams)], dtype=np.int64)
    return _tables[key]


def pad_rows(layout: int, n: int) -> int:
    rng = {1: 1024, 2: 2048, 3: 128}[layout]
    return (n + rng - 1) // rng * rng


# ---------------------------------------------------------------- the checkers
class StageError(AssertionError):
    pass


def _first(mask: np.ndarray):
    return tuple(int(v) for v in np.argwhere(mask)[0])


def check_keys(keys: np.ndarray, rows: np.ndarray, queries: np.ndarray, table: np.ndarray, allowed_rows: np.ndarray | None = None,
               q_block: int = 1024) -> float:
    """keys uint32 [nq][streams][2] against the fp32 rows [n][dim] and queries [nq][dim] they were scanned from.  allowed_rows:
    bool [n] of a masked scan, or bool [nq][n]: a mask per query (the tile scan of the library neighbours strikes PAIRS).
    Every (query, stream) takes part.  Returns max(|key - exact| / E) over the keys that name a row."""
    nq, streams, _ = keys.shape
    n = len(rows)
    assert table.shape == (streams, STREAM_ROWS) and len(queries) == nq
    in_range = table < n
    tclip = np.where(in_range, table, 0)
    per_query = allowed_rows is not None and np.ndim(allowed_rows) == 2
    if per_query:
        assert allowed_rows.shape == (nq, n)
        valid_all = None                                                                    # V of every (query, stream), built per block
    else:
        valid_all = (in_range & (allowed_rows[tclip] if allowed_rows is not None else True))[None]      # V of every stream [1][streams][128]
    E = bound(rows, queries)
    worst = 0.0
    q_block = max(1, min(q_block, (1 << 22) // (streams * STREAM_ROWS)))                     # <= 32 MiB per [queries][streams][128] fp64 array
    for q0 in range(0, nq, q_block):
        kb = keys[q0:q0 + q_block]
        nb = len(kb)
        valid = in_range[None] & allowed_rows[q0:q0 + q_block][:, tclip] if per_query else valid_all          # [nb or 1][streams][128]
        nvalid = valid.sum(2)
        kf = kb.view(np.float32).astype(np.float64)
        local = (kb & 127).astype(np.int64)
        is_row = kb.view(np.float32) > NO_ROW_BELOW
        if np.isnan(kf).any():
            raise StageError(f"query {q0 + _first(np.isnan(kf))[0]}: a key is NaN")
        bad = ~(kf[..., 0] >= kf[..., 1])
        if bad.any():
            q, s = _first(bad)
            raise StageError(f"query {q0 + q} stream {s}: key1 {kf[q, s, 0]} < key2 {kf[q, s, 1]}")
        want_rows = np.minimum(nvalid, 2)
        bad = is_row.sum(2) != want_rows
        if bad.any():
            q, s = _first(bad)
            raise StageError(f"query {q0 + q} stream {s}: {int(is_row[q, s].sum())} keys name a row, the stream holds {int(nvalid[q if per_query else 0, s])} "
                             f"(allowed) rows below n = {n}")
        bad = is_row & ~np.take_along_axis(np.broadcast_to(valid, (nb, streams, STREAM_ROWS)), local, axis=2)
        if bad.any():
            q, s, w = _first(bad)
            raise StageError(f"query {q0 + q} stream {s} key {w + 1}: names row {int(table[s, local[q, s, w]])}, which is past n = {n} "
                             f"or not allowed")
        bad = is_row[..., 0] & is_row[..., 1] & (local[..., 0] == local[..., 1])
        if bad.any():
            q, s = _first(bad)
            raise StageError(f"query {q0 + q} stream {s}: both keys name row {int(table[s, local[q, s, 0]])}")
        ex = exact_scores(rows, queries[q0:q0 + q_block])                                    # [nb][n]
        per = np.where(valid, ex[:, tclip.reshape(-1)].reshape(nb, streams, STREAM_ROWS), -np.inf)     # exact score of every (stream, local)
        named = np.take_along_axis(per, local, axis=2)                                       # [nb][streams][2]
        err = np.where(is_row, np.abs(kf - named), 0.0)
        Eb = E[q0:q0 + q_block][:, None, None]
        bad = err > Eb
        if bad.any():
            q, s, w = _first(bad)
            raise StageError(f"query {q0 + q} stream {s} key {w + 1}: {kf[q, s, w]!r} names row {int(table[s, local[q, s, w]])} whose exact "
                             f"score is {named[q, s, w]!r}: off by {err[q, s, w]:.4g} = {err[q, s, w] / Eb[q, 0, 0]:.3f} E")
        worst = max(worst, float((err / Eb).max()))
        # soundness: every row of V the stream did not emit lies at or below key2 + E
        rest = per.copy()
        np.put_along_axis(rest, np.where(is_row, local, local[..., :1]), -np.inf, axis=2)     # (a "no row" key removes nothing new)
        if not is_row[..., 0].all():                                                        # key1 itself "no row": nothing may be removed
            rest = np.where(is_row[..., :1], rest, per)
        top = rest.max(2)
        key2 = np.where(is_row[..., 1], kf[..., 1], -np.inf)                                # a "no row" second key bounds nothing
        bad = top > key2 + Eb[..., 0]
        if bad.any():
            q, s = _first(bad)
            r = int(table[s, int(rest[q, s].argmax())])
            raise StageError(f"query {q0 + q} stream {s}: row {r} was not emitted, its exact score {top[q, s]!r} exceeds key2 "
                             f"{key2[q, s]!r} + E ({Eb[q, 0, 0]:.4g}) by {(top[q, s] - key2[q, s]) / Eb[q, 0, 0]:.3f} E")
    return worst


def check_group_best(best: np.ndarray, rows: np.ndarray, queries: np.ndarray, labels: np.ndarray, n_groups: int,
                     allowed_groups: np.ndarray | None = None) -> float:
    """best float32 [nq][G] (NaN = no row seen) against the largest exact score over each group's rows.  No index bits are packed
    into a group maximum; the bound is the same E.  Returns max(|best - exact max| / E)."""
    nq = len(queries)
    assert best.shape == (nq, n_groups) and len(labels) == len(rows)
    ex = exact_scores(rows, queries)
    want = np.full((nq, n_groups), -np.inf)
    order = np.argsort(labels, kind="stable")
    starts = np.searchsorted(labels[order], np.arange(n_groups))
    assert (np.bincount(labels, minlength=n_groups) > 0).all(), "labels are dense"
    want = np.maximum.reduceat(ex[:, order], starts, axis=1)
    seen = np.ones(n_groups, bool) if allowed_groups is None else np.asarray(allowed_groups, bool)
    none = np.isnan(best)
    bad = none != ~seen[None, :]
    if bad.any():
        q, g = _first(bad)
        raise StageError(f"query {q} group {g}: reads {'none' if none[q, g] else best[q, g]}, the group {'has' if seen[g] else 'has no'} allowed row")
    E = bound(rows, queries)[:, None]
    err = np.where(seen[None, :], np.abs(np.where(none, 0.0, best.astype(np.float64)) - want), 0.0)
    bad = err > E
    if bad.any():
        q, g = _first(bad)
        raise StageError(f"query {q} group {g}: best {best[q, g]!r}, the group's largest exact score is {want[q, g]!r}: off by "
                         f"{err[q, g] / E[q, 0]:.3f} E")
    return float((err / E).max())


# ---------------------------------------------------------------- a plain numpy scan
def fp16_scores(rows: np.ndarray, queries: np.ndarray, skip_slice: tuple | None = None) -> np.ndarray:
    """[nq][n] float32: RNE to fp16, exact products (22 significant bits: exact in fp32), sequential fp32 accumulation.
    skip_slice = (row, k0): PLANTED DEFECT, the 32 elements from k0 are left out of that row's score."""
    r16 = rows.astype(np.float16).astype(np.float32)
    q16 = queries.astype(np.float16).astype(np.float32)
    acc = np.zeros((len(queries), len(rows)), np.float32)
    for k in range(rows.shape[1]):
        p = q16[:, k:k + 1] * r16[None, :, k]
        if skip_slice is not None and skip_slice[1] <= k < skip_slice[1] + 32:
            p[:, skip_slice[0]] = 0.0
        acc = acc + p
    return acc


def emulate_keys(rows: np.ndarray, queries: np.ndarray, table: np.ndarray, allowed_rows: np.ndarray | None = None,
                 stream_label: np.ndarray | None = None, n_scan: int | None = None, drop: tuple | None = None,
                 skip_slice: tuple | None = None, third: bool = False) -> np.ndarray:
    """uint32 [nq][streams][2] (third: [..][3], the third best behind them).  allowed_rows: the masked scan; stream_label [streams]:
    the label all 128 rows of a stream share or -1, with allowed_rows a uniformly disallowed stream is skipped (two bare sentinels).
    PLANTED DEFECTS: n_scan, the row count the ragged mask uses (the rows behind n read as zeros, like the device's pad);
    drop = (stream, local), a row the fold skips; skip_slice as in fp16_scores."""
    n, dim = rows.shape
    streams = len(table)
    n_mask = n if n_scan is None else n_scan
    padded = np.zeros((int(table.max()) + 1, dim), np.float32)
    padded[:n] = rows
    sc = fp16_scores(padded, queries, skip_slice)                                          # [nq][n_pad]
    live = table < n_mask
    if allowed_rows is not None and np.ndim(allowed_rows) == 2:                              # a mask per query [nq][n] (no stream is skipped)
        assert stream_label is None
        ok = np.zeros((len(queries), len(padded)), bool)
        ok[:, :n] = allowed_rows
        live = live[None] & ok[:, table]
    elif allowed_rows is not None:
        ok = np.zeros(len(padded), bool)
        ok[:n] = allowed_rows
        live = live & ok[table]
    if drop is not None:
        live = live.copy()
        live[..., drop[0], drop[1]] = False
    if live.ndim == 2:
        live = live[None]
    v = np.where(live, sc[:, table.reshape(-1)].reshape(len(queries), streams, STREAM_ROWS), SENTINEL).astype(np.float32)
    bits = (v.view(np.uint32) & np.uint32(0xFFFFFF80)) | np.arange(STREAM_ROWS, dtype=np.uint32)[None, None, :]
    if drop is not None:                                                                    # a skipped row is not folded at all
        bits[:, drop[0], drop[1]] = np.float32(-np.inf).view(np.uint32)
    order = np.argsort(-bits.view(np.float32).astype(np.float64), axis=2, kind="stable")[..., :3 if third else 2]
    out = np.take_along_axis(bits, order, axis=2)
    if allowed_rows is not None and stream_label is not None:
        for s in range(streams):
            if stream_label[s] >= 0 and not live[0, s].any():
                out[:, s, :] = SENTINEL.view(np.uint32)
    return np.ascontiguousarray(out)


def emulate_group_best(rows: np.ndarray, queries: np.ndarray, labels: np.ndarray, n_groups: int,
                       allowed_groups: np.ndarray | None = None, truncate_row: int | None = None) -> np.ndarray:
    """float32 [nq][G], NaN where no allowed row was seen.  PLANTED DEFECT: truncate_row, a row a run of labels loses."""
    sc = fp16_scores(rows, queries)
    best = np.full((len(queries), n_groups), np.nan, np.float32)
    for g in range(n_groups):
        if allowed_groups is not None and not allowed_groups[g]:
            continue
        members = np.flatnonzero(labels == g)
        if truncate_row is not None:
            members = members[members != truncate_row]
        if len(members):
            best[:, g] = sc[:, members].max(1)
    return best


# ---------------------------------------------------------------- input classes (rows are stored as given: normalize = 0)
def unit(x: np.ndarray) -> np.ndarray:
    x = x.astype(np.float64)
    return (x / np.sqrt((x ** 2).sum(-1, keepdims=True))).astype(np.float32)


def gaussian_unit(rng, n: int, dim: int) -> np.ndarray:
    return unit(rng.standard_normal((n, dim)))


def midpoints(rng, n: int, dim: int) -> np.ndarray:
    """Every element c (1 + 2^-11), c a random power of two with a random sign: exactly half way between two fp16 values, so every
    conversion takes the full half ulp.  Each row is scaled by a power of two (midpoints stay midpoints) into 0.5 <= |row|^2 < 2."""
    c = 2.0 ** -rng.integers(1, 6, (n, dim)).astype(np.float64) * rng.choice([-1.0, 1.0], (n, dim))
    x = c * (1.0 + 2.0 ** -11)
    scale = 2.0 ** -np.round(np.log2(np.sqrt((x ** 2).sum(1, keepdims=True))))
    return (x * scale).astype(np.float32)


def outlier_rows(rng, n: int, dim: int) -> np.ndarray:
    """One channel carries the row; every other element lies in fp16's subnormal range (below 2^-14), where rounding is absolute."""
    x = (rng.uniform(2.0 ** -24, 2.0 ** -15, (n, dim)) * rng.choice([-1.0, 1.0], (n, dim)))
    x[np.arange(n), rng.integers(0, dim, n)] = rng.choice([-1.0, 1.0], n) * rng.uniform(0.98, 1.0, n)
    return x.astype(np.float32)


def scaled_queries(rng, nq: int, dim: int) -> np.ndarray:
    """Gaussian directions at |q|^2 = 0.26 and 3.9 alternately: the ends of the range the fp16 proof covers."""
    q = gaussian_unit(rng, nq, dim).astype(np.float64)
    q *= np.sqrt(np.where(np.arange(nq) % 2 == 0, 0.26, 3.9))[:, None]
    return q.astype(np.float32)


def unnormalised_rows(rng, n: int, dim: int) -> np.ndarray:
    x = gaussian_unit(rng, n, dim).astype(np.float64) * np.sqrt(rng.uniform(0.51, 1.99, (n, 1)))
    x[0] *= np.sqrt(1.99) / np.sqrt((x[0] ** 2).sum())                                      # the ends of the spread are present
    if n > 1:
        x[-1] *= np.sqrt(0.51) / np.sqrt((x[-1] ** 2).sum())
    return x.astype(np.float32)


def identical_rows(rng, n: int, dim: int) -> np.ndarray:
    return np.repeat(gaussian_unit(rng, 1, dim), n, axis=0)


def input_class(name: str, rng, n: int, nq: int, dim: int):
    """(rows, queries) of one of the classes every kernel family is run on once."""
    if name == "gaussian":
        return gaussian_unit(rng, n, dim), gaussian_unit(rng, nq, dim)
    if name == "midpoints":
        rows = midpoints(rng, n, dim)
        return rows, rows[rng.integers(0, n, nq)].copy()
    if name == "outlier":
        rows = outlier_rows(rng, n, dim)
        qs = gaussian_unit(rng, nq, dim)
        qs[::2] = rows[rng.integers(0, n, len(qs[::2]))]                                    # queried by itself and by Gaussian queries
        return rows, qs
    if name == "qnorm":
        return gaussian_unit(rng, n, dim), scaled_queries(rng, nq, dim)
    if name == "unnormalised":
        return unnormalised_rows(rng, n, dim), gaussian_unit(rng, nq, dim)
    if name == "identical":
        return identical_rows(rng, n, dim), gaussian_unit(rng, nq, dim)
    raise KeyError(name)


INPUT_CLASSES = ("gaussian", "midpoints", "outlier", "qnorm", "unnormalised", "identical")


def stream_labels(labels: np.ndarray) -> np.ndarray:
    """Per 128-row stream the label all its rows share, or -1 (the labels are padded with -1: a ragged stream is mixed)."""
    n = len(labels)
    streams = (n + STREAM_ROWS - 1) // STREAM_ROWS
    pad = np.full(streams * STREAM_ROWS, -1, np.int64)
    pad[:n] = labels
    pad = pad.reshape(streams, STREAM_ROWS)
    return np.where((pad == pad[:, :1]).all(1), pad[:, 0], -1)


# ---------------------------------------------------------------- read-back through the debug entries (GPU tests)
def read_scan_keys(lib, check, handle):
    """-> (info dict, keys uint32 [cur][streams][2])"""
    info = (ctypes.c_int64 * 5)()
    check(lib.vq_index_debug_read_scan_keys(handle, info, None, 0))
    q0, cur, layout, streams, masked = (int(v) for v in info)
    keys = np.empty((cur, streams, 2), np.uint32)
    check(lib.vq_index_debug_read_scan_keys(handle, info, keys.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), keys.size))
    return dict(q0=q0, cur=cur, layout=layout, streams=streams, masked=masked), keys


def read_group_best(lib, check, handle):
    """-> (info dict, best float32 [cur][n_groups], NaN = none)"""
    info = (ctypes.c_int64 * 3)()
    check(lib.vq_index_debug_read_group_best(handle, info, None, 0))
    q0, cur, G = (int(v) for v in info)
    best = np.empty((cur, G), np.float32)
    check(lib.vq_index_debug_read_group_best(handle, info, best.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), best.size))
    return dict(q0=q0, cur=cur, n_groups=G), best
