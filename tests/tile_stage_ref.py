"""Stage reference of the streamed 256 x 256 tile scans (csrc/scan_stream256.h), in numpy and fp64: pass 1 of the library
neighbours (neighbors_tile_kernel), of zero-shot labelling (label_tile_kernel), of the shared-footage search
(match_tile_kernel) and of the clip search (set_group_max_kernel, checked by scan_stage_ref.check_group_best as it is).

What the four kernels share, restated from their comments: a workgroup keeps 256 RESIDENT fp16 rows (asked rows, stored rows,
queries) and streams up to eight 256-row tiles of the other operand past them in one K loop; wave (wr, wc) owns resident rows
128 wr .. + 127 and streamed rows 64 wc .. + 63 of every tile, and a finished tile is folded a QUADRANT (hm, hn) at a time:
resident rows 128 wr + 64 hm .. + 63 against streamed rows 64 wc + 32 hn .. + 31, for every wave at once.  A lane's streamed
rows of one range are a 128-row stream; the 7-bit local index of row (tile t, ni, r) is t * 16 + ni * 4 + r.

  neighbours   keys as the batch scans' (layout 2): fp32 score, local index over the low 7 bits; a struck pair (equal tags)
               and a pad row enter the fold as the sentinel -3e38; a tile that holds no row is not folded (-inf stays).
  label        per (row, range of 2,048 prompts): K1, J1, K2, J2, F: the three largest order-preserving keys (score_key, the
               INVERTED local index in the low 7 bits; decoding clears them), the prompts of the first two; pad prompts: key 0.
  match        x = fp32(s16 - T) against e_i = fp32(E_i + MATCH_SLACK): sure hit / sure miss / filed; the final table holds
               the sure hits and the filed pairs the exact chain decided.

The tolerance is scan_stage_ref's E = eps_unit(dim) * max(1, max|row|) * |q|, and for the filed band 2 E + MATCH_SLACK + 2^-22
(knn_match.h derives it: |s16 - T32| <= e_i = E_i + slack, |s16 - s| <= E_i, and T32, the difference and the reported distance
round by at most 2^-22 together).  Nothing is read from the library.

emulate_* run the same folds in numpy over scan_stage_ref.fp16_scores, with the defects this mainloop can have as switches:
  plant = ("stale", t, half, k0)     the 64-wide K slice from k0 of streamed tile t, 128-row half `half`, holds tile t - 1's
  plant = ("noclear", t, hm, hn)     quadrant (hm, hn) of tile t starts from tile t - 1's accumulators
  plant = ("fold", t, hm, hn)        quadrant (hm, hn) of tile t is folded under tile number t - 1
(t counts the streamed tiles of the whole operand; t % 8 != 0, so t - 1 is in the same range.)
"""
from __future__ import annotations

import ctypes

import numpy as np

from scan_stage_ref import (INPUT_CLASSES, NO_ROW_BELOW, SENTINEL, STREAM_ROWS, StageError, _first, bound, check_group_best, check_keys,  # noqa: F401
                            emulate_group_best, eps_unit, exact_scores, fp16_scores, input_class, unnormalised_rows)

TILE = 256                     # resident rows per workgroup, streamed rows per tile
RANGE = 2048                   # streamed rows (prompts) per workgroup: eight tiles
MATCH_SLACK = 2.0 ** -19       # knn_match.h
LABEL_PARTS = 5                # k1, j1, k2, j2, f
PAD_TAG = -2 ** 31


def round_up(v: int, m: int) -> int:
    return (v + m - 1) // m * m


# ---------------------------------------------------------------- geometry (key layout 2, restated; the CPU test compares it
# with the library's vq_debug_scan_row_of)
def local_of(col: np.ndarray) -> np.ndarray:
    """lane-local index of streamed row `col` (counted from its range's first row): t * 16 + ni * 4 + r"""
    c = col % TILE
    return (col // TILE) * 16 + ((c % 64) // 16) * 4 + c % 4


def stream_of(row: np.ndarray) -> np.ndarray:
    """the 128-row stream of matrix row `row`: range * 16 + wc * 4 + lane group"""
    c = row % TILE
    return (row // RANGE) * 16 + (c // 64) * 4 + (c % 16) // 4


def table2(streams: int) -> np.ndarray:
    """[streams][128] int64: the row of (stream, local)"""
    rows = np.arange(streams * STREAM_ROWS)
    t = np.empty((streams, STREAM_ROWS), np.int64)
    t[stream_of(rows), local_of(rows % RANGE)] = rows
    return t


def quadrant(res: np.ndarray, col: np.ndarray, t: int, hm: int, hn: int) -> np.ndarray:
    """bool [len(res)][len(col)]: the cells of quadrant (hm, hn) of streamed tile t, for every wave"""
    return (((res % 128) // 64 == hm)[:, None]) & ((col // TILE == t) & ((col % 64) // 32 == hn))[None, :]


# ---------------------------------------------------------------- the mainloop in numpy
def tile_scores(resident: np.ndarray, streamed: np.ndarray, plant: tuple | None = None) -> np.ndarray:
    """float32 [len(resident)][len(streamed)]; len(streamed) % 256 == 0 (pad rows zero).  plant: "stale" or "noclear" (above)."""
    assert len(streamed) % TILE == 0
    w = streamed
    if plant is not None and plant[0] == "stale":
        _, t, half, k0 = plant
        assert t % 8 != 0 and (t + 1) * TILE <= len(streamed)
        w = streamed.copy()
        at = t * TILE + half * 128
        w[at:at + 128, k0:k0 + 64] = streamed[at - TILE:at - TILE + 128, k0:k0 + 64]
    sc = fp16_scores(w, resident)
    if plant is not None and plant[0] == "noclear":
        _, t, hm, hn = plant
        assert t % 8 != 0 and (t + 1) * TILE <= len(streamed)
        cells = quadrant(np.arange(len(resident)), np.arange(len(streamed)), t, hm, hn)
        sc = np.where(cells, sc + np.roll(sc, TILE, axis=1), sc).astype(np.float32)
    return sc


# ---------------------------------------------------------------- library neighbours
def allowed_from_tags(qtag: np.ndarray, rtag: np.ndarray) -> np.ndarray:
    """bool [nq][n]: a pair is struck when its tags are equal"""
    return qtag[:, None] != rtag[None, :]


def emulate_neighbor_keys(rows: np.ndarray, asked: np.ndarray, tags: np.ndarray, plant: tuple | None = None, n_scan: int | None = None,
                          leak: tuple | None = None) -> np.ndarray:
    """uint32 [len(asked)][streams][2] of one chunk.  tags [n]: the rows' numbers (exclude = 0) or labels (exclude = 1).
    PLANTED DEFECTS: plant (module docstring); n_scan: the row count the pad mask uses; leak = (asked index, row): a struck
    pair that is folded as if it were eligible."""
    n, dim = rows.shape
    n_pad = round_up(n, RANGE)
    streams = n_pad // STREAM_ROWS
    n_mask = n if n_scan is None else n_scan
    x = np.zeros((n_pad, dim), np.float32)
    x[:n] = rows
    q = rows[asked]
    used = round_up(max(n, n_mask), TILE)                                                   # (the tiles behind hold zeros and are not folded)
    sc = np.zeros((len(asked), n_pad), np.float32)
    sc[:, :used] = tile_scores(q, x[:used], plant if plant and plant[0] != "fold" else None)
    col = np.arange(n_pad)
    ok = np.zeros((len(asked), n_pad), bool)
    ok[:, :n_mask] = True
    ok[:, :n] &= allowed_from_tags(tags[asked], tags)
    if leak is not None:
        ok[leak] = True
    v = np.where(ok, sc, SENTINEL).astype(np.float32)
    loc = np.broadcast_to(local_of(col % RANGE)[None, :], v.shape).astype(np.uint32)
    if plant is not None and plant[0] == "fold":
        _, t, hm, hn = plant
        assert t % 8 != 0
        loc = np.where(quadrant(np.arange(len(asked)) % TILE, col, t, hm, hn), loc - 16, loc).astype(np.uint32)
    bits = (v.view(np.uint32) & np.uint32(0xFFFFFF80)) | loc
    folded = (col // TILE * TILE) < n                                                       # a tile without a row is not streamed
    bits = np.where(folded[None, :], bits, np.float32(-np.inf).view(np.uint32))
    order = np.argsort(stream_of(col), kind="stable")                                       # columns grouped by stream, 128 each
    per = bits[:, order].reshape(len(asked), streams, STREAM_ROWS)
    top = np.argsort(-per.view(np.float32).astype(np.float64), axis=2, kind="stable")[..., :2]
    return np.ascontiguousarray(np.take_along_axis(per, top, axis=2))


# ---------------------------------------------------------------- labelling
def score_key(s: np.ndarray) -> np.ndarray:
    u = np.ascontiguousarray(s, np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def label_key_score(key: np.ndarray) -> np.ndarray:
    """fp64 score of a label key, index bits cleared (knn_label.h label_key_score); key 0 ("nothing") decodes to -inf here"""
    k = np.asarray(key, np.uint32) & np.uint32(0xFFFFFF80)
    u = np.where(k & np.uint32(0x80000000), k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32)
    return np.where(np.asarray(key) == 0, -np.inf, u.view(np.float32).astype(np.float64))


def label_shape(n: int, P: int):
    """-> (n_pad, ranges)"""
    return round_up(n, TILE), (round_up(P, TILE) // TILE + 7) // 8


def emulate_label_parts(rows: np.ndarray, prompts: np.ndarray, plant: tuple | None = None, p_scan: int | None = None,
                        floor_rank: int = 3) -> np.ndarray:
    """uint32 [ranges][5][n_pad].  PLANTED DEFECTS: plant (module docstring); p_scan: the prompt count the pad mask uses;
    floor_rank = 4: F is the fourth largest key."""
    n, dim = rows.shape
    P = len(prompts)
    n_pad, ranges = label_shape(n, P)
    p_pad = round_up(P, TILE)
    p_mask = P if p_scan is None else p_scan
    x = np.zeros((n_pad, dim), np.float32)
    x[:n] = rows
    w = np.zeros((p_pad, dim), np.float32)
    w[:P] = prompts
    sc = np.zeros((n_pad, p_pad), np.float32)                                               # (a pad row is zero: so are its scores)
    sc[:n] = tile_scores(x[:n], w, plant if plant and plant[0] != "fold" else None)
    col = np.arange(p_pad)
    loc = np.broadcast_to(local_of(col % RANGE)[None, :], sc.shape).astype(np.uint32)
    name = np.broadcast_to(col[None, :], sc.shape).astype(np.int64)
    if plant is not None and plant[0] == "fold":
        _, t, hm, hn = plant
        assert t % 8 != 0
        cells = quadrant(np.arange(n_pad) % TILE, col, t, hm, hn)
        loc = np.where(cells, loc - 16, loc).astype(np.uint32)
        name = np.where(cells, name - TILE, name)
    key = (score_key(sc).reshape(sc.shape) & np.uint32(0xFFFFFF80)) | (np.uint32(127) - loc)
    key = np.where((col < p_mask)[None, :], key, np.uint32(0))
    parts = np.zeros((ranges, LABEL_PARTS, n_pad), np.uint32)
    for g in range(ranges):
        kk, nn = key[:, g * RANGE:(g + 1) * RANGE], name[:, g * RANGE:(g + 1) * RANGE]
        kk = np.concatenate([kk, np.zeros((n_pad, 4), np.uint32)], axis=1)                   # a range of fewer than four prompts
        nn = np.concatenate([nn, np.full((n_pad, 4), -1, np.int64)], axis=1)
        top = np.argsort(-kk.astype(np.int64), axis=1, kind="stable")[:, :4]
        k = np.take_along_axis(kk, top, axis=1)
        j = np.where(k == 0, -1, np.take_along_axis(nn, top, axis=1))
        parts[g, 0], parts[g, 1] = k[:, 0], j[:, 0].astype(np.int32).view(np.uint32)
        parts[g, 2], parts[g, 3] = k[:, 1], j[:, 1].astype(np.int32).view(np.uint32)
        parts[g, 4] = k[:, floor_rank - 1]
    return parts


def check_label_parts(parts: np.ndarray, n: int, rows: np.ndarray, prompts: np.ndarray) -> float:
    """parts uint32 [ranges][5][n_pad] against the fp32 rows [n][dim] and prompts [P][dim].  Every (row < n, range) takes part.
    E(j) = eps_unit(dim) * max(1, max|row|) * |p_j|; where a key's prompt is not known (the floor F) the range's largest E.
    Returns max(|decode(K) - exact| / E) over K1 and K2."""
    P, dim = prompts.shape
    n_pad, ranges = label_shape(n, P)
    assert parts.shape == (ranges, LABEL_PARTS, n_pad) and len(rows) == n
    worst = 0.0
    for g in range(ranges):
        j0, j1 = g * RANGE, min(P, (g + 1) * RANGE)
        cnt = j1 - j0
        K1, K2, F = parts[g, 0, :n], parts[g, 2, :n], parts[g, 4, :n]
        J1, J2 = parts[g, 1, :n].view(np.int32).astype(np.int64), parts[g, 3, :n].view(np.int32).astype(np.int64)
        where = f"range {g}"

        def fail(mask, text):
            r = _first(mask)[0]
            raise StageError(f"row {r} {where}: " + text(r))
        bad = (K1 == 0) | ((K2 == 0) != (cnt == 1)) | ((F == 0) != (cnt <= 2))
        if bad.any():
            fail(bad, lambda r: f"K1 {K1[r]:#x} K2 {K2[r]:#x} F {F[r]:#x}: the range holds {cnt} prompts (K2 == 0 iff one, F == 0 iff at most two)")
        has2 = K2 != 0
        bad = (J1 < j0) | (J1 >= j1) | (has2 & ((J2 < j0) | (J2 >= j1)))
        if bad.any():
            fail(bad, lambda r: f"J1 {J1[r]} J2 {J2[r]}: outside the range's prompts {j0} .. {j1 - 1} (P = {P})")
        bad = has2 & (J1 == J2)
        if bad.any():
            fail(bad, lambda r: f"both keys name prompt {J1[r]}")
        d1, d2, dF = label_key_score(K1), label_key_score(K2), label_key_score(F)
        bad = ~((d1 >= d2) & (d2 >= dF))
        if bad.any():
            fail(bad, lambda r: f"K1 {d1[r]!r} >= K2 {d2[r]!r} >= F {dF[r]!r} does not hold")
        ex = exact_scores(prompts[j0:j1], rows)                                              # [n][cnt]
        E = bound(rows, prompts[j0:j1])                                                      # [cnt]
        rr = np.arange(n)
        for which, d, J, has in ((1, d1, J1, np.ones(n, bool)), (2, d2, J2, has2)):
            jj = np.where(has, J - j0, 0)
            err = np.where(has, np.abs(np.where(has, d, 0.0) - ex[rr, jj]), 0.0)
            bad = err > E[jj]
            if bad.any():
                fail(bad, lambda r: f"K{which} {d[r]!r} names prompt {J[r]} whose exact score is {ex[r, jj[r]]!r}: off by "
                                    f"{err[r] / E[jj[r]]:.3f} E")
            worst = max(worst, float((err / E[jj]).max()))
        if cnt > 2:
            rest = ex - E[None, :]                                                           # s(j) - E(j) <= decode(F) for every other prompt
            rest[rr, J1 - j0] = -np.inf
            rest[rr, J2 - j0] = -np.inf
            top = rest.max(1)
            bad = top > dF
            if bad.any():
                fail(bad, lambda r: f"prompt {j0 + int(rest[r].argmax())} is neither J1 nor J2, its exact score "
                                    f"{ex[r, int(rest[r].argmax())]!r} exceeds the floor {dF[r]!r} + E")
            third = -np.partition(-ex, 2, axis=1)[:, 2]
            bad = dF > third + E.max()
            if bad.any():
                fail(bad, lambda r: f"the floor {dF[r]!r} exceeds the third largest exact score {third[r]!r} + E")
    return worst


# ---------------------------------------------------------------- shared-footage search
def pack_bits(hit: np.ndarray) -> np.ndarray:
    """bool [m][n] -> uint32 [m][ceil(n / 32)], bit r & 31 of word r >> 5"""
    m, n = hit.shape
    W = (max(n, 1) + 31) // 32
    padded = np.zeros((m, W * 32), np.uint8)
    padded[:, :n] = hit
    return np.packbits(padded.reshape(m, W, 32), axis=2, bitorder="little").view(np.uint32).reshape(m, W)


def unpack_bits(bits: np.ndarray) -> np.ndarray:
    """uint32 [m][W] -> bool [m][W * 32]"""
    m, W = bits.shape
    return np.unpackbits(np.ascontiguousarray(bits).view(np.uint8).reshape(m, W * 4), axis=1, bitorder="little").astype(bool)


def match_threshold(max_dist) -> float:
    return 1.0 - float(np.float64(np.float32(max_dist)))


def threshold_conditions(ex: np.ndarray, max_dist) -> tuple:
    """-> (a pair lies within MATCH_SLACK / 2 of T, no score lies within 2^-21 of T)"""
    gap = np.abs(ex - match_threshold(max_dist)).min()
    return bool(gap <= MATCH_SLACK / 2), bool(gap > 2.0 ** -21)


def choose_max_dist(ex: np.ndarray, skip: int = 4) -> np.float32:
    """A threshold just beside one of the largest exact scores: T = that score - 1.5 * 2^-21 or so, so that the pair is a hit
    inside MATCH_SLACK / 2 of T and no score is within 2^-21 of T (where the device's own fp32 roundings may decide either way)."""
    top = np.unique(ex)[::-1]
    for s in top[min(skip, len(top) - 1):][:400]:
        max_dist = np.float32(1.0 - (s - 1.5 * 2.0 ** -21))
        if all(threshold_conditions(ex, max_dist)):
            return max_dist
    raise AssertionError("no threshold beside one of the largest 400 scores satisfies both conditions")


def emulate_match(rows: np.ndarray, queries: np.ndarray, max_dist, cap: int = 1 << 24, plant: tuple | None = None):
    """-> (bits uint32 [m][W], filed uint64 [count] = (query << 32) | row, info dict).  The filed pairs are decided by the exact
    scores (the caller's threshold keeps every score 2^-21 away from T)."""
    m, dim = queries.shape
    n = len(rows)
    x = np.zeros((round_up(n, RANGE), dim), np.float32)
    x[:n] = rows
    sc = tile_scores(queries, x[:round_up(n, TILE)], plant)[:, :n]
    T = match_threshold(max_dist)
    T32 = np.float32(T)
    rmax = max(1.0, float(np.sqrt((rows.astype(np.float64) ** 2).sum(1).max())))
    e = (np.float32(eps_unit(dim) * rmax) * np.sqrt((queries.astype(np.float64) ** 2).sum(1)).astype(np.float32)
         + np.float32(MATCH_SLACK)).astype(np.float32)[:, None]
    d = (sc - T32).astype(np.float32)
    sure = d > e
    undecided = ~(d > e) & ~(d < -e)
    qi, ri = np.nonzero(undecided)
    filed = (qi.astype(np.uint64) << np.uint64(32)) | ri.astype(np.uint64)
    hit = sure | (undecided & (exact_scores(rows, queries) > T))
    info = dict(m=m, W=(max(n, 1) + 31) // 32, n=n, cursor=len(filed), flag=0, cap=cap)
    return pack_bits(hit), filed, info


def check_match_bits(bits: np.ndarray, filed: np.ndarray, info: dict, rows: np.ndarray, queries: np.ndarray, max_dist,
                     redone: bool = False) -> float:
    """The final bit table and the filed list of a tile-path call against the exact scores; T = 1 - float64(max_dist).
    redone: the call whose list overflowed (flag == 2): only the table is checked.  Returns max(|s - T| / band) over the
    filed pairs, band = 2 E_q + MATCH_SLACK + 2^-22."""
    m, n = len(queries), len(rows)
    W = (max(n, 1) + 31) // 32
    assert (info["m"], info["W"], info["n"]) == (m, W, n) and bits.shape == (m, W), info
    T = match_threshold(max_dist)
    ex = exact_scores(rows, queries)
    dist = np.abs(ex - T)
    worst = 0.0
    if not redone:
        if info["flag"] != 0:
            raise StageError(f"the call is flagged {info['flag']}")
        if info["cursor"] > info["cap"] or len(filed) != info["cursor"]:
            raise StageError(f"the cursor {info['cursor']} exceeds the capacity {info['cap']}, or {len(filed)} pairs were read")
        fq, fr = (filed >> np.uint64(32)).astype(np.int64), (filed & np.uint64(0xFFFFFFFF)).astype(np.int64)
        bad = (fq >= m) | (fr >= n)
        if bad.any():
            i = _first(bad)[0]
            raise StageError(f"filed pair {i}: query {fq[i]} row {fr[i]} is outside m = {m}, n = {n}")
        if len(np.unique(filed)) != len(filed):
            u, c = np.unique(filed, return_counts=True)
            d = int(u[c > 1][0])
            raise StageError(f"query {d >> 32} row {d & 0xFFFFFFFF} is filed {int(c[c > 1][0])} times")
        band = 2.0 * bound(rows, queries) + MATCH_SLACK + 2.0 ** -22
        bad = dist[fq, fr] > band[fq]
        if bad.any():
            i = _first(bad)[0]
            raise StageError(f"query {fq[i]} row {fr[i]} is filed, its exact score {ex[fq[i], fr[i]]!r} is {dist[fq[i], fr[i]]:.4g} from T = {T!r}: "
                             f"outside the band {band[fq[i]]:.4g}")
        if len(filed):
            worst = float((dist[fq, fr] / band[fq]).max())
        is_filed = np.zeros((m, n), bool)
        is_filed[fq, fr] = True
        bad = (dist <= MATCH_SLACK / 2) & ~is_filed
        if bad.any():
            q, r = _first(bad)
            raise StageError(f"query {q} row {r} is not filed, its exact score {ex[q, r]!r} is {dist[q, r]:.4g} from T = {T!r}: a sure "
                             f"verdict needs more than MATCH_SLACK")
    got = unpack_bits(bits)
    bad = got[:, :n] != (ex > T)
    if bad.any():
        q, r = _first(bad)
        raise StageError(f"query {q} row {r}: the bit is {int(got[q, r])}, the exact score {ex[q, r]!r} is {'above' if ex[q, r] > T else 'below'} "
                         f"T = {T!r} by {dist[q, r]:.4g}")
    bad = got[:, n:]
    if bad.any():
        q, r = _first(bad)
        raise StageError(f"query {q}: the bit of row {n + r} is set, the index holds {n} rows")
    return worst


def match_inputs(cls: str, dim: int, m: int, n: int):
    """(rows, queries, max_dist) of one shared-footage case: the class's rows and queries; on Gaussian rows up to twelve rows are
    near-copies of queries at growing distances, so that hits exist and the threshold falls among them.  The CPU test asserts
    threshold_conditions for every case the GPU test runs."""
    rng = np.random.default_rng([41, dim, m, n])
    rows, qs = input_class(cls, rng, n, m, dim)
    if cls == "gaussian":
        for i, noise in enumerate(np.linspace(0.05, 0.6, min(n, 12))):
            v = qs[i % m].astype(np.float64) + noise * rng.standard_normal(dim) / np.sqrt(dim)
            rows[(i * 37) % n] = (v / np.sqrt((v ** 2).sum())).astype(np.float32)
    return rows, qs, choose_max_dist(exact_scores(rows, qs), skip=min(4, n * m - 1))


MATCH_N = (1, 31, 33, 2047, 2049, 2048 + 300, 4 * 2048 + 1)
MATCH_CASES = [("gaussian", 512, m, n) for m in (1, 255, 257) for n in MATCH_N] + \
              [("gaussian", dim, 257, 2348) for dim in (256, 768)] + [(cls, 512, 257, 2348) for cls in INPUT_CLASSES[1:]]


# ---------------------------------------------------------------- read-back through the debug entries (GPU tests)
def read_label_parts(lib, check, handle):
    """-> (info dict, parts uint32 [ranges][5][n_pad])"""
    info = (ctypes.c_int64 * 4)()
    check(lib.vq_index_debug_read_label_parts(handle, info, None, 0))
    n, n_pad, ranges, P = (int(v) for v in info)
    parts = np.empty((ranges, LABEL_PARTS, n_pad), np.uint32)
    check(lib.vq_index_debug_read_label_parts(handle, info, parts.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), parts.size))
    return dict(n=n, n_pad=n_pad, ranges=ranges, P=P), parts


def read_match_bits(lib, check, handle):
    """-> (info dict, bits uint32 [m][W], filed uint64 [min(cursor, cap)])"""
    info = (ctypes.c_int64 * 6)()
    check(lib.vq_index_debug_read_match_bits(handle, info, None, 0, None, 0))
    m, W, n, cursor, flag, cap = (int(v) for v in info)
    bits, filed = np.empty((m, W), np.uint32), np.empty(min(cursor, cap), np.uint64)
    check(lib.vq_index_debug_read_match_bits(handle, info, bits.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), bits.size,
                                             filed.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), filed.size))
    assert [int(v) for v in info] == [m, W, n, cursor, flag, cap]
    return dict(m=m, W=W, n=n, cursor=cursor, flag=flag, cap=cap), bits, filed


def read_group_scan_kind(lib, check, handle):
    info = (ctypes.c_int64 * 3)()
    check(lib.vq_index_debug_group_scan_kind(handle, info))
    return dict(kind=int(info[0]), chunks=int(info[1]), tile_chunks=int(info[2]))
