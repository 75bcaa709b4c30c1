"""Stage reference of the fp16 re-score kernels (pass 2 of every fp16 search), in numpy.

Pass 1 leaves, per (query, stream), two keys under a contract (scan_stage_ref.check_keys): each key within E of the exact score
of the row it names, key1 >= key2, every row the stream did not emit at or below key2 + E.  Pass 2 (csrc/knn_scan_f16.h) must
turn ANY table inside that contract into the exact top-k (flag 0, or 1 after stream rescans) or a flag (2).  A scan does not
produce tables at the edge of the contract; this module writes them: rows planted at chosen exact scores, keys moved by up to
f E against the proof, and the row that decides the proof hidden behind each of the kernels' truncating containers in turn.

Everything is built in COSINES: the queries are g_j e_j with e_j orthonormal, a row is sum_j b_j e_j + (the rest) u with u
orthogonal to every e_j, so its exact score against query j is g_j b_j and E_j = Ec g_j, Ec = eps_unit(dim) max(1, |row|max).
Every table is certified by check_keys (<= 1.0) before use: that call, not the construction, says a table is inside the contract.

model_state restates the documented proof rule and is used by the CPU test only: it shows that each class's required outcome
follows from the rule and that each planted defect of the rule is caught by some class.
"""
from __future__ import annotations

import ctypes

import numpy as np

import scan_stage_ref as ref
from oracle import knn_oracle

F = 0.97                     # keys move by at most F E; the 3 % left: the index bits (2^-16 relative) and fp32 rounding
RESCAN_MAX = 4               # RV_RESCAN_MAX
EPS_HOST = 1.0001            # the host hands the kernels scan_eps_unit(dim) x 1.0001 max(1, |row|max) (refresh_norm_range)
Q2_MIN, Q2_MAX = 0.25, 4.0   # SCAN_Q2_MIN, SCAN_Q2_MAX
BG = 0.2                     # background cosines lie in [-BG, BG]
TOP = 0.9                    # the best planted cosine
HAIR = 0.01                  # (E units) what separates two keys that must keep their order through the index bits (64 ulps ~ 0.004 E)


class Params:
    """The containers of one re-score kernel.  batch: SHARES = 256 / QPW interleaved stream shares, KEEP keys kept per share, the
    best C re-scored.  small: a wave threshold, the keys above it collected (at most 4 C), the best C re-scored in two passes."""

    def __init__(self, name, kind, C, QPW=1, KEEP=0):
        self.name, self.kind, self.C, self.QPW, self.KEEP = name, kind, C, QPW, KEEP
        self.SHARES = 256 // QPW

    def __repr__(self):
        return self.name


# by vq_scan_plan.rescore
PARAMS = {0: Params("BATCH8", "batch", 32, 8, 6), 1: Params("LARGE4", "batch", 80, 4, 10), 2: Params("XLARGE4", "batch", 128, 4, 12),
          3: Params("LARGE1", "batch", 80, 1, 10), 4: Params("XLARGE1", "batch", 128, 1, 12),
          5: Params("SMALL32", "small", 32), 6: Params("SMALL64", "small", 64)}
BATCH8, LARGE4, XLARGE4, LARGE1, XLARGE1, SMALL32, SMALL64 = range(7)


def first_pass(P, k):
    """candidates the small kernels re-score before they look whether the others can matter"""
    return min(P.C, max(16, (k + 6 + 7) & ~7))


class Unfit(Exception):
    """the geometry cannot hold the class (too few streams, k too small): a mistake in the list of cases"""


class Geo:
    """Which row every (stream, local index) names, for n rows: scan_stage_ref.row_table (the library's own row functions)."""

    def __init__(self, lib, layout, streams, n):
        self.layout, self.streams, self.n = layout, streams, n
        self.table = ref.row_table(lib, layout, streams)
        self.valid = self.table < n
        self.nvalid = self.valid.sum(1)

    def row(self, stream, j):
        """the j-th valid row of the stream, in local order"""
        return int(self.table[stream, np.flatnonzero(self.valid[stream])[j]])

    def take(self, used, count, min_rows=1, share=None, shares=1):
        """`count` streams with at least min_rows rows that no query of the scene uses yet, in stream order (consecutive streams lie
        in consecutive shares); share: only streams of that share"""
        out = []
        for s in range(self.streams):
            if len(out) == count:
                break
            if s not in used and self.nvalid[s] >= min_rows and (share is None or s % shares == share):
                out.append(s)
        if len(out) < count:
            raise Unfit(f"{count} free streams with {min_rows} rows wanted, {len(out)} there")
        used.update(out)
        return out


class Spec:
    """One query of a scene: planted (row, cosine, delta), groups of rows made identical, the background's delta, the outcome."""

    def __init__(self, cls, required, gain=1.0, bg_delta=1.0):
        self.cls, self.required, self.gain, self.bg_delta = cls, required, gain, bg_delta
        self.planted, self.same, self.must_hold, self.nan_at = [], [], [], None

    def plant(self, row, cos, delta):
        self.planted.append((row, cos, delta))
        return row


# ---------------------------------------------------------------- the classes (cosines; E = Ec)
def _tops(spec, geo, used, count, Ec, first=0):
    """`count` top rows 4 E apart, one per stream, understated"""
    for i, s in enumerate(geo.take(used, count)):
        spec.plant(geo.row(s, 0), TOP - 4 * Ec * (first + i), -1.0)


def cls_clear(geo, used, P, k, Ec, gain=1.0):
    """k top rows 4 E apart, one per stream, understated by F E; the background overstated: nothing is open.  -> 0"""
    spec = Spec("clear", 0, gain)
    _tops(spec, geo, used, k, Ec)
    return spec


def cls_hidden(geo, used, P, k, Ec, h, deep=False, with_h=True, gap2=None):
    """h streams each hold A, B and H.  H is in the true top-k by 1e-6 over the rows N; the stream's 2nd key is key(B) = H - 0.96 E
    and H is not emitted (any score of H a scan could have had lies below it).  Only the 2nd-key rule, with the full EPS, finds H.
    A is a clear top row where k leaves room (k >= 2 h: a rescanned stream's candidate that is part of the answer), else just
    above B.  deep (small kernels): so many rows N, overstated, that key(B) ranks behind the first re-score pass.
    with_h = False (no-rescan): no H, and key(B) = s_k - gap2 E: the rule must NOT fire.  -> 1 for h <= 4, 2 for h = 5; 0 without H"""
    if k < h:
        raise Unfit("hidden: k < h")
    high_a = k >= 2 * h
    n_top = k - h - (h if high_a else 0) if with_h else k - h
    name = ("hidden-deep(%d)" if deep else "hidden(%d)") % h if with_h else "no-rescan"
    spec = Spec(name, (1 if h <= RESCAN_MAX else 2) if with_h else 0)
    hs = geo.take(used, h, min_rows=3)
    level = TOP - 4 * Ec * (k + 2)                        # below every top row
    if with_h:
        _tops(spec, geo, used, n_top, Ec, first=h)
        n_n = h
        if deep:
            c1 = first_pass(P, k)
            if c1 >= P.C:
                raise Unfit("hidden-deep: the first pass re-scores every candidate")
            n_n = max(h, c1 - (k - h) + 1)
        for i, s in enumerate(geo.take(used, n_n)):
            spec.plant(geo.row(s, 0), level - 1e-6 - 2e-7 * i, 1.0)              # N: pushed out of the top-k by H alone
        for i, s in enumerate(hs):
            H = level + 2e-7 * i
            B = H - (2 * F - HAIR) * Ec
            spec.plant(geo.row(s, 0), TOP - 4 * Ec * i if high_a else B + HAIR / 2 * Ec, -1.0 if high_a else 1.0)     # A
            spec.plant(geo.row(s, 1), B, 1.0)
            spec.must_hold.append(spec.plant(geo.row(s, 2), H, -1.0))
    else:                                                 # A is the k-th best row (k = 1: the best); key(B) = s_k - gap2 E
        _tops(spec, geo, used, k - 1, Ec)
        s_k = TOP - 4 * Ec * (k - 1)
        spec.plant(geo.row(hs[0], 0), s_k, -1.0)
        spec.plant(geo.row(hs[0], 1), s_k - (gap2 + F) * Ec, 1.0)
    return spec


def cls_no_rescan(geo, used, P, k, Ec):
    """as hidden(1) without H; key2 = s_k - 1.03 E: an EPS more than 3 % too large rescans here.  -> 0"""
    return cls_hidden(geo, used, P, k, Ec, 1, with_h=False, gap2=1.03)


def cls_rest_bound(geo, used, P, k, Ec):
    """k - 1 clear tops; C - (k - 1) decoys at v - 2 F E, overstated; the victim V at v, the true k-th, understated: its key ranks
    C + 1, so it is re-scored by nobody and only the (C+1)-th key's bound knows of it.  -> 2"""
    spec = Spec("rest-bound", 2)
    _tops(spec, geo, used, k - 1, Ec)
    v = TOP - 4 * Ec * (k + 2)
    for i, s in enumerate(geo.take(used, P.C - (k - 1))):
        spec.plant(geo.row(s, 0), v - (2 * F - HAIR) * Ec + 1e-7 * i, 1.0)
    spec.must_hold.append(spec.plant(geo.row(geo.take(used, 1)[0], 0), v, -1.0))
    return spec


def cls_share_floor(geo, used, P, k, Ec, share=0):
    """batch kernels: KEEP + 1 rows of the true top-k as first and second keys (up to four pairs) and first keys of streams of ONE share: the share's list drops one
    of them, and only its floor knows (k further clear rows: every other bound is closed).  -> 2"""
    if P.kind != "batch" or k <= P.KEEP:
        raise Unfit("share-floor: a batch kernel and k > KEEP")
    spec = Spec("share-floor", 2)
    m = P.KEEP + 1
    pairs = min(RESCAN_MAX, m // 2)                       # (every pair's second key asks for a rescan: no more of them than the kernels grant)
    ss = geo.take(used, m - pairs, min_rows=2, share=share, shares=P.SHARES)
    for i in range(m):                                    # the pairs on top, then one row per stream: the share drops the last
        s, j = (ss[i // 2], i % 2) if i < 2 * pairs else (ss[i - pairs], 0)
        spec.must_hold.append(spec.plant(geo.row(s, j), TOP - 4 * Ec * i, -1.0))
    _tops(spec, geo, used, k - m + 1, Ec, first=m)         # and a (k+1)-th clear row: without the floor the proof would close on it
    return spec


def cls_tie_run(geo, used, P, k, Ec):
    """more than 4 C identical rows at the same local index of as many streams, the best of the index: equal first keys, more than
    the collected list holds.  -> 2 (any state on the 32-candidate batch kernel, which ranks all kept keys)"""
    spec = Spec("tie-run", None if P.kind == "batch" and P.C <= 32 else 2)
    full = [s for s in range(geo.streams) if geo.valid[s, 0] and s not in used][:4 * P.C + 1]
    if len(full) < 4 * P.C + 1:
        raise Unfit("tie-run: more than 4 C streams")
    used.update(full)
    spec.same.append([spec.plant(int(geo.table[s, 0]), 0.6, -1.0) for s in full])
    return spec


def cls_norm_gate(geo, used, P, k, Ec, q2):
    """clear at |q|^2 = q2 (NaN: one element of the query is NaN, the table is that of the clean query).  -> 0 inside [0.25, 4], else 2"""
    nan = not np.isfinite(q2)
    g2 = 1.0 if nan else q2
    spec = cls_clear(geo, used, P, k, Ec, gain=float(np.sqrt(g2)))
    spec.cls, spec.required = f"norm-gate({q2})", 0 if (not nan and Q2_MIN <= g2 <= Q2_MAX) else 2
    spec.nan_at = 3 if nan else None
    return spec


def cls_ties_at_k(geo, used, P, k, Ec):
    """clear, but the k-th best row has three identical copies in other streams: which of them is listed is the tie order's choice"""
    spec = Spec("ties-at-k", 0)
    _tops(spec, geo, used, k - 1, Ec)
    spec.same.append([spec.plant(geo.row(s, 0), TOP - 4 * Ec * (k - 1), -1.0) for s in geo.take(used, 4)])
    return spec


# ---------------------------------------------------------------- rows, queries, keys
def planted_rows(rng, n, dim, specs, pool=32):
    """rows [n][dim] fp32 of unit norm and queries [nq][dim]: query j is gain_j e_j; row r is sum_j b_rj e_j + sqrt(1 - |b|^2) u_r,
    u_r one of `pool` unit vectors orthogonal to every e_j.  b_rj is the cosine spec j plants on r, else background in [-BG, BG]
    (a tenth of that on rows another query plants, so that the row fits the unit sphere)."""
    nq = len(specs)
    basis = np.linalg.qr(rng.standard_normal((dim, nq + pool)))[0].T                   # orthonormal rows
    e, u = basis[:nq], basis[nq:]
    b = rng.uniform(-BG, BG, (n, nq))
    mine = np.zeros((n, nq), bool)
    for j, sp in enumerate(specs):
        for row, cos, _ in sp.planted:
            assert not mine[row].any(), f"row {row} is planted twice"
            mine[row, j] = True
            b[row] *= 0.1
            b[row, j] = cos
    rest = 1.0 - (b ** 2).sum(1)
    assert rest.min() > 0.02, "a row does not fit the unit sphere"
    which = rng.integers(0, pool, n)
    rows = np.empty((n, dim), np.float32)
    for r0 in range(0, n, 1 << 16):                                                   # (blocks: the 8193-stream case holds 1M rows)
        sl = slice(r0, r0 + (1 << 16))
        rows[sl] = b[sl] @ e + np.sqrt(rest[sl])[:, None] * u[which[sl]]
    for sp in specs:
        for group in sp.same:
            rows[group[1:]] = rows[group[0]]
    qs = np.stack([sp.gain * e[j] for j, sp in enumerate(specs)]).astype(np.float32)
    return rows, qs


def pack_index(values: np.ndarray, local: np.ndarray) -> np.ndarray:
    """fp32 values -> key words: the local index over the low 7 bits, the word nearest to the value (at most 64 ulps away)"""
    bits = np.ascontiguousarray(values, np.float32).view(np.uint32).astype(np.int64)
    sign, mag = bits & 0x80000000, bits & 0x7FFFFFFF
    cands = np.stack([((np.maximum((mag >> 7) + d, 0)) << 7) | local for d in (-1, 0, 1)])
    best = np.take_along_axis(cands, np.abs(cands - mag).argmin(0)[None], 0)[0]
    return (sign | best).astype(np.uint32)


def make_keys(exact: np.ndarray, delta: np.ndarray, table: np.ndarray, n: int, E: float, f: float = F) -> np.ndarray:
    """One query's table uint32 [streams][2]: every row reads exact + delta f E (delta in [-1, 1] per row), a stream emits its two
    largest readings with the local index packed in, re-sorted if the packing flipped them; where a stream has fewer than two
    rows, the sentinel with the pad row's local index, as the scans write it."""
    assert np.abs(delta).max() <= 1.0
    reading = exact + delta * f * E
    valid = table < n
    per = np.where(valid, reading[np.where(valid, table, 0)], -np.inf)
    local = np.argsort(-per, axis=1, kind="stable")[:, :2]
    val = np.take_along_axis(per, local, 1)
    keys = pack_index(np.where(np.isfinite(val), val, ref.SENTINEL).astype(np.float32), local)
    flip = keys[:, 0].view(np.float32) < keys[:, 1].view(np.float32)
    keys[flip] = keys[flip][:, ::-1]
    return np.ascontiguousarray(keys)


class Scene:
    """rows, queries and a certified key table for a list of specs (one per query)"""

    def __init__(self, rng, geo, dim, specs, rows=None, qs=None, deltas=None):
        self.geo, self.specs = geo, specs
        n = geo.n
        if rows is None:
            rows, qs = planted_rows(rng, n, dim, specs)
        self.rows = rows
        self.exact = ref.exact_scores(rows, qs)
        self.E = ref.bound(rows, qs)
        keys = []
        for j, sp in enumerate(specs):
            if deltas is not None:
                delta = deltas[j]
            else:
                delta = np.full(n, sp.bg_delta) if np.isscalar(sp.bg_delta) else sp.bg_delta.copy()
                for row, _, d in sp.planted:
                    delta[row] = d
                for group in sp.same:
                    delta[group] = delta[group[0]]
            keys.append(make_keys(self.exact[j], delta, geo.table, n, self.E[j]))
        self.keys = np.stack(keys)
        self.worst = ref.check_keys(self.keys, rows, qs, geo.table)       # raises outside the contract
        assert self.worst <= 1.0
        self.qs = qs.copy()                                               # what the kernels are given
        for j, sp in enumerate(specs):
            if sp.nan_at is not None:
                self.qs[j, sp.nan_at] = np.nan
        self.clean_qs = qs


def gaussian_scene(rng, geo, dim, nq, mode, identical=False):
    """adversarial: gaussian rows (or all identical), delta random in [-1, 1] or "worst sign": the true top-C understated, every
    other row overstated"""
    rows = ref.identical_rows(rng, geo.n, dim) if identical else ref.gaussian_unit(rng, geo.n, dim)
    qs = ref.gaussian_unit(rng, nq, dim)
    ex = ref.exact_scores(rows, qs)
    if mode == "random":
        deltas = rng.uniform(-1.0, 1.0, ex.shape)
    else:
        deltas = np.ones(ex.shape)
        top = np.argsort(-ex, axis=1, kind="stable")[:, :mode]
        np.put_along_axis(deltas, top, -1.0, 1)
    specs = [Spec("identical" if identical else f"adversarial-{mode}", None) for _ in range(nq)]
    return Scene(rng, geo, dim, specs, rows, qs, deltas)


# ---------------------------------------------------------------- the expected answer
def expected(rows, qs, k, rank=None):
    """oracle.knn_oracle.topk on the fp32 data; with id ranks the (distance, rank) order over the oracle's distances"""
    if rank is None:
        return knn_oracle.topk(rows, qs, k)
    ids, dist = np.full((len(qs), k), -1, np.int32), np.full((len(qs), k), np.inf, np.float32)
    for j, q in enumerate(qs):
        d = knn_oracle.distances(rows, q)
        order = np.lexsort((rank, d))[:k]
        ids[j, :len(order)], dist[j, :len(order)] = order, d[order]
    return ids, dist


# ---------------------------------------------------------------- the proof rule, restated (CPU test only)
DEFECTS = ("eps_095", "eps_105", "no_rest_bound", "no_share_floor", "no_second_key", "second_key_first_pass_only", "fifth_rescan_dropped",
           "rescanned_candidates_stay", "no_norm_gate")


def _small_threshold(kf, P):
    """the small kernels' collection threshold: thread t owns streams p0(t) + 256 u; T = the smallest, over the four waves, of the
    wave's (C / 4)-th largest thread maximum (of first keys)"""
    streams = len(kf)
    tid = np.arange(256)
    p0 = np.where(streams < 512, 4 * (tid & 63) + (tid >> 6), tid)
    mx = np.full(256, -np.inf)
    for t in range(256):
        own = kf[p0[t]::256, 0]
        if len(own):
            mx[t] = own.max()
    thr = min(np.sort(mx[tid >> 6 == w])[::-1][P.C // 4 - 1] for w in range(4))
    return max(thr, -3.4e38)


def model_state(keys, dist32, E, P, k, geo, q2=1.0, defect=None, rank=None):
    """keys uint32 [streams][2] of one query, dist32 [n] its exact fp32 distances (the oracle's) -> (state, ids or None, info).
    share lists and floors (or threshold and below), best C, (C+1)-th key, s_k, 2nd-key rescans <= 4."""
    assert defect is None or defect in DEFECTS
    kf = keys.view(np.float32).astype(np.float64)
    streams = len(keys)
    eps = E * EPS_HOST * (0.95 if defect == "eps_095" else 1.05 if defect == "eps_105" else 1.0)
    order_of = (lambda r: r) if rank is None else (lambda r: int(rank[r]))
    floors, overflow = [], False
    if P.kind == "batch":
        kept = []                                                      # (value, slot, src)
        for sh in range(P.SHARES):
            mine = sorted(((-kf[s, w], 2 * s + w) for s in range(sh, streams, P.SHARES) for w in (0, 1)))
            kept += [(-v, sh * P.KEEP + i, src) for i, (v, src) in enumerate(mine[:P.KEEP])]
            floors.append(-mine[P.KEEP][0] if len(mine) > P.KEEP else -np.inf)
        kept.sort(key=lambda e: (-e[0], e[1]))
        if P.C > 32:                                                   # two-level selection: the keys >= T1 must fit 4 C entries
            per = (P.C + 1 + P.SHARES - 1) // P.SHARES
            firsts = [e[0] for e in kept if e[1] % P.KEEP < per]
            firsts += [-np.inf] * (P.SHARES * per - len(firsts))      # (a list shorter than KEEP ends in -inf)
            t1 = sorted(firsts, reverse=True)[P.C]
            overflow = sum(1 for e in kept if e[0] >= t1 and e[0] > -np.inf) > 4 * P.C
        ranked = [(v, src) for v, _, src in kept]
        limit = P.C
    else:
        ranked = sorted(((kf[s, w], 2 * s + w) for s in range(streams) for w in (0, 1)), key=lambda e: (-e[0], e[1]))
        overflow = int((kf >= _small_threshold(kf, P)).sum()) > 4 * P.C
        limit = first_pass(P, k)
    cand = ranked[:P.C]
    rest = ranked[P.C][0] if len(ranked) > P.C else -np.inf

    def row_of(v, src):
        if not v > -np.inf:
            return -1
        r = int(geo.table[src >> 1, int(np.float32(v).view(np.uint32)) & 127])
        return r if r < geo.n else -1
    crow = [row_of(v, src) for v, src in cand]
    kk = min(k, P.C)

    def kth(upto):
        ds = sorted(float(dist32[r]) for r in crow[:upto] if r >= 0)
        return (len(ds), 1.0 - ds[kk - 1]) if len(ds) >= kk else (len(ds), -np.inf)
    info = dict(pass2=False)
    have, sk = kth(limit)
    if P.kind == "small" and limit < P.C:
        nxt = cand[limit][0] if len(cand) > limit else -np.inf
        if nxt > -np.inf and not nxt + eps < sk:
            limit, info["pass2"] = P.C, True
            have, sk = kth(limit)
    gate = Q2_MIN <= q2 <= Q2_MAX or defect == "no_norm_gate"           # (NaN: False)
    state, resc = 0, []
    if have < kk or not gate or overflow:
        state = 2
    else:
        if defect != "no_rest_bound" and not rest + eps < sk:
            state = 2
        if defect != "no_share_floor" and any(not fl + eps < sk for fl in floors):
            state = 2
        if state == 0 and defect != "no_second_key":
            upto = first_pass(P, k) if defect == "second_key_first_pass_only" else limit
            for v, src in cand[:min(upto, limit)]:
                if src & 1 and v + eps >= sk:
                    if len(resc) < RESCAN_MAX:
                        resc.append(src >> 1)
                    elif defect != "fifth_rescan_dropped":
                        state = 2
            if state == 0 and resc:
                state = 1
    info.update(rescans=list(resc), sk=sk)
    if state == 2:
        return 2, None, info
    pool = [r for (v, src), r in zip(cand[:limit], crow[:limit])
            if r >= 0 and (defect == "rescanned_candidates_stay" or (src >> 1) not in resc)]
    for s in resc:
        pool += [int(r) for r in geo.table[s] if r < geo.n]
    pool.sort(key=lambda r: (float(dist32[r]), order_of(r)))
    ids = pool[:k] + [-1] * (k - len(pool))
    return state, np.array(ids, np.int32), info


# ---------------------------------------------------------------- the debug entry (GPU tests)
def run_rescore(lib, check, handle, qs, k, keys):
    """vq_index_debug_rescore -> (ids [nq][k], dist [nq][k], flags [nq])"""
    qs, keys = np.ascontiguousarray(qs, np.float32), np.ascontiguousarray(keys, np.uint32)
    nq = len(qs)
    ids, dist, flags = np.empty((nq, k), np.int32), np.empty((nq, k), np.float32), np.empty(nq, np.int32)
    f32, i32 = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int32)
    check(lib.vq_index_debug_rescore(handle, qs.ctypes.data_as(f32), nq, k, keys.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), keys.size,
                                     ids.ctypes.data_as(i32), dist.ctypes.data_as(f32), flags.ctypes.data_as(i32)))
    return ids, dist, flags


# ---------------------------------------------------------------- the cases: the smallest shapes that reach each kernel and its geometry branches
CLASSES = {
    "clear": cls_clear,
    "hidden1": lambda g, u, P, k, Ec: cls_hidden(g, u, P, k, Ec, 1),
    "hidden4": lambda g, u, P, k, Ec: cls_hidden(g, u, P, k, Ec, 4),
    "hidden5": lambda g, u, P, k, Ec: cls_hidden(g, u, P, k, Ec, 5),
    "hidden-deep": lambda g, u, P, k, Ec: cls_hidden(g, u, P, k, Ec, 1, deep=True),
    "no-rescan": cls_no_rescan,
    "rest-bound": cls_rest_bound,
    "share-floor": cls_share_floor,
    "tie-run": cls_tie_run,
    "gate0.26": lambda g, u, P, k, Ec: cls_norm_gate(g, u, P, k, Ec, 0.26),
    "gate3.9": lambda g, u, P, k, Ec: cls_norm_gate(g, u, P, k, Ec, 3.9),
    "gate0.24": lambda g, u, P, k, Ec: cls_norm_gate(g, u, P, k, Ec, 0.24),
    "gate4.1": lambda g, u, P, k, Ec: cls_norm_gate(g, u, P, k, Ec, 4.1),
    "gateNaN": lambda g, u, P, k, Ec: cls_norm_gate(g, u, P, k, Ec, float("nan")),
    "ties-at-k": cls_ties_at_k,
}
STD = ("clear", "hidden1", "hidden4", "hidden5", "no-rescan", "rest-bound", "gate0.26", "gate3.9", "gate0.24", "gate4.1", "gateNaN")
GATES = ("gate0.26", "gate3.9", "gate0.24", "gate4.1", "gateNaN")
RANGE_ROWS = {1: 1024, 2: 2048, 3: 128}


class Case:
    """One index geometry and k: the planted classes it runs (cut into scenes of nq queries), and whether it also runs the
    gaussian scenes (random deltas, worst sign, identical rows).  reversed_ranks: under vq_index_set_id_ranks, ids reversed."""

    def __init__(self, rescore, layout, dim, streams, nq, k, classes, env=None, gaussian=False, reversed_ranks=False, cpu=False):
        self.rescore, self.layout, self.dim, self.streams, self.nq, self.k = rescore, layout, dim, streams, nq, k
        self.classes, self.env, self.gaussian, self.reversed_ranks, self.cpu = tuple(classes), env or {}, gaussian, reversed_ranks, cpu
        self.P = PARAMS[rescore]
        self.n = streams * 128 - (37 if layout == 3 else RANGE_ROWS[layout] - 37)      # ragged; layouts 1, 2: a last range of 37 rows, whole streams of it empty

    @property
    def id(self):
        env = "".join(f"-{k[7:]}={v}" for k, v in self.env.items())
        return f"{self.P.name}-L{self.layout}-d{self.dim}-s{self.streams}-q{self.nq}-k{self.k}{'-ranks' if self.reversed_ranks else ''}{env}-{'+'.join(self.classes) if len(self.classes) < 3 else len(self.classes)}"

    def seed(self):
        return [41, self.rescore, self.layout, self.dim, self.streams, self.nq, self.k]

    def scenes(self, lib):
        """-> the case's Scene objects; a planted scene takes classes until the streams run out, and its other queries get plain
        background (random deltas, any state)"""
        rng = np.random.default_rng(self.seed())
        geo = Geo(lib, self.layout, self.streams, self.n)
        Ec = ref.eps_unit(self.dim)
        todo = list(self.classes)
        while todo:
            used, specs = set(), []
            while todo and len(specs) < self.nq:
                mark = set(used)
                try:
                    specs.append(CLASSES[todo[0]](geo, used, self.P, self.k, Ec))
                    todo.pop(0)
                except Unfit:
                    if not specs:
                        raise
                    used.clear(); used.update(mark)
                    break
            while len(specs) < self.nq:
                specs.append(Spec("background", None, bg_delta=rng.uniform(-1.0, 1.0, self.n)))
            yield Scene(rng, geo, self.dim, specs)
        if self.gaussian:
            yield gaussian_scene(rng, geo, self.dim, self.nq, "random")
            yield gaussian_scene(rng, geo, self.dim, self.nq, self.P.C)
            yield gaussian_scene(rng, geo, self.dim, self.nq, "random", identical=True)


def _cases():
    c = []
    S32, S64 = SMALL32, SMALL64
    # SMALL32: dim 256; 8 / 33 streams, the list's 64 | 65, the thread -> stream map's 511 | 512 | 513; one query files its own flag
    c.append(Case(S32, 3, 256, 8, 1, 1, ("clear", "hidden1", "no-rescan") + GATES, gaussian=True, cpu=True))
    c.append(Case(S32, 3, 256, 33, 1, 10, STD + ("hidden-deep",), gaussian=True, cpu=True))
    c.append(Case(S32, 3, 256, 64, 3, 20, STD, gaussian=True))
    c.append(Case(S32, 3, 256, 65, 3, 10, STD + ("hidden-deep",), cpu=True))
    c.append(Case(S32, 3, 256, 511, 3, 20, STD + ("tie-run",), gaussian=True, cpu=True))
    c.append(Case(S32, 3, 256, 512, 1, 10, ("clear", "hidden1", "hidden4", "hidden5", "rest-bound", "tie-run")))
    c.append(Case(S32, 3, 256, 513, 3, 10, STD + ("hidden-deep", "tie-run")))
    c.append(Case(S32, 3, 512, 33, 1, 10, ("clear", "hidden1")))                  # LDS row stride and threads per row change with dim
    c.append(Case(S32, 3, 768, 33, 1, 10, ("clear", "hidden1")))
    c.append(Case(S32, 3, 256, 8193, 1, 10, ("hidden1",)))                       # the keys no longer stay in registers
    c.append(Case(S32, 3, 256, 65, 3, 10, ("ties-at-k", "clear", "hidden1"), reversed_ranks=True, cpu=True))
    c.append(Case(S32, 3, 256, 1, 1, 20, ()))                                     # short: see SHORT
    # SMALL64: dim 256, 512; k 21, 40
    c.append(Case(S64, 3, 256, 63, 1, 21, tuple(x for x in STD if x != "rest-bound") + ("hidden-deep",), gaussian=True, cpu=True))      # (rest-bound takes C + 1 streams)
    c.append(Case(S64, 3, 256, 64, 3, 40, ("clear", "hidden1", "no-rescan")))
    c.append(Case(S64, 3, 512, 128, 3, 40, STD, gaussian=True))
    c.append(Case(S64, 3, 512, 129, 3, 21, STD + ("hidden-deep",)))
    c.append(Case(S64, 3, 256, 512, 1, 40, STD + ("hidden-deep", "tie-run"), cpu=True))
    # LARGE1 / XLARGE1: the prefetch loop's 8 x 256 streams
    c.append(Case(LARGE1, 3, 256, 300, 1, 41, STD, gaussian=True))
    c.append(Case(LARGE1, 3, 256, 300, 3, 64, STD, cpu=True))
    c.append(Case(LARGE1, 3, 768, 300, 3, 21, STD))
    c.append(Case(LARGE1, 3, 256, 2047, 3, 64, STD + ("share-floor", "tie-run"), cpu=True))
    c.append(Case(LARGE1, 3, 256, 2049, 1, 41, ("clear", "hidden1", "rest-bound", "share-floor")))
    c.append(Case(XLARGE1, 3, 256, 300, 3, 65, STD, gaussian=True))
    c.append(Case(XLARGE1, 3, 256, 300, 1, 100, STD, cpu=True))
    c.append(Case(XLARGE1, 3, 256, 2047, 3, 100, STD + ("tie-run",)))
    c.append(Case(XLARGE1, 3, 256, 2049, 1, 65, ("clear", "hidden1", "rest-bound", "share-floor"), cpu=True))
    # BATCH8: layouts 1 (dim 192) and 2 (dim 128), nine queries = a workgroup with one live query; 12 x 32 streams and its neighbours
    c.append(Case(BATCH8, 1, 192, 376, 9, 20, STD + ("share-floor", "tie-run"), gaussian=True, cpu=True))
    c.append(Case(BATCH8, 1, 192, 384, 9, 10, STD + ("share-floor",)))
    c.append(Case(BATCH8, 1, 192, 392, 9, 1, ("clear", "hidden1", "no-rescan") + GATES))
    c.append(Case(BATCH8, 2, 128, 368, 9, 10, STD + ("share-floor",), gaussian=True))
    c.append(Case(BATCH8, 2, 128, 384, 9, 20, STD + ("share-floor", "tie-run"), cpu=True))
    c.append(Case(BATCH8, 2, 128, 400, 9, 1, ("clear", "hidden1", "no-rescan") + GATES))
    c.append(Case(BATCH8, 1, 192, 376, 9, 10, ("ties-at-k", "clear", "hidden1", "hidden4"), reversed_ranks=True, cpu=True))
    # LARGE4 / XLARGE4: 8 x 64 streams and its neighbours; once on the streaming scan's keys
    c.append(Case(LARGE4, 1, 192, 504, 5, 21, STD + ("share-floor", "tie-run"), gaussian=True, cpu=True))
    c.append(Case(LARGE4, 1, 192, 512, 5, 64, STD + ("share-floor",)))
    c.append(Case(LARGE4, 2, 128, 528, 5, 64, STD + ("share-floor", "tie-run"), cpu=True))
    c.append(Case(LARGE4, 2, 128, 496, 5, 21, STD, gaussian=True))
    c.append(Case(XLARGE4, 1, 192, 520, 5, 65, STD + ("share-floor", "tie-run"), gaussian=True, cpu=True))
    c.append(Case(XLARGE4, 1, 192, 504, 5, 100, STD))
    c.append(Case(XLARGE4, 2, 128, 512, 5, 100, STD, cpu=True))
    c.append(Case(XLARGE4, 2, 128, 528, 5, 65, STD + ("share-floor", "tie-run")))
    c.append(Case(LARGE4, 3, 256, 300, 5, 64, STD, env={"VQ_AMD_RESCORE_QPW4": 1}))
    c.append(Case(XLARGE4, 3, 256, 300, 5, 100, STD, env={"VQ_AMD_RESCORE_QPW4": 1}))
    return [x for x in c if x.classes]


CASES = _cases()
# short: fewer rows than k, and fewer keys than k -> 2 for every query.  (rescore, layout, dim, n, nq, k)
SHORT = [(SMALL32, 3, 256, 5, 1, 10), (SMALL32, 3, 256, 8 * 128 - 37, 3, 20), (SMALL64, 3, 256, 30, 1, 40), (LARGE1, 3, 256, 16 * 128, 3, 41),
         (BATCH8, 1, 192, 7, 9, 10), (BATCH8, 2, 128, 7, 9, 20), (LARGE4, 1, 192, 1024, 5, 21), (XLARGE4, 2, 128, 2048, 5, 65)]
