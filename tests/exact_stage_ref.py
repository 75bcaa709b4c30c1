"""Dictated distance layouts with a closed-form answer, for the stage tests of the exact redo and the exact selection
(tests/test_exact_stages.py on the GPU, tests/test_exact_stages_cpu.py without one).

Every distance is exact by construction, so the reference owes nothing to the kernels' arithmetic or to the C oracle:
  rows     a_r e0 + b_r e1, a_r and b_r integer multiples of 2^-12 with |a_r|, |b_r| <= V 2^-12 (V = 3968); e0 is component 0
           and e1 the LAST component, so a kernel's ragged-dimension edge carries signal; b is a mirrored (n - 1 - r), so
           the three query kinds see three layouts.  fp16-path rows (the fallback entry needs near-unit rows) carry a filler
           sqrt(1 - a^2 - b^2) in component dim / 2, which no query touches; exact-mode rows carry eighths there instead;
  queries  s_j e0, s_j e1, s_j (e0 + e1) by j % 3, s_j = +/-(1 + (j % 512) 2^-10) 2^(j / 512): a scale of its own per query, so
           an answer filed in another query's slot shows.  Queries 1 and 3 .. 7 are special: zero, 2^100, 2, 2 on e1,
           -2^100, 2^100 on e0 + e1;
  dot      s_j (a_r | b_r | a_r + b_r): integers of at most 13 and 11 bits, exact in fp64 AND in fp32 (asserted), so the
           kernels' index-order fp64 chain, its rounding to fp32 and `1.0f - dot` are one IEEE subtraction here:
           d = fp32(1) - fp32(dot).
The expected list is a numpy sort of (d, tie) over the allowed rows; tie = the row, or the row's id rank.

A layout CLASS says where the k best rows of query 0 (+e0) lie, by the plan's geometry (rows per split, the 256-row tile, the
8,192-row chunk); the other queries see its mirror, its sum with the mirror and their negations.  The numpy MODELS at the end
restate the three mechanisms (tile filter + fold and k-way merge of the redo, threshold + collect + rank of the one-workgroup
selection, chunk lists + merge) so that the CPU test can plant defects and show which class catches each.
"""
import collections
import ctypes

import numpy as np

TILE, FAST_SLOTS, QG, KMAX, MAX_SPLITS = 256, 64, 8, 100, 4096        # csrc/knn_fallback.h
SEL_CHUNK, SMALL_MAX_N, SMALL_LIST, EDS_MAX_Q = 8192, 32768, 1024, 8   # csrc/knn_kernels.h
UNIT = 2.0 ** -12
V = 3968
LOW = -V
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)

RANKS = (None, "reversed", "random")
MASKS = (None, "stripes", "few", "splits", "one")


def cdiv(a, b):
    return -(-a // b)


# ---------------------------------------------------------------- the plan
Plan = collections.namedtuple("Plan", "fast_splits fast_rows splits rows round_q partial")


def fallback_plan(lib, check, n, nq, k):
    out = (ctypes.c_int64 * 6)()
    check(lib.vq_debug_fallback_plan(n, nq, k, out))
    return Plan(*[int(v) for v in out])


def rounds(plan, nq, flagged):
    """launch_fallback's rounds that find work: [(slot_base, slots taken, rows per split, splits)]"""
    out = [(0, min(flagged, FAST_SLOTS), plan.fast_rows, plan.fast_splits)] if flagged else []
    for base in range(FAST_SLOTS, nq, plan.round_q):
        if flagged > base:
            out.append((base, min(flagged - base, plan.round_q), plan.rows, plan.splits))
    return out


# ---------------------------------------------------------------- layout classes: levels (higher = nearer to query 0)
def _dedupe(rows, n, skip=()):
    seen, out = set(int(r) for r in skip), []
    for r in rows:
        r = int(r)
        if 0 <= r < n and r not in seen:
            seen.add(r)
            out.append(r)
    return out


def _ranked(n, rows, plateau=(), m=0):
    """rows[i] holds level V - i; the plateau rows hold V - m; every other row LOW"""
    v = np.full(n, LOW, np.int64)
    if len(plateau):
        v[np.asarray(plateau, np.int64)] = V - m
    for i, r in enumerate(rows):
        v[r] = V - i
    return v


def _split(n, S, s):
    return s * S, min(n, (s + 1) * S) - s * S            # first row, rows


def ascending(n, k, S):
    return V - (np.arange(n, dtype=np.int64) * 2 * V) // n


def descending(n, k, S):
    return ascending(n, k, S)[::-1].copy()


def last_rows(n, k, S):
    """the k best are the last k rows, the best one last: the last tile, the tail split"""
    m = min(n, k)
    return _ranked(n, [n - 1 - i for i in range(m)])


def last_row(n, k, S):
    """descending, and the single best row is the last one (the 1-row tail split where n % rows == 1)"""
    v = np.minimum(descending(n, k, S), V - 1)
    v[n - 1] = V
    return v


def one_per_split(n, k, S):
    splits = cdiv(n, S)
    rows = []
    for i in range(k):
        s = i % splits if k >= splits else (i * splits) // k
        first, size = _split(n, S, s)
        rows.append(first + ((i // splits) * 61 + 17 * s + 5) % size)
    return _ranked(n, _dedupe(rows, n))


def one_split(n, k, S):
    """every result from ONE split: its merge list walks to k"""
    first, size = _split(n, S, cdiv(n, S) // 2)
    return _ranked(n, _dedupe([first + (i * 37 + 11) % size for i in range(k)], n))


def alternating(n, k, S):
    splits = cdiv(n, S)
    sb = splits - 1 if _split(n, S, splits - 1)[1] >= k else max(0, splits - 2)
    ra, rb = (_split(n, S, 0), _split(n, S, sb)) if sb > 0 else ((0, cdiv(n, 2)), (cdiv(n, 2), n - cdiv(n, 2)))
    rows = []
    for i in range(k):
        first, size = rb if i % 2 else ra
        if size > 0:
            rows.append(first + ((i // 2) * 5 + 1) % size)
    return _ranked(n, _dedupe(rows, n))


def plateau_k(n, k, S):
    """k / 2 rows nearer than a scattered plateau of 2k + 3 equal distances that straddles rank k"""
    m = k // 2
    better = _dedupe([(i * 97 + 13) % n for i in range(m)], n)
    plateau = _dedupe([(j * 89 + 5) % n for j in range(2 * k + 3)], n, better)
    return _ranked(n, better, plateau, m)


def _plateau_at(B):
    def f(n, k, S):
        """a contiguous plateau over row B (a tile, split or chunk boundary; `split`: S): row order takes it from before B to
        behind it, reversed ranks from its end, and it straddles rank k; k / 2 nearer rows lie behind it"""
        b = S if B == "split" else B
        if not 0 < b < n:
            b = n // 2
        m = k // 2
        p = max(1, (k - m + 1) // 2)
        lo, hi = max(0, b - p), min(n, b + 3 * p)
        plateau = list(range(lo, hi))
        better = _dedupe([(hi + 3 * i) % n for i in range(m + len(plateau) + 4)], n, plateau)[:m]
        return _ranked(n, better, plateau, m)
    return f


def signs(n, k, S):
    """levels around 1/2: under the scale 2 the distances run from negative through +0.0 to positive inside the list"""
    w = max(k, 2)
    return 2048 + (np.arange(n, dtype=np.int64) * 7) % (2 * w + 1) - w


def thread_of(r):
    """select_small_kernel: piece p = r >> 2 goes to thread p & 255"""
    return (np.asarray(r) >> 2) & 255


def column_threads(k):
    t = [(i * 37 + 3) % 256 for i in range(min(k, 256))]
    return t[:-1], t[-1]


def thread_column(n, k, S):
    """k - 1 threads own ALL the nearest rows (the nearest of them last in row order) and the k-th thread's minimum is the next
    value: the threshold admits (k - 1) x rows per thread + 1 keys"""
    r = np.arange(n, dtype=np.int64)
    v = LOW + r % 100
    full, last = column_threads(k)
    mine = np.nonzero(np.isin(thread_of(r), full))[0]
    if len(mine):
        v[mine] = V - 63 + (np.arange(len(mine)) * 64) // len(mine)
    own = np.nonzero(thread_of(r) == last)[0]
    if len(own):
        v[own[len(own) // 2]] = V - 64
    return v


CLASSES = collections.OrderedDict([
    ("ascending", ascending), ("descending", descending), ("last_rows", last_rows), ("last_row", last_row),
    ("one_per_split", one_per_split), ("one_split", one_split), ("alternating", alternating), ("plateau_k", plateau_k),
    ("plateau_tile", _plateau_at(TILE)), ("plateau_split", _plateau_at("split")), ("plateau_chunk", _plateau_at(SEL_CHUNK)),
    ("plateau_32768", _plateau_at(SMALL_MAX_N)), ("signs", signs), ("thread_column", thread_column)])


def levels(cls, n, k, S):
    a = CLASSES[cls](n, k, S)
    assert a.shape == (n,) and np.abs(a).max() <= V
    return a, a[::-1].copy()


def rows_of(a, b, dim, filler):
    n = len(a)
    x = np.zeros((n, dim), np.float32)
    if not filler and dim > 2:
        x[:] = (((np.arange(n)[:, None] + np.arange(dim)[None, :]) % 7) - 3) * 0.125      # read by no query: times zero
    if filler:
        fa, fb = a * UNIT, b * UNIT
        x[:, dim // 2] = np.sqrt(np.maximum(0.0, 1.0 - fa * fa - fb * fb))
    x[:, 0] = a * UNIT
    x[:, dim - 1] = b * UNIT
    return x


# ---------------------------------------------------------------- queries
SPECIAL = {1: (1, 0.0), 3: (0, 2.0 ** 100), 4: (0, 2.0), 5: (1, 2.0), 6: (0, -2.0 ** 100), 7: (2, 2.0 ** 100)}
Queries = collections.namedtuple("Queries", "kind scale q")


def queries(nq, dim):
    kind, scale = np.empty(nq, np.int64), np.empty(nq, np.float64)
    for j in range(nq):
        kind[j], scale[j] = SPECIAL.get(j, (j % 3, (-1.0 if (j // 3) % 4 >= 2 else 1.0) * (1.0 + (j % 512) / 1024.0) * 2.0 ** (j // 512)))
    assert len(set(zip(kind.tolist(), scale.tolist()))) == nq
    q = np.zeros((nq, dim), np.float32)
    q[:, 0] = np.where(kind != 1, scale, 0.0)
    q[:, dim - 1] = np.where(kind != 0, scale, 0.0)
    assert (q[:, 0].astype(np.float64) == np.where(kind != 1, scale, 0.0)).all()
    return Queries(kind, scale, q)


def distances(a, b, Q, j):
    """d[r] of query j: fp32(1) - fp32(s (a | b | a + b) 2^-12), the dot exact in fp64 and in fp32"""
    lvl = (a, b, a + b)[int(Q.kind[j])]
    dot = (Q.scale[j] * UNIT) * lvl.astype(np.float64)
    d32 = dot.astype(np.float32)
    assert (d32.astype(np.float64) == dot).all()
    return np.float32(1.0) - d32


def rank_of(kind, n):
    if kind is None:
        return None
    if kind == "reversed":
        return np.arange(n, dtype=np.int32)[::-1].copy()
    return np.random.default_rng([61, n]).permutation(n).astype(np.int32)


def topk(d, k, tie=None, allowed=None):
    """the k smallest (d, tie) of the allowed rows -> ids [k] (-1 behind the last), dist [k] (+inf behind the last)"""
    rows = np.arange(len(d)) if allowed is None else np.nonzero(allowed)[0]
    dd = d[rows]
    tt = rows if tie is None else tie[rows]
    ids, dist = np.full(k, -1, np.int32), np.full(k, np.inf, np.float32)
    kk = min(k, len(rows))
    if kk:
        kth = np.partition(dd, kk - 1)[kk - 1]
        lo, eq = np.nonzero(dd < kth)[0], np.nonzero(dd == kth)[0]
        need = kk - len(lo)
        if len(eq) > need:
            eq = eq[np.argpartition(tt[eq], need - 1)[:need]]
        cand = np.concatenate([lo, eq])
        order = cand[np.lexsort((tt[cand], dd[cand]))]
        ids[:kk], dist[:kk] = rows[order], dd[order]
    return ids, dist


def closed_form(a, b, Q, k, tie=None, allowed=None, which=None):
    """-> ids, dist [nq][k]; rows of queries outside `which` are left -1 / +inf"""
    nq = len(Q.kind)
    ids, dist = np.full((nq, k), -1, np.int32), np.full((nq, k), np.inf, np.float32)
    for j in (range(nq) if which is None else which):
        ids[j], dist[j] = topk(distances(a, b, Q, j), k, tie, allowed)
    return ids, dist


def same_bits(ids, dist, want_ids, want_dist):
    return np.array_equal(ids, want_ids) and np.array_equal(np.ascontiguousarray(dist).view(np.uint32), np.ascontiguousarray(want_dist).view(np.uint32))


# ---------------------------------------------------------------- masks
def allowed_rows(mask, n, k, S):
    r = np.arange(n)
    if mask is None:
        return None
    if mask == "stripes":
        ok = (r // 3) % 2 == 0
    elif mask == "few":                                  # fewer than k rows (k >= 2): -1 / +inf fill the tail
        ok = np.isin(r, _dedupe([(i * 53 + 1) % n for i in range(max(1, k // 2))], n))
    elif mask == "splits":                               # whole splits without an allowed row, between full ones
        ok = (r // S) % 2 == 1 if n > S else (r // TILE) % 2 == 1 if n > TILE else r >= 0
    elif mask == "one":
        ok = r == (2 * n) // 3
    else:
        raise ValueError(mask)
    return ok


def labels_of(ok, exclude):
    """a filter that allows exactly the rows `ok`: -> labels [n], n_groups, label list, exclude"""
    n = len(ok)
    if ok.all():
        return np.zeros(n, np.int32), 1, np.array([0], np.int32), 0
    lab = np.where(ok, 0, 1).astype(np.int32)
    lab4 = lab + 2 * (np.arange(n, dtype=np.int32) & 1)
    if len(np.unique(lab4)) == 4:
        return lab4, 4, np.array([3, 1, 3] if exclude else [2, 0], np.int32), exclude
    return lab, 2, np.array([1] if exclude else [0], np.int32), exclude


# ---------------------------------------------------------------- the cases
FB_NS, FB_KS, FB_DIMS, FB_COUNTS = (1, 513, 16385), (1, 10, 32, 100), (64, 128), (0, 1, 8, 9, 64, 65, 73)
FB_CLASSES = ("ascending", "descending", "last_rows", "last_row", "one_per_split", "one_split", "alternating", "plateau_k", "plateau_tile",
              "plateau_split", "signs")
FbCase = collections.namedtuple("FbCase", "n cls ranks")
FbRun = collections.namedtuple("FbRun", "mask k count dim exclude")


def fb_cases():
    out = [FbCase(1, cls, rk) for cls in ("ascending", "plateau_k") for rk in RANKS]
    return out + [FbCase(n, cls, rk) for n in FB_NS[1:] for cls in FB_CLASSES for rk in RANKS]


def fb_runs(case):
    ci, ri = FB_CLASSES.index(case.cls), RANKS.index(case.ranks)
    masks = (None, "one") if case.n == 1 else MASKS
    return [FbRun(mask, FB_KS[(ci + ri + mi) % 4], FB_COUNTS[(2 * ci + ri + 3 * mi) % 7], FB_DIMS[(ci + mi) % 2], (ci + ri + mi) % 2)
            for mi, mask in enumerate(masks)]


def fb_id(c):
    return f"n{c.n}-{c.cls}-{c.ranks or 'rows'}"


def fb_flags(count):
    """`count` flagged queries at the odd positions between unflagged ones; flag values outside 0 .. 2 count as flagged"""
    nq = 2 * count + 1
    flags = np.array([(0, 1)[(j // 2) % 2] for j in range(nq)], np.int32)
    odd = (2, -5, 3, 2, 7, 2, 2 ** 31 - 1, 2, -2 ** 31)
    for i in range(count):
        flags[2 * i + 1] = odd[i % len(odd)]
    return flags


def sentinels(nq, k):
    """a pattern of its own in every slot (the distances: NaN payloads, compared as bits)"""
    slot = np.arange(nq * k, dtype=np.int64).reshape(nq, k)
    return (-1000 - slot).astype(np.int32), (0x7FC00000 + slot).astype(np.uint32).view(np.float32)


Scene = collections.namedtuple("Scene", "a b rows Q tie allowed")


def scene(cls, n, k, S, dim, nq, ranks, mask, filler):
    a, b = levels(cls, n, k, S)
    return Scene(a, b, rows_of(a, b, dim, filler), queries(nq, dim), rank_of(ranks, n), allowed_rows(mask, n, k, S))


EX_NS, EX_KS, EX_DIMS = (1, 8, 1020, 8192, 8193, 32768, 32769), (1, 9, 10, 255, 256, 257, 1024), (4, 36, 64, 100, 1536, 1540)
EX_NQS = (8, 9, 33, 1)
EX_CLASSES = ("ascending", "descending", "last_rows", "last_row", "one_per_split", "one_split", "alternating", "plateau_k", "plateau_tile",
              "plateau_chunk", "plateau_32768", "signs")
ExCase = collections.namedtuple("ExCase", "n cls")
ExRun = collections.namedtuple("ExRun", "ranks nq k dim")


def ex_cases():
    out = []
    for n in EX_NS:
        for cls in EX_CLASSES:
            if (cls == "plateau_32768" and n <= SMALL_MAX_N) or (cls == "plateau_chunk" and n <= SEL_CHUNK) or (cls == "plateau_tile" and n <= TILE):
                continue
            if n == 1 and cls not in ("ascending", "plateau_k", "last_row"):
                continue
            out.append(ExCase(n, cls))
    return out


def ex_runs(case):
    ci, ni = EX_CLASSES.index(case.cls), EX_NS.index(case.n)
    out = []
    for ri, ranks in enumerate(RANKS):
        for qi, nq in enumerate(EX_NQS):
            t = ri * 4 + qi
            k, dim = EX_KS[(ci + ni + t) % 7], EX_DIMS[(ci + t) % 4]
            if case.n <= 8193 and nq == 1:
                dim = 1540                               # the one-launch distance kernel does not fit: tiles, chunks, merge
            elif case.n <= 8193 and nq == 8 and ri == 1:
                dim = 1536                               # ... and the largest dim at which it does
            out.append(ExRun(ranks, nq, k, dim))
    return out


def ex_id(c):
    return f"n{c.n}-{c.cls}"


def exact_path(n, nq, dim):
    """search_exact's choice"""
    return "small" if nq <= EDS_MAX_Q and n <= SMALL_MAX_N and dim % 4 == 0 and EDS_MAX_Q * dim * 8 <= 96 << 10 else "chunks"


# the thread-column layout: (n, k, what the case is about).  rows per thread = n / 256.  n = 1,020 and 200 (ascending rows): fewer
# pieces than results, so the empty key is the threshold and padding keys are collected: past the list's size, and inside it
COLUMN = [(32768, 9, "overflow"), (32768, 8, "fits"), (32768, 10, "overflow"), (8192, 255, "overflow"), (8192, 33, "overflow"), (8192, 32, "fits"),
          (1020, 256, "padding"), (1020, 255, "fits"), (200, 256, "padding-list")]


# ---------------------------------------------------------------- the mechanisms, restated (CPU test only)
DEFECTS = ("no_displace", "ragged_tile_dropped", "merge_one_per_list", "no_slot_base", "mask_ignored", "tie_by_row", "unsigned_bits",
           "list_truncated", "threshold_low", "chunk_tail_real")
MECHANISM = {"no_displace": ("fallback",), "ragged_tile_dropped": ("fallback", "small", "chunks"), "merge_one_per_list": ("fallback", "chunks"),
             "no_slot_base": ("fallback",), "mask_ignored": ("fallback",), "tie_by_row": ("fallback", "small", "chunks"),
             "unsigned_bits": ("fallback", "small", "chunks"), "list_truncated": ("small",), "threshold_low": ("small",),
             "chunk_tail_real": ("fallback", "small", "chunks")}


def _mono(d32, defect):
    u = np.ascontiguousarray(d32, np.float32).view(np.uint32).astype(np.uint64)
    if defect == "unsigned_bits":
        return u
    return np.where(u >> np.uint64(31) == 1, ~u & np.uint64(0xFFFFFFFF), u | np.uint64(0x80000000))


def make_keys(d32, tie, defect=None, upto=None):
    """dist_key of every row; upto > n: rows n .. upto - 1 read as real zero rows (distance 1, tie = the row)"""
    n = len(d32)
    t = np.arange(n, dtype=np.uint64) if tie is None or defect == "tie_by_row" else tie.astype(np.uint64)
    keys = (_mono(d32, defect) << np.uint64(32)) | t
    if upto is not None and upto > n:
        ghost = (_mono(np.ones(upto - n, np.float32), defect) << np.uint64(32)) | np.arange(n, upto, dtype=np.uint64)
        keys = np.concatenate([keys, ghost])
    return keys


def read_keys(keys, k, n, tie, defect=None):
    """key_dist / tie_row of a list -> ids, dist [k]"""
    ids, dist = np.full(k, -1, np.int32), np.full(k, np.inf, np.float32)
    real = keys[keys != EMPTY][:k]
    u = (real >> np.uint64(32)).astype(np.uint32)
    if defect != "unsigned_bits":
        u = np.where(u >> 31 == 1, u & np.uint32(0x7FFFFFFF), ~u)
    t = (real & np.uint64(0xFFFFFFFF)).astype(np.int64)
    if tie is not None and defect != "tie_by_row":
        inv = np.empty(n, np.int64)
        inv[tie] = np.arange(n)
        t = np.where(t < n, inv[np.minimum(t, n - 1)], t)
    ids[:len(real)], dist[:len(real)] = t, u.astype(np.uint32).view(np.float32)
    return ids, dist


def model_split_lists(d32, tie, ok, k, S, defect=None):
    """exact_fallback_kernel: per split, tile after tile: the keys below the list's k-th enter, the k smallest stay"""
    n = len(d32)
    ghost = defect == "chunk_tail_real"
    keys = make_keys(d32, tie, defect, cdiv(n, TILE) * TILE if ghost else None)
    if ok is None or defect == "mask_ignored":
        ok = np.ones(n, bool)
    ok = np.concatenate([ok, np.ones(len(keys) - n, bool)])
    lists = []
    for r_begin in range(0, n, S):
        r_end = min(n, r_begin + S)
        best = np.full(k, EMPTY, np.uint64)
        for r0 in range(r_begin, r_end, TILE):
            t_end = min(r0 + TILE, r_end)
            if defect == "ragged_tile_dropped" and t_end - r0 < TILE:
                continue
            if ghost and t_end == n:
                t_end = len(keys)
            kt = keys[r0:t_end]
            cand = kt[ok[r0:t_end] & (kt < best[k - 1])]
            if defect == "no_displace" and r0 > r_begin:
                held = best[best != EMPTY]
                cand = np.sort(cand)[:k - len(held)]                      # the free entries fill; nothing held leaves
            best = np.sort(np.concatenate([best, cand]))[:k]
        lists.append(best)
    return lists


def model_merge(lists, k, defect=None):
    """fallback_merge_kernel / merge_topk_kernel: the k smallest keys of the ascending lists"""
    if defect == "merge_one_per_list":
        lists = [l[:1] for l in lists]
    allk = np.sort(np.concatenate(lists))
    return np.concatenate([allk, np.full(k, EMPTY, np.uint64)])[:k]


def model_fallback(sc, k, flags, plan, defect=None, only=None):
    """collect_flags_kernel + launch_fallback on sentinel-filled results -> ids, dist [nq][k], counters [4]
    only: the flagged-list positions to work out (the others keep the sentinel)"""
    nq, n = len(flags), len(sc.a)
    ids, dist = sentinels(nq, k)
    ids, dist = ids.copy(), dist.copy()
    f = np.where((flags < 0) | (flags > 2), 2, flags)
    slots = np.nonzero(f == 2)[0]
    counters = [len(slots)] + [int((f == s).sum()) for s in (0, 1, 2)]
    memo = {}
    for base, taken, S, _ in rounds(plan, nq, len(slots)):
        for s in range(taken):
            if only is not None and base + s not in only:
                continue
            scan =int(slots[s] if defect == "no_slot_base" else slots[base + s])        # whose lists the scan builds
            if (scan, S) not in memo:
                memo[scan, S] = model_merge(model_split_lists(distances(sc.a, sc.b, sc.Q, scan), sc.tie, sc.allowed, k, S, defect), k, defect)
            ids[slots[base + s]], dist[slots[base + s]] = read_keys(memo[scan, S], k, n, sc.tie, defect)
    return ids, dist, counters


def model_select_small(d32, tie, k, defect=None):
    """select_small_kernel -> ids, dist [k], info: the collected count c, the branch taken, padding keys in the list"""
    n = len(d32)
    pieces = (n + 3) >> 2
    real_upto = pieces * 4 if defect == "chunk_tail_real" else None
    keys = make_keys(d32, tie, defect, real_upto)
    if defect == "ragged_tile_dropped" and n % 4:
        keys = keys[:n - n % 4]
    mins = np.full(256, EMPTY, np.uint64)
    np.minimum.at(mins, thread_of(np.arange(len(keys))), keys)
    kk = min(k, n)
    at = min(kk, 256) - 1 - (defect == "threshold_low")
    thr = EMPTY - np.uint64(1) if kk > 256 else np.sort(mins)[at] if at >= 0 else np.uint64(0)
    got = keys[keys <= thr]
    # a thread walks 4 x 4 key slots per step of 1,024 pieces: the slots past n hold the empty key
    slots = 16 * sum(cdiv(pieces - t, 1024) for t in range(min(256, pieces)))
    padding = slots - len(keys) if thr == EMPTY else 0
    c = len(got) + padding
    info = dict(c=c, padding=padding, branch="slow" if c > SMALL_LIST else "list")
    if c > SMALL_LIST and defect == "list_truncated":
        got = got[:SMALL_LIST]                                            # (the order of the atomics: here, row order)
    elif c > SMALL_LIST:
        got = keys                                                        # kk rounds over global memory
    return read_keys(np.sort(got)[:kk], k, n, tie, defect) + (info,)


def model_chunks(d32, tie, k, defect=None):
    """select_chunk_kernel + merge_topk_kernel"""
    n = len(d32)
    keys = make_keys(d32, tie, defect, cdiv(n, SEL_CHUNK) * SEL_CHUNK if defect == "chunk_tail_real" else None)
    lists = []
    for base in range(0, n, SEL_CHUNK):
        ck = keys[base:base + SEL_CHUNK]
        if defect == "ragged_tile_dropped" and len(ck) < SEL_CHUNK:
            continue
        lists.append(np.concatenate([np.sort(ck), np.full(k, EMPTY, np.uint64)])[:k])
    merged = model_merge(lists, k, defect) if lists else np.full(k, EMPTY, np.uint64)
    return read_keys(merged, k, n, tie, defect)


def model_exact(sc, k, j, path, defect=None):
    d = distances(sc.a, sc.b, sc.Q, j)
    return model_select_small(d, sc.tie, k, defect)[:2] if path == "small" else model_chunks(d, sc.tie, k, defect)


# ---------------------------------------------------------------- the Gaussian class: the fp64 chain at ragged dims, against the C oracle
def gaussian(rng, n, nq, dim, unit):
    rows = rng.standard_normal((n, dim))
    qs = rng.standard_normal((nq, dim))
    if unit:
        rows /= np.linalg.norm(rows, axis=1, keepdims=True)
        qs /= np.linalg.norm(qs, axis=1, keepdims=True)
    return rows.astype(np.float32), qs.astype(np.float32)


def oracle_expected(knn_oracle, rows, qs, k, tie=None, allowed=None):
    """knn_oracle.distances, then the (distance, tie) order over the allowed rows"""
    ids, dist = np.full((len(qs), k), -1, np.int32), np.full((len(qs), k), np.inf, np.float32)
    for j, q in enumerate(qs):
        ids[j], dist[j] = topk(knn_oracle.distances(rows, q), k, tie, allowed)
    return ids, dist
