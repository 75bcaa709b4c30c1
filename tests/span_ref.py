"""The span search's definition (include/vq_amd.h, vq_index_search_spans) restated in numpy, twice: `span_brute` tries every
index range of a group, `span_scan` walks the prefix sums as the kernels do (the smallest prefix in front of every end, ties
to the largest index, then the best end).  `span_answer` runs either over a whole index: the C oracle's distances in, per
query the (label, D, mass, length, (start, end, peak) rows) list out."""
import numpy as np

NO_LIMIT = 2 ** 40
CAP = 2 ** 32                                                     # positions are 32-bit: a limit of 2^32 or more is none
GAIN_CAP = float(2 ** 31)


def gains(d, tau):
    """w = (int64) rint(((double)tau - (double)d) * 2^24), kept within +-2^31 (NaN: -2^31).  d: float32 array, tau: float32."""
    g = np.rint((np.float64(np.float32(tau)) - np.asarray(d, dtype=np.float32).astype(np.float64)) * 16777216.0)
    return np.fmin(np.fmax(g, -GAIN_CAP), GAIN_CAP).astype(np.int64)


def rank_value(mass):
    """D = fp32(-(double)S * 2^-24)"""
    return np.float32(-float(int(mass)) * 2.0 ** -24)


def _better(c, best):
    """(S, length, a): largest S, then shortest, then earliest"""
    return best is None or (-c[0], c[1], c[2]) < (-best[0], best[1], best[2])


def span_brute(w, pos, max_gap=NO_LIMIT, max_span=NO_LIMIT):
    """One group in (position, tie) order: w int64 gains, pos positions.  Every admissible [a, b] is tried.
    -> None, or (S, a, b, tie_decided) — tie_decided: another admissible span has the same mass, so length or start chose."""
    w = [int(x) for x in w]
    pos = [int(p) for p in pos]
    max_gap, max_span = min(int(max_gap), CAP), min(int(max_span), CAP)
    L = len(w)
    best, rivals = None, 0
    for a in range(L):
        s = 0
        for b in range(a, L):
            if b > a and pos[b] - pos[b - 1] > max_gap:
                break
            if pos[b] - pos[a] > max_span:
                break
            s += w[b]
            if s <= 0:
                continue
            c = (s, b - a + 1, a)
            if best is not None and s == best[0]:
                rivals += 1
            elif best is None or s > best[0]:
                rivals = 0
            if _better(c, best):
                best = c
    if best is None:
        return None
    return best[0], best[2], best[2] + best[1] - 1, rivals > 0


def span_scan(w, pos, max_gap=NO_LIMIT, max_span=NO_LIMIT):
    """`span_brute` by prefix sums: for every end b the start a(b) in [lo(b), b] with the smallest P (ties to the largest
    index), then the best candidate (P[b+1] - P[a(b)], length, a(b)) over b.  tie_decided here: two ENDS give the best mass."""
    w = np.asarray(w, dtype=np.int64)
    pos = np.asarray(pos, dtype=np.int64)
    max_gap, max_span = min(int(max_gap), CAP), min(int(max_span), CAP)
    L = len(w)
    P = np.concatenate([[0], np.cumsum(w)]).astype(np.int64)
    idx = np.arange(L)
    brk = np.where(np.concatenate([[False], np.diff(pos) > max_gap]), idx, 0)
    seg = np.maximum.accumulate(brk)
    lo = np.maximum(seg, np.searchsorted(pos, pos - max_span, side="left"))
    if not lo.any():                                               # the prefix minimum, ties to the largest index
        a_of = np.empty(L, dtype=np.int64)
        cur = 0
        for b in range(L):
            if P[b] <= P[cur]:
                cur = b
            a_of[b] = cur
    else:
        a_of = np.array([b - int(np.argmin(P[lo[b]:b + 1][::-1])) for b in range(L)], dtype=np.int64)
    S = P[1:] - P[a_of]
    top = int(S.max()) if L else 0
    if top <= 0:
        return None
    ends = np.flatnonzero(S == top)
    length = ends - a_of[ends] + 1
    j = np.lexsort((a_of[ends], length))[0]
    b = int(ends[j])
    return top, int(a_of[b]), b, len(ends) > 1


def span_answer(dist, labels, pos, tie, tau, max_gap=NO_LIMIT, max_span=NO_LIMIT, k=10, allowed=None, one=span_scan):
    """dist [nq][n] float32 (the oracle's d(i, r) for every row of the index); labels / pos / tie per row.
    -> per query ([(label, D float32, mass, length, (start row, end row, peak row))] — the first k by (D, label) —,
                  {label: tie_decided}, groups that hold a span, two holding groups share a D?)"""
    labels = np.asarray(labels)
    pos = np.asarray(pos, dtype=np.int64)
    tie = np.asarray(tie, dtype=np.int64)
    orders = {}
    for g in range(int(labels.max()) + 1):
        if allowed is not None and g not in allowed:
            continue
        rows = np.flatnonzero(labels == g)
        if len(rows):
            orders[g] = rows[np.lexsort((tie[rows], pos[rows]))]
    answers = []
    for d in dist:
        d = np.asarray(d, dtype=np.float32)
        out, decided = [], {}
        for g, rows in orders.items():
            res = one(gains(d[rows], tau), pos[rows], max_gap, max_span)
            if res is None:
                continue
            s, a, b, dec = res
            inside = rows[a:b + 1]
            peak = inside[np.lexsort((tie[inside], d[inside]))[0]]
            out.append((g, rank_value(s), s, b - a + 1, (int(rows[a]), int(rows[b]), int(peak))))
            decided[g] = dec
        out.sort(key=lambda t: (t[1], t[0]))
        ds = [t[1].tobytes() for t in out]
        answers.append((out[:k], decided, len(out), len(set(ds)) < len(ds)))
    return answers
