"""Warped clip alignment's definition (include/vq_amd.h, vq_index_align_clip) restated in numpy, twice: `align_brute` fills the
DP table cell by cell with the stated predecessor order, `align_scan` builds every DP row from one prefix sum and one prefix
minimum as the kernels do.  `align_answer` runs either over a whole index: the C oracle's distances in, the
(label, D, C, (start row, end row), per-frame (first row, last row)) list out."""
import numpy as np

COST_CAP = float(2 ** 31)


def costs(d):
    """c = (int64) rint((double)d * 2^24), kept within +-2^31 (NaN: +2^31).  d: float32 array."""
    d = np.asarray(d, dtype=np.float32).astype(np.float64)
    with np.errstate(invalid="ignore"):
        c = np.fmin(np.fmax(np.rint(d * 16777216.0), -COST_CAP), COST_CAP)
    return np.where(np.isnan(d), COST_CAP, c).astype(np.int64)


def rank_value(cost, m):
    """D = fp32((double)C * 2^-24 / (double)m)"""
    return np.float32(float(int(cost)) * 2.0 ** -24 / float(m))


def _finish(last_c, last_a, pred):
    """The best end of the last DP row and the path behind it.  pred(i, j) -> (entry column of DP row i's cell j, came down the
    diagonal?).  -> (C, a, b, [(first j, last j)] per clip frame)"""
    L = len(last_c)
    b = min(range(L), key=lambda j: (int(last_c[j]), j - int(last_a[j]) + 1, int(last_a[j])))
    m = pred.m
    pairs = [None] * m
    j = b
    for i in range(m - 1, -1, -1):
        col, diag = pred(i, j)
        pairs[i] = (col, j)
        j = col - 1 if diag else col
    assert pairs[0][0] == int(last_a[b])
    return int(last_c[b]), int(last_a[b]), b, pairs


def align_brute(c):
    """c [m][L] integer costs of one group in (position, tie) order.  Cell (i, j) holds the smallest key (C, -a) over the paths
    that end there; its predecessor is the first, in the order diagonal, vertical, [i = 0: starts here], horizontal, whose key
    equals that minimum."""
    c = [[int(v) for v in row] for row in c]
    m, L = len(c), len(c[0])
    C = [[0] * L for _ in range(m)]
    A = [[0] * L for _ in range(m)]
    step = [[None] * L for _ in range(m)]
    for i in range(m):
        for j in range(L):
            cands = []
            if i > 0 and j > 0:
                cands.append(((C[i - 1][j - 1], -A[i - 1][j - 1]), "d"))
            if i > 0:
                cands.append(((C[i - 1][j], -A[i - 1][j]), "v"))
            if i == 0:
                cands.append(((0, -j), "s"))
            if j > 0:
                cands.append(((C[i][j - 1], -A[i][j - 1]), "h"))
            best = min(key for key, _ in cands)
            step[i][j] = next(s for key, s in cands if key == best)
            C[i][j] = best[0] + c[i][j]
            A[i][j] = -best[1]

    def pred(i, j):
        col = j
        while step[i][col] == "h":
            col -= 1
        return col, step[i][col] == "d"
    pred.m = m
    return _finish(C[m - 1], A[m - 1], pred)


def align_scan(c):
    """`align_brute` row by row: P = the exclusive prefix sums of c(i, .); E(j) = the smaller key of the previous DP row at j - 1
    and at j, ties to j - 1 (i = 0: (0, -j)); cell (i, j) = P[j + 1] + the prefix minimum over j' <= j of
    (E(j').C - P[j'], -E(j').a, -j')."""
    c = np.asarray(c, dtype=np.int64)
    m, L = c.shape
    assert L < 2 ** 20
    idx = np.arange(L, dtype=np.int64)
    entry = np.empty((m, L), dtype=np.int64)
    diag = np.zeros((m, L), dtype=bool)
    BIG = 4 * (L + 1) ** 2
    C = A = None
    for i in range(m):
        P = np.concatenate([[0], np.cumsum(c[i])]).astype(np.int64)
        if i == 0:
            EC, EA, dg = np.zeros(L, dtype=np.int64), idx.copy(), np.zeros(L, dtype=bool)
        else:
            lC, lA = np.concatenate([[0], C[:-1]]), np.concatenate([[0], A[:-1]])
            dg = (idx > 0) & ((lC < C) | ((lC == C) & (lA >= A)))
            EC, EA = np.where(dg, lC, C), np.where(dg, lA, A)
        v = EC - P[:-1]
        vmin = np.minimum.accumulate(v)
        # among the columns that hold the prefix minimum: the latest start, then the latest column.  A running minimum of
        # s = -(a (L + 1) + j') inside every stretch of equal vmin (each starts at a column that holds it)
        run = np.concatenate([[0], np.cumsum(vmin[1:] != vmin[:-1])]).astype(np.int64)
        s = -(EA * (L + 1) + idx)
        t = np.where(v == vmin, s, BIG) - run * (2 * BIG)
        best = -(np.minimum.accumulate(t) + run * (2 * BIG))
        A, col = best // (L + 1), best % (L + 1)
        C = P[1:] + vmin
        entry[i], diag[i] = col, dg[col]

    def pred(i, j):
        return int(entry[i][j]), bool(diag[i][j])
    pred.m = m
    return _finish(C, A, pred)


def align_answer(dist, labels, pos, tie, max_dist=np.inf, k=10, allowed=None, one=align_scan):
    """dist [m][n] float32 (the oracle's d(i, r) of every clip frame to every row of the index); labels / pos / tie per row.
    -> ([(label, D float32, C, (start row, end row), [(first row, last row)] per clip frame)] — the first k by (C, label) among
        the groups with D <= max_dist —, groups with a result, two such groups share a D?)"""
    dist = np.asarray(dist, dtype=np.float32)
    m = len(dist)
    labels = np.asarray(labels)
    pos = np.asarray(pos, dtype=np.int64)
    tie = np.asarray(tie, dtype=np.int64)
    out = []
    for g in range(int(labels.max()) + 1 if len(labels) else 0):
        if allowed is not None and g not in allowed:
            continue
        rows = np.flatnonzero(labels == g)
        if not len(rows):
            continue
        rows = rows[np.lexsort((tie[rows], pos[rows]))]
        cost, a, b, pairs = one(costs(dist[:, rows]))
        D = rank_value(cost, m)
        if D <= np.float32(max_dist):
            out.append((g, D, cost, (int(rows[a]), int(rows[b])), [(int(rows[f]), int(rows[l])) for f, l in pairs]))
    out.sort(key=lambda t: (t[2], t[0]))
    ds = [t[1].tobytes() for t in out]
    return out[:k], len(out), len(set(ds)) < len(ds)
