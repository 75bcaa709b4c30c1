"""The definition of library clustering (include/vq_amd.h, vq_index_cluster) restated in numpy, shared by tests/test_cluster.py
(over the C oracle's distances) and tests/test_cluster_cpu.py (hand-made cases).  The order of every floating-point operation is
the definition's: rows of a cluster in ascending row number, pieces of 1,024, one fp64 chain per column and piece, the pieces'
sums added in piece order, the chain over the columns for |mean|^2.  Every numpy operation below is one IEEE fp64 operation per
element (add, divide, square root) or a rounding to fp32; nothing here calls ``sum``."""
import numpy as np

import label_ref

PIECE = 1024


def column_sums(stored, rows):
    """fp64 [dim]: the rows' columns, piece by piece, each piece a chain from 0.0 in list order."""
    dim = stored.shape[1]
    s = np.zeros(dim, dtype=np.float64)
    for b in range(0, len(rows), PIECE):
        piece = np.zeros(dim, dtype=np.float64)
        for r in rows[b:b + PIECE]:
            piece = piece + stored[r].astype(np.float64)
        s = s + piece
    return s


def cancelling_rows(rng, n, dim):
    """Rows on which the ORDER of a sum decides its value: a third of them +g, a third -g with |g| from 1 down to 1e-20, the rest
    of magnitude 1e-20, shuffled.  Everything large cancels exactly, so what an fp64 sum returns is what its additions rounded
    away on the way: a chain, a chain per piece and a tree give different fp32 means in every column (test_cluster_cpu.py)."""
    k = n // 3
    g = (rng.standard_normal((k, dim)) * 10.0 ** -rng.uniform(0, 20, (k, 1))).astype(np.float32)
    rest = (rng.standard_normal((n - 2 * k, dim)) * 1e-20).astype(np.float32)
    return np.concatenate([g, -g, rest])[rng.permutation(n)]


def update(stored, L, C):
    """C_{t+1} float32 [P][dim] from the labels L [n] and C_t: a cluster without rows, or with a zero mean, keeps its bits."""
    stored = np.asarray(stored, dtype=np.float32)
    nxt = np.array(C, dtype=np.float32, copy=True)
    for j in range(len(nxt)):
        rows = np.flatnonzero(np.asarray(L) == j)
        if len(rows) == 0:
            continue
        m = (column_sums(stored, rows) / np.float64(len(rows))).astype(np.float32)
        n2 = np.float64(0.0)
        for v in m.astype(np.float64):
            n2 = n2 + v * v                       # the product of two fp32 values is exact in fp64
        if n2 == 0.0:
            continue
        nxt[j] = (m.astype(np.float64) / np.sqrt(n2)).astype(np.float32)
    return nxt


def show_rows(L, best, tie, P):
    """int32 [P]: per cluster the row with the smallest (best, tie); -1 without rows."""
    show = np.full(P, -1, dtype=np.int32)
    for j in range(P):
        rows = np.flatnonzero(L == j)
        if len(rows):
            show[j] = min(rows.tolist(), key=lambda r: (best[r], tie[r]))
    return show


def cluster(stored, C1, max_iter, tie=None, distances=label_ref.distances):
    """-> dict(centroids, labels, distances, counts, show, iterations, changed); ``distances(stored, C)`` gives float32 [P][n]."""
    stored = np.ascontiguousarray(stored, dtype=np.float32)
    C = np.array(C1, dtype=np.float32, copy=True)
    n, P = len(stored), len(C)
    tie = np.arange(n) if tie is None else np.asarray(tie)
    prev, changed = None, []
    for t in range(1, max_iter + 1):
        L, best = label_ref.row_labels(distances(stored, C))
        changed.append(n if prev is None else int((L != prev).sum()))
        if (t > 1 and changed[-1] == 0) or t == max_iter:
            break
        C, prev = update(stored, L, C), L
    return dict(centroids=C, labels=L, distances=best, counts=np.bincount(L, minlength=P).astype(np.int32), show=show_rows(L, best, tie, P),
                iterations=t, changed=changed)
