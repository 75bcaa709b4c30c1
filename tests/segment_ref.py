"""The definition of chapter segmentation (include/vq_amd.h, vq_index_segment_groups) restated in numpy, shared by
tests/test_segment.py (over the exported rows) and tests/test_segment_cpu.py (hand-made cases).  The order of every
floating-point operation is the definition's: one fp64 chain per column along the (position, tie) order for the prefix rows, one
fp64 subtraction rounded to fp32 per column of a run, the fp64 chain over the columns for |u|^2, one square root, one fp64
addition per step of the dynamic programme.  Every numpy operation below is one IEEE operation per element (add, subtract,
multiply of two fp32 values widened to fp64 — exact —, divide, square root) or a rounding to fp32; nothing here calls ``sum``."""
import numpy as np


def order_of(rows, pos, tie):
    """The rows of a group in ascending (position, tie) order.  pos / tie: per row of the index."""
    return sorted((int(r) for r in rows), key=lambda r: (int(pos[r]), int(tie[r])))


def prefix_rows(stored, order):
    """fp64 [L + 1][dim]: P_0 = 0, P_{t+1} = P_t + x_{order[t]}, one chain per column."""
    P = np.zeros((len(order) + 1, stored.shape[1]), dtype=np.float64)
    for t, r in enumerate(order):
        P[t + 1] = P[t] + stored[r].astype(np.float64)
    return P


def tree_prefix_rows(stored, order):
    """The same sums in ANOTHER order (a Hillis-Steele scan: P_t gathers its terms pairwise): what a blocked or tree scan on the
    device would produce.  Not the definition; test_segment_cpu.py shows that it gives other cost bits on cancelling rows."""
    X = np.stack([stored[r].astype(np.float64) for r in order]) if len(order) else np.zeros((0, stored.shape[1]))
    step = 1
    while step < len(X):
        Y = X.copy()
        Y[step:] = X[step:] + X[:-step]
        X, step = Y, step * 2
    return np.concatenate([np.zeros((1, stored.shape[1])), X])


def run_direction(P, a, b):
    """u of the run [a, b): one fp64 subtraction per column, rounded to fp32."""
    return (P[b] - P[a]).astype(np.float32)


def cost_table(P, W, block=32):
    """fp64 [L + 1][W]: C[b][b - a - 1] = cost(a, b) for 0 <= a < b <= L, b - a <= W; NaN elsewhere."""
    L, dim = len(P) - 1, P.shape[1]
    C = np.full((L + 1, max(W, 1)), np.nan, dtype=np.float64)
    for b0 in range(1, L + 1, block):
        bi, ai = [], []
        for b in range(b0, min(b0 + block, L + 1)):
            a = np.arange(max(0, b - W), b)
            ai.append(a)
            bi.append(np.full(len(a), b))
        bi, ai = np.concatenate(bi), np.concatenate(ai)
        U = np.ascontiguousarray((P[bi] - P[ai]).astype(np.float32).astype(np.float64).T)      # [dim][pairs]
        V = np.zeros(len(bi), dtype=np.float64)
        for i in range(dim):
            V = V + U[i] * U[i]                     # the product of two fp32 values is exact in fp64
        C[bi, bi - ai - 1] = (bi - ai).astype(np.float64) - np.sqrt(V)
    return C


def chapters(C, L, W, k, penalty):
    """Steps 3 - 5 over a cost table: (cuts [(a, b)] in time order, E_kappa(L) or None).  kappa = len(cuts)."""
    K = min(k, L)
    E = np.full(L + 1, np.nan)
    defined = np.zeros(L + 1, dtype=bool)
    E[0], defined[0] = 0.0, True
    b = np.arange(L + 1)[:, None]
    d = np.arange(W)[None, :]
    a = b - 1 - d                                                    # [L + 1][W]
    back, EL = [], []
    for c in range(1, K + 1):
        ok = (a >= c - 1) & (a >= 0) & (b >= c) & defined[np.clip(a, 0, L)]
        with np.errstate(invalid="ignore"):
            S = np.where(ok, E[np.clip(a, 0, L)] + C[:, :W], np.inf)
        # the smallest (sum, a): a falls as d grows, so among equal sums the LAST d
        dbest = W - 1 - np.argmin(np.where(ok, S, np.inf)[:, ::-1], axis=1)
        any_ok = ok.any(axis=1)
        E = np.where(any_ok, S[np.arange(L + 1), dbest], np.nan)
        defined = any_ok
        back.append(np.where(any_ok, np.arange(L + 1) - 1 - dbest, -1))
        EL.append(E[L] if defined[L] else None)
    penalty = np.float64(np.float32(penalty))
    kappa, best = 0, None
    for c in range(1, K + 1):
        if EL[c - 1] is None:
            continue
        F = EL[c - 1] + np.float64(c) * penalty
        if kappa == 0 or F < best:
            kappa, best = c, F
    cuts, bb = [], L
    for c in range(kappa, 0, -1):
        aa = int(back[c - 1][bb])
        cuts.append((aa, bb))
        bb = aa
    return cuts[::-1], (EL[kappa - 1] if kappa else None)


def show_row(stored, order, tie, P, a, b):
    """The row of the run [a, b) with the smallest (1.0f - (float)chain(x_r . u), tie)."""
    u = run_direction(P, a, b).astype(np.float64)
    X = np.ascontiguousarray(np.stack([stored[r] for r in order[a:b]]).astype(np.float64).T)       # [dim][rows]
    acc = np.zeros(b - a, dtype=np.float64)
    for i in range(len(u)):
        acc = acc + X[i] * u[i]
    dist = np.float32(1.0) - acc.astype(np.float32)
    return min(range(a, b), key=lambda p: (dist[p - a], int(tie[order[p]])))


def segment(stored, order, tie, k, penalty, W, table=None):
    """One group.  order: its rows in (position, tie) order; tie: per row of the index; W: the longest run (L without max_len).
    table: (P, C) of an earlier call with the same stored / order / W.
    -> dict(count, first, last, len, spread, show: arrays of count entries; mean_spread float32)"""
    stored = np.asarray(stored, dtype=np.float32)
    L = len(order)
    P, C = table if table is not None else tables(stored, order, W)
    cuts, total = chapters(C, L, W, k, penalty)
    first = np.array([order[a] for a, b in cuts], dtype=np.int32)
    last = np.array([order[b - 1] for a, b in cuts], dtype=np.int32)
    lens = np.array([b - a for a, b in cuts], dtype=np.int32)
    spread = np.array([C[b][b - a - 1] / np.float64(b - a) for a, b in cuts], dtype=np.float64).astype(np.float32)
    show = np.array([order[show_row(stored, order, tie, P, a, b)] for a, b in cuts], dtype=np.int32)
    mean = np.float32(total / np.float64(L)) if cuts else np.float32(np.inf)
    return dict(count=len(cuts), first=first, last=last, len=lens, spread=spread, show=show, mean_spread=mean, cuts=cuts)


def tables(stored, order, W):
    P = prefix_rows(np.asarray(stored, dtype=np.float32), order)
    return P, cost_table(P, W)


def run_limit(L, max_len):
    return L if not max_len else min(L, int(max_len))
